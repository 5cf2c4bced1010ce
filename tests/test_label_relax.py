"""The regulariser of SPEC.md §30 on the CPU: the symbol table (include/gcs_relax.h <-> ``_lib.RELAX_EXTENSIONS`` <-> the built
library's exports), the argument rules of the two entry points (refused before anything is launched, so they run without a GPU),
the restatement (tests/label_relax_ref.py) on the worked examples of the SPEC and on the facts the SPEC proves, and the host
logic - the plan's ``regularize``, the beta arithmetic, the refusals - through the stand-in ops (tests/label_relax_ops.py). No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kmeans_model_ref as km
import label_relax_ref as lr
from gabor_color_image_segmentation_amd import Segmenter, make_bank
from gabor_color_image_segmentation_amd.segmenter import relax_beta
from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
from kmeans_seed_ops import KMeansSeedOps
from label_relax_ops import LabelRelaxOps
from oracle import spec_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the library: symbols and argument rules

@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def test_header_table_and_exports_agree(lib):
    from gabor_color_image_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gcs_relax.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gcs_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.RELAX_EXTENSIONS) == {"gcs_kmeans_costs", "gcs_label_relax"}, declared ^ set(_lib.RELAX_EXTENSIONS)
    assert 'extern "C"' in hdr and "ABI 18" in hdr and '#include "gcs.h"' in hdr
    assert "torch" not in hdr.lower() and "at::" not in hdr
    for name, (res, args) in _lib.RELAX_EXTENSIONS.items():
        fn = getattr(lib, name)                               # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):                        # pointers and the stream: void pointers; everything else: int
            assert (a is C.c_void_p) == ("*" in p or p.startswith("gcs_stream_t")), (name, p)
    others = set(_lib.SIGNATURES) | set(_lib.EXTENSIONS) | set(_lib.THIN_EXTENSIONS) | set(_lib.MATCH_EXTENSIONS) \
        | set(_lib.MODEL_EXTENSIONS) | set(_lib.SEED_EXTENSIONS)
    assert not set(_lib.RELAX_EXTENSIONS) & others
    assert lib.gcs_abi_version() == 18 and _lib.ABI_VERSION == 18
    for name in ("gcs.h", "gcs_cues.h", "gcs_thin.h", "gcs_match.h", "gcs_model.h", "gcs_seed.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert "gcs_label_relax" not in text and "gcs_kmeans_costs" not in text, name


def test_ops_refuse_a_library_without_the_symbols():
    from gabor_color_image_segmentation_amd import _lib
    from gabor_color_image_segmentation_amd.segmenter import HipOps

    class Old:
        pass
    ops = HipOps.__new__(HipOps)
    ops.lib = Old()
    with pytest.raises(_lib.GcsError, match="does not export gcs_kmeans_costs"):
        HipOps.kmeans_costs.__wrapped__(ops, None, None, 1, 8, 8, 2, 1, None)
    with pytest.raises(_lib.GcsError, match="does not export gcs_label_relax"):
        HipOps.label_relax.__wrapped__(ops, None, None, 1, 8, 8, 2, 8, 1, None, None)


def test_entry_points_validate_before_launching(lib):
    """Argument errors are reported with code 1 and a message, without touching the GPU (so this runs on the CPU box)."""
    p = [C.c_void_p(q << 40) for q in range(1, 8)]            # non-NULL dummies far apart, never dereferenced
    good = dict(costs=p[0], beta=p[1], B=3, H=19, W=23, k=8, nb=8, sweeps=4, lin=p[2], lout=p[3], ws=p[4], ch=p[5], en=p[6])

    def relax(**bad):
        a = dict(good, **bad)
        return lib.gcs_label_relax(a["costs"], a["beta"], a["B"], a["H"], a["W"], a["k"], a["nb"], a["sweeps"], a["lin"], a["lout"],
                                   a["ws"], a["ch"], a["en"], None)
    for bad in (dict(costs=None), dict(beta=None), dict(lin=None), dict(lout=None)):
        assert relax(**bad) == 1 and b"NULL" in lib.gcs_last_error(), bad
    for bad in (dict(k=0), dict(k=-1), dict(k=17)):
        assert relax(**bad) == 1 and b"k must be in 1..16" in lib.gcs_last_error(), bad
    for bad in (dict(nb=0), dict(nb=6), dict(nb=-8), dict(nb=16)):
        assert relax(**bad) == 1 and b"neighbours must be 4 or 8" in lib.gcs_last_error(), bad
    for bad in (dict(sweeps=-1), dict(sweeps=65)):
        assert relax(**bad) == 1 and b"sweeps must be in 0..64" in lib.gcs_last_error(), bad
    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097)):
        assert relax(**bad) == 1 and b"bad shape" in lib.gcs_last_error(), bad
    for sweeps in (2, 64):
        assert relax(sweeps=sweeps, ws=None) == 1 and b"workspace" in lib.gcs_last_error()
    n = 3 * 19 * 23 * 4
    for lout in (p[2], C.c_void_p(p[2].value + 4), C.c_void_p(p[2].value + n - 4), C.c_void_p(p[2].value - n + 4)):
        assert relax(lout=lout) == 1 and b"overlap" in lib.gcs_last_error(), lout
    assert b"gcs_label_relax" in lib.gcs_last_error()

    goodc = dict(feats=p[0], cent=p[1], B=3, H=19, W=23, ns=4, no=6, k=8, n_sets=3, costs=p[2])

    def costs(**bad):
        a = dict(goodc, **bad)
        return lib.gcs_kmeans_costs(a["feats"], a["cent"], a["B"], a["H"], a["W"], a["ns"], a["no"], a["k"], a["n_sets"], a["costs"], None)
    for bad in (dict(feats=None), dict(cent=None), dict(costs=None)):
        assert costs(**bad) == 1 and b"NULL" in lib.gcs_last_error(), bad
    for bad in (dict(k=0), dict(k=17)):
        assert costs(**bad) == 1 and b"k must be in 1..16" in lib.gcs_last_error(), bad
    for bad in (dict(n_sets=0), dict(n_sets=2), dict(n_sets=4)):
        assert costs(**bad) == 1 and b"n_sets" in lib.gcs_last_error(), bad
    for bad in (dict(B=0, n_sets=1), dict(B=65536, n_sets=1), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(ns=0), dict(ns=9),
                dict(no=0), dict(ns=8, no=65)):
        assert costs(**bad) == 1 and b"bad shape or bank" in lib.gcs_last_error(), bad
    assert costs(B=64, n_sets=1, H=4096, W=4096) == 1 and b"P * D < 2^31" in lib.gcs_last_error()
    assert b"gcs_kmeans_costs" in lib.gcs_last_error()
    # (a call inside every rule would launch, so it is made on the GPU: tests/test_gpu_label_relax.py)


# ---- the restatement

def test_the_worked_examples():
    c = np.array([[0, 10], [5, 4], [0, 10]], np.int64).T.reshape(2, 1, 3)          # pixel x j -> (k, 1, 3)
    start = np.array([[0, 1, 0]])
    assert lr.total_energy(c, start, 3, 4) == 4 + 3 * 2 == 10
    lab = start.astype(np.int64).copy()
    assert lr.sub_pass(c, lab, 3, 0, 4) == 0 and lab.tolist() == [[0, 1, 0]]       # E = (3, 10) at both ends: they stay
    assert lr.sub_pass(c, lab, 3, 1, 4) == 1 and lab.tolist() == [[0, 0, 0]]       # E_0 = 5, E_1 = 4 + 6
    out, changed, (unary, pairs) = lr.relax(c, start, 3, 1, 4)
    assert out.tolist() == [[0, 0, 0]] and changed == [1] and (unary, pairs) == (5, 0) and out.dtype == np.int32
    assert lr.relax(c, start, 3, 1, 8)[0].tolist() == [[0, 0, 0]]                  # (a single row has no diagonal neighbours)
    # the tie: E = (6, 6), the pixel keeps label 1; from label 0 it would keep 0
    c[:, 0, 1] = (6, 4)
    for own in (1, 0):
        out, changed, _ = lr.relax(c, np.array([[0, own, 0]]), 1, 1, 4)
        assert out.tolist() == [[0, own, 0]] and changed == [0]


def _volume(rng, k, h, w, top):
    return rng.integers(0, top, size=(k, h, w), dtype=np.int64)


def test_energy_never_rises_and_falls_strictly_with_every_change():
    rng = np.random.default_rng(30)
    moved = 0
    for case in range(24):
        k, h, w = int(rng.integers(1, 9)), int(rng.integers(1, 14)), int(rng.integers(1, 14))
        nb, beta = (4, 8)[case & 1], int(rng.integers(0, 6))
        c = _volume(rng, k, h, w, 4 if case % 3 else 1000)
        lab = rng.integers(-1 if case % 4 == 0 else 0, k + (case % 4 == 0), size=(h, w))
        e = lr.total_energy(c, lab, beta, nb)
        fixed = False
        for s in range(8):
            nxt, changed, (unary, pairs) = lr.relax(c, lab, beta, 1, nb)
            e_next = unary + beta * pairs
            assert e_next == lr.total_energy(c, nxt, beta, nb)
            assert e_next <= e
            if changed[0] > 0:
                assert e_next < e and not fixed, (case, s)
                moved += 1
            else:
                assert np.array_equal(nxt, lab)               # a fixed point: every later sweep is the identity
                fixed = True
            # every sub-pass on its own never raises the energy either
            step = lab.astype(np.int64).copy()
            for cls in range(4):
                before = lr.total_energy(c, step, beta, nb)
                lr.sub_pass(c, step, beta, cls, nb)
                assert lr.total_energy(c, step, beta, nb) <= before
            assert np.array_equal(step, nxt)
            lab, e = nxt, e_next
        many, changed, _ = lr.relax(c, lab, beta, 3, nb)
        if fixed:
            assert changed == [0, 0, 0] and np.array_equal(many, lab)
    assert moved > 24, "hardly a sweep changed a label: the cases prove nothing"


def test_sweeps_compose_and_changed_counts_labels():
    rng = np.random.default_rng(31)
    c = _volume(rng, 5, 9, 11, 4)
    lab = rng.integers(0, 5, size=(9, 11))
    out, changed, en = lr.relax(c, lab, 2, 5, 8)
    step, seen = lab, []
    for s in range(5):
        nxt = lr.relax(c, step, 2, 1, 8)[0]
        seen.append(int((nxt != step).sum()))
        step = nxt
    assert np.array_equal(out, step) and changed == seen and changed[0] > 0
    assert lr.relax(c, lab, 2, 0, 8)[0].tolist() == lab.tolist() and lr.relax(c, lab, 2, 0, 8)[1] == []
    assert en == lr.energy(c, out, 8) and lr.energy(c, out, 4)[1] < en[1]


def test_beta_zero_is_the_argmin_with_ties_to_the_current_label():
    rng = np.random.default_rng(32)
    for k in (1, 2, 7, 16):
        c = _volume(rng, k, 8, 9, 3)                          # costs in 0..2: ties everywhere
        lab = rng.integers(0, k, size=(8, 9))
        out, changed, (unary, pairs) = lr.relax(c, lab, 0, 1, 8)
        low = c.min(axis=0)
        keeps = np.take_along_axis(c, lab[None], axis=0)[0] == low
        assert np.array_equal(out, np.where(keeps, lab, c.argmin(axis=0)))
        assert unary == int(low.sum()) and changed == [int((~keeps).sum())]
        assert lr.relax(c, out, 0, 1, 8)[1] == [0]
        if k > 1:
            assert keeps.any() and (~keeps).any() and (lab[keeps] != c.argmin(axis=0)[keeps]).any()


def test_labels_out_of_range_are_no_label():
    c = np.array([[[4, 4, 4]], [[5, 5, 5]]], np.int64)                             # k = 2, 1 x 3
    # "no label" costs nothing as a pixel's own label and differs from every j: it stays while that is strictly cheaper
    assert lr.energy(c, np.array([[7, -3, 2]]), 4) == (0, 0)                       # (every "no label" is the same value)
    assert lr.energy(c, np.array([[0, -3, 1]]), 4) == (9, 2)
    out, changed, en = lr.relax(c, np.array([[0, 9, 0]]), 1, 1, 4)                  # E_none = 2, E_0 = 4: it stays, raw value kept
    assert out.tolist() == [[0, 9, 0]] and changed == [0] and en == (8, 2)
    out, changed, en = lr.relax(c, np.array([[0, 9, 0]]), 2, 1, 4)                  # E_none = 4 = E_0: it never wins a tie
    assert out.tolist() == [[0, 0, 0]] and changed == [1] and en == (12, 0)
    out, changed, en = lr.relax(c, np.array([[-1, -1, -1]]), 5, 2, 4)               # E_none = 0 everywhere: a fixed point
    assert out.tolist() == [[-1, -1, -1]] and changed == [0, 0] and en == (0, 0)
    z = np.zeros((3, 4, 5), np.int64)
    out, changed, _ = lr.relax(z, np.full((4, 5), 3), 0, 1, 8)                     # k = 3: label 3 is out of range; 0 = 0 is a tie
    assert (out == 0).all() and changed == [20]
    # the energy still never rises from a map that holds them
    rng = np.random.default_rng(33)
    c = _volume(rng, 3, 7, 7, 4)
    lab = rng.integers(-2, 6, size=(7, 7))
    e = lr.total_energy(c, lab, 1, 8)
    for _ in range(4):
        lab = lr.relax(c, lab, 1, 1, 8)[0]
        assert lr.total_energy(c, lab, 1, 8) <= e
        e = lr.total_energy(c, lab, 1, 8)


def test_beta_is_clamped_and_large_costs_do_not_overflow():
    top = (1 << 62) - 1
    c = np.array([[[top, top - 1]], [[top - 3, top]]], np.int64)                   # k = 2, 1 x 2
    out, changed, (unary, pairs) = lr.relax(c, np.array([[0, 1]]), 1 << 60, 1, 8)  # beta -> 2^58 - 1
    assert out.tolist() == [[1, 1]] and (unary, pairs) == (2 * top - 3, 0)         # E_1 = top - 3 beats E_0 = top + beta
    assert lr.clamp_beta(-5) == 0 and lr.clamp_beta(1 << 60) == (1 << 58) - 1 and lr.relax(c, np.array([[0, 1]]), -7, 1, 8)[0].tolist() == [[1, 0]]


def test_beta_from_the_stats_table():
    stats = np.array([[[10, 1000], [30, 2999]], [[1, 7], [0, 0]]], np.int64)       # m = floor(3999 / 40) = 99; m = 7
    assert lr.q_of(0.25) == 64 and lr.q_of(1) == 256 and lr.q_of(1 / 512) == 1 and lr.q_of(255.998) == 65535
    assert lr.beta_of(stats, 64).tolist() == [24, 1] and lr.beta_of(stats, 256).tolist() == [99, 7]
    assert lr.beta_of(stats, 1).tolist() == [0, 0] and lr.beta_of(stats, 65535).tolist() == [(65535 * 99) >> 8, (65535 * 7) >> 8]
    for q in (1, 64, 256, 65535):
        assert relax_beta(torch.from_numpy(stats), q).tolist() == lr.beta_of(stats, q).tolist()
    big = np.array([[[1, 1536 << 32]]], np.int64)             # the largest mean a slab can give: q * m stays inside int64
    assert relax_beta(torch.from_numpy(big), 65535).tolist() == [(65535 * (1536 << 32)) >> 8]


# ---- the host logic through the stand-in ops

K, N_ITER = 5, 4


def _seg(**kw):
    kw.setdefault("k", K)
    kw.setdefault("n_iter", N_ITER)
    return Segmenter(ops=LabelRelaxOps(make_bank()), **kw)


def _t(imgs):
    return torch.from_numpy(np.ascontiguousarray(imgs))


@pytest.fixture(scope="module")
def feats():
    bank = make_bank()
    imgs = synthetic_batch(3, 24, 40, seed=11)
    tapq = bank.tapq.astype(np.int64)
    x = np.stack([so.gabor_features(im, tapq, bank.shift, bank.n_orient).reshape(bank.n_features, -1).T for im in imgs])
    return imgs, x.astype(np.int64)                           # (B, P, D)


def _want(x, h, w, mode, lam, sweeps=4, nb=8, c0=None, n_iter=N_ITER):
    """Restatement: features -> SPEC.md §4's schedule -> stats, beta, cost volume -> the sweeps."""
    b = x.shape[0]
    if c0 is None:
        c0 = np.stack([so.kmeans_init(x[i], K) for i in range(b)]) if mode == "per_image" else so.kmeans_init(x[0], K)
    labels, cent = km.schedule(x, c0, n_iter, mode)
    stats = km.evaluate_batch(x, cent)[3]
    beta = lr.beta_of(stats, lr.q_of(lam))
    beta = beta if mode == "per_image" else np.repeat(beta, b)
    out, changed, _ = lr.relax_batch(lr.cost_volume(x, cent, h, w), labels.reshape(b, h, w), beta, sweeps, nb)
    return out, changed, labels.reshape(b, h, w), beta


def test_regularize_zero_calls_neither_op_and_returns_todays_labels(feats):
    imgs, x = feats
    for mode in ("per_image", "global"):
        plain = Segmenter(ops=KMeansSeedOps(make_bank()), k=K, n_iter=N_ITER)       # ops that do not even have the launches
        off = _seg(regularize=0.0, regularize_sweeps=7, regularize_neighbours=4)
        a, b = plain.segment_device(_t(imgs), mode), off.segment_device(_t(imgs), mode)
        assert np.array_equal(a.numpy(), b.numpy())
        assert plain.ops.calls == off.ops.calls and not any(c[0] in ("costs", "relax", "evaluate") for c in off.ops.calls)
        assert np.array_equal(off.segment_batch(imgs, mode), a.numpy())
    assert off._opt.relax is None and Segmenter(ops=KMeansSeedOps(make_bank()))._opt.relax is None
    assert off.model_signature == plain.model_signature == _seg(regularize=0.5).model_signature


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_regularised_plan_is_the_restatement_behind_the_schedule(feats, mode):
    imgs, x = feats
    h, w = imgs.shape[1:3]
    seg = _seg(regularize=0.25)
    got = seg.segment_device(_t(imgs), mode).numpy()
    want, changed, raw, beta = _want(x, h, w, mode, 0.25)
    assert np.array_equal(got, want)
    assert changed[:, 0].min() > 0 and not np.array_equal(want, raw), "no label changes: the case proves nothing"
    n_sets = 3 if mode == "per_image" else 1
    tail = [c for c in seg.ops.calls if c[0] in ("evaluate", "costs", "relax")]
    assert tail == [("evaluate", 3, h, w, K, n_sets, ("stats",)), ("costs", 3, h, w, K, n_sets),
                    ("relax", 3, h, w, K, 8, 4, tuple(int(v) for v in beta))]
    assert len(set(beta.tolist())) == (3 if mode == "per_image" else 1)
    # the other settings reach the launch
    alt = _seg(regularize=1.0, regularize_sweeps=2, regularize_neighbours=4)
    assert np.array_equal(alt.segment_device(_t(imgs), mode).numpy(), _want(x, h, w, mode, 1.0, 2, 4)[0])
    # the model's entry points describe the model and ignore the option
    del seg.ops.calls[:]
    fit, own = seg.fit_device(_t(imgs), mode), seg.evaluate_device(_t(imgs), mode=mode)
    assert not any(c[0] in ("costs", "relax") for c in seg.ops.calls)
    assert np.array_equal(own["labels"].numpy(), raw)
    assert np.array_equal(seg.confidence_device(_t(imgs), mode=mode)[0].numpy(), raw)
    plain = _seg().fit_device(_t(imgs), mode)
    assert np.array_equal(fit.centroids.numpy(), plain.centroids.numpy()) and fit.signature == plain.signature
    # behind a codebook, frozen and refined
    for m in (0, 2):
        got = seg.predict_device(_t(imgs), fit, refine=m, mode=mode).numpy()
        c0 = fit.centroids.numpy().view(np.uint16).astype(np.int64)
        assert np.array_equal(got, _want(x, h, w, mode, 0.25, c0=c0 if mode == "per_image" else c0[0], n_iter=m + 1)[0])


def test_host_paths_groups_and_post_passes_see_the_relaxed_map(feats):
    imgs, x = feats
    h, w = imgs.shape[1:3]
    want = _want(x, h, w, "per_image", 0.25)[0]
    seg = _seg(regularize=0.25)
    for i in range(3):
        assert np.array_equal(seg(imgs[i]), want[i])
    for group in (1, 2):
        assert np.array_equal(seg.segment_device(_t(imgs), group=group).numpy(), want)
    assert np.array_equal(seg.segment_batch(imgs), want)
    assert seg.segment_batch(imgs, out_dtype=np.uint8).dtype == np.uint8
    assert np.array_equal(np.concatenate(list(seg.segment_stream([imgs[:2], imgs[2:]]))), want)
    assert np.array_equal(np.stack(list(seg.segment_images(list(imgs), batch=2))), want)
    conn = _seg(regularize=0.25, connectivity=True).segment_device(_t(imgs)).numpy()
    assert np.array_equal(conn, np.stack([so.connected_regions(m) for m in want]))


def test_device_entry_points(feats):
    imgs, x = feats
    h, w = imgs.shape[1:3]
    seg = _seg(regularize=0.25)                               # (both ignore the plan's option)
    for mode in ("per_image", "global"):
        want, changed, raw, beta = _want(x, h, w, mode, 0.25, sweeps=3, nb=4)
        costs, labels, stats = seg.kmeans_costs_device(_t(imgs), mode=mode)
        cent = km.schedule(x, np.stack([so.kmeans_init(x[i], K) for i in range(3)]) if mode == "per_image"
                           else so.kmeans_init(x[0], K), N_ITER, mode)[1]
        assert np.array_equal(costs.numpy(), lr.cost_volume(x, cent, h, w)) and np.array_equal(labels.numpy(), raw)
        assert np.array_equal(stats.numpy(), km.evaluate_batch(x, cent)[3])
        assert np.array_equal(costs.numpy().argmin(axis=1), raw)
        out, ch, en = seg.relax_labels_device(costs, labels, torch.from_numpy(beta), sweeps=3, neighbours=4)
        assert np.array_equal(out.numpy(), want) and np.array_equal(ch.numpy(), changed) and ch.dtype == torch.int32
        assert en.tolist() == [list(lr.energy(c, m, 4)) for c, m in zip(costs.numpy(), want)]
        assert np.array_equal(labels.numpy(), raw)            # the inputs are not changed
    model = _seg().fit_device(_t(imgs[:2]), "global")
    costs, labels, stats = seg.kmeans_costs_device(_t(imgs), model)
    c = model.centroids.numpy().view(np.uint16).astype(np.int64)
    assert np.array_equal(costs.numpy(), lr.cost_volume(x, c, h, w)) and tuple(stats.shape) == (1, K, 2)
    out, ch, en = seg.relax_labels_device(costs, labels, 7, sweeps=0)
    assert np.array_equal(out.numpy(), labels.numpy()) and tuple(ch.shape) == (3, 0)
    for bad in (dict(sweeps=-1), dict(sweeps=65), dict(sweeps=1.5), dict(neighbours=6), dict(neighbours=None)):
        with pytest.raises(ValueError, match="sweeps must be|neighbours must be"):
            seg.relax_labels_device(costs, labels, 7, **bad)
    with pytest.raises(ValueError, match="costs must be"):
        seg.relax_labels_device(costs.to(torch.int32), labels, 7)
    with pytest.raises(ValueError, match="labels must be"):
        seg.relax_labels_device(costs, labels[:2], 7)
    with pytest.raises(ValueError, match="beta must be"):
        seg.relax_labels_device(costs, labels, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="beta must be"):
        seg.relax_labels_device(costs, labels, 0.5)


def test_module_level_calls_pass_the_options_through(feats):
    import gabor_color_image_segmentation_amd.segmenter as sg
    imgs, x = feats
    kw = dict(k=K, n_iter=N_ITER, regularize=0.25, regularize_sweeps=2, regularize_neighbours=4)
    seg = _seg(regularize=0.25, regularize_sweeps=2, regularize_neighbours=4)
    saved = dict(sg._default)
    try:
        sg._default.clear()
        sg._default[tuple(sorted(kw.items()))] = seg
        want = _want(x, *imgs.shape[1:3], "per_image", 0.25, 2, 4)[0]
        assert np.array_equal(sg.segment(imgs[1], **kw), want[1])
        assert np.array_equal(sg.segment_batch(imgs, **kw), want)
        assert np.array_equal(np.stack(list(sg.segment_images(list(imgs), **kw))), want)
        assert list(sg._default) == [tuple(sorted(kw.items()))]
    finally:
        sg._default.clear()
        sg._default.update(saved)


def test_refusals(feats):
    imgs, x = feats
    t = _t(imgs)
    for bad in (-0.25, float("nan"), float("inf"), "1", None, True, 256.0, 1 / 1024):
        with pytest.raises(ValueError, match="regularize"):
            _seg(regularize=bad)
    _seg(regularize=1 / 512), _seg(regularize=255.998)        # q = 1 and q = 65535
    for bad in (0, 65, 2.5, None):
        with pytest.raises(ValueError, match="regularize_sweeps must be"):
            _seg(regularize=0.25, regularize_sweeps=bad)
    for bad in (0, 6, 16, None, "8"):
        with pytest.raises(ValueError, match="regularize_neighbours must be"):
            _seg(regularize_neighbours=bad)                   # (checked with the option off too)
    with pytest.raises(ValueError, match="ops that have kmeans_evaluate, kmeans_costs and label_relax"):
        Segmenter(ops=KMeansSeedOps(make_bank()), regularize=0.25)
    seg = _seg(regularize=0.25)
    with pytest.raises(ValueError, match="dist_group"):
        seg.segment_device(t, dist_group=object())
    import torch.distributed as td
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(td, "is_initialized", lambda: True)
        mp.setattr(td, "get_world_size", lambda group=None: 2)
        with pytest.raises(ValueError, match="more than one rank"):
            seg.segment_device(t, "global")
    strip = _t(np.zeros((1, 32, 32, 3), np.uint8))
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_rows_sharded_device(strip, 0, 32, 0, 32)
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_owned_rows_device(strip, 32)

    class EdgeOps(LabelRelaxOps):                             # (the stand-in has no edge stages: the plan rule fires first)
        texton_gradient = cue_gradient = feature_gradient = None
    edge = Segmenter(ops=EdgeOps(make_bank()), k=K, n_iter=N_ITER, regularize=0.25)
    with pytest.raises(ValueError, match="plain k-means map"):
        edge.texton_edges_device(t)
    with pytest.raises(ValueError, match="plain k-means map"):
        edge.cue_edges_device(t)
    assert seg.ops.calls == [] and edge.ops.calls == []        # refused before any launch

    class SpOps(LabelRelaxOps):
        superpixels = None
    with pytest.raises(ValueError, match="n_superpixels = 0"):
        Segmenter(ops=SpOps(make_bank()), regularize=0.25, n_superpixels=64)


def test_the_option_is_in_no_default_and_not_in_the_benchmark():
    import inspect
    sig = inspect.signature(Segmenter.__init__).parameters
    assert sig["regularize"].default == 0.0 and sig["regularize_sweeps"].default == 4 and sig["regularize_neighbours"].default == 8
    assert "regulari" not in open(os.path.join(ROOT, "bench.py")).read()
