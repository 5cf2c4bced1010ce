"""k-means++ seeding (SPEC.md §29) on the CPU: the symbol table (include/gcs_seed.h <-> ``_lib.SEED_EXTENSIONS`` <-> the built
library's exports), the argument rules of gcs_kmeans_seed (refused before anything is launched, so they run without a GPU), the
restatement (tests/kmeans_seed_ref.py) on the worked examples of the SPEC and on its own properties, and the host logic - the
plan's ``init``, ``seed_device``, restarts, refusals - through the stand-in ops (tests/kmeans_seed_ops.py). No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kmeans_model_ref as km
import kmeans_seed_ref as ks
from gabor_color_image_segmentation_amd import Segmenter, make_bank, seed_stride
from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
from kmeans_model_ops import KMeansModelOps
from kmeans_seed_ops import KMeansSeedOps
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
    hdr = open(os.path.join(ROOT, "include", "gcs_seed.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gcs_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SEED_EXTENSIONS) == {"gcs_kmeans_seed"}, declared ^ set(_lib.SEED_EXTENSIONS)
    assert 'extern "C"' in hdr and "ABI 18" in hdr and '#include "gcs.h"' in hdr
    assert "torch" not in hdr.lower() and "at::" not in hdr
    for name, (res, args) in _lib.SEED_EXTENSIONS.items():
        fn = getattr(lib, name)                               # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):                        # pointers and the stream: void pointers; the seed: 64 bits; else int
            assert (a is C.c_void_p) == ("*" in p or p.startswith("gcs_stream_t")), (name, p)
            assert (a is C.c_uint64) == p.startswith("uint64_t"), (name, p)
    others = set(_lib.SIGNATURES) | set(_lib.EXTENSIONS) | set(_lib.THIN_EXTENSIONS) | set(_lib.MATCH_EXTENSIONS) \
        | set(_lib.MODEL_EXTENSIONS)
    assert not set(_lib.SEED_EXTENSIONS) & others
    assert lib.gcs_abi_version() == 18 and _lib.ABI_VERSION == 18
    for name in ("gcs.h", "gcs_cues.h", "gcs_thin.h", "gcs_match.h", "gcs_model.h"):    # the earlier headers do not know the symbol
        assert "gcs_kmeans_seed" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_ops_refuse_a_library_without_the_symbol():
    from gabor_color_image_segmentation_amd import _lib
    from gabor_color_image_segmentation_amd.segmenter import HipOps

    class Old:                                               # what the method asks of its library, without the symbol
        pass
    ops = HipOps.__new__(HipOps)
    ops.lib = Old()
    with pytest.raises(_lib.GcsError, match="does not export gcs_kmeans_seed"):
        HipOps.kmeans_seed.__wrapped__(ops, None, 1, 8, 8, 2, 1, None, 8)


def test_seed_validates_before_launching(lib):
    """Argument errors are reported with code 1 and a message, without touching the GPU (so this runs on the CPU box)."""
    p = [C.c_void_p(q << 34) for q in range(1, 5)]           # non-NULL dummies far apart, never dereferenced
    good = dict(feats=p[0], B=3, H=19, W=23, ns=4, no=6, k=8, n_sets=3, stride=8, trials=4, seed=0, cent=p[1], picks=p[2], pot=p[3])

    def call(**bad):
        a = dict(good, **bad)
        return lib.gcs_kmeans_seed(a["feats"], a["B"], a["H"], a["W"], a["ns"], a["no"], a["k"], a["n_sets"], a["stride"],
                                   a["trials"], a["seed"], a["cent"], a["picks"], a["pot"], None)
    for bad in (dict(feats=None), dict(cent=None)):
        assert call(**bad) == 1 and b"NULL" in lib.gcs_last_error(), bad
    for bad in (dict(k=0), dict(k=-1), dict(k=17)):
        assert call(**bad) == 1 and b"k must be in 1..16" in lib.gcs_last_error(), bad
    for bad in (dict(trials=0), dict(trials=-1), dict(trials=9)):
        assert call(**bad) == 1 and b"trials must be in 1..8" in lib.gcs_last_error(), bad
    for bad in (dict(stride=0), dict(stride=-8), dict(stride=3), dict(stride=12), dict(stride=8192)):
        assert call(**bad) == 1 and b"stride must be a power of two" in lib.gcs_last_error(), bad
    for bad in (dict(n_sets=0), dict(n_sets=2), dict(n_sets=4), dict(n_sets=-1)):
        assert call(**bad) == 1 and b"n_sets" in lib.gcs_last_error(), bad
    for bad in (dict(B=0, n_sets=1), dict(B=-1, n_sets=1), dict(B=65536, n_sets=1), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097),
                dict(ns=0), dict(ns=9), dict(no=0), dict(ns=8, no=65)):       # (8 x 65 filters: 1560 features)
        assert call(**bad) == 1 and b"bad shape or bank" in lib.gcs_last_error(), bad
    # n <= 4096: 64 x 64 at stride 1 is exactly 4096 and would launch; one row more, or one image more in a single set, is refused
    for bad in (dict(B=1, n_sets=1, H=65, W=64, stride=1), dict(B=2, n_sets=1, H=64, W=64, stride=1),
                dict(B=65, n_sets=1, H=481, W=321, stride=32), dict(B=4097, n_sets=1, H=8, W=8, stride=4096)):
        assert call(**bad) == 1 and b"more than 4096 candidates" in lib.gcs_last_error(), bad
    assert b"gcs_kmeans_seed" in lib.gcs_last_error()
    # (a call inside every rule would launch, so it is made on the GPU: tests/test_gpu_kmeans_seed.py)


# ---- the restatement

def test_mix_vectors_and_the_worked_examples():
    assert ks.mix(0) == 0xE220A8397B1DCDAF and ks.mix(1) == 0x910A2DEC89025CC1
    assert ks.u(0, 0, 0) == 0xA706DD2F4D197E6F
    x = np.array([10, 20, 30, 100, 101, 12])[:, None]
    cent, picks, pot, rounds = ks.seed_trace(x, 3, seed=0, trials=2)
    assert picks.tolist() == [3, 1, 0] and cent.ravel().tolist() == [100, 20, 10] and pot == 105
    assert rounds[1] == (27145, [(12416, 1, 265), (11539, 1, 265)])          # a tie: trial 0 is taken
    assert rounds[2] == (265, [(155, 2, 165), (59, 0, 105)])
    cent, picks, pot = ks.seed_set(x, 3, seed=1, trials=2)
    assert picks.tolist() == [2, 3, 5] and pot == 69 and picks.dtype == np.int32


def test_stride_rule_and_candidates():
    assert ks.seed_stride(1, 481, 321) == seed_stride(1, 481, 321) == 8 and len(ks.candidates(481, 321, 8)) == 61 * 41 == 2501
    assert ks.seed_stride(64, 481, 321) == seed_stride(64, 481, 321) == 64 and 64 * len(ks.candidates(481, 321, 64)) == 3072
    for b, h, w in ((1, 8, 8), (1, 4096, 4096), (7, 100, 333), (4096, 40, 50), (4096, 4096, 4096), (300, 481, 321)):
        s = seed_stride(b, h, w)
        assert s == ks.seed_stride(b, h, w) and s >= 8 and s & (s - 1) == 0
        assert b * len(ks.candidates(h, w, s)) <= 4096 and (s == 8 or b * len(ks.candidates(h, w, s // 2)) > 4096)
    for rule in (seed_stride, ks.seed_stride):
        with pytest.raises(ValueError, match="4096 images"):
            rule(4097, 8, 8)
    # the last row and column of the grid are clamped into the image
    ys, xs = ks.grid(9, 21, 8)
    assert ys.tolist() == [4, 8] and xs.tolist() == [4, 12, 20]
    ys, xs = ks.grid(5, 17, 8)
    assert ys.tolist() == [4] and xs.tolist() == [4, 12, 16]
    assert ks.candidates(3, 4, 1).tolist() == list(range(12))


def _features(b, h, w, seed, bank=None):
    bank = bank or make_bank()
    imgs = synthetic_batch(b, h, w, seed=seed)
    tapq = bank.tapq.astype(np.int64)
    x = np.stack([so.gabor_features(im, tapq, bank.shift, bank.n_orient).reshape(bank.n_features, -1).T for im in imgs])
    return imgs, x.astype(np.int64)                           # (B, P, D)


@pytest.fixture(scope="module")
def feats():
    return _features(3, 24, 40, seed=11)


def test_one_trial_is_plain_d2_sampling_and_picks_have_mass(feats):
    _, x = feats
    cand = x[0]                                               # 960 candidates
    for seed in (0, 1, (1 << 63) + 5):
        cent, picks, pot, rounds = ks.seed_trace(cand, 8, seed, trials=1)
        m = km.distances(cand, cand[picks[:1]])[:, 0]
        for r in range(1, 8):                                 # D^2 sampling by hand: one draw per round on the running minimum
            rho = ks.pick(ks.u(seed, r, 0), int(m.sum()))
            q = int(np.nonzero(np.cumsum(m) > rho)[0][0])
            assert q == picks[r] and m[q] > 0
            m = np.minimum(m, km.distances(cand, cand[q:q + 1])[:, 0])
        assert pot == m.sum() and np.array_equal(cent, cand[picks])
        # greedy trials: every drawn candidate of a round with T > 0 has mass, the winner is the least potential, lowest t first
        cent4, picks4, pot4, rounds4 = ks.seed_trace(cand, 8, seed, trials=4)
        m = km.distances(cand, cand[picks4[:1]])[:, 0]
        for r in range(1, 8):
            total, tried = rounds4[r]
            assert total == m.sum() > 0 and len(tried) == 4
            assert all(m[q] > 0 and 0 <= rho < total for rho, q, _ in tried)
            pots = [p for _, _, p in tried]
            assert picks4[r] == tried[pots.index(min(pots))][1]
            m = np.minimum(m, km.distances(cand, cand[picks4[r]:picks4[r] + 1])[:, 0])
        assert pot4 == m.sum()


def test_constant_candidates_take_the_uniform_branch_and_a_single_candidate():
    x = np.full((37, 5), 1234, np.int64)
    cent, picks, pot, rounds = ks.seed_trace(x, 6, seed=3, trials=4)
    assert pot == 0 and (cent == 1234).all() and all(r == (0, None) for r in rounds[1:])
    assert picks.tolist() == [ks.pick(ks.u(3, r, 0), 37) for r in range(6)]
    assert len(set(picks.tolist())) > 1                       # (uniform draws, not one index repeated)
    cent, picks, pot = ks.seed_set(np.array([[7, 9]]), 4, seed=9)             # n = 1: every seed is the one candidate
    assert picks.tolist() == [0] * 4 and cent.tolist() == [[7, 9]] * 4 and pot == 0
    # two distinct points, k = 3: after both are seeds, T = 0 and the third is a uniform pick
    cent, picks, pot, rounds = ks.seed_trace(np.array([[0], [65535]]), 3, seed=0, trials=8)
    assert sorted(picks[:2].tolist()) == [0, 1] and rounds[1][0] == 65535 ** 2 and rounds[2] == (0, None) and pot == 0


# ---- the host logic through the stand-in ops

K, N_ITER = 5, 4


def _seg(**kw):
    kw.setdefault("k", K)
    kw.setdefault("n_iter", N_ITER)
    return Segmenter(ops=KMeansSeedOps(make_bank()), **kw)


def _t(imgs):
    return torch.from_numpy(np.ascontiguousarray(imgs))


def _cent(model):
    return model.centroids.numpy().astype(np.int64)


def _want(x, h, w, mode, seed, n_iter=N_ITER, k=K, trials=4):
    """Restatement: features -> seeds at the host's stride -> SPEC.md §4's schedule from them -> (labels (B, P), centroids)."""
    b = x.shape[0]
    n_sets = b if mode == "per_image" else 1
    c0, _, _ = ks.seed_batch(x, h, w, k, n_sets, ks.seed_stride(1 if mode == "per_image" else b, h, w), seed, trials)
    return km.schedule(x, c0 if mode == "per_image" else c0[0], n_iter, mode)


def test_spec_init_records_the_call_list_of_a_plan_without_the_option(feats):
    imgs, x = feats
    for mode in ("per_image", "global"):
        plain = Segmenter(ops=KMeansModelOps(make_bank()), k=K, n_iter=N_ITER)
        spec = _seg(init="spec", seed=77, seed_trials=2)
        a, b = plain.segment_device(_t(imgs), mode), spec.segment_device(_t(imgs), mode)
        assert np.array_equal(a.numpy(), b.numpy())
        assert plain.ops.calls == spec.ops.calls and not any(c[0] == "seed" for c in spec.ops.calls)
        assert np.array_equal(spec.segment_batch(imgs, mode), a.numpy())
    assert spec.model_signature == plain.model_signature == _seg(init="kmeans++").model_signature


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_seeded_plan_is_the_schedule_from_the_seeds(feats, mode):
    imgs, x = feats
    h, w = imgs.shape[1:3]
    seg = _seg(init="kmeans++", seed=5)
    got = seg.segment_device(_t(imgs), mode).numpy().reshape(3, -1)
    want, cents = _want(x, h, w, mode, 5)
    assert np.array_equal(got, want)
    spec = _seg().segment_device(_t(imgs), mode).numpy().reshape(3, -1)
    assert not np.array_equal(got, spec), "the seeding changes no label: the case proves nothing"
    seeds = [c for c in seg.ops.calls if c[0] == "seed"]
    assert seeds == [("seed", 3, h, w, K, 3 if mode == "per_image" else 1, 8, 4, 5)]          # one launch, the rule's stride
    # the model of the fit is that loop's; refined m times from the seeds = the schedule from the seeds
    fit = seg.fit_device(_t(imgs), mode)
    assert np.array_equal(_cent(fit), cents)
    assert np.array_equal(seg.predict_device(_t(imgs), fit, mode=mode).numpy().reshape(3, -1), want)
    seeded = seg.seed_device(_t(imgs), mode)
    n_sets = 3 if mode == "per_image" else 1
    c0, _, _ = ks.seed_batch(x, h, w, K, n_sets, 8, 5, 4)
    assert np.array_equal(_cent(seeded), c0)
    _, _, _, stats = km.evaluate_batch(x, c0)
    assert np.array_equal(seeded.counts.numpy(), stats[:, :, 0]) and np.array_equal(seeded.inertia.numpy(), stats[:, :, 1])
    for m in (0, 2):
        refined = seg.predict_device(_t(imgs), seeded, refine=m, mode=mode).numpy().reshape(3, -1)
        assert np.array_equal(refined, km.schedule(x, c0 if mode == "per_image" else c0[0], m + 1, mode)[0])
    # evaluate and confidence without a model follow the plan's init
    own = seg.evaluate_device(_t(imgs), mode=mode)
    assert np.array_equal(own["labels"].numpy().reshape(3, -1), want)
    assert np.array_equal(own["stats"].numpy(), km.evaluate_batch(x, cents)[3])
    assert np.array_equal(seg.confidence_device(_t(imgs), mode=mode)[0].numpy().reshape(3, -1), want)


def test_single_image_is_its_batch_row_whatever_the_group_size(feats):
    imgs, x = feats
    seg = _seg(init="kmeans++", seed=(1 << 63) + 5, seed_trials=2)
    whole = seg.segment_device(_t(imgs)).numpy()
    for i in range(3):
        assert np.array_equal(seg(imgs[i]), whole[i])
        assert np.array_equal(seg.segment_device(_t(imgs[i:i + 1])).numpy()[0], whole[i])
    for group in (1, 2):
        assert np.array_equal(seg.segment_device(_t(imgs), group=group).numpy(), whole)
    assert np.array_equal(seg.segment_batch(imgs), whole)
    assert np.array_equal(np.concatenate(list(seg.segment_stream([imgs[:2], imgs[2:]]))), whole)
    assert np.array_equal(np.stack(list(seg.segment_images(list(imgs), batch=2))), whole)
    # seed_device on a plan whose init is "spec": the same seeds
    a, b = seg.seed_device(_t(imgs)), _seg().seed_device(_t(imgs), seed=(1 << 63) + 5, trials=2)
    assert np.array_equal(_cent(a), _cent(b))
    assert not np.array_equal(_cent(a), _cent(seg.seed_device(_t(imgs), stride=16)))


def test_a_codebook_wins_over_the_seeding(feats):
    imgs, x = feats
    seg = _seg(init="kmeans++")
    model = _seg().fit_device(_t(imgs[:2]), "global")
    del seg.ops.calls[:]
    got = seg.predict_device(_t(imgs), model, refine=1).numpy()
    assert not any(c[0] == "seed" for c in seg.ops.calls)
    assert np.array_equal(got, _seg().predict_device(_t(imgs), model, refine=1).numpy())
    warm = seg.fit_device(_t(imgs), "global", init=model)
    assert not any(c[0] == "seed" for c in seg.ops.calls)
    assert np.array_equal(_cent(warm), km.schedule(x, _cent(model)[0], N_ITER, "global")[1])


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_restarts_keep_the_least_inertia_per_set(feats, mode):
    imgs, x = feats
    h, w = imgs.shape[1:3]
    seg = _seg(init="kmeans++", seed=2, n_iter=2)
    model = seg.fit_device(_t(imgs), mode, n_init=3)
    runs = [_want(x, h, w, mode, 2 + i, n_iter=2)[1] for i in range(3)]       # centroids (n_sets, k, D) of every restart
    tables = [km.evaluate_batch(x, c)[3] for c in runs]
    keep = ks.best_restart([t[:, :, 1].sum(axis=1) for t in tables])
    for s, i in enumerate(keep):
        assert np.array_equal(_cent(model)[s], runs[i][s])
        assert np.array_equal(model.inertia.numpy()[s], tables[i][s, :, 1]) and np.array_equal(model.counts.numpy()[s], tables[i][s, :, 0])
    if mode == "per_image":
        assert len(set(keep.tolist())) > 1, "every image keeps the same restart: the per-set choice is not exercised"
    assert [c[-1] for c in seg.ops.calls if c[0] == "seed"] == [2, 3, 4]
    # the seed wraps at 2^64; n_init = 1 is the plain fit
    assert np.array_equal(_cent(seg.fit_device(_t(imgs), mode, n_init=1)), runs[0])
    edge = _seg(init="kmeans++", seed=(1 << 64) - 1, n_iter=2)
    edge.fit_device(_t(imgs[:1]), mode, n_init=2)
    assert [c[-1] for c in edge.ops.calls if c[0] == "seed"] == [(1 << 64) - 1, 0]


def test_restart_ties_go_to_the_lowest_restart():
    assert ks.best_restart([[5, 3], [5, 2], [4, 2]]).tolist() == [2, 1]
    # on a constant image every restart ends on the same inertia: restart 0 is kept
    imgs = np.full((2, 16, 16, 3), 90, np.uint8)
    seg = _seg(init="kmeans++", seed=0, n_iter=2, k=3)
    many, one = seg.fit_device(_t(imgs), "per_image", n_init=3), seg.fit_device(_t(imgs), "per_image")
    assert np.array_equal(_cent(many), _cent(one)) and np.array_equal(many.inertia.numpy(), one.inertia.numpy())


def test_module_level_calls_pass_the_options_through(feats):
    import gabor_color_image_segmentation_amd.segmenter as sg
    imgs, x = feats
    kw = dict(k=K, n_iter=N_ITER, init="kmeans++", seed=5)
    seg = _seg(init="kmeans++", seed=5)
    saved = dict(sg._default)
    try:
        sg._default.clear()
        sg._default[tuple(sorted(kw.items()))] = seg
        want = seg.segment_device(_t(imgs)).numpy()
        assert np.array_equal(sg.segment(imgs[1], **kw), want[1])
        fit = sg.fit_codebook(imgs, "per_image", n_init=2, **kw)
        assert np.array_equal(_cent(fit), _cent(seg.fit_device(_t(imgs), "per_image", n_init=2)))
        assert list(sg._default) == [tuple(sorted(kw.items()))]
    finally:
        sg._default.clear()
        sg._default.update(saved)


def test_refusals(feats):
    imgs, x = feats
    t = _t(imgs)
    for bad in ("random", "k-means++", None, 1):
        with pytest.raises(ValueError, match="init must be"):
            _seg(init=bad)
    for bad in (-1, 1 << 64, 0.5, "3", None, True):
        with pytest.raises(ValueError, match="seed must be"):
            _seg(seed=bad)
    for bad in (0, 9, 2.5, None):
        with pytest.raises(ValueError, match="seed_trials must be"):
            _seg(seed_trials=bad)
    with pytest.raises(ValueError, match="ops that have kmeans_seed"):
        Segmenter(ops=KMeansModelOps(make_bank()), init="kmeans++")
    Segmenter(ops=KMeansModelOps(make_bank()), init="spec")                 # (the default needs no such ops)
    seg = _seg(init="kmeans++")
    with pytest.raises(ValueError, match="dist_group"):
        seg.segment_device(t, dist_group=object())
    import torch.distributed as td
    with pytest.MonkeyPatch.context() as mp:                  # a world of two ranks: every rank would draw from its own slab
        mp.setattr(td, "is_initialized", lambda: True)
        mp.setattr(td, "get_world_size", lambda group=None: 2)
        with pytest.raises(ValueError, match="more than one rank"):
            seg.segment_device(t, "global")
    strip = _t(np.zeros((1, 32, 32, 3), np.uint8))
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_rows_sharded_device(strip, 0, 32, 0, 32)
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_owned_rows_device(strip, 32)
    many = torch.zeros((4097, 8, 8, 3), dtype=torch.uint8)
    del seg.ops.calls[:]
    with pytest.raises(ValueError, match="4096 images"):
        seg.segment_device(many, "global")
    with pytest.raises(ValueError, match="4096 images"):
        seg.seed_device(many, "global")
    assert seg.ops.calls == []                                # refused before any launch
    for n_init in (0, -1, 1.5, None):
        with pytest.raises(ValueError, match="n_init must be"):
            seg.fit_device(t, n_init=n_init)
    with pytest.raises(ValueError, match="n_init > 1"):
        _seg().fit_device(t, n_init=2)                         # a plan with the init of SPEC.md §4
    with pytest.raises(ValueError, match="n_init > 1"):
        seg.fit_device(t, init=seg.fit_device(t), n_init=2)
    for bad in (3, 0, 8192, 2.5):
        with pytest.raises(ValueError, match="stride must be"):
            seg.seed_device(t, stride=bad)
    with pytest.raises(ValueError, match="ops that have kmeans_seed"):
        Segmenter(ops=KMeansModelOps(make_bank())).seed_device(t)


def test_superpixel_plans_refuse_the_seeding():
    from gabor_color_image_segmentation_amd import segmenter as sg

    class SpOps(KMeansSeedOps):                               # (the stand-in has no superpixel stage: the rule fires first)
        superpixels = None
    with pytest.raises(ValueError, match="n_superpixels = 0"):
        Segmenter(ops=SpOps(make_bank()), init="kmeans++", n_superpixels=64)
    assert sg._check_seeding("spec", 0, 4) is None and sg._check_seeding("kmeans++", 7, 2) == (7, 2)
