"""Thin boundary maps (SPEC.md §26) on the CPU: the section's worked examples, the step table against double-precision
trigonometry for every n, gcs_thin_steps against the restatement, the contract the frozen symbol tables cannot carry
(include/gcs_thin.h <-> ``_lib.THIN_EXTENSIONS`` <-> the built library's exports; gcs.h, gcs_cues.h, ``SIGNATURES`` and
``EXTENSIONS`` do not know the symbols), the argument rules of gcs_edge_thin (refused before anything is launched, so they run
without a GPU), the host calls and their ValueErrors through the stand-in ops (tests/edge_thin_ops.py), the one-to-one matching
score (``evaluate.match_scores``) against a brute force and on crafted maps, and the per-image figures of
tools/edge_thin_quality.py. No GPU."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import cue_gradient_ref as cg
import edge_thin_ref as et
import texton_gradient_ref as tg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
QUALITY = os.path.join(ROOT, "profiles", "edge_thin_quality.json")


# ---- the definition

def _row(values, n=1, dirs=None):
    e = np.array([values], np.int32)
    d = np.zeros(e.shape, np.uint8) if dirs is None else np.array([dirs], np.uint8)
    slow, fast = et.thin(e, d, n), et.thin_fast(e, d, n)
    assert slow.dtype == np.int32 and np.array_equal(slow, fast)
    return slow[0].tolist()


def test_worked_examples():
    """SPEC.md §26: the three rows (n = 1, dir = 0: the neighbours are left and right) and the 3 x 3 diagonal example."""
    assert et.steps(1).tolist() == [[0, 1, 0, 1, 1024, 0, 0, 0]]
    assert _row([0, 10, 11, 30]) == [0, 0, 0, 30]            # the last pixel's plus neighbour is itself
    assert _row([3, 5, 5, 3]) == [0, 5, 0, 0]                # one pixel of a two-pixel plateau survives
    assert _row([5, 5, 3]) == [0, 0, 0]                      # a plateau on the left border loses to the clamp
    assert _row([-4, 0, 7, -1]) == [0, 0, 7, 0]              # negatives count as 0
    assert _row([1, 2, 3], dirs=[0, 1, 0]) == [0, 0, 3]      # dir >= n gives 0
    # direction 1 of 8: (a, b) = (946, 392): q1 = (0, 1) with w1 = 554, q2 = (1, 1) with w2 = 392, m = 946
    assert et.normal(1, 8) == (946, 392) and et.steps(8)[1].tolist() == [0, 1, 1, 1, 554, 392, 0, 0]
    e = np.array([[9, 0, 0], [20, 30, 10], [0, 0, 40]], np.int32)
    d = np.full((3, 3), 1, np.uint8)
    # centre: plus = 554 * 10 + 392 * 40 = 21220, minus = 554 * 20 + 392 * 9 = 14608, m V = 946 * 30 = 28380: kept
    assert 946 * 30 > 554 * 20 + 392 * 9 and 946 * 30 >= 554 * 10 + 392 * 40
    # (1, 0): plus = 554 * 30 + 392 * 0 = 16620 < 946 * 20 = 18920, minus = 554 * 20 + 392 * 9 = 14608 (the left neighbour is
    # the pixel itself, the upper left one is clamped to (0, 0)): kept. (1, 2): minus = 554 * 30 + 392 * 0 > 946 * 10: dropped.
    # (2, 2): every plus neighbour is the pixel itself, minus = 554 * 0 + 392 * 30: kept. (0, 0): plus = 392 * 30 > 946 * 9.
    want = [[0, 0, 0], [20, 30, 0], [0, 0, 40]]
    assert et.thin(e, d, 8).tolist() == want and et.thin_fast(e, d, 8).tolist() == want
    d[1, 1] = 5                                               # (a, b) = (-392, 946): q1 = (1, 0), q2 = (1, -1): 554 * 0 + 392 * 0
    assert et.steps(8)[5].tolist() == [1, 0, 1, -1, 554, 392, 0, 0] and et.thin(e, d, 8)[1, 1] == 30
    e[0, 1] = 60                                              # its minus side: 554 * 60 > 946 * 30
    assert et.thin(e, d, 8)[1, 1] == 0


@pytest.mark.parametrize("n", range(1, 17))
def test_the_whole_array_form_of_the_restatement_is_the_pixel_loop(n):
    """``thin_fast`` (what the tools and the large GPU shapes use) == ``thin`` on maps full of ties, on the int32 range, with
    directions out of range, under §26's table and under any table (offsets outside -1 .. 1 are clamped, w1 + w2 up to 2048)."""
    rng = np.random.default_rng(n)
    shape = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (17, 23), (11, 6), (5, 31)][n % 8]
    d = rng.integers(0, n + 2, size=shape).astype(np.uint8)
    d[rng.random(shape) < 0.05] = 255
    any_table = np.zeros((n, 8), np.int64)
    any_table[:, :4] = rng.integers(-3, 4, size=(n, 4))
    any_table[:, 4] = rng.integers(0, 2049, size=n)
    any_table[:, 5] = np.where(any_table[:, 4] == 0, 1, rng.integers(0, 2049, size=n) % (2049 - any_table[:, 4]))
    assert ((any_table[:, 4] + any_table[:, 5] >= 1) & (any_table[:, 4] + any_table[:, 5] <= 2048)).all()
    info = np.iinfo(np.int32)
    for e in (rng.integers(-3, 4, size=shape), rng.choice([0, 7, 9], size=shape),
              rng.choice([info.min, info.max, info.max - 1, 1 << 30], size=shape)):
        for table in (None, any_table.astype(np.int32)):
            assert np.array_equal(et.thin(e.astype(np.int32), d, n, table), et.thin_fast(e.astype(np.int32), d, n, table))


@pytest.mark.parametrize("n", range(1, 17))
def test_step_table_against_double_trigonometry(n):
    """The normal of direction i crosses the ring of the eight neighbours at (sign cos, tan) or (cot, sign sin): between the
    axis neighbour q1 and the diagonal neighbour q2, at the fraction min(|cos|, |sin|) / max(|cos|, |sin|) from q1. The integer
    weights carry that fraction to within the rounding of a and b: each is off by at most 1/2 in 1024, the larger is at least
    1024 / sqrt(2) - 1/2, so the quotient is off by less than 2 * 0.5 / 723.5 < 1.4e-3."""
    table = et.steps(n)
    assert table.dtype == np.int32 and table.shape == (n, 8) and not table[:, 6:].any()
    for i in range(n):
        c, s = math.cos(math.pi * i / n), math.sin(math.pi * i / n)
        sign = lambda v: 0 if abs(v) < 1e-9 else (1 if v > 0 else -1)
        dy1, dx1, dy2, dx2, w1, w2 = (int(v) for v in table[i, :6])
        assert (dy2, dx2) == (sign(s), sign(c))               # the diagonal neighbour of the normal's quadrant (an axis one at 0, 90)
        # |cos| = |sin| only at 45 and 135 degrees, where a and b round alike and w1 = 0: either axis neighbour is exact
        assert (dy1, dx1) == ((0, sign(c)) if abs(c) >= abs(s) else (sign(s), 0)) or w1 == 0
        m = w1 + w2
        assert w1 >= 0 and w2 >= 0 and 724 <= m <= 1024
        assert abs(w2 / m - min(abs(c), abs(s)) / max(abs(c), abs(s))) < 1.4e-3, (n, i)
        assert m == max(abs(v) for v in et.normal(i, n)) and et.normal(i, n) == tg.direction(i, n)


# ---- the library: symbols and argument rules

@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("n", range(1, 17))
def test_gcs_thin_steps_is_the_restatements_table(lib, n):
    got = np.full((n + 1, 8), -77, np.int32)
    assert lib.gcs_thin_steps(n, got.ctypes.data) == 0
    assert np.array_equal(got[:n], et.steps(n)) and (got[n] == -77).all()


def test_gcs_thin_steps_refuses_bad_arguments(lib):
    room = np.zeros((16, 8), np.int32)
    for n in (0, -1, 17):
        assert lib.gcs_thin_steps(n, room.ctypes.data) == 1 and b"gcs_thin_steps" in lib.gcs_last_error()
    assert lib.gcs_thin_steps(8, None) == 1 and b"NULL" in lib.gcs_last_error()
    assert not room.any()


def test_header_table_and_exports_agree(lib):
    from gabor_color_image_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gcs_thin.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gcs_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.THIN_EXTENSIONS) == {"gcs_thin_steps", "gcs_edge_thin"}, declared ^ set(_lib.THIN_EXTENSIONS)
    assert 'extern "C"' in hdr and "ABI 18" in hdr and '#include "gcs.h"' in hdr
    assert "torch" not in hdr.lower() and "at::" not in hdr
    for name, (res, args) in _lib.THIN_EXTENSIONS.items():
        fn = getattr(lib, name)                               # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):                        # pointers and the stream are void pointers, the rest ints
            assert (a is C.c_void_p) == ("*" in p or p.startswith("gcs_stream_t")), (name, p)
    assert not set(_lib.THIN_EXTENSIONS) & (set(_lib.SIGNATURES) | set(_lib.EXTENSIONS))
    assert lib.gcs_abi_version() == 18 and _lib.ABI_VERSION == 18


def test_the_frozen_headers_and_tables_do_not_know_the_symbols():
    from gabor_color_image_segmentation_amd import _lib
    for name in ("gcs.h", "gcs_cues.h"):
        hdr = open(os.path.join(ROOT, "include", name)).read()
        assert "gcs_thin" not in hdr and "edge_thin" not in hdr, name
    assert not [k for k in list(_lib.SIGNATURES) + list(_lib.EXTENSIONS) if "thin" in k]
    assert set(_lib.EXTENSIONS) == {"gcs_cue_gradient"}


def test_a_library_without_the_symbols_still_loads_and_the_ops_refuse(built):
    from gabor_color_image_segmentation_amd import _lib
    from gabor_color_image_segmentation_amd.segmenter import HipOps
    saved, held = dict(_lib.THIN_EXTENSIONS), _lib._lib
    try:
        _lib.THIN_EXTENSIONS["gcs_not_in_this_library"] = (C.c_int, [])
        _lib._lib = None
        lib = _lib.load()
        assert not hasattr(lib, "gcs_not_in_this_library") and hasattr(lib, "gcs_edge_thin") and hasattr(lib, "gcs_thin_steps")
    finally:
        _lib.THIN_EXTENSIONS.clear()
        _lib.THIN_EXTENSIONS.update(saved)
        _lib._lib = held

    class Old:                                               # what the methods ask of their library, without the symbols
        pass
    ops = HipOps.__new__(HipOps)
    ops.lib = Old()
    with pytest.raises(ValueError, match="need ops that have them"):
        HipOps.edge_thin.__wrapped__(ops, None, None, 1, 8, 8, 8, None)
    with pytest.raises(ValueError, match="need ops that have them"):
        ops.thin_steps(8)


def test_edge_thin_validates_before_launching(lib):
    """Argument errors are reported without touching the GPU (so this runs on the CPU box)."""
    p = [C.c_void_p(q << 34) for q in range(1, 6)]           # non-NULL dummies far apart, never dereferenced
    good = dict(edges=p[0], dirs=p[1], B=2, H=19, W=23, n=8, steps=p[2], out=p[3])

    def call(**bad):
        a = dict(good, **bad)
        return lib.gcs_edge_thin(a["edges"], a["dirs"], a["B"], a["H"], a["W"], a["n"], a["steps"], a["out"], None)
    for bad in (dict(edges=None), dict(dirs=None), dict(steps=None), dict(out=None)):
        assert call(**bad) == 1 and b"NULL" in lib.gcs_last_error(), bad
    for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097)):
        assert call(**bad) == 1 and b"shape" in lib.gcs_last_error(), bad
    for bad in (dict(n=0), dict(n=-3), dict(n=17)):
        assert call(**bad) == 1 and b"argument" in lib.gcs_last_error(), bad
    px = 2 * 19 * 23
    at = lambda q, off: C.c_void_p(q.value + off)
    for bad in (dict(out=p[0]), dict(out=at(p[0], 4 * px - 1)), dict(out=at(p[0], -4 * px + 1)), dict(out=p[1]),
                dict(out=at(p[1], px - 1)), dict(out=at(p[1], -4 * px + 1)), dict(out=p[2]), dict(out=at(p[2], 8 * 32 - 1)),
                dict(out=at(p[2], -4 * px + 1))):
        assert call(**bad) == 1 and b"overlaps" in lib.gcs_last_error(), bad
    assert b"gcs_edge_thin" in lib.gcs_last_error()
    # (ranges that only touch do not overlap; such a call would launch, so it is made on the GPU: tests/test_gpu_edge_thin.py)


# ---- the host calls, through the stand-in

PLAN = dict(n_scales=4, n_orient=2, k=4, n_iter=3)


@pytest.fixture(scope="module")
def standin(built):
    from gabor_color_image_segmentation_amd import make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from edge_thin_ops import EdgeThinOps
    import feature_gradient_ref as fg
    import position_ref as pr
    img = synthetic_batch(1, 24, 40, seed=11)[0]
    ops = EdgeThinOps(make_bank(n_scales=4, n_orient=2))
    grad = fg.gradient(pr.features(img, 0.0, 0, 0, 4, 2), 4, 2)
    labels = pr.segment(img, k=4, n_iter=3, n_scales=4, n_orient=2)
    return img, ops, grad, labels


def test_thin_edges_device_takes_any_map(standin):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    ops = standin[1]
    seg = Segmenter(ops=ops, **PLAN)
    rng = np.random.default_rng(4)
    e = rng.integers(-5, 50, size=(2, 7, 13)).astype(np.int32)
    d = rng.integers(0, 7, size=(2, 7, 13)).astype(np.uint8)
    for n in (8, 5, 16):
        got = seg.thin_edges_device(torch.from_numpy(e), torch.from_numpy(d), n_directions=n)
        assert ops.calls[-1] == ("thin", 2, 7, 13, n, False) and got.dtype == torch.int32
        for i in range(2):
            assert np.array_equal(got[i].numpy(), et.thin(e[i], d[i], n))
    assert np.array_equal(seg.thin_edges_device(torch.from_numpy(e), torch.from_numpy(d)).numpy(),
                          seg.thin_edges_device(torch.from_numpy(e), torch.from_numpy(d), n_directions=8).numpy())


def test_chains_thin_behind_the_gradient_and_leave_the_default_alone(standin):
    import torch
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter
    img, ops, grad, labels = standin
    seg = Segmenter(ops=ops, **PLAN)
    dev = torch.from_numpy(img[None])
    lab = torch.from_numpy(labels[None].astype(np.int32))
    # cue chain
    del ops.calls[:]
    thick = seg.cue_edges_device(dev, radius=3, n_directions=6, bins=8)
    plain = list(ops.calls)
    assert "thin" not in [c[0] for c in plain] and plain[-1][0] == "cue" and plain[-1][-1] is False
    del ops.calls[:]
    same = seg.cue_edges_device(dev, radius=3, n_directions=6, bins=8, thin=False)
    assert list(ops.calls) == plain and torch.equal(same, thick)
    del ops.calls[:]
    thin = seg.cue_edges_device(dev, radius=3, n_directions=6, bins=8, thin=True)
    assert ops.calls[:len(plain) - 1] == plain[:-1] and ops.calls[len(plain) - 1] == plain[-1][:-1] + (True,)
    assert [c[0] for c in ops.calls[len(plain):]] in (["thin"], ["steps", "thin"]) and ops.calls[-1] == ("thin", 1, 24, 40, 6, False)
    pb, d = cg.cue_gradient(labels, img, 4, 8, (2, 2, 1, 1), 3, 6)
    want = et.thin(tg.joined(pb, np.maximum(grad, 0)), d, 6)
    assert np.array_equal(thin[0].numpy(), want) and 0 < np.count_nonzero(want) < np.count_nonzero(thick[0].numpy())
    assert np.array_equal(thick[0].numpy()[want > 0], want[want > 0])
    # texton chain
    del ops.calls[:]
    t_thick = seg.texton_edges_device(dev, radius=3, n_directions=6)
    plain = list(ops.calls)
    del ops.calls[:]
    t_thin = seg.texton_edges_device(dev, radius=3, n_directions=6, thin=True)
    assert ops.calls[:len(plain) - 1] == plain[:-1] and ops.calls[len(plain) - 1] == plain[-1][:-1] + (True,)
    assert ops.calls[-1] == ("thin", 1, 24, 40, 6, False)
    t, d = tg.texton_gradient(labels, 4, 3, 6)
    assert np.array_equal(t_thin[0].numpy(), et.thin(tg.joined(t, np.maximum(grad, 0)), d, 6))
    assert np.array_equal(t_thick[0].numpy(), tg.joined(t, np.maximum(grad, 0)))
    # the label-map entry points: thin with and without the direction map
    out, dirs = seg.cue_gradient_device(lab, dev, radius=3, n_directions=6, bins=8, directions=True, thin=True)
    assert np.array_equal(out[0].numpy(), et.thin(pb, d * 0 + cg.cue_gradient(labels, img, 4, 8, (2, 2, 1, 1), 3, 6)[1], 6))
    assert np.array_equal(dirs[0].numpy(), cg.cue_gradient(labels, img, 4, 8, (2, 2, 1, 1), 3, 6)[1])
    alone = seg.texton_gradient_device(lab, radius=3, n_directions=6, thin=True)
    assert np.array_equal(alone[0].numpy(), et.thin(t, d, 6)) and ops.calls[-1][0] == "thin"
    del ops.calls[:]
    seg.texton_gradient_device(lab, radius=3, n_directions=6)
    assert [c[0] for c in ops.calls if c[0] != "masks"] == ["texton"] and ops.calls[-1][-1] is False
    # the one-shot calls
    got = pkg.segment_cue_edges(img, radius=3, n_directions=6, bins=8, thin=True, ops=ops, **PLAN)
    assert got.dtype == np.float32 and np.array_equal(got, tg.normalised(want)) and got.max() == 1.0
    got = pkg.segment_texton_edges(img, radius=3, n_directions=6, thin=True, ops=ops, **PLAN)
    assert np.array_equal(got, tg.normalised(t_thin[0].numpy()))
    assert np.array_equal(pkg.segment_cue_edges(img, radius=3, n_directions=6, bins=8, ops=ops, **PLAN), tg.normalised(thick[0].numpy()))
    flat = pkg.segment_cue_edges(np.full((16, 16, 3), 77, np.uint8), thin=True, ops=ops, **PLAN)
    assert flat.dtype == np.float32 and flat.shape == (16, 16) and not flat.any()


def test_every_host_value_error_comes_before_any_launch(standin):
    import inspect
    import torch
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    from gabor_color_image_segmentation_amd.segmenter import HipOps
    from cue_gradient_ops import CueGradientOps
    img, ops, _, labels = standin
    dev = torch.from_numpy(img[None])
    lab = torch.from_numpy(labels[None].astype(np.int32))
    seg = Segmenter(ops=ops, **PLAN)
    e = torch.zeros((2, 7, 13), dtype=torch.int32)
    d = torch.zeros((2, 7, 13), dtype=torch.uint8)
    n_calls = len(ops.calls)
    for a, b in ((e.to(torch.int64), d), (e[0], d[0]), (e, d.to(torch.int32)), (e, d[:, :6]), (e, d[0]), (None, d), (e, None),
                 (e.numpy(), d.numpy())):
        with pytest.raises(ValueError):
            seg.thin_edges_device(a, b)
    for n in (0, 17, 2.5, "8", None):
        with pytest.raises(ValueError):
            seg.thin_edges_device(e, d, n_directions=n)
    for kw in (dict(n_directions=0), dict(n_directions=17), dict(radius=0), dict(radius=16)):
        for call in (lambda: seg.cue_edges_device(dev, thin=True, **kw), lambda: seg.texton_edges_device(dev, thin=True, **kw),
                     lambda: seg.cue_gradient_device(lab, dev, thin=True, **kw), lambda: seg.texton_gradient_device(lab, thin=True, **kw),
                     lambda: pkg.segment_cue_edges(img, thin=True, ops=ops, **PLAN, **kw),
                     lambda: pkg.segment_texton_edges(img, thin=True, ops=ops, **PLAN, **kw)):
            with pytest.raises(ValueError):
                call()
    assert len(ops.calls) == n_calls                         # refused before any stage
    # ops without the thin launch: refused before any stage too, and only when thinning is asked for
    old_ops = CueGradientOps(make_bank(n_scales=4, n_orient=2))
    old = Segmenter(ops=old_ops, **PLAN)
    for call in (lambda: old.cue_edges_device(dev, thin=True), lambda: old.texton_edges_device(dev, thin=True),
                 lambda: old.cue_gradient_device(lab, dev, thin=True), lambda: old.texton_gradient_device(lab, thin=True),
                 lambda: old.thin_edges_device(e, d)):
        with pytest.raises(ValueError, match="ops that have them"):
            call()
    assert not old_ops.calls
    assert old.cue_edges_device(dev, radius=3, n_directions=6).max() > 0
    # §22's map has no direction map: no ``thin``
    assert "thin" not in inspect.signature(Segmenter.edges_device).parameters
    with pytest.raises(TypeError):
        seg.edges_device(dev, thin=True)
    for fn in (Segmenter.cue_edges_device, Segmenter.texton_edges_device, Segmenter.cue_gradient_device,
               Segmenter.texton_gradient_device, pkg.segment_cue_edges, pkg.segment_texton_edges):
        assert inspect.signature(fn).parameters["thin"].default is False
    # HipOps.edge_thin checks its tensors before the library is called
    class Never:
        def gcs_edge_thin(self, *a):
            raise AssertionError("launched")
        gcs_thin_steps = gcs_edge_thin
    raw = HipOps.__new__(HipOps)
    raw.lib, raw.torch, raw._thin_steps = Never(), torch, {}
    steps = torch.zeros((8, 8), dtype=torch.int32)
    good = dict(edges=e, dirs=d, b=2, h=7, w=13, n=8, out=torch.zeros_like(e), steps=steps)
    for kw in (dict(edges=None), dict(dirs=None), dict(out=None), dict(edges=e.to(torch.int64)), dict(dirs=d.to(torch.int8)),
               dict(out=e[:, :6]), dict(edges=e.transpose(1, 2)), dict(b=3), dict(steps=steps[:7]), dict(steps=steps.to(torch.int64)),
               dict(n=7)):
        with pytest.raises(ValueError):
            HipOps.edge_thin.__wrapped__(raw, **dict(good, **kw))
    for n in (0, 17):
        with pytest.raises(ValueError):
            raw.thin_steps(n)


# ---- the matching score

def _brute(p_mask, q_mask, d2):
    """The maximum matching by scipy.optimize.linear_sum_assignment on the 0 / 1 pair matrix (maximise the allowed pairs used)."""
    from scipy.optimize import linear_sum_assignment
    p, q = np.argwhere(p_mask), np.argwhere(q_mask)
    if len(p) == 0 or len(q) == 0:
        return 0
    allowed = (((p[:, None, :] - q[None, :, :]) ** 2).sum(axis=2) <= d2).astype(np.int64)
    r, c = linear_sum_assignment(allowed, maximize=True)
    return int(allowed[r, c].sum())


def test_thin_boundaries_owns_each_pair_once():
    from gabor_color_image_segmentation_amd.evaluate import thin_boundaries
    s = np.array([[0, 0, 1], [0, 2, 1], [3, 3, 3]])
    want = [[False, True, False], [True, True, True], [False, False, False]]
    assert thin_boundaries(s).tolist() == want and thin_boundaries(s).dtype == bool
    assert not thin_boundaries(np.zeros((4, 5), int)).any() and thin_boundaries(np.zeros((1, 1), int)).shape == (1, 1)
    rng = np.random.default_rng(1)
    s = rng.integers(0, 3, size=(9, 11))
    for y in range(9):
        for x in range(11):
            here = (x + 1 < 11 and s[y, x] != s[y, x + 1]) or (y + 1 < 9 and s[y, x] != s[y + 1, x])
            assert thin_boundaries(s)[y, x] == here


@pytest.mark.parametrize("seed", range(12))
def test_match_scores_equals_a_brute_force(seed):
    from gabor_color_image_segmentation_amd.evaluate import match_count, match_scores, thin_boundaries
    rng = np.random.default_rng(seed)
    h, w = [(7, 9), (5, 5), (1, 9), (7, 1), (3, 8), (6, 7)][seed % 6]
    edges = rng.integers(0, 4, size=(h, w)).astype(np.int32)
    truth = [rng.integers(0, 2 + seed % 3, size=(h, w)) for _ in range(3)]
    for t in truth:
        t[0, 0], t[-1, -1] = 0, 1                             # (every annotator has a boundary somewhere ...)
        if not thin_boundaries(t).any():
            t.flat[:: 2] = 5
    th = [-1, 0, 1, 2, 3]
    for d2 in (0, 1, 2, 4, 5, 18):
        got = match_scores(edges, truth, th, max_dist2=d2)
        for j, theta in enumerate(th):
            p = edges > theta
            ms = [_brute(p, thin_boundaries(t), d2) for t in truth]
            for t, m in zip(truth, ms):
                assert match_count(p, thin_boundaries(t), d2) == m <= min(p.sum(), thin_boundaries(t).sum())
            if not p.any():
                assert (got["recall"][j], got["precision"][j], got["fmeasure"][j]) == (0.0, 0.0, 0.0)      # the zero rule
                continue
            rec = sum(m / thin_boundaries(t).sum() for t, m in zip(truth, ms)) / 3
            prec = sum(m / p.sum() for m in ms) / 3
            assert got["recall"][j] == rec and got["precision"][j] == prec
            assert got["fmeasure"][j] == (0.0 if rec + prec == 0 else 2.0 * prec * rec / (rec + prec))
    # on shapes this small the default distance is 0: only a pixel on the truth matches
    assert np.array_equal(match_scores(edges, truth, th)["fmeasure"], match_scores(edges, truth, th, max_dist2=0)["fmeasure"])


def test_match_scores_on_crafted_maps():
    from gabor_color_image_segmentation_amd.evaluate import edge_scores, match_distance2, match_scores, thin_boundaries
    assert match_distance2(321, 481) == 18 and match_distance2(481, 321) == 18 and match_distance2(100, 100) == 1
    assert match_distance2(94, 94) == 0 and match_distance2(95, 94) == 1 and match_distance2(4096, 4096) == 1887
    h, w = 100, 120                                           # D2 = 9 * 24400 // 160000 = 1: one pixel, no diagonal
    assert match_distance2(h, w) == 1
    y, x = np.mgrid[0:h, 0:w]
    s1 = (x >= 60).astype(np.int32)                           # a straight line
    s2 = ((y >= 40) + 2 * (x + y >= 110)).astype(np.int32)    # a line and a staircase
    truth = [s1, s2]
    both = [thin_boundaries(s) for s in truth]
    assert both[0].sum() == h and (both[0][:, 59]).all()
    for t, s in zip(both, truth):                             # a map equal to the thin truth: 1 / 1 against that annotator
        sc = match_scores(t.astype(np.int32), [s], [0])
        assert (sc["recall"][0], sc["precision"][0], sc["fmeasure"][0]) == (1.0, 1.0, 1.0)
        inner = np.zeros_like(t)                              # the truth without the image's frame, moved by one pixel each way:
        inner[1:-1, 1:-1] = t[1:-1, 1:-1]                     # nothing wraps, every pixel has its partner one step away
        for shift in ((0, 1), (1, 0), (0, -1), (-1, 0)):
            moved = np.roll(inner, shift, axis=(0, 1))
            sc = match_scores(moved.astype(np.int32), [s], [0])
            assert sc["precision"][0] == 1.0 and sc["recall"][0] == inner.sum() / t.sum(), shift
    moved = np.roll(both[0], 1, axis=1)                       # the straight line one column on: 1 / 1
    sc = match_scores(moved.astype(np.int32), [s1], [0])
    assert (sc["recall"][0], sc["precision"][0], sc["fmeasure"][0]) == (1.0, 1.0, 1.0)
    far = np.roll(both[0], 2, axis=1)                         # two columns on: out of reach
    sc = match_scores(far.astype(np.int32), [s1], [0])
    assert (sc["recall"][0], sc["precision"][0], sc["fmeasure"][0]) == (0.0, 0.0, 0.0)
    ribbon = np.zeros((h, w), np.int32)                       # three columns over the one-pixel line: precision 1/3, recall 1
    ribbon[:, 58:61] = 9
    sc = match_scores(ribbon, [s1], [0, 8, 9])
    assert sc["recall"].tolist() == [1.0, 1.0, 0.0] and sc["precision"].tolist() == [1 / 3, 1 / 3, 0.0]
    assert sc["fmeasure"].tolist() == [0.5, 0.5, 0.0]         # the zero rule at 9
    thick = edge_scores(ribbon, [s1], [0])                    # the metric of §22 does not charge the ribbon for its width
    assert thick["precision"][0] == 1.0
    two = match_scores(ribbon, truth, [0])                    # annotator means
    alone = [match_scores(ribbon, [s], [0]) for s in truth]
    for key in ("recall", "precision"):
        assert two[key][0] == (alone[0][key][0] + alone[1][key][0]) / 2
    assert set(two) == {"recall", "precision", "fmeasure"} and all(v.dtype == np.float64 and v.shape == (1,) for v in two.values())
    with pytest.raises(ZeroDivisionError):
        match_scores(ribbon, [np.zeros((h, w), np.int32)], [0])      # an annotator without a boundary
    assert match_scores(ribbon, [np.zeros((h, w), np.int32)], [9])["fmeasure"][0] == 0.0        # (the zero rule comes first, as in §22)
    with pytest.raises(ZeroDivisionError):
        match_scores(ribbon, [], [0])
    for bad in (ribbon.astype(np.float32), ribbon[0]):
        with pytest.raises(ValueError):
            match_scores(bad, truth, [0])
    with pytest.raises(ValueError):
        match_scores(ribbon, [s1[:, :-1]], [0])


# ---- quality (profiles/edge_thin_quality.json, written by tools/edge_thin_quality.py)

def test_quality_table_is_consistent_and_thin_is_above_thick():
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    doc = json.load(open(QUALITY))
    assert doc["images"] == 24 and doc["levels"] == 256 and len(doc["match_taus"]) == 32 and doc["n_directions"] == 8
    rows = {r["row"]: r for r in doc["rows"]}
    assert list(rows) == ["Ep_thick", "Ep_thin", "E_thick", "E_thin"] and list(doc["per_image"]) == ["Ep_thick", "Ep_thin"]
    for kind in ("Ep", "E"):                                  # the acceptance condition of §26: the ordering
        gain = rows[kind + "_thin"]["match"]["ODS"] - rows[kind + "_thick"]["match"]["ODS"]
        assert doc["thin_minus_thick"][kind] == gain > 0
        assert rows[kind + "_thin"]["match"]["OIS"] > rows[kind + "_thick"]["match"]["OIS"]
        assert rows[kind + "_thin"]["thick"]["ODS"] < rows[kind + "_thick"]["thick"]["ODS"]      # what §8 predicted
    assert doc["thin_above_thick"] is True
    for name, per in doc["per_image"].items():
        m = rows[name]["match"]
        assert m["OIS"] == ods_ois([[per[i]["best_f"]] for i in doc["ids"]], [0])["OIS"]
        assert m["ODS"] == ods_ois([[per[i]["f_at_ods"]] for i in doc["ids"]], [0])["ODS"]
        assert rows[name]["step"] == -(-(max(per[i]["map_max"] for i in doc["ids"]) + 1) // 256)
        assert (m["ODS_threshold"] + 1) // rows[name]["step"] - 1 in doc["match_taus"]
    # the thick rows under the thick metric are the figures already on record (SPEC.md §25, §24)
    old = json.load(open(os.path.join(ROOT, "profiles", "cue_gradient_quality.json")))
    for mine, theirs in (("Ep_thick", "Ep_colour_w2-2-1-1_b16_r8"), ("E_thick", "E_colour_k8_r8")):
        was = [r for r in old["rows"] if r["row"] == theirs][0]
        assert rows[mine]["thick"]["ODS"] == was["ODS"] and rows[mine]["thick"]["OIS"] == was["OIS"]


def test_quality_scores_of_the_first_three_images_are_reproduced():
    """Colour bank, k = 8, weights (2, 2, 1, 1), 16 bins, r = 8: E' and its thinned map from the restatements, the scores from
    ``evaluate.match_scores`` at each row's ODS threshold and at every image's best one. The thinned map scores above the thick
    one on each of the three."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cue_gradient_quality as inputs
    from gabor_color_image_segmentation_amd.evaluate import match_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(QUALITY))
    rows = {r["row"]: r for r in doc["rows"]}
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    for i in doc["ids"][:3]:
        lab, i0, g = inputs.cue_inputs(val["img_" + i], "colour")
        pb, d = cg.cue_gradient(lab, i0, 8, 16, (2, 2, 1, 1), 8, 8)
        ep = tg.joined(pb, g)
        maps = {"Ep_thick": ep, "Ep_thin": et.thin_fast(ep, d, 8)}
        got = {}
        for name, m in maps.items():
            want = doc["per_image"][name][i]
            assert int(m.max()) == want["map_max"]
            sc = match_scores(m, truth[i], [rows[name]["match"]["ODS_threshold"], want["best_threshold"]])
            for key, v in (("f_at_ods", sc["fmeasure"][0]), ("recall_at_ods", sc["recall"][0]),
                           ("precision_at_ods", sc["precision"][0]), ("best_f", sc["fmeasure"][1])):
                assert abs(v - want[key]) <= 1e-12, (i, name, key, v, want[key])
            got[name] = sc["fmeasure"]
        assert got["Ep_thin"][0] > got["Ep_thick"][0] and got["Ep_thin"][1] > got["Ep_thick"][1], i
