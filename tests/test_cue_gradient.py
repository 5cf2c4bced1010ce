"""The cue gradient (SPEC.md §25) on the CPU: the section's two worked examples, weights (1, 0, 0, 0) against the texton gradient of
§24, the quantiser at 0, 255 and every bin edge, the contract the frozen symbol table cannot carry (include/gcs_cues.h <->
``_lib.EXTENSIONS`` <-> the built library's exports; gcs.h and ``SIGNATURES`` do not know the symbol), the argument rules of
gcs_cue_gradient (refused before anything is launched, so they run without a GPU), the host chain (``Segmenter.cue_edges_device``,
``cue_gradient_device``, ``segment_cue_edges``) and every host ValueError through the stand-in ops (tests/cue_gradient_ops.py), and
the per-image scores of tools/cue_gradient_quality.py. No GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import cue_gradient_ref as cg
import texton_gradient_ref as tg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
QUALITY = os.path.join(ROOT, "profiles", "cue_gradient_quality.json")


# ---- the definition

def test_worked_example_one_channel_steps():
    """SPEC.md §25, example 1: one row, channel 0 = [10, 10, 200, 200], channels 1 and 2 constant, 2 bins, r = 1, n = 1."""
    img = np.zeros((1, 4, 3), np.uint8)
    img[0, :, 0], img[0, :, 1], img[0, :, 2] = [10, 10, 200, 200], 50, 250
    assert cg.shift_of(2) == 7 and cg.quantise(img[..., 0], 2).tolist() == [[0, 0, 1, 1]]
    assert cg.quantise(img[..., 1], 2).tolist() == [[0] * 4] and cg.quantise(img[..., 2], 2).tolist() == [[1] * 4]
    pb, d = cg.cue_gradient(None, img, 1, 2, (0, 3, 1, 1), 1, 1)
    assert pb.tolist() == [[0, 384, 384, 0]] and d.tolist() == [[0, 0, 0, 0]] and pb.dtype == np.int32 and d.dtype == np.uint8
    for wts, want in (((0, 0, 1, 1), 0), ((0, 16, 0, 0), 2048), ((0, 1, 16, 16), 128)):      # only channel 0 answers
        assert cg.cue_gradient(None, img, 1, 2, wts, 1, 1)[0].tolist() == [[0, want, want, 0]]
    assert cg.cue_edges(None, img, np.array([[5, 6, -4, 7]]), 1, 2, (0, 3, 1, 1), 1, 1).tolist() == [[0, 48, 0, 0]]


def test_worked_example_two_cues_two_directions():
    """SPEC.md §25, example 2: r = 1, n = 2. The labels step across a vertical edge (direction 0 answers), channel 0 across a
    horizontal one (direction 1): the maximum of the per-direction sums is not the sum of the maxima."""
    lab = np.array([[0, 1, 1]] * 3, np.int32)
    img = np.zeros((3, 3, 3), np.uint8)
    img[1:, :, 0] = 255
    assert tg.masks(1, 2).tolist() == [[[0, 0b100, 0], [0, 0b001, 0]], [[0, 0, 0b010], [0b010, 0, 0]]]
    chi = cg.cue_chi_squares(lab, img, 2, 2, (1, 1, 0, 0), 1, 2)
    assert chi[0][:, 1, 1].tolist() == [128, 0] and chi[1][:, 1, 1].tolist() == [0, 128]
    pb, d = cg.cue_gradient(lab, img, 2, 2, (1, 1, 0, 0), 1, 2)
    assert (pb[1, 1], d[1, 1]) == (128, 0)                   # P = (128, 128): the lowest direction of the maximum
    assert cg.summed_maxima(lab, img, 2, 2, (1, 1, 0, 0), 1, 2)[1, 1] == 256
    pb, d = cg.cue_gradient(lab, img, 2, 2, (1, 2, 0, 0), 1, 2)
    assert (pb[1, 1], d[1, 1]) == (256, 1)                   # P = (128, 256)
    assert cg.summed_maxima(lab, img, 2, 2, (1, 2, 0, 0), 1, 2)[1, 1] == 384


@pytest.mark.parametrize("shape,K,r,n", [((1, 1), 3, 8, 8), ((5, 9), 4, 8, 8), ((20, 23), 5, 3, 16), ((9, 33), 64, 15, 3)])
def test_texton_weight_alone_is_the_texton_gradient(shape, K, r, n):
    rng = np.random.default_rng(shape[1] + r)
    lab = rng.integers(-1, K + 1, size=shape).astype(np.int32)
    img = rng.integers(0, 256, size=shape + (3,)).astype(np.uint8)
    want = tg.texton_gradient(lab, K, r, n)
    for got in (cg.cue_gradient(lab, img, K, 16, (1, 0, 0, 0), r, n), cg.cue_gradient(lab, None, K, 64, (1, 0, 0, 0), r, n)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    five = cg.cue_gradient(lab, img, K, 16, (5, 0, 0, 0), r, n)
    assert np.array_equal(five[0], 5 * want[0]) and np.array_equal(five[1], want[1])
    # a channel alone is the texton gradient of its quantised plane, and the sum over cues is taken per direction
    for c in range(3):
        wts = tuple(int(i == c + 1) for i in range(4))
        one = tg.texton_gradient(cg.quantise(img[..., c], 8), 8, r, n)
        got = cg.cue_gradient(None, img, K, 8, wts, r, n)
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])
    p = cg.direction_sums(lab, img, K, 8, (1, 2, 3, 16), r, n)
    by_hand = tg.chi_squares(lab, K, r, n) + sum(wc * tg.chi_squares(cg.quantise(img[..., c], 8), 8, r, n)
                                                 for c, wc in enumerate((2, 3, 16)))
    assert np.array_equal(p, by_hand) and int(p.max()) < 1 << 23


@pytest.mark.parametrize("bins", cg.BINS)
def test_quantiser_at_the_ends_and_every_bin_edge(bins):
    shift = cg.shift_of(bins)
    assert shift == 8 - int(np.log2(bins)) and 2 <= shift <= 7 and bins << shift == 256
    q = lambda v: int(cg.quantise(np.array([[v]], np.uint8), bins)[0, 0])
    assert q(0) == 0 and q(255) == bins - 1
    for k in range(1, bins):
        assert q((k << shift) - 1) == k - 1 and q(k << shift) == k
    assert cg.quantise(np.arange(256, dtype=np.uint8)[None], bins).tolist() == [[v * bins // 256 for v in range(256)]]
    with pytest.raises(AssertionError):
        cg.shift_of(3)


# ---- the library: symbols and argument rules

@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def test_extension_header_table_and_exports_agree(lib):
    from gabor_color_image_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gcs_cues.h")).read()
    declared = set(re.findall(r"\b(gcs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXTENSIONS) == {"gcs_cue_gradient"}, declared ^ set(_lib.EXTENSIONS)
    assert 'extern "C"' in hdr and "ABI 18" in hdr and '#include "gcs.h"' in hdr
    assert "torch" not in hdr.lower() and "at::" not in hdr
    for name, (res, args) in _lib.EXTENSIONS.items():
        fn = getattr(lib, name)                               # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == args
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):                        # pointers and the stream are void pointers, the rest ints
            assert (a is C.c_void_p) == ("*" in p or p.startswith("gcs_stream_t")), (name, p)
    assert not set(_lib.EXTENSIONS) & set(_lib.SIGNATURES)
    assert lib.gcs_abi_version() == 18 and _lib.ABI_VERSION == 18


def test_the_frozen_header_and_table_do_not_know_the_symbol():
    from gabor_color_image_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gcs.h")).read()
    assert "gcs_cue" not in hdr and "gcs_cues.h" not in hdr
    assert not [k for k in _lib.SIGNATURES if "cue" in k]


def test_a_library_without_the_symbol_still_loads_and_the_ops_refuse(built, tmp_path):
    """``load`` sets up the extension symbols it finds and no others: a table entry the library does not export is passed over
    (an older library of the same ABI), and ``HipOps.cue_gradient`` refuses with the optional stages' words."""
    from gabor_color_image_segmentation_amd import _lib
    from gabor_color_image_segmentation_amd.segmenter import HipOps
    saved, held = dict(_lib.EXTENSIONS), _lib._lib
    try:
        _lib.EXTENSIONS["gcs_not_in_this_library"] = (C.c_int, [])
        _lib._lib = None
        lib = _lib.load()
        assert not hasattr(lib, "gcs_not_in_this_library") and hasattr(lib, "gcs_cue_gradient")
    finally:
        _lib.EXTENSIONS.clear()
        _lib.EXTENSIONS.update(saved)
        _lib._lib = held

    class Old:                                               # what the method asks of its library, without the symbol
        pass
    ops = HipOps.__new__(HipOps)
    ops.lib = Old()
    with pytest.raises(ValueError, match="needs ops that have it"):
        HipOps.cue_gradient.__wrapped__(ops, None, None, 1, 8, 8, 1, 16, (1, 1, 1, 1), 1, 1, None, None, None)


def test_cue_gradient_validates_before_launching(lib):
    """Argument errors are reported without touching the GPU (so this runs on the CPU box)."""
    p = [C.c_void_p(q << 32) for q in range(1, 8)]           # non-NULL dummies far apart, never dereferenced
    good = dict(lab=p[0], img=p[1], B=2, H=19, W=23, K=8, shift=4, w=(2, 2, 1, 1), r=8, n=8, masks=p[2], grad=p[3], out=p[4], dirs=p[5])

    def call(**bad):
        a = dict(good, **bad)
        return lib.gcs_cue_gradient(a["lab"], a["img"], a["B"], a["H"], a["W"], a["K"], a["shift"], *a["w"], a["r"], a["n"], a["masks"],
                                    a["grad"], a["out"], a["dirs"], None)
    for bad in (dict(masks=None), dict(out=None)):
        assert call(**bad) == 1 and b"NULL" in lib.gcs_last_error(), bad
    for bad in (dict(lab=None), dict(img=None), dict(lab=None, w=(1, 0, 0, 0)), dict(img=None, w=(0, 0, 0, 1))):
        assert call(**bad) == 1 and b"no plane" in lib.gcs_last_error(), bad
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097)):
        assert call(**bad) == 1 and b"shape" in lib.gcs_last_error(), bad
    for bad in (dict(K=0), dict(K=65), dict(r=0), dict(r=16), dict(n=0), dict(n=17)):
        assert call(**bad) == 1 and b"argument" in lib.gcs_last_error(), bad
    for bad in (dict(shift=1), dict(shift=8), dict(shift=0), dict(shift=-1)):
        assert call(**bad) == 1 and b"shift" in lib.gcs_last_error(), bad
    for c in range(4):
        for v in (-1, 17):
            assert call(w=tuple(v if i == c else 1 for i in range(4))) == 1 and b"weight" in lib.gcs_last_error(), (c, v)
    assert call(w=(0, 0, 0, 0)) == 1 and b"every weight is 0" in lib.gcs_last_error()
    px = 2 * 19 * 23
    at = lambda q, off: C.c_void_p(q.value + off)
    for bad in (dict(out=p[0]), dict(out=at(p[0], 4 * px - 1)), dict(out=at(p[1], 3 * px - 1)), dict(out=at(p[3], -4 * px + 1)),
                dict(out=p[2]), dict(dirs=at(p[0], 4 * px - 1)), dict(dirs=p[1]), dict(dirs=p[3]), dict(dirs=at(p[2], 8 * 2 * 17 * 4 - 1)),
                dict(dirs=at(p[4], 4 * px - 1)), dict(dirs=at(p[4], -px + 1))):
        assert call(**bad) == 1 and b"overlaps" in lib.gcs_last_error(), bad
    assert b"gcs_cue_gradient" in lib.gcs_last_error()


# ---- the host calls, through the stand-in

@pytest.fixture(scope="module")
def standin(built):
    from gabor_color_image_segmentation_amd import make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from cue_gradient_ops import CueGradientOps
    import feature_gradient_ref as fg
    import position_ref as pr
    img = synthetic_batch(1, 24, 40, seed=11)[0]
    ops = CueGradientOps(make_bank(n_scales=4, n_orient=2))
    grad = fg.gradient(pr.features(img, 0.0, 0, 0, 4, 2), 4, 2)
    labels = pr.segment(img, k=4, n_iter=3, n_scales=4, n_orient=2)
    return img, ops, grad, labels


PLAN = dict(n_scales=4, n_orient=2, k=4, n_iter=3)


def test_cue_edges_device_runs_the_chain_in_order(standin):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    img, ops, grad, labels = standin
    seg = Segmenter(ops=ops, **PLAN)
    dev = torch.from_numpy(img[None])
    del ops.calls[:]
    got = seg.cue_edges_device(dev, radius=3, n_directions=6, bins=8, weights=(2, 2, 1, 1))
    want = cg.cue_edges(labels, img, grad, 4, 8, (2, 2, 1, 1), 3, 6)                # no chroma_gain: the cues are R, G, B
    assert got.dtype == torch.int32 and np.array_equal(got[0].numpy(), want) and got.max() > 0
    names = [c[0] for c in ops.calls]
    assert names[0] == "gabor" and ops.calls[-1] == ("cue", 1, 4, 8, (2, 2, 1, 1), 3, 6, True, True, True, False)
    assert names.index("gradient") < names.index("assign") < names.index("cue") and "unpack" not in names and "texton" not in names
    del ops.calls[:]
    alone = seg.cue_edges_device(dev, radius=3, n_directions=6, bins=8, joined=False)
    assert np.array_equal(alone[0].numpy(), cg.cue_gradient(labels, img, 4, 8, (2, 2, 1, 1), 3, 6)[0])
    assert "gradient" not in [c[0] for c in ops.calls] and ops.calls[-1][-2:] == (False, False)
    # without the texton cue: no Lloyd pass, no label map, and the clustering options play no part
    del ops.calls[:]
    light = seg.cue_edges_device(dev, radius=3, n_directions=6, weights=(0, 1, 1, 1))
    assert np.array_equal(light[0].numpy(), cg.cue_edges(None, img, grad, 4, 16, (0, 1, 1, 1), 3, 6))
    names = [c[0] for c in ops.calls]
    assert names == ["gabor", "gradient", "masks", "cue"] or names == ["gabor", "gradient", "cue"], names
    assert ops.calls[-1][7:9] == (False, True)
    for plan in (dict(n_superpixels=24), dict(connectivity=True), dict(min_region_size=9), dict(tree_nodes="clusters")):
        other = Segmenter(ops=ops, **PLAN, **plan)
        assert np.array_equal(other.cue_edges_device(dev, radius=3, n_directions=6, weights=(0, 1, 1, 1)).numpy(), light.numpy())
    both = seg.cue_edges_device(torch.from_numpy(np.stack([img, img[::-1].copy()])), radius=3, n_directions=6, mode="global")
    assert tuple(both.shape) == (2, 24, 40) and ops.calls[-1][:2] == ("cue", 2)


def test_cue_edges_device_on_a_colour_plan_reads_the_transformed_image(built):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from cue_gradient_ops import CueGradientOps
    import colour_ref
    import feature_gradient_ref as fg
    import position_ref as pr
    img = synthetic_batch(1, 24, 40, seed=12)[0]
    bank = make_bank(n_scales=4, n_orient=2, color_weight=0.125)
    ops = CueGradientOps(bank, chroma_gain=4)
    seg = Segmenter(ops=ops, n_scales=4, n_orient=2, color_weight=0.125, chroma_gain=4, k=4, n_iter=3)
    grad = fg.gradient(pr.features(img, 0.125, 4, 0, 4, 2), 4, pr.n_slots(2, 0.125, 0))
    got = seg.cue_edges_device(torch.from_numpy(img[None]), radius=3, n_directions=6, weights=(0, 1, 2, 3))
    i0 = colour_ref.opponent(img, 4)
    assert not np.array_equal(i0, img)
    assert np.array_equal(got[0].numpy(), cg.cue_edges(None, i0, grad, 4, 16, (0, 1, 2, 3), 3, 6))


@pytest.mark.parametrize("joined", [True, False])
def test_cue_edges_device_at_the_texton_weight_alone_is_texton_edges_device(standin, joined):
    """One chain behind both: the same map, and the same recorded calls up to the last one."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    img, ops, _, _ = standin
    seg = Segmenter(ops=ops, **PLAN)
    dev = torch.from_numpy(img[None])
    got, calls = {}, {}
    for name, run in (("cue", lambda: seg.cue_edges_device(dev, radius=3, n_directions=6, weights=(1, 0, 0, 0), joined=joined)),
                      ("texton", lambda: seg.texton_edges_device(dev, radius=3, n_directions=6, joined=joined))):
        del ops.calls[:]
        got[name] = run()
        calls[name] = list(ops.calls)
    assert got["cue"].dtype == got["texton"].dtype == torch.int32 and torch.equal(got["cue"], got["texton"]) and got["cue"].max() > 0
    assert calls["cue"][:-1] == calls["texton"][:-1] and len(calls["cue"]) == len(calls["texton"]) > 2
    assert calls["cue"][-1] == ("cue", 1, 4, 16, (1, 0, 0, 0), 3, 6, True, True, joined, False)
    assert calls["texton"][-1] == ("texton", 1, 4, 3, 6, joined, False)
    assert ("gradient" in [c[0] for c in calls["cue"]]) == joined


def test_every_host_value_error_comes_before_any_stage(standin):
    import torch
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    from texton_gradient_ops import TextonGradientOps
    img, ops, _, labels = standin
    dev = torch.from_numpy(img[None])
    lab = torch.from_numpy(labels[None].astype(np.int32))
    seg = Segmenter(ops=ops, **PLAN)
    n = len(ops.calls)
    bad = (dict(bins=0), dict(bins=3), dict(bins=128), dict(bins=16.5), dict(bins="16"), dict(bins=True),
           dict(weights=(0, 0, 0, 0)), dict(weights=(1, 2, 3)), dict(weights=(1, 2, 3, 4, 5)), dict(weights=(1, 1, 1, 17)),
           dict(weights=(-1, 1, 1, 1)), dict(weights=(1.5, 1, 1, 1)), dict(weights=5), dict(weights="2211"), dict(weights=None),
           dict(radius=0), dict(radius=16), dict(n_directions=0), dict(n_directions=17))
    for kw in bad:
        with pytest.raises(ValueError):
            seg.cue_edges_device(dev, **kw)
        with pytest.raises(ValueError):
            seg.cue_gradient_device(lab, dev, **kw)
        with pytest.raises(ValueError):
            pkg.segment_cue_edges(img, ops=ops, **PLAN, **kw)
    with pytest.raises(ValueError):
        seg.cue_edges_device(dev, mode="strips")
    with pytest.raises(ValueError):
        seg.cue_edges_device(dev[:, :4])                      # smaller than 8 x 8: the entry points' common rule
    with pytest.raises(ValueError):
        seg.cue_edges_device(dev[..., 0])
    with pytest.raises(TypeError):
        seg.cue_edges_device(dev, y0=8)                       # no such argument: whole images only
    for plan in (dict(n_superpixels=24), dict(connectivity=True), dict(min_region_size=9), dict(tree_nodes="clusters")):
        other = Segmenter(ops=ops, **PLAN, **plan)
        with pytest.raises(ValueError, match="plain k-means map"):
            other.cue_edges_device(dev)
    for kw in (dict(K=0), dict(K=65), dict(K=2.5)):
        with pytest.raises(ValueError):
            seg.cue_gradient_device(lab, dev, **kw)
    for a, b in ((lab.to(torch.int64), dev), (lab[0], dev), (lab, dev[..., :2]), (lab, dev.to(torch.int32)), (None, dev), (lab, None),
                 (lab[:, :8], dev)):
        with pytest.raises(ValueError):
            seg.cue_gradient_device(a, b)
    with pytest.raises(ValueError):
        pkg.segment_cue_edges(img[..., 0], ops=ops, **PLAN)
    assert len(ops.calls) == n                               # refused before any stage
    old = Segmenter(n_scales=4, n_orient=2, ops=TextonGradientOps(make_bank(n_scales=4, n_orient=2)))
    for call in (lambda: old.cue_edges_device(dev), lambda: old.cue_gradient_device(lab, dev)):
        with pytest.raises(ValueError, match="ops that have it"):
            call()


def test_cue_gradient_device_takes_any_map_and_image(standin):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    img, ops, grad, labels = standin
    seg = Segmenter(n_scales=4, n_orient=2, ops=ops)
    rng = np.random.default_rng(8)
    lab = rng.integers(0, 11, size=(2, 7, 13)).astype(np.int32)
    im = rng.integers(0, 256, size=(2, 7, 13, 3)).astype(np.uint8)
    out, dirs = seg.cue_gradient_device(torch.from_numpy(lab), torch.from_numpy(im), radius=2, n_directions=3, directions=True)
    assert ops.calls[-1] == ("cue", 2, 11, 16, (2, 2, 1, 1), 2, 3, True, True, False, True)      # K = labels.max() + 1
    for i in range(2):
        p, d = cg.cue_gradient(lab[i], im[i], 11, 16, (2, 2, 1, 1), 2, 3)
        assert np.array_equal(out[i].numpy(), p) and np.array_equal(dirs[i].numpy(), d) and dirs.dtype == torch.uint8
    g = rng.integers(-9, 2 ** 20, size=lab.shape).astype(np.int32)
    e = seg.cue_gradient_device(None, torch.from_numpy(im), radius=2, n_directions=3, bins=4, weights=(0, 1, 0, 16),
                                gradient=torch.from_numpy(g))
    assert ops.calls[-1][7:9] == (False, True)
    assert np.array_equal(e[1].numpy(), cg.cue_edges(None, im[1], g[1], 1, 4, (0, 1, 0, 16), 2, 3))
    t = seg.cue_gradient_device(torch.from_numpy(lab), None, K=16, radius=2, n_directions=3, weights=(1, 0, 0, 0))
    assert ops.calls[-1][7:9] == (True, False) and np.array_equal(t[0].numpy(), tg.texton_gradient(lab[0], 16, 2, 3)[0])


def test_segment_cue_edges_normalises_the_map(standin):
    import gabor_color_image_segmentation_amd as pkg
    img, ops, grad, labels = standin
    got = pkg.segment_cue_edges(img, radius=3, n_directions=6, ops=ops, **PLAN)
    want = cg.cue_edges(labels, img, grad, 4, 16, (2, 2, 1, 1), 3, 6)
    assert got.dtype == np.float32 and np.array_equal(got, tg.normalised(want)) and got.max() == 1.0 and got.min() >= 0.0
    flat = pkg.segment_cue_edges(np.full((16, 16, 3), 77, np.uint8), ops=ops, **PLAN)
    assert flat.dtype == np.float32 and flat.shape == (16, 16) and not flat.any()
    assert "segment_cue_edges" in dir(pkg)


# ---- quality (profiles/cue_gradient_quality.json, written by tools/cue_gradient_quality.py)

def test_quality_table_is_consistent_and_names_the_default():
    import inspect
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    doc = json.load(open(QUALITY))
    assert doc["images"] == 24 and doc["levels"] == 256 and doc["n_directions"] == 8 and doc["k"] == 8
    rows = {r["row"]: r for r in doc["rows"]}
    assert len(rows) == 2 + 4 * 2 * 2 + 4 + 2 + 2             # E per bank; Ep colour; Ep default; PB; SM
    assert list(doc["per_image"]) == ["Ep_colour_w2-2-1-1_b16_r8"]
    for row in doc["rows"]:
        assert (row["ODS_threshold"] + 1) % row["step"] == 0 and row["OIS"] >= row["ODS"] > 0
        per = doc["per_image"].get(row["row"])
        if per is not None:
            assert row["OIS"] == ods_ois([[per[i]["best_f"]] for i in doc["ids"]], [0])["OIS"]
            assert row["ODS"] == ods_ois([[per[i]["f_at_ods"]] for i in doc["ids"]], [0])["ODS"]
            assert row["step"] == -(-(max(per[i]["map_max"] for i in doc["ids"]) + 1) // 256)
    old = json.load(open(os.path.join(ROOT, "profiles", "texton_gradient_quality.json")))
    for bank in ("colour", "default"):                        # the E rows are the figures already on record
        was = [r for r in old["rows"] if r["row"] == "E_%s_s0_k8_r8" % bank][0]
        assert rows["E_%s_k8_r8" % bank]["ODS"] == was["ODS"] and rows["E_%s_k8_r8" % bank]["OIS"] == was["OIS"]
    # the ranking is the table's own, and the defaults of the host calls are its first row
    ranked = sorted((r for r in doc["rows"] if r["map"] == "Ep" and r["bank"] == "colour" and r["radius"] <= 8),
                    key=lambda r: (-r["ODS"], r["row"]))
    assert doc["ranking_r_le_8"] == [r["row"] for r in ranked]
    first = rows[doc["ranking_r_le_8"][0]]
    for fn in (Segmenter.cue_edges_device, Segmenter.cue_gradient_device):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items()}
        assert (list(d["weights"]), d["bins"], d["radius"]) == (first["weights"], first["bins"], first["radius"])
    assert doc["first_minus_E"] == first["ODS"] - rows["E_colour_k8_r8"]["ODS"]
    assert doc["first_beats_E_by_more_than_the_spread"] == (doc["first_minus_E"] > doc["spread"])


def test_quality_scores_of_the_first_two_images_are_reproduced():
    """Colour bank, k = 8, weights (2, 2, 1, 1), 16 bins, r = 8: the E' maps from the restatements, the scores from
    ``evaluate.edge_scores`` at the row's ODS threshold and at every image's best one."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cue_gradient_quality as tool
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(QUALITY))
    name = tool.row_name("Ep", "colour", (2, 2, 1, 1), 16, 8)
    row = [r for r in doc["rows"] if r["row"] == name][0]
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    for i in doc["ids"][:2]:
        want = doc["per_image"][name][i]
        lab, i0, g = tool.cue_inputs(val["img_" + i], "colour")
        e = cg.cue_edges(lab, i0, g, 8, 16, (2, 2, 1, 1), 8, 8)         # the restatement itself, not the tool's shared sums
        assert int(e.max()) == want["map_max"]
        sc = edge_scores(e, truth[i], [row["ODS_threshold"], want["best_threshold"]])
        for key, got in (("f_at_ods", sc["fmeasure"][0]), ("recall_at_ods", sc["recall"][0]),
                         ("precision_at_ods", sc["precision"][0]), ("best_f", sc["fmeasure"][1])):
            assert abs(got - want[key]) <= 1e-12, (i, key, got, want[key])
