"""The texton gradient (SPEC.md §24) on the CPU: the section's worked examples, the restatement (tests/texton_gradient_ref.py)
against an independent form (``scipy.ndimage.correlate`` of one-hot planes, ``mode="mirror"``), the host-only entry point
gcs_texton_masks against the restatement for every radius and direction count, the argument rules of gcs_texton_gradient, constant
maps and steps, the host chain (``Segmenter.texton_edges_device``, ``texton_gradient_device``, ``segment_texton_edges``) through the
stand-in ops (tests/texton_gradient_ops.py) and the per-image scores of tools/texton_gradient_quality.py. No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import texton_gradient_ref as tg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
QUALITY = os.path.join(HERE, "..", "profiles", "texton_gradient_quality.json")


# ---- the definition

def test_worked_example_one_row():
    """SPEC.md §24: one row [0, 0, 1, 1], r = 1, n = 1. Half A = {(0, +1)}, half B = {(0, -1)}; the vertical offsets have s = 0."""
    m = tg.masks(1, 1)
    assert m.tolist() == [[[0, 0b100, 0], [0, 0b001, 0]]]
    t, d = tg.texton_gradient(np.array([[0, 0, 1, 1]]), 2, 1, 1)
    assert t.tolist() == [[0, 128, 128, 0]] and d.tolist() == [[0, 0, 0, 0]]
    assert tg.mirror(np.array([4, -1, -2, 7, 0]), 4).tolist() == [2, 1, 2, 1, 0] and tg.mirror(np.array([-5, 3]), 1).tolist() == [0, 0]


def test_worked_example_one_bin():
    """A bin with g = 2, h = 1 adds floor(64 / 3) = 21: a table whose A holds two taps on label 1 and whose B holds one."""
    table = np.zeros((1, 2, 3), np.uint32)
    table[0, 0, 1] = 0b100                                   # A: (0, +1) ...
    table[0, 0, 2] = 0b010                                   # ... and (+1, 0)
    table[0, 1, 0] = 0b010                                   # B: (-1, 0)
    lab = np.array([[9, 1, 9], [9, 9, 1], [9, 1, 9]])        # centre: A sees 1, 1; B sees 1; 9 is outside 0 .. K-1
    assert int(tg.chi_squares(lab, 2, 1, 1, table)[0, 1, 1]) == 21
    assert tg.joined(np.array([[21, 0, 3]]), np.array([[2 ** 20 - 1, 5, 12]])).tolist() == [[4692, 0, 6]]


def test_directions_are_the_rounded_normals():
    assert tg.direction(0, 8) == (1024, 0) and tg.direction(4, 8) == (0, 1024) and tg.direction(2, 8) == (724, 724)
    for n in range(1, 17):                                   # no 1024 cos is near a half-integer: the rounding is robust
        for i in range(n):
            for v in (1024 * np.cos(np.pi * i / n), 1024 * np.sin(np.pi * i / n)):
                assert abs(v - np.floor(v) - 0.5) > 1e-3, (n, i)
    m = tg.masks(8, 8)
    a0, b0 = m[0, 0], m[0, 1]
    assert all(int(a) & ((1 << 9) - 1) == 0 for a in a0) and all(int(b) >> 8 == 0 for b in b0)     # direction 0: right | left
    assert int(m[4, 0, :9].sum()) == 0 and int(m[4, 1, 8:].sum()) == 0                           # direction n/2: below | above
    assert sum(bin(int(v)).count("1") for v in m[0].ravel()) == 197 - 17                         # the disc without its s = 0 column


def _independent(lab, K, r, n):
    """chi-squares from correlations of the one-hot planes with the halves as 0/1 kernels, scipy's mirror border."""
    from scipy import ndimage as ndi
    table = tg.masks(r, n)
    width = 2 * r + 1
    chi = np.zeros((n,) + lab.shape, np.int64)
    for i in range(n):
        kern = [np.array([[(int(table[i, side, m]) >> c) & 1 for c in range(width)] for m in range(width)], np.int64)
                for side in range(2)]
        for j in range(K):
            plane = (lab == j).astype(np.int64)
            g, h = (ndi.correlate(plane, k, mode="mirror") for k in kern)
            chi[i] += np.where(g + h > 0, 64 * (g - h) ** 2 // np.maximum(g + h, 1), 0)
    return chi.max(0).astype(np.int32), chi.argmax(0).astype(np.uint8)


@pytest.mark.parametrize("shape,K,r,n", [((1, 1), 3, 8, 8), ((1, 9), 3, 8, 8), ((5, 9), 4, 8, 8), ((20, 23), 5, 8, 8),
                                         ((13, 11), 2, 1, 1), ((9, 33), 16, 2, 3), ((40, 37), 7, 15, 16), ((17, 18), 64, 4, 5)])
def test_restatement_equals_an_independent_form(shape, K, r, n):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + r)
    lab = rng.integers(0, K, size=shape).astype(np.int32)
    want = _independent(lab, K, r, n)                        # (scipy reflects as often as a small image needs)
    got = tg.texton_gradient(lab, K, r, n)
    assert got[0].dtype == np.int32 and got[1].dtype == np.uint8
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if shape == (1, 1):
        assert got[0].tolist() == [[0]]                      # every tap mirrors onto the pixel itself


def test_scipy_mirror_is_the_sections_mirror():
    """scipy's ``mirror`` is mir(t, N), also for lines shorter than the reach."""
    from scipy import ndimage as ndi
    for size in (1, 2, 3, 7):
        x = np.arange(size)
        for shift in range(-8, 9):
            k = np.zeros(17, np.int64)
            k[8 + shift] = 1
            assert ndi.correlate(x, k, mode="mirror").tolist() == tg.mirror(x + shift, size).tolist()


@pytest.mark.parametrize("r", range(1, 16))
def test_constant_map_gives_zero_everywhere(r):
    t, d = tg.texton_gradient(np.full((9, 12), 2), 4, r, 8)
    assert not t.any() and not d.any()


@pytest.mark.parametrize("r,n", [(3, 8), (8, 8), (5, 16), (2, 4)])
def test_steps_answer_to_their_direction(r, n):
    """A vertical step: direction 0 (the normal points along x); a horizontal one: direction n / 2. Far from the step: zero."""
    lab = np.zeros((40, 44), np.int32)
    lab[:, 22:] = 1
    t, d = tg.texton_gradient(lab, 2, r, n)
    assert (d[:, 21:23] == 0).all() and (t[:, 21:23] > 0).all() and not t[:, :22 - r].any() and not t[:, 22 + r:].any()
    assert (t[:, 21] == t[0, 21]).all()                      # the mirror: a border parallel to a direction's normal adds nothing
    t2, d2 = tg.texton_gradient(lab.T.copy(), 2, r, n)
    assert (d2[21:23] == n // 2).all() and np.array_equal(t2, t.T)


def test_values_outside_the_range_count_nowhere():
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 3, size=(12, 15)).astype(np.int32)
    hole = lab.copy()
    hole[lab == 2] = -1
    far = lab.copy()
    far[lab == 2] = 2
    a = tg.chi_squares(hole, 2, 3, 4)
    b = tg.chi_squares(far, 2, 3, 4)                         # K = 2: the value 2 = K is outside as well
    assert np.array_equal(a, b) and not np.array_equal(a, tg.chi_squares(lab, 3, 3, 4))


# ---- the library: host entry point and argument rules

@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def test_library_masks_equal_the_restatement(lib):
    for r in range(1, 16):
        for n in range(1, 17):
            got = np.full((n, 2, 2 * r + 1), 0xdeadbeef, np.uint32)
            assert lib.gcs_texton_masks(r, n, got.ctypes.data) == 0
            assert np.array_equal(got, tg.masks(r, n)), (r, n)
    buf = np.zeros(16 * 2 * 31, np.uint32)
    for r, n in ((0, 8), (16, 8), (8, 0), (8, 17), (-1, 1)):
        assert lib.gcs_texton_masks(r, n, buf.ctypes.data) == 1, (r, n)
        assert b"gcs_texton_masks" in lib.gcs_last_error()
    assert lib.gcs_texton_masks(8, 8, None) == 1 and b"NULL" in lib.gcs_last_error()
    assert not buf.any()                                     # a refused call writes nothing


def test_texton_gradient_validates_before_launching(lib):
    """Argument errors are reported without touching the GPU (so this runs on the CPU box)."""
    from gabor_color_image_segmentation_amd import _lib
    assert _lib.ABI_VERSION == 18 and lib.gcs_abi_version() == 18
    p = [C.c_void_p(q << 24) for q in range(1, 6)]           # non-NULL dummies far apart, never dereferenced
    good = dict(lab=p[0], B=2, H=19, W=23, K=8, r=8, n=8, masks=p[1], grad=p[2], out=p[3], dirs=p[4])

    def call(**bad):
        a = dict(good, **bad)
        return lib.gcs_texton_gradient(a["lab"], a["B"], a["H"], a["W"], a["K"], a["r"], a["n"], a["masks"], a["grad"], a["out"],
                                       a["dirs"], None)
    for bad in (dict(lab=None), dict(masks=None), dict(out=None)):
        assert call(**bad) == 1, bad
        assert b"NULL" in lib.gcs_last_error()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097)):
        assert call(**bad) == 1, bad
        assert b"shape" in lib.gcs_last_error()
    for bad in (dict(K=0), dict(K=65), dict(r=0), dict(r=16), dict(n=0), dict(n=17)):
        assert call(**bad) == 1, bad
        assert b"gcs_texton_gradient" in lib.gcs_last_error() and b"argument" in lib.gcs_last_error()


# ---- the host calls, through the stand-in

@pytest.fixture(scope="module")
def standin(built):
    from gabor_color_image_segmentation_amd import make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from texton_gradient_ops import TextonGradientOps
    import feature_gradient_ref as fg
    import position_ref as pr
    img = synthetic_batch(1, 24, 40, seed=11)[0]
    ops = TextonGradientOps(make_bank(n_scales=4, n_orient=2))
    grad = fg.gradient(pr.features(img, 0.0, 0, 0, 4, 2), 4, 2)
    labels = pr.segment(img, k=4, n_iter=3, n_scales=4, n_orient=2)
    return img, ops, grad, labels


def test_texton_edges_device_runs_the_chain_in_order(standin):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    img, ops, grad, labels = standin
    seg = Segmenter(n_scales=4, n_orient=2, k=4, n_iter=3, ops=ops)
    dev = torch.from_numpy(img[None])
    assert np.array_equal(seg.segment_device(dev)[0].numpy(), labels)
    tgm = tg.texton_gradient(labels, 4, 3, 6)[0]
    del ops.calls[:]
    got = seg.texton_edges_device(dev, radius=3, n_directions=6)
    assert got.dtype == torch.int32 and np.array_equal(got[0].numpy(), tg.joined(tgm, grad)) and got.max() > 0
    names = [c[0] for c in ops.calls]
    assert names[0] == "gabor" and names[-1] == "texton" and ops.calls[-1] == ("texton", 1, 4, 3, 6, True, False)
    assert names.index("gradient") < names.index("assign") < names.index("texton")       # G, the Lloyd loop, the kernel
    assert "unpack" not in names                             # one slab: the canonical tensor is never made
    del ops.calls[:]
    alone = seg.texton_edges_device(dev, radius=3, n_directions=6, joined=False)
    assert np.array_equal(alone[0].numpy(), tgm) and "gradient" not in [c[0] for c in ops.calls]
    assert ops.calls[-1] == ("texton", 1, 4, 3, 6, False, False)
    both = seg.texton_edges_device(torch.from_numpy(np.stack([img, img[::-1].copy()])), radius=3, n_directions=6, mode="global")
    assert tuple(both.shape) == (2, 24, 40) and ops.calls[-1][:2] == ("texton", 2)


def test_texton_edges_device_refusals_launch_nothing(standin):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from texton_gradient_ops import TextonGradientOps
    from gabor_color_image_segmentation_amd import make_bank
    img, ops, _, _ = standin
    dev = torch.from_numpy(img[None])
    seg = Segmenter(n_scales=4, n_orient=2, k=4, n_iter=3, ops=ops)
    n = len(ops.calls)
    for kw in (dict(radius=0), dict(radius=16), dict(n_directions=0), dict(n_directions=17), dict(mode="strips")):
        with pytest.raises(ValueError):
            seg.texton_edges_device(dev, **kw)
    with pytest.raises(ValueError):
        seg.texton_edges_device(dev[:, :4])                  # smaller than 8 x 8: the entry points' common rule
    with pytest.raises(ValueError):
        seg.texton_edges_device(dev[..., 0])
    with pytest.raises(TypeError):
        seg.texton_edges_device(dev, dist_group=object())    # no such argument: one rank, whole images
    for plan in (dict(n_superpixels=24), dict(connectivity=True), dict(min_region_size=9), dict(tree_nodes="clusters")):
        other = Segmenter(n_scales=4, n_orient=2, k=4, n_iter=3, ops=ops, **plan)
        with pytest.raises(ValueError, match="plain k-means map"):
            other.texton_edges_device(dev)
    assert len(ops.calls) == n                               # refused before any stage
    from feature_gradient_ops import FeatureGradientOps
    old = Segmenter(n_scales=4, n_orient=2, ops=FeatureGradientOps(make_bank(n_scales=4, n_orient=2)))
    with pytest.raises(ValueError, match="ops that have it"):
        old.texton_edges_device(dev)


def test_texton_gradient_device_takes_any_label_map(standin):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    img, ops, grad, labels = standin
    seg = Segmenter(n_scales=4, n_orient=2, ops=ops)
    rng = np.random.default_rng(8)
    lab = rng.integers(0, 11, size=(2, 7, 13)).astype(np.int32)
    out, dirs = seg.texton_gradient_device(torch.from_numpy(lab), radius=2, n_directions=3, directions=True)
    assert ops.calls[-1] == ("texton", 2, 11, 2, 3, False, True)       # K = labels.max() + 1
    for i in range(2):
        t, d = tg.texton_gradient(lab[i], 11, 2, 3)
        assert np.array_equal(out[i].numpy(), t) and np.array_equal(dirs[i].numpy(), d) and dirs.dtype == torch.uint8
    g = rng.integers(0, 2 ** 20, size=lab.shape).astype(np.int32)
    e = seg.texton_gradient_device(torch.from_numpy(lab), K=16, radius=2, n_directions=3, gradient=torch.from_numpy(g))
    assert np.array_equal(e[0].numpy(), tg.joined(tg.texton_gradient(lab[0], 16, 2, 3)[0], g[0]))
    for kw in (dict(K=0), dict(K=65), dict(radius=16), dict(n_directions=0)):
        with pytest.raises(ValueError):
            seg.texton_gradient_device(torch.from_numpy(lab), **kw)
    with pytest.raises(ValueError):
        seg.texton_gradient_device(torch.from_numpy(lab.astype(np.int64)))
    with pytest.raises(ValueError):
        seg.texton_gradient_device(torch.from_numpy(lab[0]))


def test_segment_texton_edges_normalises_the_map(standin):
    import gabor_color_image_segmentation_amd as pkg
    img, ops, grad, labels = standin
    kw = dict(n_scales=4, n_orient=2, k=4, n_iter=3, ops=ops)
    got = pkg.segment_texton_edges(img, radius=3, n_directions=6, **kw)
    want = tg.joined(tg.texton_gradient(labels, 4, 3, 6)[0], grad)
    assert got.dtype == np.float32 and np.array_equal(got, tg.normalised(want)) and got.max() == 1.0 and got.min() >= 0.0
    flat = pkg.segment_texton_edges(np.full((16, 16, 3), 77, np.uint8), **kw)
    assert flat.dtype == np.float32 and flat.shape == (16, 16) and not flat.any()
    with pytest.raises(ValueError):
        pkg.segment_texton_edges(img[..., 0], **kw)


# ---- quality (profiles/texton_gradient_quality.json, written by tools/texton_gradient_quality.py)

def test_quality_table_is_consistent():
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    doc = json.load(open(QUALITY))
    assert doc["images"] == 24 and doc["levels"] == 256 and doc["n_directions"] == 8
    assert len(doc["rows"]) == 4 * (1 + 2 * 2 * 3)           # per (bank, smoothing): G, and TG and E per (k, r)
    assert list(doc["per_image"]) == ["E_colour_s0_k8_r8"]   # per-image figures are kept for the recommended setting
    for row in doc["rows"]:
        assert (row["ODS_threshold"] + 1) % row["step"] == 0 and row["OIS"] >= row["ODS"] > 0
        per = doc["per_image"].get(row["row"])
        if per is not None:
            assert row["OIS"] == ods_ois([[per[i]["best_f"]] for i in doc["ids"]], [0])["OIS"]
            assert row["ODS"] == ods_ois([[per[i]["f_at_ods"]] for i in doc["ids"]], [0])["ODS"]
            assert row["step"] == -(-(max(per[i]["map_max"] for i in doc["ids"]) + 1) // 256)
    fgq = json.load(open(os.path.join(HERE, "..", "profiles", "feature_gradient_quality.json")))
    for old in fgq["rows"]:                                  # the G rows are the figures already on record
        new = [r for r in doc["rows"] if r["row"] == "G_%s_s%g" % (old["bank"], old["smoothing"])][0]
        assert new["ODS"] == old["ODS"] and new["OIS"] == old["OIS"] and new["step"] == old["step"]


def test_quality_scores_of_the_first_six_images_are_reproduced():
    """Colour bank, no smoothing, k = 8, r = 8: the E maps from the restatements, the scores from ``evaluate.edge_scores`` at the
    row's ODS threshold and at every image's best one."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    import texton_gradient_quality as tool
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(QUALITY))
    name = tool.row_name("E", "colour", 0.0, 8, 8)
    row = [r for r in doc["rows"] if r["row"] == name][0]
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    for i in doc["ids"][:6]:
        want = doc["per_image"][name][i]
        e = tool.image_maps(val["img_" + i], "colour", 0.0, ks=(8,), radii=(8,))[name]
        assert int(e.max()) == want["map_max"]
        sc = edge_scores(e, truth[i], [row["ODS_threshold"], want["best_threshold"]])
        for key, got in (("f_at_ods", sc["fmeasure"][0]), ("recall_at_ods", sc["recall"][0]),
                         ("precision_at_ods", sc["precision"][0]), ("best_f", sc["fmeasure"][1])):
            assert abs(got - want[key]) <= 1e-12, (i, key, got, want[key])
