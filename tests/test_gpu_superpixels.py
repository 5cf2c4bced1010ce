"""GPU superpixels (SPEC.md §13): gcs_superpixel_segment and Segmenter(n_superpixels=n) against the NumPy restatement
(tests/superpixel_ref.py on the features of tests/position_ref.py), bit for bit and never against the GPU's own output: labels and
centres over shapes, grids, weights and banks, hot banks (features up to 46 339: the 64-bit distance), batches, the compositions
with connectivity and min_region_size, every host path, graph replay, n_superpixels = 0, and the scores of the 24 val fixture
images against the numbers tools/superpixel_quality.py wrote (profiles/superpixel_quality.json)."""
import json
import os

import numpy as np
import pytest

import position_ref as pr
import superpixel_ref as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)          # the recommended bank of the quality table
COLOUR_REF = dict(w=0.125, g=4, n_orient=5)


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _synth(b, h, w, seed):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    return synthetic_batch(b, h, w, seed=seed)


def _check(torch, seg, imgs, n, lam, n_iter, ref_kw):
    """Labels and centres of ``superpixels_device`` == the restatement's, image by image."""
    lab, cen = seg.superpixels_device(torch.from_numpy(imgs).cuda())
    lab, cen = lab.cpu().numpy(), cen.cpu().numpy()
    assert lab.dtype == np.int32 and cen.dtype == np.int32
    for i, im in enumerate(imgs):
        want, wc = sr.segment(im, n, lam=lam, n_iter=n_iter, return_centres=True, **ref_kw)
        assert cen[i].shape == wc.shape, (cen[i].shape, wc.shape)
        assert np.array_equal(lab[i], want), (i, n, lam, int((lab[i] != want).sum()))
        assert np.array_equal(cen[i], wc), (i, n, lam, int((cen[i] != wc).sum()))
    return lab


@pytest.mark.parametrize("n", [2, 64, 300, 1200])
@pytest.mark.parametrize("lam", [1, 576, 65535])
def test_small_odd_shape_every_grid_and_weight(torch_cuda, n, lam):
    """37 x 53: n = 2 is a 1 x 2 grid (ny = 1), n = 1200 has S = 1 and 1961 one-pixel cells (the tiles then see more centres than
    they hold in LDS: the global-memory form of the pass)."""
    from gabor_color_image_segmentation_amd import Segmenter
    assert sr.grid(37, 53, 2)[1:] == (1, 2) and sr.grid(37, 53, 1200) == (1, 37, 53)
    seg = Segmenter(n_superpixels=n, spatial_weight=lam, n_iter=5)
    _check(torch_cuda, seg, _synth(2, 37, 53, seed=n + lam), n, lam, 5, {})


@pytest.mark.parametrize("h,wd,n", [(16, 200, 8), (200, 9, 5), (96, 130, 64), (96, 130, 1200), (130, 96, 300)])
def test_strips_and_mid_shapes(torch_cuda, h, wd, n):
    """A one-row grid (16 x 200, n = 8), a one-column grid (200 x 9), and shapes whose tiles hold several cells."""
    from gabor_color_image_segmentation_amd import Segmenter
    _, ny, nx = sr.grid(h, wd, n)
    if (h, wd) == (16, 200):
        assert ny == 1 and nx > 1
    if (h, wd) == (200, 9):
        assert nx == 1 and ny > 1
    seg = Segmenter(n_superpixels=n, n_iter=6, **COLOUR)
    _check(torch_cuda, seg, _synth(2, h, wd, seed=h), n, 576, 6, COLOUR_REF)


@pytest.mark.parametrize("h,wd,n,lam,bank,ref", [
    (321, 481, 300, 576, COLOUR, COLOUR_REF),
    (481, 321, 300, 576, COLOUR, COLOUR_REF),
    (481, 321, 1200, 1, {}, {}),
    (321, 481, 64, 65535, {}, {}),
    (321, 481, 2, 576, dict(n_orient=4, color_weight=0.125, chroma_gain=4, position_weight=6), dict(w=0.125, g=4, mu=6, n_orient=4)),
    (481, 321, 300, 2304, dict(smoothing=1.0), dict(smoothing=1.0)),
])
def test_bsd_shapes_and_banks(torch_cuda, h, wd, n, lam, bank, ref):
    """Both BSD orientations; the default bank, the colour bank, a bank with the coordinate slot, smoothing = 1."""
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(n_superpixels=n, spatial_weight=lam, n_iter=4, **bank)
    _check(torch_cuda, seg, _synth(1, h, wd, seed=n), n, lam, 4, ref)


def test_batch_of_mixed_content_keeps_its_centres_apart(torch_cuda):
    """B = 5 images of different content in one call: every image equals its own single-image reference (and the maps differ)."""
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(5, 72, 104, seed=11)
    imgs[1] = 255 - imgs[1]
    imgs[3] = imgs[3][::-1]
    seg = Segmenter(n_superpixels=64, n_iter=6)
    lab = _check(torch_cuda, seg, imgs, 64, 576, 6, {})
    assert not np.array_equal(lab[0], lab[1]) and not np.array_equal(lab[2], lab[3])


@pytest.mark.parametrize("cfg,h,wd,n,lam", [((4, 6, 13, 8), 72, 104, 64, 1), ((4, 6, 13, 7), 81, 121, 300, 576),
                                           ((2, 3, 7, 7), 64, 96, 64, 65535)])
def test_hot_banks_use_the_whole_64_bit_distance(torch_cuda, cfg, h, wd, n, lam):
    """Features up to 46 339 (tests/hot_banks.py): squared differences near 2^31 per plane, distances far beyond 2^32."""
    import hot_banks as hb
    from oracle import c_oracle as co
    torch = torch_cuda
    bank = hb.hot_bank(*cfg)
    seg = hb.hot_segmenter(bank, n_superpixels=n, spatial_weight=lam, n_iter=5)
    imgs = hb.hot_images(8, h, wd, seed=h + wd)
    lab, cen = seg.superpixels_device(torch.from_numpy(imgs).cuda())
    lab, cen = lab.cpu().numpy(), cen.cpu().numpy()
    top = 0
    for i, im in enumerate(imgs):
        x = co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient)
        top = max(top, int(x.max()))
        want, wc = sr.superpixels(x, n, lam, 5, return_centres=True)
        assert np.array_equal(lab[i], want), (i, int((lab[i] != want).sum()))
        assert np.array_equal(cen[i], wc), i
    # (a shift-8 bank cannot pass 36 635, the ceiling include/gcs.h states for it; the shift-7 banks reach beyond 40 000)
    assert top > (36000 if cfg[3] == 8 else 40000), top


def test_raw_entry_point_refuses_what_is_outside_the_domain(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    b, d, h, w = 1, 6, 16, 24
    x = torch.zeros((b, d, h, w), dtype=torch.int16, device="cuda")
    ws = torch.zeros(lib.gcs_superpixel_workspace_bytes(b, h, w, d, 6), dtype=torch.uint8, device="cuda")
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = dict(feats=x.data_ptr(), B=b, H=h, W=w, D=d, ny=2, nx=3, lam=576, n_iter=3, ws=ws.data_ptr(), out=out.data_ptr())
    for bad in (dict(feats=None), dict(ws=None), dict(out=None), dict(B=0), dict(H=0), dict(W=4097), dict(D=0), dict(D=208),
                dict(ny=0), dict(ny=17), dict(nx=25), dict(lam=0), dict(lam=65536), dict(n_iter=0)):
        a = dict(good, **bad)
        rc = lib.gcs_superpixel_segment(a["feats"], a["B"], a["H"], a["W"], a["D"], a["ny"], a["nx"], a["lam"], a["n_iter"], a["ws"],
                                        a["out"], None, st)
        assert rc == 1, bad
    torch.cuda.current_stream().synchronize()
    assert int((out != -7).sum()) == 0                                  # nothing was launched
    assert lib.gcs_superpixel_workspace_bytes(1, 90, 90, 72, 4096) == 0     # S = 1: 90 x 90 centres
    assert lib.gcs_superpixel_workspace_bytes(1, 37, 53, 208, 64) == 0
    a = good
    assert lib.gcs_superpixel_segment(a["feats"], b, h, w, d, 2, 3, 576, 3, a["ws"], a["out"], None, st) == 0
    torch.cuda.current_stream().synchronize()
    got = out.cpu().numpy()[0]
    assert np.array_equal(got, sr.superpixels(np.zeros((d, h, w), np.uint16), 6, 576, 3))


def test_grid_helper_is_the_restated_grid(built):
    import ctypes as C
    from gabor_color_image_segmentation_amd import _lib, superpixel_grid
    lib = _lib.load()
    rng = np.random.default_rng(5)
    cases = [(321, 481, 300), (481, 321, 300), (8, 8, 64), (37, 53, 2), (50, 50, 1000), (9, 9, 36)]       # (9 x 9 / 36: sqrt = 1.5)
    cases += [(int(rng.integers(1, 600)), int(rng.integers(1, 600)), int(rng.integers(2, 4097))) for _ in range(300)]
    for h, w, n in cases:
        s, ny, nx = C.c_int(), C.c_int(), C.c_int()
        assert lib.gcs_superpixel_grid(h, w, n, C.byref(s), C.byref(ny), C.byref(nx)) == 0
        s0 = max(1, int(np.rint(np.sqrt(np.float64(h * w) / n))))
        want = (s0, max(1, int(np.rint(np.float64(h) / s0))), max(1, int(np.rint(np.float64(w) / s0))))
        assert (s.value, ny.value, nx.value) == want == superpixel_grid(h, w, n), (h, w, n)


# ---- compositions and host paths

def test_post_passes_on_top_of_the_superpixel_map(torch_cuda):
    """min_region_size = S^2 / 4 == merge_ref.merge_small_regions of the reference labels; connectivity=True == §7 of them."""
    from merge_ref import merge_small_regions
    from oracle import spec_oracle as so
    from gabor_color_image_segmentation_amd import Segmenter
    for h, wd in ((96, 130), (321, 481)):
        imgs = _synth(2, h, wd, seed=21)
        s = sr.grid(h, wd, 300)[0]
        ref = [sr.segment(im, 300, n_iter=4, **COLOUR_REF) for im in imgs]
        got = Segmenter(n_superpixels=300, n_iter=4, min_region_size=s * s // 4, **COLOUR).segment_batch(imgs)
        conn = Segmenter(n_superpixels=300, n_iter=4, connectivity=True, **COLOUR).segment_batch(imgs)
        for i in range(2):
            assert np.array_equal(got[i], merge_small_regions(ref[i], s * s // 4)), (h, wd, i)
            assert np.array_equal(conn[i], so.connected_regions(ref[i])), (h, wd, i)


def test_every_host_path_and_graph_replay(torch_cuda):
    """segment, segment_batch (graph replay and eager), segment_images with mixed shapes, segment_stream, uint8 output."""
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.segmenter import DebugSwitches
    kw = dict(n_superpixels=64, spatial_weight=144, n_iter=4)
    a, b = _synth(3, 72, 104, seed=1), _synth(2, 104, 72, seed=2)
    ref_a = np.stack([sr.segment(im, 64, lam=144, n_iter=4) for im in a])
    ref_b = np.stack([sr.segment(im, 64, lam=144, n_iter=4) for im in b])
    seg = Segmenter(**kw)
    assert np.array_equal(seg(a[0]), ref_a[0])
    assert np.array_equal(pkg.segment(a[1], **kw), ref_a[1])
    first = seg.segment_batch(a)
    assert first.dtype == np.int32 and np.array_equal(first, ref_a)
    assert any(e["graph"] is not None for e in seg._graphs.values())              # the small call was captured ...
    assert np.array_equal(seg.segment_batch(a[::-1].copy()), ref_a[::-1])         # ... and its replay follows the new input
    eager = Segmenter(**kw)
    eager.debug = DebugSwitches("no_graph")
    assert np.array_equal(eager.segment_batch(a), ref_a) and not eager._graphs
    u8 = seg.segment_batch(a, out_dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, ref_a)
    mixed = [a[0], b[0], a[1], b[1], a[2]]
    got = list(seg.segment_images(mixed, batch=2))
    for g, want in zip(got, [ref_a[0], ref_b[0], ref_a[1], ref_b[1], ref_a[2]]):
        assert np.array_equal(g, want)
    got = list(pkg.segment_images(mixed, batch=3, **kw))
    assert np.array_equal(got[3], ref_b[1])
    outs = list(seg.segment_stream([a, a[::-1].copy(), a]))
    assert len(outs) == 3 and np.array_equal(outs[0], ref_a) and np.array_equal(outs[1], ref_a[::-1]) and np.array_equal(outs[2], ref_a)
    big = np.concatenate([_synth(1, 321, 481, seed=s) for s in range(8)])       # more than the graph limit: the plain path
    lab = seg.segment_batch(big)
    for i in (0, 7):
        assert np.array_equal(lab[i], sr.segment(big[i], 64, lam=144, n_iter=4)), i


def test_n_superpixels_zero_is_the_plan_without_the_argument(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    from oracle import spec_oracle
    small, big = _synth(2, 72, 104, seed=3), _synth(8, 321, 481, seed=4)
    off, plain = Segmenter(n_superpixels=0, spatial_weight=99, n_iter=4), Segmenter(n_iter=4)
    for imgs in (small, big):
        assert np.array_equal(off.segment_batch(imgs), plain.segment_batch(imgs))
        dev = torch.from_numpy(imgs).cuda()
        assert torch.equal(off.segment_device(dev), plain.segment_device(dev))
    assert np.array_equal(off(small[0]), spec_oracle.segment(small[0], n_iter=4))


def test_value_errors_on_the_device(torch_cuda):
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(n_superpixels=300)
    dev = torch.from_numpy(_synth(1, 72, 104, seed=0)).cuda()
    with pytest.raises(ValueError):
        seg.segment_device(dev, mode="global")
    with pytest.raises(ValueError):
        seg.segment_batch(dev.cpu().numpy(), out_dtype=np.uint8)           # 300 -> more than 256 centres
    with pytest.raises(ValueError):
        seg.segment_rows_sharded_device(dev, 0, 72, 0, 72)
    with pytest.raises(ValueError):
        Segmenter(n_superpixels=4096).segment_batch(_synth(1, 90, 90, seed=0))       # S = 1: 90 x 90 centres


def test_quality_on_the_val_fixture_through_the_gpu(torch_cuda):
    """The 24 val images at the recommended setting through Segmenter and the batched GPU scorer against the per-image numbers of
    tools/superpixel_quality.py (CPU restatement, ``evaluate.metrics``). The labels are compared bit for bit on six images; the
    scores with ``==`` where the GPU scorer and the host mirror run the same float operations (recall, precision, F, density,
    regions) and to 1e-12 for underseg, undersegNP, compactness, PRI, VoI and covering, whose sums the scorer takes in another
    order (the distance tests/test_gpu_scoring.py and tests/test_gpu_region_agreement.py state for these keys)."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(os.path.join(HERE, "..", "profiles", "superpixel_quality.json")))
    rec = doc["recommended"]
    assert (rec["bank"], rec["n_superpixels"]) == ("colour", 300)
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"]]
    assert ids == doc["ids"]
    for state, post in (("raw", {}), ("merged", dict(min_region_size=sr.grid(321, 481, 300)[0] ** 2 // 4))):
        seg = Segmenter(n_superpixels=300, spatial_weight=rec["spatial_weight"], **COLOUR, **post)
        labs = dict(zip(ids, seg.segment_images([val["img_" + i] for i in ids], batch=16)))
        if state == "raw":
            for i in ids[:6]:
                assert np.array_equal(labs[i], sr.segment(val["img_" + i], 300, lam=rec["spatial_weight"], **COLOUR_REF)), i
        rows = {}
        for shape in ((321, 481), (481, 321)):
            group = [i for i in ids if val["img_" + i].shape[:2] == shape]
            scores = all_scores_batch_device(torch.from_numpy(np.stack([labs[i] for i in group])).cuda(), pt.to_device(group),
                                             agreement=True)
            rows.update(zip(group, scores))
        for i in ids:
            want, got = doc["recommended_per_image"][state][i], rows[i]
            print(state, i, {k: got[k] for k in ("recall", "underseg", "compactness", "regions")})
            for key in ("recall", "precision", "fmeasure", "density", "regions"):
                assert got[key] == want[key], (state, i, key, got[key], want[key])
            for key in ("underseg", "undersegNP", "compactness", "PRI", "VoI", "covering"):
                assert abs(got[key] - want[key]) <= 1e-12, (state, i, key, got[key], want[key])
        row = [r for r in doc["rows"] if (r["bank"], r["n_superpixels"], r["spatial_weight"], r["merge"]) ==
               ("colour", 300, rec["spatial_weight"], int(state == "merged"))][0]
        keys = ("recall", "precision", "fmeasure", "underseg", "undersegNP", "compactness", "density", "PRI", "VoI", "covering",
                "regions", "regions")                                    # (the tool's table: 24 rows x 12 columns, mean over axis 0)
        mean = np.array([[float(rows[i][k]) for k in keys] for i in ids]).mean(axis=0)
        for j in (0, 1, 2, 6, 10):
            assert float(mean[j]) == row[keys[j]], (state, keys[j], float(mean[j]), row[keys[j]])
        for j in (3, 4, 5, 7, 8, 9):
            assert abs(float(mean[j]) - row[keys[j]]) <= 1e-12, (state, keys[j])
