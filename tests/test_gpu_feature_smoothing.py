"""GPU smoothing of the feature levels (SPEC.md §10): gcs_smooth_features and Segmenter(smoothing=K) against the NumPy
restatement (tests/smooth_ref.py), bit for bit - the smoothed slab read back through gcs_features_unpack for split and wide slabs,
packed edge strips and levels smaller than the radius, the flag words of the split slab, labels on every call path, the
composition with min_region_size, and the scores of the 24 val fixture images."""
import os

import numpy as np
import pytest

import smooth_ref as sr
from oracle import c_oracle as co
from oracle import spec_oracle as so
from slab_layout import flag_bytes as _flags, tile_of_pixels as _tile_of_pixels

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
K_MAX = 4.525483399593902          # the largest K the 4x6 (and 8x8) bank accepts: radius 24 on the odd scales


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _synth(b, h, w, seed):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    return synthetic_batch(b, h, w, seed=seed)


_RAW = {}


def _raw_features(img, ns, no):
    key = (img.tobytes(), img.shape, ns, no)
    if key not in _RAW:
        tapq, shift = so.bank(ns, no)
        _RAW[key] = co.gabor_features(img, tapq, shift, no)
    return _RAW[key]


def _device_features(torch, seg, imgs):
    """Gabor stage + smoothing on the device -> (slab, canonical (B, D, H, W) uint16)."""
    b, h, w, _ = imgs.shape
    feats = seg.ops.feature_slab(b, h, w)
    seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
    seg.ops.smooth_features(feats, b, h, w)
    return feats, seg.ops.features_unpack(feats, b, h, w).cpu().numpy().view(np.uint16)


def _check_features(torch, imgs, ns, no, K):
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(n_scales=ns, n_orient=no, smoothing=K)
    _, got = _device_features(torch, seg, imgs)
    for i in range(len(imgs)):
        want = sr.smooth_features(_raw_features(imgs[i], ns, no), K, ns, no)
        assert np.array_equal(got[i], want), (imgs.shape, ns, no, K, i, int((got[i] != want).sum()))


BANKS = [(4, 6), (8, 8), (2, 6), (5, 6)]          # split 2 levels, wide 4 levels, 1 level, 3 levels


@pytest.mark.parametrize("ns,no", BANKS)
@pytest.mark.parametrize("K", [0.5, 1.0, 3.0, K_MAX])
def test_smoothed_slab_small_shapes(torch_cuda, ns, no, K):
    """8x8 (a 4x4 level 1 and 1x1 level 3 under radii up to 24), 9x13 and 17x8 (packed strips for two-level banks), 64x64."""
    for h, w in ((8, 8), (9, 13), (17, 8), (64, 64)):
        _check_features(torch_cuda, _synth(2, h, w, seed=h * w), ns, no, K)


@pytest.mark.parametrize("h,w", [(321, 481), (481, 321)])
@pytest.mark.parametrize("K", [0.5, 1.0, 3.0, K_MAX])
def test_smoothed_slab_bsd_shapes(torch_cuda, h, w, K):
    _check_features(torch_cuda, _synth(2, h, w, seed=7), 4, 6, K)


@pytest.mark.parametrize("ns,no", [(8, 8), (2, 6), (5, 6)])
def test_smoothed_slab_bsd_shape_other_banks(torch_cuda, ns, no):
    _check_features(torch_cuda, _synth(1, 321, 481, seed=8), ns, no, 1.0)


def test_invalid_device_taps_leave_the_slab_as_it_is(torch_cuda):
    """The kernels check every scale's radius and tap sum on the device: a scale that fails is left unsmoothed."""
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    torch = torch_cuda
    imgs = _synth(1, 40, 56, seed=3)
    seg = Segmenter(smoothing=1.0)
    b, h, w, _ = imgs.shape
    raw = seg.ops.feature_slab(b, h, w)
    seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), raw)
    before = raw.clone()
    taps, radius = sr.taps_array(1.0)
    taps[1, 24] += 1                                          # scale 1 sums to 4097
    radius[2] = 25                                            # scale 2 out of range
    t, r = torch.from_numpy(taps).cuda(), torch.from_numpy(radius).cuda()
    ws = seg.ops.smooth_scratch(b, h, w)
    _lib.check(seg.ops.lib.gcs_smooth_features(raw.data_ptr(), b, h, w, 4, 6, t.data_ptr(), r.data_ptr(), ws.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "gcs_smooth_features")
    got = seg.ops.features_unpack(raw, b, h, w).cpu().numpy().view(np.uint16)[0]
    ref = seg.ops.features_unpack(before, b, h, w).cpu().numpy().view(np.uint16)[0]
    sm = sr.smooth_features(ref, 1.0, 4, 6)
    for d in range(72):
        s = (d % 24) // 6
        assert np.array_equal(got[d], ref[d] if s in (1, 2) else sm[d]), d


# ---- flag words of the split slab

def _grating(h, w, f=0.4):
    xx = np.mgrid[0:h, 0:w][1]
    g = np.where(np.sin(2 * np.pi * f * xx) >= 0, 255, 0).astype(np.uint8)
    return np.stack([g, g, g], -1)


def _with_patch(img, y0, x0, size=16):
    out = img.copy()
    y0, x0 = min(y0, img.shape[0] - size), min(x0, img.shape[1] - size)
    out[y0:y0 + size, x0:x0 + size] = _grating(size, size)
    return out


@pytest.mark.parametrize("h,w", [(64, 96), (81, 121), (321, 481)])
def test_flag_words_after_smoothing(torch_cuda, h, w):
    """A tile's flag word is non-zero exactly where a smoothed value of the tile is 4096 or more; its byte L exactly where one of
    level L is. A full-contrast grating has every tile flagged before smoothing; a 3x3 patch loses its flags to it."""
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    base = _synth(3, h, w, seed=201)
    imgs = np.stack([base[0], _grating(h, w), _with_patch(base[1], h // 3, w // 4), _with_patch(base[2], h - 16, w - 16),
                     _with_patch(base[0], h - 16, 3), _with_patch(base[1], 5, w - 16),
                     _with_patch(base[1], 20, 30, size=3), _with_patch(base[2], h - 3, w - 3, size=3)])
    b = len(imgs)
    tile = _tile_of_pixels(h, w)
    seg0 = Segmenter()
    raw = seg0.ops.feature_slab(b, h, w)
    seg0.ops.gabor_features(torch.from_numpy(imgs).cuda(), raw)
    flags0, ntiles = _flags(seg0, raw, b, h, w)
    seg = Segmenter(smoothing=1.0)
    feats, got = _device_features(torch, seg, imgs)
    flags, _ = _flags(seg, feats, b, h, w)
    assert tile.max() + 1 == ntiles
    cleared = []
    for i in range(b):
        want = sr.smooth_features(_raw_features(imgs[i], 4, 6), 1.0, 4, 6)
        assert np.array_equal(got[i], want), i
        for L, rows in ((0, [c * 24 + f for c in range(3) for f in range(12)]), (1, [c * 24 + f for c in range(3) for f in range(12, 24)])):
            wl = np.zeros(ntiles, bool)
            wl[np.unique(tile[(want[rows] >= 4096).any(axis=0)])] = True
            assert np.array_equal(flags[i, :, L] != 0, wl), (i, L)
        assert not flags[i, :, 2:].any()
        cleared.append(int(((flags0[i] != 0).any(axis=1) & ~(flags[i] != 0).any(axis=1)).sum()))
    assert (flags0[1] != 0).any(axis=1).all()                                            # the grating: every tile flagged before
    assert cleared[6] > 0, cleared               # a 3x3 patch: a few values >= 4096 before smoothing, none after


# ---- labels and call paths

@pytest.mark.parametrize("mode", ["per_image", "global"])
@pytest.mark.parametrize("k", [1, 8, 16])
def test_labels_both_codebook_modes(torch_cuda, mode, k):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(3, 97, 131, seed=k)
    got = Segmenter(k=k, smoothing=1.0).segment_batch(imgs, mode)
    assert np.array_equal(got, sr.segment_batch(imgs, 1.0, k=k, mode=mode))


def test_labels_deep_bank_full_size(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(2, 321, 481, seed=12)
    got = Segmenter(n_scales=8, n_orient=8, smoothing=1.5).segment_batch(imgs)
    assert np.array_equal(got, sr.segment_batch(imgs, 1.5, n_scales=8, n_orient=8))


def test_batch_64_global_codebook_every_label(torch_cuda):
    """The timed configuration's shape at K = 1 (global codebook, 64 x 481x321): every label against the C oracle on the
    restated features."""
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _synth(64, 321, 481, seed=0)
    got = Segmenter(smoothing=1.0).segment_batch(imgs, "global")
    x = np.stack([sr.smooth_features(_raw_features(im, 4, 6), 1.0, 4, 6) for im in imgs]).reshape(64, 72, -1)
    want = co.kmeans(x, 8, 10)[0].reshape(64, 321, 481)
    assert np.array_equal(got, want), int((got != want).sum())


def test_every_call_path_agrees(torch_cuda):
    """segment == the row of segment_batch (graph path and the chunked fast path) == segment_stream == segment_images ==
    segment_device; graph replay == eager; features_device == the restatement; smoothing=0 == no argument."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, segment, segment_batch, segment_images
    imgs = _synth(8, 321, 481, seed=21)                       # 8 x 481x321 > 2^20 pixels: segment_batch's chunked fast path
    want = sr.segment_batch(imgs, 1.0)
    seg = Segmenter(smoothing=1.0)
    assert np.array_equal(seg.segment_batch(imgs), want)
    assert np.array_equal(segment_batch(imgs[:2], smoothing=1.0), want[:2])          # graph path
    assert np.array_equal(segment(imgs[3], smoothing=1.0), want[3])
    assert np.array_equal(seg.segment_device(torch.from_numpy(imgs).cuda()).cpu().numpy(), want)
    outs = list(seg.segment_stream([imgs[:4], imgs[4:]]))
    assert np.array_equal(np.concatenate(outs), want)
    mixed = [imgs[0], np.ascontiguousarray(imgs[1].transpose(1, 0, 2)), imgs[2]]
    got = list(segment_images(mixed, batch=2, smoothing=1.0))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], sr.segment(mixed[1], 1.0))
    for i in range(8):
        assert np.array_equal(seg(imgs[i]), want[i])                                   # replayed graph
    eager = Segmenter(smoothing=1.0)
    eager.debug.no_graph = True
    assert np.array_equal(eager.segment_batch(imgs[:1]), want[:1])
    f = seg.features_device(torch.from_numpy(imgs[:2]).cuda()).cpu().numpy().view(np.uint16)
    for i in range(2):
        assert np.array_equal(f[i], sr.features(imgs[i], 1.0))
    plain = Segmenter().segment_batch(imgs[:2])
    assert np.array_equal(Segmenter(smoothing=0).segment_batch(imgs[:2]), plain)
    assert np.array_equal(segment(imgs[0], smoothing=0.0), plain[0])
    assert not np.array_equal(plain, want[:2])


def test_smoothing_with_min_region_size(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    from merge_ref import merge_small_regions
    imgs = _synth(2, 321, 481, seed=31)
    got = Segmenter(smoothing=1.0, min_region_size=64).segment_batch(imgs)
    for i in range(2):
        assert np.array_equal(got[i], merge_small_regions(sr.segment(imgs[i], 1.0), 64)), i


# means over the 24 val fixture images of boundary F, PRI, VoI, covering, from the restatement on the CPU
QUALITY_24 = {
    1.0: (0.2812788924107641, 0.6905625948486281, 3.813324555123767, 0.28788706526325997),
    1.5: (0.2781950999461324, 0.6967866589453166, 3.7558760227527532, 0.29045117037477725),
}


@pytest.mark.parametrize("K", [1.0, 1.5])
def test_quality_on_the_val_fixture_through_the_gpu(torch_cuda, K):
    """The 24 val images through Segmenter(smoothing=K) and the batched GPU scorer: the restatement's labels, and its means."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"]]
    seg = Segmenter(smoothing=K)
    rows = {}
    for shape in ((321, 481), (481, 321)):
        group = [i for i in ids if val["img_" + i].shape[:2] == shape]
        labs = seg.segment_batch(np.stack([val["img_" + i] for i in group]))
        scores = all_scores_batch_device(torch.from_numpy(labs).cuda(), pt.to_device(group), agreement=True)
        for i, lab, sc in zip(group, labs, scores):
            assert np.array_equal(lab, sr.segment(val["img_" + i], K)), i
            rows[i] = [sc["fmeasure"], sc["PRI"], sc["VoI"], sc["covering"]]
    got = np.mean([rows[i] for i in ids], axis=0)
    assert np.all(np.abs(got - np.array(QUALITY_24[K])) <= 1e-12), got.tolist()
