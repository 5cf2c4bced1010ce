"""Small-region merging (SPEC.md §9) on the CPU: the NumPy restatement (tests/merge_ref.py) against the rule's stated
properties and hand-built cases, its quality on the 24 val fixture maps, the Segmenter plumbing of ``min_region_size`` through
a CPU stand-in, and the host-only argument checks of gcs_merge_small_regions (nothing is launched)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gabor_color_image_segmentation_amd import Segmenter, _lib, make_bank
from gabor_color_image_segmentation_amd.evaluate import boundary_scores, region_agreement
from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
from oracle import spec_oracle as so
from fake_ops import OracleOps
from merge_ref import merge_small_regions, round_bound

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def checkerboard(h, w):
    return (np.arange(h)[:, None] + np.arange(w)[None, :]) % 2


# ---- the restatement against the rule

def test_m_zero_and_one_are_the_connected_regions():
    rng = np.random.default_rng(0)
    for _ in range(5):
        lab = rng.integers(0, 4, (23, 31))
        for m in (0, 1):
            out, rounds = merge_small_regions(lab, m, return_rounds=True)
            assert np.array_equal(out, so.connected_regions(lab)) and rounds == 0


def test_regions_are_connected_and_large_enough():
    rng = np.random.default_rng(1)
    for trial in range(12):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        lab = rng.integers(0, int(rng.integers(1, 6)), (h, w))
        for m in (2, 3, 7, 30, 200):
            out = merge_small_regions(lab, m)
            assert np.array_equal(so.connected_regions(out), out)      # 4-connected, numbered in raster order of first pixel
            sizes = np.bincount(out.ravel())
            assert sizes.size == 1 or sizes.min() >= m


def test_rounds_stay_under_the_halving_bound():
    rng = np.random.default_rng(2)
    worst = 0
    for _ in range(10):
        h, w = int(rng.integers(2, 60)), int(rng.integers(2, 60))
        lab = rng.integers(0, 3, (h, w))
        for m in (2, 5, 50, 500):
            _, rounds = merge_small_regions(lab, m, return_rounds=True)
            assert rounds <= round_bound(h, w)
            worst = max(worst, rounds)
    assert worst >= 2
    assert round_bound(321, 481) == 18


# ---- hand-built cases

def test_a_speckle_is_absorbed():
    lab = np.zeros((9, 11), int)
    lab[4, 5] = 3
    assert np.array_equal(merge_small_regions(lab, 2), np.zeros((9, 11)))


def test_a_sliver_joins_the_larger_neighbour():
    lab = np.zeros((5, 10), int)
    lab[:, 6] = 1
    lab[:, 7:] = 2                                   # left 30 px, sliver 5 px, right 15 px
    want = np.zeros((5, 10), int)
    want[:, 7:] = 1
    assert np.array_equal(merge_small_regions(lab, 6), want)


def test_an_equal_size_tie_goes_to_the_earlier_first_pixel():
    lab = np.zeros((5, 5), int)
    lab[:, 2] = 1
    lab[:, 3:] = 2                                   # 10 | 5 | 10 pixels: the left block's first pixel comes first
    want = np.zeros((5, 5), int)
    want[:, 3:] = 1
    assert np.array_equal(merge_small_regions(lab, 6), want)
    lab = np.zeros((5, 5), int)
    lab[2] = 1
    lab[3:] = 2                                      # the same on its side: the upper block wins
    want = np.zeros((5, 5), int)
    want[3:] = 1
    assert np.array_equal(merge_small_regions(lab, 6), want)


def test_a_mutual_pair_of_small_regions_merges():
    out, rounds = merge_small_regions(np.array([[0, 0, 1, 1]]), 3, return_rounds=True)
    assert np.array_equal(out, np.zeros((1, 4))) and rounds == 1


def test_a_checkerboard_becomes_one_region_in_one_round():
    """Every pixel is a one-pixel region; each picks its earliest neighbour, so the picks chain all H*W of them."""
    out, rounds = merge_small_regions(checkerboard(13, 17), 2, return_rounds=True)
    assert np.array_equal(out, np.zeros((13, 17))) and rounds == 1


def test_an_image_smaller_than_m_is_one_region():
    lab = np.random.default_rng(3).integers(0, 3, (6, 7))
    assert np.array_equal(merge_small_regions(lab, 1000), np.zeros((6, 7)))
    assert np.array_equal(merge_small_regions(np.full((4, 4), 5), 1000), np.zeros((4, 4)))


# ---- quality on the 24 val fixture maps

QUALITY = {   # m: mean boundary F, PRI, VoI (bits), covering over the 24 images
    16: (0.2825945472876316, 0.7465096833468765, 4.798808535311168, 0.3155085872355758),
    64: (0.28713012644066394, 0.7489320336025673, 4.167163441853922, 0.33516694309554346),
    256: (0.28539396059249167, 0.751872995298332, 3.374831979884572, 0.36974508924837046),
}


def test_quality_on_the_val_fixture_maps():
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    assert len(val["ids"]) == 24
    for m, want in QUALITY.items():
        rows = []
        for i in val["ids"]:
            i = str(i)
            out = merge_small_regions(val["labels_" + i], m)
            bs, ra = boundary_scores(out, pt[i]), region_agreement(out, pt[i])
            rows.append([bs["fmeasure"], ra["PRI"], ra["VoI"], ra["covering"]])
        got = np.mean(rows, axis=0)
        assert np.all(np.abs(got - np.array(want)) <= 1e-12), (m, got.tolist())


# ---- Segmenter plumbing through a CPU stand-in

class MergeOps(OracleOps):
    def merge_small_regions(self, labels_i32, min_size, out):
        self.calls.append(("merge", int(min_size)))
        out.copy_(torch.from_numpy(np.stack([merge_small_regions(l, min_size) for l in labels_i32.numpy()]).astype(np.int32)))


def _seg(**kw):
    return Segmenter(ops=MergeOps(make_bank()), n_iter=3, **kw)


def test_min_region_size_one_equals_connectivity():
    imgs = synthetic_batch(2, 24, 40, seed=9)
    got = _seg(min_region_size=1).segment_batch(imgs)
    assert np.array_equal(got, _seg(connectivity=True).segment_batch(imgs))
    assert got.dtype == np.int32


def test_min_region_size_zero_is_the_plain_output():
    imgs = synthetic_batch(2, 24, 40, seed=9)
    seg = _seg(min_region_size=0)
    got = seg.segment_device(torch.from_numpy(imgs)).numpy()
    for b in range(2):
        assert np.array_equal(got[b], so.segment(imgs[b], n_iter=3))
    assert not any(c[0] == "merge" for c in seg.ops.calls)


def test_min_region_size_merges_after_the_lloyd_passes():
    imgs = synthetic_batch(3, 24, 40, seed=4)
    seg = _seg(min_region_size=20)
    got = seg.segment_batch(imgs)
    for b in range(3):
        assert np.array_equal(got[b], merge_small_regions(so.segment(imgs[b], n_iter=3), 20))
    assert ("merge", 20) in seg.ops.calls
    ims = [imgs[0], imgs[1][:16], imgs[2]]
    for im, lab in zip(ims, seg.segment_images(ims, batch=2)):
        assert np.array_equal(lab, merge_small_regions(so.segment(im, n_iter=3), 20))
    assert np.array_equal(seg(imgs[1]), got[1])


def test_min_region_size_argument_errors():
    with pytest.raises(ValueError):
        _seg(min_region_size=-1)
    with pytest.raises(ValueError):
        _seg(min_region_size=2.5)
    seg = _seg(min_region_size=16)
    imgs = synthetic_batch(1, 16, 24, seed=1)
    with pytest.raises(ValueError):
        seg.segment_batch(imgs, out_dtype=np.uint8)
    with pytest.raises(ValueError):
        list(seg.segment_images([imgs[0]], out_dtype=np.uint8))
    with pytest.raises(ValueError):
        list(seg.segment_stream([imgs], out_dtype=np.uint8))
    strip = torch.from_numpy(synthetic_batch(1, 32, 24, seed=1))
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_rows_sharded_device(strip, 0, 32, 0, 32)
    with pytest.raises(ValueError, match="row strips"):
        seg.segment_owned_rows_device(strip, 32)


# ---- C ABI: host-only checks

@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


def test_merge_entry_validates_before_launching(lib):
    one, two = C.c_void_p(16), C.c_void_p(32)               # non-NULL dummies, never dereferenced
    assert lib.gcs_merge_small_regions(None, 1, 16, 16, 4, one, two, None) == 1
    assert lib.gcs_merge_small_regions(one, 1, 16, 16, 4, None, two, None) == 1
    assert lib.gcs_merge_small_regions(one, 1, 16, 16, 4, two, None, None) == 1
    assert lib.gcs_merge_small_regions(one, 1, 16, 16, -1, two, two, None) == 1
    assert b"min_size" in lib.gcs_last_error()
    assert lib.gcs_merge_small_regions(one, 0, 16, 16, 4, two, two, None) == 1
    assert lib.gcs_merge_small_regions(one, 1, 0, 16, 4, two, two, None) == 1
    assert lib.gcs_merge_small_regions(one, 1, 65536, 65536, 4, two, two, None) == 1
    assert lib.gcs_merge_small_regions(one, 1, 16, 16, 4, two, one, None) == 1   # out aliases labels
    assert b"alias" in lib.gcs_last_error()


def test_merge_scratch_size(lib):
    assert lib.gcs_merge_scratch_bytes(2, 10, 12, 64) == 2 * 10 * 12 * 20 + 32 * 2 * 4
    assert lib.gcs_merge_scratch_bytes(64, 321, 481, 64) < 210 << 20
    for bad in ((0, 10, 12, 4), (1, 0, 12, 4), (1, 10, -1, 4), (1, 65536, 65536, 4), (1, 10, 12, -1)):
        assert lib.gcs_merge_scratch_bytes(*bad) == 0
