"""GPU small-region merging (SPEC.md §9): gcs_merge_small_regions and Segmenter(min_region_size=...) against the NumPy
restatement (tests/merge_ref.py), bit for bit."""
import os

import numpy as np
import pytest

from merge_ref import merge_small_regions

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _run(lab, m):
    import torch
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    lab = np.ascontiguousarray(lab, np.int32)
    b, h, w = lab.shape
    d = torch.from_numpy(lab).cuda()
    out = torch.full_like(d, -7)
    scratch = torch.empty(lib.gcs_merge_scratch_bytes(b, h, w, m), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gcs_merge_small_regions(d.data_ptr(), b, h, w, m, scratch.data_ptr(), out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "gcs_merge_small_regions")
    got = out.cpu().numpy()
    assert np.array_equal(d.cpu().numpy(), lab)                  # the input is left alone
    return got


def _check(lab, m):
    lab = np.asarray(lab)
    got = _run(lab, m)
    for b in range(lab.shape[0]):
        assert np.array_equal(got[b], merge_small_regions(lab[b], m)), (b, m)
    return got


def _spiral(n=101):
    lab = np.zeros((n, n), np.int32)                   # a 1-pixel-wide spiral of 1s on 0s, drawn inward from the corner
    y, x, dy, dx = 0, 0, 0, 1
    lab[0, 0] = 1
    while True:
        moved = False
        for _ in range(4):
            ny, nx = y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and lab[ny, nx] == 0 and lab[y + dy, x + dx] == 0 and \
                    not (0 <= ny + dy < n and 0 <= nx + dx < n and lab[ny + dy, nx + dx] == 1):
                lab[y + dy, x + dx] = lab[ny, nx] = 1
                y, x = ny, nx
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return lab


def _checkerboard(h, w):
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2).astype(np.int32)


@pytest.mark.parametrize("m", [2, 5, 50, 500])
def test_random_maps(built, m):
    _check(np.random.default_rng(1).integers(0, 4, (3, 97, 131)), m)


@pytest.mark.parametrize("m", [0, 1])
def test_m_le_one_is_connected_regions(built, m):
    from oracle import spec_oracle as so
    lab = np.random.default_rng(2).integers(0, 4, (2, 37, 53))
    got = _run(lab, m)
    for b in range(2):
        assert np.array_equal(got[b], so.connected_regions(lab[b]))


def test_special_images(built):
    """The checkerboard (every pixel a region: one round, one chain through all of them), a 1-pixel spiral, a single-label image
    and an image with fewer than m pixels."""
    got = _check(_checkerboard(64, 97)[None], 2)
    assert got.max() == 0
    _check(_checkerboard(31, 33)[None], 3)
    sp = _spiral()
    assert sp.sum() > 1000
    _check(sp[None], 2)
    assert _check(sp[None], 5001).max() == 0            # the 5 000-pixel background joins the spiral
    assert _check(np.full((1, 40, 50), 9), 64).max() == 0
    assert _check(np.random.default_rng(3).integers(0, 3, (1, 20, 30)), 601).max() == 0


def test_mixed_batch_images_are_independent(built):
    """One batch of different maps gives, image by image, what each gives alone."""
    rng = np.random.default_rng(4)
    h, w = 101, 101
    small = np.zeros((h, w), np.int32)
    small[:12, :20] = rng.integers(0, 3, (12, 20))
    imgs = np.stack([_checkerboard(h, w), _spiral(), np.full((h, w), 3, np.int32), rng.integers(0, 4, (h, w)), small])
    for m in (2, 40, 800):
        got = _check(imgs, m)
        for b in range(len(imgs)):
            assert np.array_equal(got[b], _run(imgs[b:b + 1], m)[0])


@pytest.mark.parametrize("m", [64, 256])
def test_val_fixture_maps(built, m):
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"]]
    for shape in sorted({val["labels_" + i].shape for i in ids}):
        _check(np.stack([val["labels_" + i] for i in ids if val["labels_" + i].shape == shape]), m)


def test_segmenter_end_to_end_on_the_fixture_images(built):
    """Segmenter(min_region_size=64) through segment_batch, segment() and segment_images: the restatement applied to the
    stored labels (which the plain path reproduces bit for bit: tests/test_gpu_golden.py)."""
    from gabor_color_image_segmentation_amd import Segmenter, segment, segment_images
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"]]
    want = {i: merge_small_regions(val["labels_" + i], 64) for i in ids}
    seg = Segmenter(min_region_size=64)
    for shape in ((321, 481), (481, 321)):
        group = [i for i in ids if val["img_" + i].shape[:2] == shape]
        got = seg.segment_batch(np.stack([val["img_" + i] for i in group]))
        assert got.dtype == np.int32
        for b, i in enumerate(group):
            assert np.array_equal(got[b], want[i]), i
    for i in ids[:3]:
        assert np.array_equal(segment(val["img_" + i], min_region_size=64), want[i]), i
    imgs = [val["img_" + i] for i in ids]
    n = 0
    for i, lab in zip(ids, segment_images(imgs, batch=5, min_region_size=64)):
        assert np.array_equal(lab, want[i]), i
        n += 1
    assert n == 24


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_full_batch_both_codebook_modes(built, mode):
    """64 synthetic 481x321 images, the plain labels merged by the restatement."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(64, 321, 481, seed=5)
    plain = Segmenter(n_iter=4).segment_batch(imgs, mode)
    got = Segmenter(n_iter=4, min_region_size=64).segment_batch(imgs, mode)
    for b in range(64):
        ref = merge_small_regions(plain[b], 64)
        assert np.array_equal(got[b], ref), b
        assert ref.max() > 0


def test_resident_scorer_on_merged_maps(built):
    """agreement=True on merged maps through the resident scorer: the host definition within the existing tolerances."""
    import torch
    from gabor_color_image_segmentation_amd.evaluate import region_agreement
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"]]
    n = 0
    for shape in sorted({val["labels_" + i].shape for i in ids}):
        group = [i for i in ids if val["labels_" + i].shape == shape]
        merged = _run(np.stack([val["labels_" + i] for i in group]), 256)
        got = all_scores_batch_device(torch.from_numpy(merged).cuda(), pt.to_device(group), agreement=True)
        for i, g, lab in zip(group, got, merged):
            ref = region_agreement(lab, pt[i])
            assert g["PRI"] == ref["PRI"], i
            for k in ("PRI", "VoI", "covering"):
                assert abs(g[k] - ref[k]) <= 1e-12, (i, k)
            assert g["regions"] == lab.max() + 1
            n += 1
    assert n == 24


# ---- the shapes that change the launch (tests/launch_shape_maps.py): P = 1, single rows / columns, P around the 1 024 threads of
# cc_rank_kernel, and P > 262 144, where the grid-stride loops of every cc_* / mr_* kernel take a second step
from launch_shape_maps import LARGE_SHAPE, SMALL_SHAPES, few_valued, maps  # noqa: E402


@pytest.mark.parametrize("m", [2, 7, 64])
@pytest.mark.parametrize("h,w", SMALL_SHAPES)
def test_small_launch_shapes_one_by_one_and_in_batches_of_five(built, h, w, m):
    ms = maps(h, w)
    names = list(ms)
    want = {n: merge_small_regions(ms[n], m) for n in names}
    for n in names:
        assert np.array_equal(_run(ms[n][None], m)[0], want[n]), n
    for batch in (names[:5], names[5:], names[::-1][:5]):                       # B = 5, different content per image
        got = _run(np.stack([ms[n] for n in batch]), m)
        for b, n in enumerate(batch):
            assert np.array_equal(got[b], want[n]), (batch, n)


@pytest.mark.parametrize("m", [2, 7, 64])
def test_large_launch_shape_second_step_of_the_grid_stride_loops(built, m):
    """Maps of few label values only: the restatement's connected_regions loops over the distinct values (the checkerboard is
    the every-pixel-a-region case here)."""
    h, w = LARGE_SHAPE
    assert h * w > 1024 * 256
    ms = few_valued(h, w)
    want = {n: merge_small_regions(v, m) for n, v in ms.items()}
    for n, v in ms.items():                                                     # B = 1
        got = _run(v[None], m)[0]
        assert np.array_equal(got, want[n]), (n, int((got != want[n]).sum()))
    for pair in (("noise4", "comb_bottom"), ("checker", "constant"), ("comb_top", "noise2"), ("rows1", "cols1"),
                 ("constant", "patch")):                                         # B = 2
        got = _run(np.stack([ms[n] for n in pair]), m)
        for b, n in enumerate(pair):
            assert np.array_equal(got[b], want[n]), (pair, n)
