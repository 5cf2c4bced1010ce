"""GPU connected-regions post-pass (SPEC.md §7) against the scipy.ndimage oracle, bit for bit."""
import numpy as np
import pytest

from oracle import spec_oracle as so

pytestmark = pytest.mark.gpu


def _run(lab):
    import torch
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    lab = np.ascontiguousarray(lab, np.int32)
    b, h, w = lab.shape
    d = torch.from_numpy(lab).cuda()
    out = torch.empty_like(d)
    scratch = torch.empty(lib.gcs_connected_scratch_bytes(b, h, w), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gcs_connected_regions(d.data_ptr(), b, h, w, scratch.data_ptr(), out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "gcs_connected_regions")
    return out.cpu().numpy()


def test_random_maps_many_small_components(built):
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 4, (3, 97, 131))
    got = _run(lab)
    for b in range(3):
        assert np.array_equal(got[b], so.connected_regions(lab[b]))


def test_spiral_is_one_long_component(built):
    """A 1-pixel-wide spiral: the worst case for pointer chasing (component length ~ H*W/2)."""
    n = 101
    lab = np.zeros((n, n), np.int32)
    y = x = 0
    dy, dx = 0, 1
    top, left, bottom, right = 0, 0, n - 1, n - 1
    for _ in range(n * n):
        lab[y, x] = 1
        ny, nx = y + dy, x + dx
        if not (top <= ny <= bottom and left <= nx <= right) or (lab[ny, nx] == 1) or \
           (0 <= ny + dy < n and 0 <= nx + dx < n and lab[ny + dy, nx + dx] == 1 and (dy, dx) != (0, 0)):
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            if not (0 <= ny < n and 0 <= nx < n) or lab[ny, nx] == 1:
                break
            if 0 <= ny + dy < n and 0 <= nx + dx < n and lab[ny + dy, nx + dx] == 1:
                break
        y, x = ny, nx
    assert lab.sum() > n  # something spiral-like was drawn
    assert np.array_equal(_run(lab[None])[0], so.connected_regions(lab))


def test_segmentation_with_connectivity_full_size(built):
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(2, 321, 481, seed=3)
    plain = Segmenter(n_iter=4).segment_batch(imgs)
    got = Segmenter(n_iter=4, connectivity=True).segment_batch(imgs)
    for b in range(2):
        ref = so.connected_regions(plain[b])
        assert np.array_equal(got[b], ref)
        assert got[b].max() + 1 >= 8           # at least one region per cluster that occurs


# ---- the shapes that change the launch (tests/launch_shape_maps.py): P = 1, single rows / columns, P around the 1 024 threads of
# cc_rank_kernel, and P > 262 144, where the grid-stride loops of every cc_* kernel take a second step
from launch_shape_maps import LARGE_SHAPE, SMALL_SHAPES, few_valued, maps  # noqa: E402


def _expected(name, lab):
    if name == "own":                                    # every pixel its own region: SPEC.md §7 numbers them in raster order
        return np.arange(lab.size).reshape(lab.shape)
    return so.connected_regions(lab)


@pytest.mark.parametrize("h,w", SMALL_SHAPES)
def test_small_launch_shapes_one_by_one_and_in_batches_of_five(built, h, w):
    ms = maps(h, w)
    names = list(ms)
    want = {n: _expected(n, ms[n]) for n in names}
    assert np.array_equal(want["own"], so.connected_regions(ms["own"]))        # (cheap here: the direct form is the oracle's)
    for n in names:
        assert np.array_equal(_run(ms[n][None])[0], want[n]), n
    for batch in (names[:5], names[5:], names[::-1][:5]):                       # B = 5, different content per image
        got = _run(np.stack([ms[n] for n in batch]))
        for b, n in enumerate(batch):
            assert np.array_equal(got[b], want[n]), (batch, n)


def test_large_launch_shape_second_step_of_the_grid_stride_loops(built):
    h, w = LARGE_SHAPE
    assert h * w > 1024 * 256
    ms = dict(few_valued(h, w), own=maps(h, w)["own"])
    want = {n: _expected(n, m) for n, m in ms.items()}
    for n, m in ms.items():                                                     # B = 1
        got = _run(m[None])[0]
        assert np.array_equal(got, want[n]), (n, int((got != want[n]).sum()))
    for pair in (("noise4", "comb_bottom"), ("own", "constant"), ("checker", "noise2"), ("comb_top", "rows1"),
                 ("cols1", "noise4"), ("patch", "own")):                         # B = 2
        got = _run(np.stack([ms[n] for n in pair]))
        for b, n in enumerate(pair):
            assert np.array_equal(got[b], want[n]), (pair, n)
