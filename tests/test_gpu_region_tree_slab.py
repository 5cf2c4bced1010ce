"""gcs_region_tree_slab (SPEC.md §21) on the GPU: the tree whose node statistics come from the feature slab itself. The slabs are
filled by the library's own Gabor stage and gcs_position_features (position_weight = 255 where the shape allows it: coordinates times
255 reach 4096 inside every tile, so TOP runs and flags are exercised; a smaller weight on one shape leaves tiles without a flag),
the label maps are hand-made. Compared with ``==``, never against the kernel's own output:
  (a) the [K][D + 1] sums of the head of the workspace against exact NumPy sums of gcs_features_unpack of the same slab. The merge
      kernel adds a merged pair's rows in place (row a += row b, b's row stays as it died), so the sums the statistics launch wrote
      are recovered exactly by undoing the written rows of the merge list, last first;
  (b) per bank, the same sums against the C oracle's features of the same images;
  (c) merges, costs and alive against gcs_region_tree on the unpacked tensor and against tests/region_tree_ref.py.
Banks: one per slab format and of 1, 2 and 4 levels. Shapes: 8 x 8 (one workgroup, a tile three quarters empty), 40 x 64 (whole
tiles), 37 x 53 and 41 x 66 (one- and two-pixel packed strips on both edges, block rows that wrap inside a tile), 321 x 481 (BSD)."""
import numpy as np
import pytest

import position_ref as pr
import region_tree_ref as rt

pytestmark = pytest.mark.gpu

# name -> (make_bank keywords without the coordinate slot, split slab?, levels); the coordinate slot makes n_orient + 1 slots
BANKS = {"one_level": (dict(n_scales=2, n_orient=5), True, 1),      # D = 36
         "default": (dict(n_scales=4, n_orient=5), True, 2),        # D = 72: the default bank's shape
         "wide2": (dict(n_scales=4, n_orient=6), False, 2),         # D = 84: two levels on the wide slab
         "deep": (dict(n_scales=8, n_orient=7), False, 4)}          # D = 192: four levels, no packed strips
SHAPES = [(8, 8), (40, 64), (37, 53), (41, 66)]


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_SLABS = {}


def _slab(torch, bank, shape, b=1, mu=None):
    """(ops, imgs, slab, canonical tensor on the host (B, D, H, W) uint16, mu) of ``b`` synthetic images: made once per key."""
    key = (bank, shape, b, mu)
    if key not in _SLABS:
        from gabor_color_image_segmentation_amd import make_bank
        from gabor_color_image_segmentation_amd.segmenter import HipOps
        from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
        h, w = shape
        m = min(255, 46339 // (max(h, w) - 1)) if mu is None else mu
        ops = HipOps(make_bank(position_weight=m, **BANKS[bank][0]), "cuda:0")
        imgs = synthetic_batch(b, h, w, seed=h + w)
        feats = ops.feature_slab(b, h, w)
        ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
        ops.position_features(feats, b, h, w)
        canon = ops.features_unpack(feats, b, h, w).cpu().numpy().view(np.uint16)
        assert canon.shape[1] == 3 * BANKS[bank][0]["n_scales"] * (BANKS[bank][0]["n_orient"] + 1)
        _SLABS[key] = (ops, imgs, feats, canon, m)
    return _SLABS[key]


def _numpy_sums(canon, lab, k):
    """Exact [K][D + 1] sums of one image: D feature sums and the count per label 0 .. K-1 (float64 bincount: integers < 2^53)."""
    d = canon.shape[0]
    ok = (lab >= 0) & (lab < k)
    idx = lab[ok].astype(np.int64)
    out = np.zeros((k, d + 1), np.uint64)
    for j in range(d):
        out[:, j] = np.bincount(idx, weights=canon[j][ok].astype(np.float64), minlength=k).astype(np.uint64)
    out[:, d] = np.bincount(idx, minlength=k).astype(np.uint64)
    return out


def _raw_sums(head, merges):
    """The statistics launch's sums from the workspace head after the merge kernel: undo the written rows, last first."""
    s = head.copy()
    for a, c in merges[::-1]:
        if a >= 0:
            s[a] -= s[c]
    return s


def _run(torch, ops, feats, canon, lab, k, slab=True):
    """One call on garbage-filled outputs -> (sums [B][K][D + 1] uint64 as the statistics launch wrote them, merges, costs, alive)."""
    lib = ops.lib
    b, d, h, w = canon.shape
    ls = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
    need = lib.gcs_region_tree_workspace_bytes(b, h, w, d, k)
    assert need >= b * k * (d + 1) * 8
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    merges = torch.full((b, k - 1, 2), 7, dtype=torch.int32, device="cuda")
    costs = torch.full((b, k - 1), 7, dtype=torch.int64, device="cuda")
    alive = torch.full((b,), -5, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    mp, cp = (merges.data_ptr(), costs.data_ptr()) if k > 1 else (None, None)
    if slab:
        rc = lib.gcs_region_tree_slab(feats.data_ptr(), ls.data_ptr(), b, h, w, ops.bank.n_scales, ops.bank.n_orient, k, ws.data_ptr(),
                                      mp, cp, alive.data_ptr(), st)
    else:
        xs = torch.from_numpy(canon.view(np.int16)).cuda()
        rc = lib.gcs_region_tree(xs.data_ptr(), ls.data_ptr(), b, h, w, d, k, ws.data_ptr(), mp, cp, alive.data_ptr(), st)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    m = merges.cpu().numpy()
    head = ws[:b * k * (d + 1) * 8].cpu().numpy().view(np.uint64).reshape(b, k, d + 1)
    return np.stack([_raw_sums(head[i], m[i]) for i in range(b)]), m, costs.cpu().numpy().view(np.uint64), alive.cpu().numpy()


def _check(torch, bank, shape, lab, k, b=1, mu=None, ref=True, oracle=False):
    """(a), (c) and, with ``oracle``, (b) for one label map (B, H, W); ``ref=False`` leaves the Python tree out (many nodes)."""
    ops, imgs, feats, canon, m_used = _slab(torch, bank, shape, b, mu)
    lab = np.asarray(lab)
    assert lab.shape == (b,) + tuple(shape)
    sums, merges, costs, alive = _run(torch, ops, feats, canon, lab, k)
    for i in range(b):
        want = _numpy_sums(canon[i], lab[i], k)
        bad = np.argwhere(sums[i] != want)
        assert bad.size == 0, (bank, shape, i, len(bad), bad[:4].tolist())
        if oracle:
            x = pr.features(imgs[i], 0.0, 0, m_used, BANKS[bank][0]["n_scales"], BANKS[bank][0]["n_orient"])
            assert np.array_equal(sums[i], _numpy_sums(x, lab[i], k)), (bank, shape, i)
    sums2, merges2, costs2, alive2 = _run(torch, ops, feats, canon, lab, k, slab=False)
    assert np.array_equal(sums, sums2) and np.array_equal(merges, merges2) and np.array_equal(costs, costs2)
    assert np.array_equal(alive, alive2)
    if ref:
        for i in range(b):
            rm, rc, ra = rt.build_tree(canon[i], lab[i], k)
            assert int(alive[i]) == ra and np.array_equal(merges[i], rm) and np.array_equal(costs[i], rc), (bank, shape, i)
    return sums, merges, costs, alive


def _blocks(h, w, by, bx):
    """A coarse map of by x bx-pixel blocks, numbered in raster order."""
    y, x = np.mgrid[0:h, 0:w]
    return ((y // by) * (-(-w // bx)) + x // bx).astype(np.int32)


def _busy(h, w):
    """Blocks of 7 x 9 pixels with a patch of one-pixel labels inside the first tile: more than 32 labels in one 8 x 32 tile (the
    accumulator's overflow form) beside tiles that stay inside their slots; some labels unused. Returns (map, K)."""
    lab = _blocks(h, w, 7, 9)
    n = int(lab.max()) + 1
    ph, pw = min(6, h), min(8, w)
    lab[:ph, :pw] = n + 3 + np.arange(ph * pw, dtype=np.int32).reshape(ph, pw)         # labels n .. n + 2 stay unused
    return lab, n + 3 + ph * pw + 2


@pytest.mark.parametrize("bank", list(BANKS))
def test_8x8_single_label_and_one_pixel_labels(torch_cuda, bank):
    sums, merges, costs, alive = _check(torch_cuda, bank, (8, 8), np.zeros((1, 8, 8), np.int32), 1)
    assert alive.tolist() == [1] and int(sums[0, 0, -1]) == 64
    _, _, _, alive = _check(torch_cuda, bank, (8, 8), np.arange(64, dtype=np.int32).reshape(1, 8, 8), 64, oracle=True)
    assert alive.tolist() == [64]


@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("bank", list(BANKS))
def test_crafted_maps_on_every_bank_and_edge(torch_cuda, bank, shape):
    h, w = shape
    ops, _, _, canon, _ = _slab(torch_cuda, bank, shape)
    assert (canon >= 4096).any() and canon.max() > 4096
    assert bool(ops.lib.gcs_feature_slab_bytes(1, h, w, ops.bank.n_scales, ops.bank.n_orient))
    lab, k = _busy(h, w)
    sums, merges, costs, alive = _check(torch_cuda, bank, shape, lab[None], k, oracle=(shape == (37, 53)))
    assert int(alive[0]) == len(np.unique(lab)) < k and int(sums[0, :, -1].sum()) == h * w
    # walls of labels outside 0 .. K-1 cut the graph apart: counted nowhere, adjacent to nothing
    walls = _blocks(h, w, 10, 13)
    kw = int(walls.max()) + 1
    walls[:, w // 2] = -1
    walls[h // 2, :w // 2] = kw
    walls[h // 2, w // 2:] = 2 ** 30
    sums, merges, costs, alive = _check(torch_cuda, bank, shape, walls[None], kw)
    assert int(sums[0, :, -1].sum()) == h * w - h - w + 1 and (merges[0, int(alive[0]) - 1:] == -1).all()
    # K = 4096 capacity with few nodes
    few = _blocks(h, w, 16, 24)
    _, _, _, alive = _check(torch_cuda, bank, shape, few[None], 4096)
    assert int(alive[0]) == int(few.max()) + 1


def test_a_smaller_weight_leaves_tiles_without_top_nibbles(torch_cuda):
    """mu = 100 on 41 x 66: only the coordinate planes right of column 40 reach 4096, so tiles with and without a TOP flag mix."""
    canon = _slab(torch_cuda, "default", (41, 66), mu=100)[3]
    assert (canon[..., 41:] >= 4096).any()
    tiles = [int(canon[0, :, 8 * r:8 * r + 8, 32 * c:32 * c + 32].max()) for r in range(5) for c in range(2)]    # main blocks, 4 a tile
    print("largest value per tile:", tiles)
    assert min(tiles) < 4096 <= max(tiles)
    lab, k = _busy(41, 66)
    _check(torch_cuda, "default", (41, 66), lab[None], k, mu=100, oracle=True)


@pytest.mark.parametrize("bank", ["default", "wide2"])
def test_batch_of_three_with_a_different_map_per_image(torch_cuda, bank):
    rng = np.random.default_rng(3)
    h, w = 37, 53
    lab = np.stack([_busy(h, w)[0], _blocks(h, w, 5, 5), np.zeros((h, w), np.int32)])
    lab[1][rng.random((h, w)) < 0.1] = -1
    k = _busy(h, w)[1]
    assert int(lab[1].max()) < k
    sums, merges, costs, alive = _check(torch_cuda, bank, (h, w), lab, k, b=3)
    assert int(alive[2]) == 1 and int(alive[0]) != int(alive[1])


@pytest.mark.parametrize("bank", list(BANKS))
def test_one_bsd_sized_image(torch_cuda, bank):
    """321 x 481: BSD's one-pixel strips on both edges (banks of at most two levels pack them)."""
    h, w = 321, 481
    lab = _blocks(h, w, 40, 60)
    lab[100:106, 200:208] = int(lab.max()) + 1 + np.arange(48, dtype=np.int32).reshape(6, 8)
    k = int(lab.max()) + 1
    sums, merges, costs, alive = _check(torch_cuda, bank, (h, w), lab[None], k)
    assert int(alive[0]) == k and int(sums[0, :, -1].sum()) == h * w


def test_the_entry_point_refuses_what_is_outside_the_domain(torch_cuda):
    torch = torch_cuda
    ops, _, feats, canon, _ = _slab(torch, "default", (40, 64))
    lib = ops.lib
    b, d, h, w, k = 1, canon.shape[1], 40, 64, 6
    ns, no = ops.bank.n_scales, ops.bank.n_orient
    lab = torch.zeros((b, h, w), dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.gcs_region_tree_workspace_bytes(b, h, w, d, k), dtype=torch.uint8, device="cuda")
    merges = torch.full((b, k - 1, 2), -7, dtype=torch.int32, device="cuda")
    alive = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = [feats.data_ptr(), lab.data_ptr(), b, h, w, ns, no, k, ws.data_ptr(), merges.data_ptr(), None, alive.data_ptr(), st]
    for pos, val in ((0, None), (1, None), (8, None), (9, None), (11, None), (2, 0), (2, 65536), (3, 0), (3, 4097), (4, 4097),
                     (5, 0), (5, 9), (6, 0), (6, 18), (7, 0), (7, 4097)):       # (4 scales x 18 slots = 216 features > 207)
        args = list(good)
        args[pos] = val
        assert lib.gcs_region_tree_slab(*args) != 0, (pos, val)
    torch.cuda.current_stream().synchronize()
    assert int(alive[0]) == -7 and bool((merges == -7).all())       # nothing was launched
    assert lib.gcs_region_tree_slab(*good) == 0
    torch.cuda.current_stream().synchronize()
    assert int(alive[0]) == 1
