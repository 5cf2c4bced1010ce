"""GPU region descriptors and mean-colour pictures (SPEC.md §19): gcs_region_props, gcs_region_props_cuts and gcs_region_paint against
the restatement (tests/region_props_ref.py: relabel, then tabulate), every value ``==``; ``group`` also against gcs_region_tree_cut
on the device; the host paths on a val fixture image; two existing calls before and after. Outputs start out as 0xAB bytes."""
import os

import numpy as np
import pytest

import contour_map_ref as cm
import region_props_ref as rp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _lib():
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def _ab(torch, nbytes):
    return torch.full((int(nbytes),), 0xAB, dtype=torch.uint8, device="cuda")


def _dev(torch, a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _props(torch, lab, img, feats, k):
    """The raw leaf call on a batch: lab (B,H,W), img (B,H,W,3) or None, feats (B,D,H,W) uint16 or None -> (sums uint64 [B][k][C],
    bbox int32 [B][k][4]) and their device buffers."""
    lib = _lib()
    lab = np.asarray(lab)
    b, h, w = lab.shape
    d = 0 if feats is None else feats.shape[1]
    ls, im = _dev(torch, lab, np.int32), _dev(torch, img, np.uint8)
    fs = None if feats is None else torch.from_numpy(np.ascontiguousarray(feats, np.uint16).view(np.int16)).cuda()
    sums, bbox = _ab(torch, b * k * (6 + d) * 8), _ab(torch, b * k * 16)
    rc = lib.gcs_region_props(ls.data_ptr(), None if im is None else im.data_ptr(), None if fs is None else fs.data_ptr(), b, h, w, d, k,
                              sums.data_ptr(), bbox.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(ls.cpu().numpy(), lab)                   # the inputs are read only
    return (sums.cpu().numpy().view(np.uint64).reshape(b, k, 6 + d), bbox.cpu().numpy().view(np.int32).reshape(b, k, 4)), (sums, bbox)


def _check_leaf(torch, lab, img, feats, k):
    (sums, bbox), bufs = _props(torch, lab, img, feats, k)
    for i in range(len(lab)):
        ws, wb = rp.leaf_table(lab[i], k, None if img is None else img[i], None if feats is None else feats[i])
        assert np.array_equal(sums[i], ws), (i, np.argwhere(sums[i] != ws)[:4].tolist())
        assert np.array_equal(bbox[i], wb), (i, np.argwhere(bbox[i] != wb)[:4].tolist())
    return sums, bbox, bufs


def _rand(seed, b, h, w, d):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8), rng.integers(0, 46341, (b, d, h, w)).astype(np.uint16)


def _one_pixel(b, h, w):
    return np.stack([np.arange(h * w, dtype=np.int32).reshape(h, w)] * b)


def test_one_pixel_labels_overflow_every_tile(torch_cuda):
    """37 x 53 (K = 1961): every 8 x 32 tile sees more than 32 labels, the right and bottom tiles are ragged; 64 x 64 (K = 4096)."""
    for h, w in ((37, 53), (64, 64)):
        img, feats = _rand(h, 2, h, w, 2)
        lab = _one_pixel(2, h, w)
        lab[1] = lab[1][::-1, ::-1]
        sums, bbox, _ = _check_leaf(torch_cuda, lab, img, feats, h * w)
        assert (sums[..., 0] == 1).all() and (bbox[..., 0] == bbox[..., 2]).all()


@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (9, 33)])
def test_tiny_and_ragged_images(torch_cuda, h, w):
    """1 x 1, 1 x 70, and 9 x 33 with 3 labels: the hash path, one pixel past a tile edge in both directions."""
    img, feats = _rand(h * w, 2, h, w, 3)
    lab = (np.add.outer(np.arange(h), np.arange(w)) % 3).astype(np.int32)
    lab = np.stack([lab, (lab + 1) % 3])
    lab[1, -1, -1] = 2                                             # the pixel past both tile edges has a label of its own kind
    _check_leaf(torch_cuda, lab, img, feats, 3)


def test_pieces_unused_and_out_of_range_labels(torch_cuda):
    """A label in two far-apart pieces (its box spans both, its centroid lies in neither); labels 2 and 5 unused; -1, K and 2^30 are
    counted nowhere; without an image the colour columns are 0."""
    from gabor_color_image_segmentation_amd import region_table
    h, w, k = 40, 75, 7
    lab = np.ones((1, h, w), np.int32)
    lab[0, 2:5, 3:9] = 4
    lab[0, 30:38, 60:70] = 4
    lab[0, 10:20, 10:20] = 0
    lab[0, 0, 0], lab[0, 20, 40], lab[0, 39, 74], lab[0, 8:10, 33:66] = -1, k, 2 ** 30, 3
    lab[0, 21, 5:9] = 6
    img, feats = _rand(7, 1, h, w, 1)
    sums, bbox, _ = _check_leaf(torch_cuda, lab, img, feats, k)
    t = region_table(sums[0], bbox[0])
    assert tuple(t["bbox"][4]) == (2, 3, 37, 69) and t["area"][4] == 18 + 80
    cy, cx = t["centroid"][4]
    assert lab[0, int(cy), int(cx)] != 4
    assert t["used"].tolist() == [True, True, False, True, True, False, True]
    assert tuple(bbox[0, 2]) == (h, w, -1, -1) and (sums[0, 2] == 0).all()
    assert sums[0, :, 0].sum() == h * w - 3
    nsums, _, _ = _check_leaf(torch_cuda, lab, None, feats, k)
    assert (nsums[..., 3:6] == 0).all() and np.array_equal(nsums[..., :3], sums[..., :3]) and np.array_equal(nsums[..., 6:], sums[..., 6:])


def test_more_labels_than_any_table_on_chip(torch_cuda):
    """K = 70 000 on a 280 x 250 map of one-pixel labels: sums and boxes arrive through global atomics only."""
    h, w = 280, 250
    rng = np.random.default_rng(70)
    lab = rng.permutation(h * w).astype(np.int32).reshape(1, h, w)
    img, _ = _rand(70, 1, h, w, 0)
    sums, bbox, _ = _check_leaf(torch_cuda, lab, img, None, h * w)
    assert (sums[0, :, 0] == 1).all()


@pytest.mark.parametrize("d", [0, 1, 72, 207])
def test_accumulator_width(torch_cuda, d):
    """Features at 46340 everywhere on 64 x 64 in one label: every feature sum is 46340 * 4096 (above 2^27), the image at 255."""
    lab = np.zeros((1, 64, 64), np.int32)
    img = np.full((1, 64, 64, 3), 255, np.uint8)
    feats = np.full((1, d, 64, 64), 46340, np.uint16) if d else None
    (sums, bbox), _ = _props(torch_cuda, lab, img, feats, 2)
    assert sums[0, 0].tolist() == [4096, 63 * 32 * 64, 63 * 32 * 64, 255 * 4096, 255 * 4096, 255 * 4096] + [46340 * 4096] * d
    assert (sums[0, 1] == 0).all() and bbox[0].tolist() == [[0, 0, 63, 63], [64, 64, -1, -1]]


# ---- the tile accumulator (csrc/label_tile.h) at its slot boundary, inside one launch

def _stripes(h, w, extra=None):
    """Column stripes x % 32 (32 labels in every full tile row: every slot taken, none missing), ``extra``: one pixel of label 32."""
    lab = np.broadcast_to(np.arange(w, dtype=np.int32) % 32, (h, w)).copy()
    if extra is not None:
        lab[extra] = 32
    return lab


@pytest.mark.parametrize("d", [0, 2])
@pytest.mark.parametrize("h,w", [(8, 32), (9, 33)])
def test_tile_with_32_labels_beside_one_with_33(torch_cuda, h, w, d):
    """B = 2: image 0's first tile holds exactly 32 labels (the LDS rows and boxes), image 1's the same and a 33rd label in one pixel
    (the global rows), both in one launch; at 9 x 33 the second tiles are ragged in both directions."""
    lab = np.stack([_stripes(h, w), _stripes(h, w, (5, 13))])
    img, feats = _rand(h * w + d, 2, h, w, d)
    sums, bbox, _ = _check_leaf(torch_cuda, lab, img, feats if d else None, 33)
    assert sums[0, 32, 0] == 0 and sums[1, 32, 0] == 1 and bbox[1, 32].tolist() == [5, 13, 5, 13]


def test_tile_of_one_label_at_full_range(torch_cuda):
    """One 8 x 32 tile of one label, both features at 46339: every eight-lane sum is 8 * 46339, both LDS cells reach 256 * 46339."""
    lab = np.zeros((1, 8, 32), np.int32)
    img = np.full((1, 8, 32, 3), 255, np.uint8)
    feats = np.full((1, 2, 8, 32), 46339, np.uint16)
    sums, bbox, _ = _check_leaf(torch_cuda, lab, img, feats, 1)
    assert sums[0, 0].tolist() == [256, 28 * 32, 496 * 8, 255 * 256, 255 * 256, 255 * 256, 46339 * 256, 46339 * 256]
    assert bbox[0, 0].tolist() == [0, 0, 7, 31]


# ---- the cuts

def _cuts(torch, sums, bbox, merges, alive, regions, shape, rsum=None):
    """The raw cuts call: sums [B][k][C] uint64, bbox [B][k][4], merges [B][k-1][2] or None (a NULL pointer) -> (group [n][B][k],
    sums_out [B][Rsum][C], bbox_out [B][Rsum][4])."""
    lib = _lib()
    b, k, c = sums.shape
    n = len(regions)
    rsum = sum(min(k, max(int(r), 0)) for r in regions) if rsum is None else rsum
    sd = torch.from_numpy(np.ascontiguousarray(sums).view(np.int64)).cuda()
    bd, ms = _dev(torch, bbox, np.int32), _dev(torch, merges, np.int32)
    al, rg = _dev(torch, np.asarray(alive).reshape(-1), np.int32), _dev(torch, regions, np.int32)
    group, so, bo = _ab(torch, n * b * k * 4), _ab(torch, b * rsum * c * 8), _ab(torch, b * rsum * 16)
    rc = lib.gcs_region_props_cuts(sd.data_ptr(), bd.data_ptr(), None if ms is None else ms.data_ptr(), al.data_ptr(), rg.data_ptr(), b,
                                   shape[0], shape[1], k, c, n, rsum, group.data_ptr(), so.data_ptr(), bo.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(sd.cpu().numpy().view(np.uint64), sums) and np.array_equal(bd.cpu().numpy(), bbox)
    return (group.cpu().numpy().view(np.int32).reshape(n, b, k), so.cpu().numpy().view(np.uint64).reshape(b, rsum, c),
            bo.cpu().numpy().view(np.int32).reshape(b, rsum, 4))


def _tree_cut(torch, lab, merges, alive, k, r):
    """gcs_region_tree_cut on the device -> (B,H,W) int32."""
    lib = _lib()
    b, h, w = lab.shape
    ls, ms, al = _dev(torch, lab, np.int32), _dev(torch, merges, np.int32), _dev(torch, np.asarray(alive).reshape(-1), np.int32)
    out = torch.empty_like(ls)
    rc = lib.gcs_region_tree_cut(ls.data_ptr(), None if ms is None else ms.data_ptr(), al.data_ptr(), b, h, w, k, int(r), out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    return out.cpu().numpy()


def _check_cuts(torch, lab, img, feats, merges, alive, regions, k, against_tree_cut=True):
    """Leaf table and cuts of a batch against the restatement; ``group`` against gcs_region_tree_cut where the list is one it takes."""
    lab = np.asarray(lab)
    b, h, w = lab.shape
    sums, bbox, _ = _check_leaf(torch, lab, img, feats, k)
    group, so, bo = _cuts(torch, sums, bbox, merges, alive, regions, (h, w))
    for i in range(b):
        rows = np.zeros((0, 2), np.int32) if merges is None else merges[i]
        wg, ws, wb, _ = rp.cut_tables(lab[i], rows, alive[i], regions, k, None if img is None else img[i],
                                      None if feats is None else feats[i])
        assert np.array_equal(group[:, i], wg), (i, np.argwhere(group[:, i] != wg)[:4].tolist())
        assert np.array_equal(so[i], ws), (i, np.argwhere(so[i] != ws)[:4].tolist())
        assert np.array_equal(bo[i], wb), (i, np.argwhere(bo[i] != wb)[:4].tolist())
    if against_tree_cut:
        last = None
        for c, r in enumerate(regions):
            if last is not None and r >= last:
                continue                                           # (repeats its predecessor's cut: not the cut at r)
            last = r
            cut = _tree_cut(torch, lab, merges, alive, k, r)
            ok = (lab >= 0) & (lab < k)
            for i in range(b):
                assert np.array_equal(group[c, i][lab[i][ok[i]]], cut[i][ok[i]]), (c, r, i)
    return group, so, bo


def _noise(seed, b, h, w, k, unused=()):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, (b, h, w)).astype(np.int32)
    for i, drop in enumerate(unused):
        for q in drop:
            lab[i][lab[i] == q] = (q + 1) % k
    return lab


@pytest.mark.parametrize("make", [cm.chain, cm.star, cm.balanced])
def test_cuts_of_hand_made_lists(torch_cuda, make):
    k = 40
    lab = _noise(3, 2, 19, 23, k, unused=[(), (5, 17, 30)])
    img, feats = _rand(4, 2, 19, 23, 2)
    merges = np.stack([make(k)] * 2)
    alive = [len(np.unique(l)) for l in lab]
    assert alive == [40, 37]
    group, so, _ = _check_cuts(torch_cuda, lab, img, feats, merges, alive, [41, 40, 37, 20, 8, 2, 1], k)
    assert (group[:, 1, [5, 17, 30]] == -1).all() and (so[1, 77:80] == 0).all()    # unused leaves; R = 40, alive = 37: three rows behind the groups


def test_cuts_of_the_librarys_own_trees_with_a_different_alive_per_image(torch_cuda):
    """B = 3, K = 40, three unused-label sets: gcs_region_tree's own merge lists, R from above alive down to 1."""
    torch, lib = torch_cuda, _lib()
    k, d = 40, 3
    lab = _noise(11, 3, 19, 23, k, unused=[(), (1, 2, 3, 4, 5, 6, 7, 8), (39,)])
    yy, xx = np.mgrid[0:19, 0:23]
    lab[2] = ((yy // 4) * 6 + xx // 4).astype(np.int32)           # blocks: 30 labels, 30 .. 39 unused
    img, feats = _rand(12, 3, 19, 23, d)
    ls = _dev(torch, lab, np.int32)
    fs = torch.from_numpy(feats.view(np.int16)).cuda()
    ws = _ab(torch, lib.gcs_region_tree_workspace_bytes(3, 19, 23, d, k))
    merges = torch.empty((3, k - 1, 2), dtype=torch.int32, device="cuda")
    alive = torch.empty((3,), dtype=torch.int32, device="cuda")
    rc = lib.gcs_region_tree(fs.data_ptr(), ls.data_ptr(), 3, 19, 23, d, k, ws.data_ptr(), merges.data_ptr(), None, alive.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    merges, alive = merges.cpu().numpy(), alive.cpu().numpy().tolist()
    assert alive == [40, 32, 30]
    _check_cuts(torch, lab, img, feats, merges, alive, [64, 40, 32, 31, 30, 16, 5, 2, 1], k)


def test_cuts_of_a_list_with_rows_that_do_not_count(torch_cuda):
    """Rows with a = b, b >= K, an absorbed b, a dead a and (-1, -1) in the middle are skipped by rs_absorbers, the walk of every cut
    kernel: ``group`` is held against gcs_region_tree_cut on the list with those rows cleared and on the raw list itself."""
    k = 24
    lab = _noise(21, 1, 15, 18, k)
    img, feats = _rand(22, 1, 15, 18, 1)
    bad = cm.balanced(k).copy()
    bad[1], bad[3], bad[5], bad[7], bad[9] = (4, 4), (2, k), bad[0], (bad[0][1], 23), (-1, -1)
    clean = rp.counted(bad, k)
    assert (clean[[1, 3, 5, 7, 9]] == -1).all()
    regions = [24, 12, 6, 3, 1]
    group, so, bo = _check_cuts(torch_cuda, lab, img, feats, bad[None], [k], regions, k, against_tree_cut=False)
    for c, r in enumerate(regions):
        cut = _tree_cut(torch_cuda, lab, clean[None], [k], k, r)
        assert np.array_equal(group[c, 0][lab[0]], cut[0])
        assert np.array_equal(group[c, 0][lab[0]], _tree_cut(torch_cuda, lab, bad[None], [k], k, r)[0])
    assert group[-1, 0].max() + 1 > 1                              # a forest: more than R = 1 groups, the others have no row
    assert so.shape[1] == sum(regions) and so[0, -1, 0] < lab.size


def test_cut_edge_cases(torch_cuda):
    """K = 1 with a NULL merge list; R >= alive (the leaf table, densely); R = 1; 64 cuts; entries that are not below their
    predecessor; K = 4096 one-pixel labels under the balanced list."""
    lab = np.zeros((2, 5, 7), np.int32)
    lab[1, 0, 0] = 3                                               # out of range at K = 1
    img, feats = _rand(30, 2, 5, 7, 1)
    _check_cuts(torch_cuda, lab, img, feats, None, [1, 1], [5, 1], 1)
    k = 40
    lab = _noise(31, 1, 19, 23, k, unused=[(9,)])
    img, feats = _rand(32, 1, 19, 23, 2)
    merges = cm.balanced(k)[None]
    _check_cuts(torch_cuda, lab, img, feats, merges, [39], [4096, 39, 1], k)
    _check_cuts(torch_cuda, lab, img, feats, merges, [39], list(range(66, 2, -1)), k)
    _check_cuts(torch_cuda, lab, img, feats, merges, [39], [20, 30, 20, 8, 8, 9, 2], k)
    lab = _one_pixel(1, 64, 64)
    img, _ = _rand(33, 1, 64, 64, 0)
    _check_cuts(torch_cuda, lab, img, None, cm.balanced(4096)[None], [4096], [4096, 1000, 7, 1], 4096)


def test_no_row_at_or_past_rsum_is_written(torch_cuda):
    """The caller's Rsum bounds the rows whatever ``regions`` holds: with Rsum = 5 for regions (8, 4) only the first 5 rows exist."""
    k = 12
    lab = _noise(41, 1, 9, 11, k)
    sums, bbox, _ = _check_leaf(torch_cuda, lab, None, None, k)
    group, so, bo = _cuts(torch_cuda, sums, bbox, cm.chain(k)[None], [k], [8, 4], (9, 11), rsum=5)
    wg, ws, wb, _ = rp.cut_tables(lab[0], cm.chain(k), k, [8, 4], k)
    assert np.array_equal(group[:, 0], wg) and np.array_equal(so[0], ws[:5]) and np.array_equal(bo[0], wb[:5])


# ---- the picture

def _paint(torch, lab, group, sums, k, offset=0, rows=None):
    """``rows`` = (first, G): the picture of that run of rows of ``sums`` [B][rows][C], read in place (row_stride = its row count)."""
    lib = _lib()
    b, h, w = lab.shape
    ls, gd = _dev(torch, lab, np.int32), _dev(torch, group, np.int32)
    sd = torch.from_numpy(np.ascontiguousarray(sums).view(np.int64)).cuda()
    buf = _ab(torch, b * h * w * 3 + 16)
    out = buf[offset:offset + b * h * w * 3]
    first, g = rows or (0, sums.shape[1])
    rc = lib.gcs_region_paint(ls.data_ptr(), None if gd is None else gd.data_ptr(), sd.data_ptr() + first * sums.shape[2] * 8, b, h, w, k,
                              g, sums.shape[2], sums.shape[1], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    raw = buf.cpu().numpy()
    assert (raw[:offset] == 0xAB).all() and (raw[offset + b * h * w * 3:] == 0xAB).all()        # nothing outside the picture
    return raw[offset:offset + b * h * w * 3].reshape(b, h, w, 3)


def _check_paint(torch, lab, group, sums, k, offset=0, rows=None):
    got = _paint(torch, lab, group, sums, k, offset, rows)
    if rows:
        sums = sums[:, rows[0]:rows[0] + rows[1]]
    for i in range(len(lab)):
        want = rp.paint(lab[i], sums[i], None if group is None else group[i], k)
        assert np.array_equal(got[i], want), (i, np.argwhere(got[i] != want)[:4].tolist())
    return got


@pytest.mark.parametrize("b,h,w", [(2, 9, 33), (3, 37, 53), (1, 1, 1), (2, 1, 70)])
def test_paint_small_tables_on_ragged_shapes(torch_cuda, b, h, w):
    """W = 33 and odd H W: an image starts at any byte of a word, the 12-byte stores straddle rows and images; with and without a
    group table; out-of-range labels, negative group entries and empty rows are black; an output that starts off a word."""
    k = 9
    lab = _noise(50 + w, b, h, w, k, unused=[(4,)] * b)
    img, _ = _rand(51, b, h, w, 0)
    flat = lab.reshape(b, -1)
    if h * w >= 4:
        flat[:, 0], flat[:, 1], flat[:, -1] = -1, k, 2 ** 30
    sums, bbox, _ = _check_leaf(torch_cuda, lab, img, None, k)
    pic = _check_paint(torch_cuda, lab, None, sums, k)
    if h * w >= 4:
        assert (pic.reshape(b, -1, 3)[:, [0, 1, -1]] == 0).all()
    _check_paint(torch_cuda, lab, None, sums, k, offset=1)
    merges = np.stack([cm.star(k)] * b)
    alive = [int((sums[i, :, 0] > 0).sum()) for i in range(b)]
    group, so, _ = _cuts(torch_cuda, sums, bbox, merges, alive, [5, 2], (h, w))
    _check_paint(torch_cuda, lab, group[0], so[:, :5], k)
    _check_paint(torch_cuda, lab, group[1], so[:, 5:], k, offset=3)
    _check_paint(torch_cuda, lab, group[1], so, k, rows=(5, 2))    # the cut's rows where the cuts call left them
    _check_paint(torch_cuda, lab, group[0], so[:, :3], k)          # groups 3 and 4 are past the table: black


def test_paint_tables_in_lds_and_in_memory(torch_cuda):
    """One-pixel labels on 64 x 64: G = 4096 rows are read from memory (with and without a group table), 1000 rows sit in LDS."""
    lab = _one_pixel(2, 64, 64)
    lab[1] = lab[1].T
    img, _ = _rand(60, 2, 64, 64, 0)
    sums, bbox, _ = _check_leaf(torch_cuda, lab, img, None, 4096)
    pic = _check_paint(torch_cuda, lab, None, sums, 4096)
    assert np.array_equal(pic, img)                                # a one-pixel region's mean colour is its pixel
    merges = np.stack([cm.balanced(4096)] * 2)
    group, so, _ = _cuts(torch_cuda, sums, bbox, merges, [4096, 4096], [4096, 1000], (64, 64))
    assert np.array_equal(_check_paint(torch_cuda, lab, group[0], so[:, :4096], 4096), img)
    _check_paint(torch_cuda, lab, group[1], so, 4096, rows=(4096, 1000))


def test_argument_errors_launch_nothing(torch_cuda):
    """Every GCS_EINVAL case (the list of tests/test_region_props.py), and with real buffers: nothing is written."""
    import test_region_props as cpu
    cpu.test_argument_errors_launch_nothing(True)
    torch, lib = torch_cuda, _lib()
    ls = torch.zeros((1, 4, 4), dtype=torch.int32, device="cuda")
    sums, bbox, out = _ab(torch, 4 * 6 * 8), _ab(torch, 4 * 16), _ab(torch, 48)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.gcs_region_props(ls.data_ptr(), None, None, 1, 4, 4, 0, 0, sums.data_ptr(), bbox.data_ptr(), s) == 1
    assert lib.gcs_region_props(ls.data_ptr(), None, None, 1, 4, 4, 1, 4, sums.data_ptr(), bbox.data_ptr(), s) == 1
    assert lib.gcs_region_paint(ls.data_ptr(), None, sums.data_ptr(), 1, 4, 4, 4, 3, 6, 3, out.data_ptr(), s) == 1
    assert lib.gcs_region_props_cuts(sums.data_ptr(), bbox.data_ptr(), None, ls.data_ptr(), ls.data_ptr(), 1, 4, 4, 4, 6, 1, 2,
                                     out.data_ptr(), sums.data_ptr(), bbox.data_ptr(), s) == 1
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xAB).all() for t in (sums, bbox, out))


# ---- host paths

def _fixture_image(shape=(481, 321)):
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    i = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == shape][0]
    return val["img_" + i].copy()


def _table_equals(table, want_sums, want_bbox):
    from gabor_color_image_segmentation_amd import region_table
    want = region_table(want_sums, want_bbox)
    assert set(table) == set(want) == {"area", "centroid", "bbox", "mean_rgb", "mean_features", "used"}
    for name in want:
        assert table[name].dtype == want[name].dtype and np.array_equal(table[name], want[name], equal_nan=name == "centroid"), name


@pytest.mark.parametrize("kw", [dict(n_iter=3), dict(n_iter=3, connectivity=True),
                                dict(n_superpixels=300, n_regions=8, n_iter=4, **COLOUR),
                                dict(n_superpixels=300, n_regions=8, n_iter=4, tree_nodes="components", **COLOUR)],
                         ids=["kmeans", "connectivity", "tree", "component-tree"])
def test_segment_regions_describes_the_delivered_map(torch_cuda, kw):
    import gabor_color_image_segmentation_amd as pkg
    img = _fixture_image()
    labels, table = pkg.segment_regions(img, **kw)
    assert np.array_equal(labels, pkg.segment(img, **kw)) and labels.dtype == np.int32
    k = int(labels.max()) + 1
    if "n_regions" in kw:
        assert k == 8
    _table_equals(table, *rp.leaf_table(labels, k, img))
    assert table["area"].sum() == labels.size and table["used"].all()
    pic = pkg.render_regions(img, labels)
    assert pic.dtype == np.uint8 and np.array_equal(pic, rp.paint(labels, rp.leaf_table(labels, k, img)[0]))


def test_device_calls_of_the_segmenter(torch_cuda):
    """region_props_device (with the plan's features), cut_props_device in the caller's order of R, paint_device: against the
    restatement on the library's own tree of a 37 x 53 image pair; ``segment`` and ``region_tree_device`` give the same bits
    before and after the new calls ran."""
    from gabor_color_image_segmentation_amd import Segmenter, region_table
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    torch = torch_cuda
    imgs = synthetic_batch(2, 37, 53, seed=18)
    dev = torch.from_numpy(imgs).cuda()
    seg = Segmenter(n_superpixels=64, n_iter=3)
    plain = Segmenter(n_iter=3)
    before = [t.cpu().numpy() for t in seg.region_tree_device(dev)], plain(imgs[0])
    labels, merges, _, alive = seg.region_tree_device(dev)
    k = merges.shape[1] + 1
    sums, bbox = seg.region_props_device(dev, labels, K=k, features=True)
    feats = seg.features_device(dev).cpu().numpy().view(np.uint16)
    lab, mg, al = labels.cpu().numpy(), merges.cpu().numpy(), alive.cpu().numpy()
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (2, k, 6 + seg.bank.n_features) and tuple(bbox.shape) == (2, k, 4)
    for i in range(2):
        ws, wb = rp.leaf_table(lab[i], k, imgs[i], feats[i])
        assert np.array_equal(sums[i].cpu().numpy().view(np.uint64), ws) and np.array_equal(bbox[i].cpu().numpy(), wb)
    auto = seg.region_props_device(dev, labels)                    # K from the map, no features
    assert tuple(auto[0].shape) == (2, int(lab.max()) + 1, 6)
    assert np.array_equal(auto[0].cpu().numpy(), sums[:, :int(lab.max()) + 1, :6].cpu().numpy())
    regions = [4, 16, 8]                                           # the caller's order
    group, so, bo, offsets = seg.cut_props_device(sums, bbox, merges, alive, regions, shape=(37, 53))
    assert tuple(group.shape) == (3, 2, k) and offsets == [24, 0, 16] and tuple(so.shape) == (2, 28, sums.shape[2])
    for j, r in enumerate(regions):
        cut = seg.cut_regions_device(labels, merges, alive, r).cpu().numpy()
        for i in range(2):
            wg, ws, wb, _ = rp.cut_tables(lab[i], mg[i], al[i], [r], k, imgs[i], feats[i])
            assert np.array_equal(group[j, i].cpu().numpy(), wg[0])
            rows = slice(offsets[j], offsets[j] + r)
            assert np.array_equal(so[i, rows].cpu().numpy().view(np.uint64), ws) and np.array_equal(bo[i, rows].cpu().numpy(), wb)
            assert np.array_equal(group[j, i].cpu().numpy()[lab[i]], cut[i])
            _table_equals(region_table(so[i, rows].cpu().numpy(), bo[i, rows].cpu().numpy()), *rp.leaf_table(cut[i], r, imgs[i], feats[i]))
        pic = seg.paint_device(labels, so[:, offsets[j]:offsets[j] + r], group[j]).cpu().numpy()
        direct = seg.paint_device(torch.from_numpy(cut).cuda(), seg.region_props_device(dev, torch.from_numpy(cut).cuda(), K=r)[0])
        assert np.array_equal(pic, direct.cpu().numpy())
        assert all(np.array_equal(pic[i], rp.paint(cut[i], rp.leaf_table(cut[i], r, imgs[i])[0])) for i in range(2))
    g2 = seg.cut_props_device(sums, bbox, merges, alive, regions)  # the shape read from the leaf table's own empty boxes
    assert np.array_equal(g2[2].cpu().numpy(), bo.cpu().numpy()) and np.array_equal(g2[1].cpu().numpy(), so.cpu().numpy())
    with pytest.raises(ValueError):
        seg.cut_props_device(sums, bbox, merges, alive, [8, 8])
    with pytest.raises(ValueError):
        seg.region_props_device(dev, labels.to(torch.int64))
    after = [t.cpu().numpy() for t in seg.region_tree_device(dev)], plain(imgs[0])
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
