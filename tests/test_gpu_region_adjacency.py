"""GPU region adjacency graph (SPEC.md §20): gcs_region_adjacency and gcs_region_adjacency_cuts against the restatement
(tests/region_adjacency_ref.py), every value ``==``; the cuts also against gcs_region_adjacency on the map gcs_region_tree_cut writes;
the tree's merge rows against the public graph; the host paths on a val fixture image; existing calls before and after. Outputs and
workspace start out as 0xAB bytes, a guard band of 0xAB lies behind every output, and the inputs are compared after the call."""
import os

import numpy as np
import pytest

import contour_map_ref as cm
import region_adjacency_ref as ar

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
GUARD = 256
IMAX = 2 ** 31 - 1


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


def _ptr(t):
    return None if t is None else t.data_ptr()


def _take(buf, nbytes, dtype, shape):
    """The first ``nbytes`` of a guarded output buffer as an array; the guard band behind them must be intact."""
    raw = buf.cpu().numpy()
    assert raw.size == nbytes + GUARD and (raw[nbytes:] == 0xAB).all(), "the guard band behind an output was written"
    return raw[:nbytes].view(dtype).reshape(shape)


def _adj(torch, lab, img, plane, k, cap):
    """The raw leaf call on a batch: lab (B,H,W), img (B,H,W,3) or None, plane (B,H,W) int32 or None -> (edges int32 [B][cap][2],
    vals uint64 [B][cap][3], count int32 [B])."""
    lib = _lib()
    lab = np.asarray(lab, np.int32)
    b, h, w = lab.shape
    ls, im, pl = _dev(torch, lab, np.int32), _dev(torch, img, np.uint8), _dev(torch, plane, np.int32)
    need = lib.gcs_region_adjacency_workspace_bytes(b, cap)
    assert need > 0
    ws = _ab(torch, need)
    eo, vo, co = _ab(torch, b * cap * 8 + GUARD), _ab(torch, b * cap * 24 + GUARD), _ab(torch, b * 4 + GUARD)
    rc = lib.gcs_region_adjacency(ls.data_ptr(), _ptr(im), _ptr(pl), b, h, w, k, cap, ws.data_ptr(), eo.data_ptr(), vo.data_ptr(),
                                  co.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(ls.cpu().numpy(), lab)                   # the inputs are read only
    assert img is None or np.array_equal(im.cpu().numpy(), img)
    assert plane is None or np.array_equal(pl.cpu().numpy(), plane)
    return _take(eo, b * cap * 8, np.int32, (b, cap, 2)), _take(vo, b * cap * 24, np.uint64, (b, cap, 3)), _take(co, b * 4, np.int32, (b,))


def _same_table(got, want, what):
    (ge, gv, gc), (we, wv, wc) = got, want
    assert gc == wc, (what, int(gc), wc)
    assert np.array_equal(ge, we), (what, np.argwhere(ge != we)[:4].tolist())
    assert np.array_equal(gv, wv), (what, np.argwhere(gv != wv)[:4].tolist())


def _check_leaf(torch, lab, img, plane, k, cap):
    lab = np.asarray(lab, np.int32)
    edges, vals, count = _adj(torch, lab, img, plane, k, cap)
    for i in range(len(lab)):
        we, wv = ar.leaf_graph(lab[i], k, None if img is None else img[i], None if plane is None else plane[i])
        _same_table((edges[i], vals[i], count[i]), ar.table(we, wv, cap), i)
    return edges, vals, count


def _rand_img(seed, b, h, w):
    return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3)).astype(np.uint8)


def _rand_plane(seed, b, h, w):
    """Negatives, zeros, small values and 2^31 - 1, mixed."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 5, (b, h, w))
    small = rng.integers(1, 4097, (b, h, w))
    return np.select([pick == 0, pick == 1, pick == 2, pick == 3], [-small, 0, IMAX, -2 ** 31], small).astype(np.int32)


def _one_pixel(b, h, w):
    return np.stack([np.arange(h * w, dtype=np.int32).reshape(h, w)] * b)


def test_one_pixel_labels_overflow_every_tiles_hash(torch_cuda):
    """37 x 53 (K = 1961, 3832 edges of length 1): every 8 x 32 tile sees far more than 64 edges, the right and bottom tiles are
    ragged, pairs cross tile edges in both directions; the second image's labels are reversed."""
    h, w = 37, 53
    lab = _one_pixel(2, h, w)
    lab[1] = lab[1][::-1, ::-1]
    edges, vals, count = _check_leaf(torch_cuda, lab, _rand_img(1, 2, h, w), _rand_plane(2, 2, h, w), h * w, 4096)
    assert count.tolist() == [3832, 3832] and (vals[:, :3832, 0] == 1).all()


def test_permuted_one_pixel_labels_leave_sorted(torch_cuda):
    """The same map with the labels randomly permuted: the order of the table is not the sorted order."""
    h, w = 37, 53
    rng = np.random.default_rng(3)
    lab = np.stack([rng.permutation(h * w).reshape(h, w), rng.permutation(h * w).reshape(h, w)]).astype(np.int32)
    edges, _, count = _check_leaf(torch_cuda, lab, _rand_img(4, 2, h, w), _rand_plane(5, 2, h, w), h * w, 4096)
    key = edges[0, :3832, 0].astype(np.int64) * h * w + edges[0, :3832, 1]
    assert count.tolist() == [3832, 3832] and (np.diff(key) > 0).all()


@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (70, 1), (9, 33)])
def test_tiny_and_ragged_images(torch_cuda, h, w):
    """1 x 1 (no edge: sentinel rows only), 1 x 70, 70 x 1, and 9 x 33 with 3 labels and a pixel of its own label past both tile edges."""
    lab = (np.add.outer(np.arange(h), np.arange(w)) % 3).astype(np.int32)
    lab = np.stack([lab, (lab + 1) % 3])
    lab[1, -1, -1] = 3
    edges, vals, count = _check_leaf(torch_cuda, lab, _rand_img(h * w, 2, h, w), _rand_plane(h + w, 2, h, w), 4, 8)
    if h * w == 1:
        assert count.tolist() == [0, 0] and (edges == -1).all() and (vals == 0).all()
    if (h, w) == (9, 33):
        assert (edges[0] != 3).all() and (edges[1, :count[1], 1] == 3).sum() >= 1


def test_pieces_unused_labels_and_a_wall_of_out_of_range_labels(torch_cuda):
    """Label 4 in two far pieces, labels 2 and 5 unused, and a wall of -1, K and 2^30 between labels 1 and 0: pairs that touch the wall
    count nowhere and its two sides share no edge. Image or plane NULL gives a zero column and leaves the other columns alone."""
    h, w, k = 40, 75, 7
    lab = np.ones((1, h, w), np.int32)
    lab[0, :, 40:] = 0
    lab[0, 0:14, 39], lab[0, 14:27, 39], lab[0, 27:, 39] = -1, k, 2 ** 30
    lab[0, 2:5, 3:9] = 4
    lab[0, 30:38, 60:70] = 4
    lab[0, 8:10, 50:66] = 3
    lab[0, 21, 5:9] = 6
    img, plane = _rand_img(7, 1, h, w), _rand_plane(8, 1, h, w)
    edges, vals, count = _check_leaf(torch_cuda, lab, img, plane, k, 64)
    got = [tuple(e) for e in edges[0, :count[0]].tolist()]
    assert got == [(0, 3), (0, 4), (1, 4), (1, 6)]                 # no (0, 1): the wall separates them
    assert vals[0, 1, 0] == 2 * (8 + 10) and vals[0, 2, 0] == 2 * (3 + 6)
    e_img, v_img, c_img = _check_leaf(torch_cuda, lab, img, None, k, 64)
    e_pl, v_pl, c_pl = _check_leaf(torch_cuda, lab, None, plane, k, 64)
    assert (v_img[..., 2] == 0).all() and np.array_equal(v_img[..., :2], vals[..., :2]) and np.array_equal(e_img, edges)
    assert (v_pl[..., 1] == 0).all() and np.array_equal(v_pl[..., [0, 2]], vals[..., [0, 2]]) and np.array_equal(e_pl, edges)
    assert vals[0, :4, 1].min() > 0 and vals[0, :4, 2].min() > 0


def test_eight_labels_of_noise_contended_atomics_and_accumulator_width(torch_cuda):
    """40 x 75 of 8 random labels: all 28 edges, hundreds of crossings each. Then the plane at 2^31 - 1 everywhere and the image in
    0 / 255 columns: a tile's strength passes 2^32 many times over, every horizontal crossing has contrast 3 * 255^2."""
    h, w, k = 40, 75, 8
    lab = np.random.default_rng(9).integers(0, k, (2, h, w)).astype(np.int32)
    edges, vals, count = _check_leaf(torch_cuda, lab, _rand_img(10, 2, h, w), _rand_plane(11, 2, h, w), k, 28)
    assert count.tolist() == [28, 28] and vals[:, :, 0].min() >= 100
    img = np.zeros((2, h, w, 3), np.uint8)
    img[:, :, 1::2] = 255
    plane = np.full((2, h, w), IMAX, np.int32)
    edges, vals, count = _check_leaf(torch_cuda, lab, img, plane, k, 28)
    assert (vals[:, :, 2] == vals[:, :, 0] * np.uint64(2 * IMAX)).all() and vals[:, :, 2].min() > 2 ** 38
    assert (vals[:, :, 1] % np.uint64(3 * 255 * 255) == 0).all() and vals[:, :, 1].min() > 0


def test_largest_sort_nearly_full(torch_cuda):
    """91 x 91 one-pixel labels (K = 8281): 16 380 edges at E_cap = 16 384."""
    lab = np.random.default_rng(12).permutation(91 * 91).reshape(1, 91, 91).astype(np.int32)
    edges, vals, count = _check_leaf(torch_cuda, lab, _rand_img(13, 1, 91, 91), None, 91 * 91, 16384)
    assert count.tolist() == [16380] and (edges[0, 16380:] == -1).all()


@pytest.mark.parametrize("w", [70, 3, 2500])
def test_capacity_exactly_reached_and_passed_by_one(torch_cuda, w):
    """A row of one-pixel labels has W - 1 edges; image 0 repeats its last label (W - 2 edges = E_cap exactly), image 1 has E_cap + 1:
    count E_cap and exact rows against count -1 and sentinel rows only; the guard bands behind the outputs stay intact (``_take``).
    W = 3: E_cap = 1. W = 2500: a table that fills past its capacity from many tiles at once."""
    lab = _one_pixel(2, 1, w)
    lab[0, 0, -1] = lab[0, 0, -2]
    cap = w - 2
    edges, vals, count = _check_leaf(torch_cuda, lab, _rand_img(w, 2, 1, w), _rand_plane(w, 2, 1, w), w, cap)
    assert count.tolist() == [cap, -1] and (edges[1] == -1).all() and (vals[1] == 0).all() and (edges[0] >= 0).all()


# ---- the cuts

def _props_cuts_group(torch, lab, merges, alive, regions, k):
    """group int32 [n][B][k] of gcs_region_props_cuts (D = 0) for the leaf table of ``lab``."""
    lib = _lib()
    lab = np.asarray(lab, np.int32)
    b, h, w = lab.shape
    n = len(regions)
    rsum = sum(min(k, max(int(r), 0)) for r in regions)
    s = torch.cuda.current_stream().cuda_stream
    ls = _dev(torch, lab, np.int32)
    sums, bbox = _ab(torch, b * k * 48), _ab(torch, b * k * 16)
    assert lib.gcs_region_props(ls.data_ptr(), None, None, b, h, w, 0, k, sums.data_ptr(), bbox.data_ptr(), s) == 0, lib.gcs_last_error()
    ms, al, rg = _dev(torch, merges, np.int32), _dev(torch, np.asarray(alive).reshape(-1), np.int32), _dev(torch, regions, np.int32)
    group, so, bo = _ab(torch, n * b * k * 4), _ab(torch, b * rsum * 48), _ab(torch, b * rsum * 16)
    rc = lib.gcs_region_props_cuts(sums.data_ptr(), bbox.data_ptr(), _ptr(ms), al.data_ptr(), rg.data_ptr(), b, h, w, k, 6, n, rsum,
                                   group.data_ptr(), so.data_ptr(), bo.data_ptr(), s)
    assert rc == 0, lib.gcs_last_error()
    return group.cpu().numpy().view(np.int32).reshape(n, b, k)


def _tree_cut(torch, lab, merges, alive, k, r):
    lib = _lib()
    b, h, w = lab.shape
    ls, ms, al = _dev(torch, lab, np.int32), _dev(torch, merges, np.int32), _dev(torch, np.asarray(alive).reshape(-1), np.int32)
    out = torch.empty_like(ls)
    rc = lib.gcs_region_tree_cut(ls.data_ptr(), _ptr(ms), al.data_ptr(), b, h, w, k, int(r), out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    return out.cpu().numpy()


def _adj_cuts(torch, leaf, group, k, g, cap_out, check_inputs=True):
    """The raw cuts call: leaf = (edges [B][cap][2], vals [B][cap][3], count [B]), group [n][B][k] -> the tables [n][B]."""
    lib = _lib()
    edges, vals, count = leaf
    b, cap = edges.shape[:2]
    n = group.shape[0]
    ed, cd, gd = _dev(torch, edges, np.int32), _dev(torch, count, np.int32), _dev(torch, group, np.int32)
    vd = torch.from_numpy(np.ascontiguousarray(vals).view(np.int64)).cuda()
    need = lib.gcs_region_adjacency_workspace_bytes(n * b, cap_out)
    assert need > 0
    ws = _ab(torch, need)
    eo, vo, co = _ab(torch, n * b * cap_out * 8 + GUARD), _ab(torch, n * b * cap_out * 24 + GUARD), _ab(torch, n * b * 4 + GUARD)
    rc = lib.gcs_region_adjacency_cuts(ed.data_ptr(), vd.data_ptr(), cd.data_ptr(), gd.data_ptr(), b, k, g, cap, n, cap_out,
                                       ws.data_ptr(), eo.data_ptr(), vo.data_ptr(), co.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    if check_inputs:
        assert np.array_equal(ed.cpu().numpy(), edges) and np.array_equal(vd.cpu().numpy().view(np.uint64), vals)
        assert np.array_equal(cd.cpu().numpy(), count) and np.array_equal(gd.cpu().numpy(), group)
    return (_take(eo, n * b * cap_out * 8, np.int32, (n, b, cap_out, 2)), _take(vo, n * b * cap_out * 24, np.uint64, (n, b, cap_out, 3)),
            _take(co, n * b * 4, np.int32, (n, b)))


def _random_tree(rng, k):
    """A random merge list over k leaves: every row joins two of the current reps, a < b."""
    reps, rows = list(range(k)), []
    for _ in range(k - 1):
        i, j = sorted(rng.choice(len(reps), 2, replace=False).tolist())
        rows.append((reps[i], reps[j]))
        reps.pop(j)
    return np.array(rows, np.int32).reshape(k - 1, 2)


def _tree_case(k):
    rng = np.random.default_rng(100 + k)
    if k == 1:
        lab = np.zeros((2, 5, 7), np.int32)
    elif k == 4096:
        lab = np.stack([rng.permutation(4096).reshape(64, 64), np.arange(4096).reshape(64, 64)]).astype(np.int32)
    else:
        h, w = (19, 23) if k == 7 else (40, 75)
        lab = rng.integers(0, k, (2, h, w)).astype(np.int32)
        lab.reshape(2, -1)[:, :k] = np.arange(k)                   # every label is used
    merges = None if k == 1 else np.stack([_random_tree(rng, k), _random_tree(rng, k)])
    return lab, merges


@pytest.mark.parametrize("k", [1, 7, 294, 4096])
def test_cuts_of_random_trees(torch_cuda, k):
    """group from gcs_region_props_cuts for an R list with alive + 2, alive, a repeat, 1: the cuts call equals the restatement on the
    leaf rows, the restatement's leaf graph of the relabelled map, and gcs_region_adjacency on the map gcs_region_tree_cut writes."""
    torch = torch_cuda
    lab, merges = _tree_case(k)
    b, h, w = lab.shape
    img, plane = _rand_img(k, b, h, w), _rand_plane(k + 1, b, h, w)
    cap = 8192 if k >= 294 else 64
    leaf = _check_leaf(torch, lab, img, plane, k, cap)
    alive = [k] * b
    regions = [k + 2, k, k, max(k // 2, 1), max(k // 2, 1), max(k // 7, 1), 2, 1]
    group = _props_cuts_group(torch, lab, merges, alive, regions, k)
    eo, vo, co = _adj_cuts(torch, leaf, group, k, k, cap)
    last = None
    for c, r in enumerate(regions):
        relabelled = np.take_along_axis(group[c], lab.reshape(b, -1), 1).reshape(lab.shape)
        fresh = last is None or r < last
        if fresh:
            last = r
            cut = _tree_cut(torch, lab, merges, alive, k, r)
            assert np.array_equal(cut, relabelled)
            direct = _adj(torch, cut, img, plane, k, cap)
        for i in range(b):
            got = (eo[c, i], vo[c, i], co[c, i])
            _same_table(got, ar.table(*ar.cut_graph(leaf[0][i, :leaf[2][i]], leaf[1][i, :leaf[2][i]], group[c, i], k), cap), (c, i, "rows"))
            _same_table(got, ar.table(*ar.leaf_graph(relabelled[i], k, img[i], plane[i]), cap), (c, i, "relabelled"))
            _same_table(got, (direct[0][i], direct[1][i], direct[2][i]), (c, i, "device"))
    assert (co[-1] == 0).all() and (co[0] == leaf[2]).all()         # R = 1: no edge; R >= alive: the leaf graph


def test_cuts_hand_made_groups_small_capacity_and_overflowed_leaf(torch_cuda):
    """A group table with -1 and out-of-range entries (their leaves drop out), G below K; E_out_cap too small for one of two cuts
    only; a leaf table with count = -1 gives count = -1 in every cut of that image alone."""
    torch = torch_cuda
    k, h, w = 12, 19, 23
    lab = np.random.default_rng(20).integers(0, k, (2, h, w)).astype(np.int32)
    img, plane = _rand_img(21, 2, h, w), _rand_plane(22, 2, h, w)
    leaf = _check_leaf(torch, lab, img, plane, k, 66)
    assert leaf[2].tolist() == [66, 66]
    g = 5
    group = np.array([[[0, 1, 2, 3, 4, -1, 5, 2 ** 30, 0, 1, -7, 4], [4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3]],
                      [[0] * 12, list(range(12))]], np.int32)
    eo, vo, co = _adj_cuts(torch, leaf, group, k, g, 10)
    for c in range(2):
        for i in range(2):
            we, wv = ar.cut_graph(leaf[0][i, :66], leaf[1][i, :66], group[c, i], g)
            _same_table((eo[c, i], vo[c, i], co[c, i]), ar.table(we, wv, 10), (c, i))
    assert co.tolist() == [[10, 1], [0, 10]]
    eo, vo, co = _adj_cuts(torch, leaf, group, k, g, 9)             # 10 edges do not fit 9 rows; the other tables are unaffected
    assert co.tolist() == [[-1, 1], [0, -1]] and (eo[0, 0] == -1).all() and (vo[0, 0] == 0).all()
    _same_table((eo[0, 1], vo[0, 1], co[0, 1]), ar.table(*ar.cut_graph(leaf[0][1, :66], leaf[1][1, :66], group[0, 1], g), 9), "small")
    over = _check_leaf(torch, lab, img, plane, k, 65)
    assert over[2].tolist() == [-1, -1]
    mixed = (np.stack([leaf[0][0, :65], over[0][1]]), np.stack([leaf[1][0, :65], over[1][1]]), np.array([65, -1], np.int32))
    eo, vo, co = _adj_cuts(torch, mixed, group, k, g, 10)
    assert co[:, 1].tolist() == [-1, -1] and (eo[:, 1] == -1).all() and (vo[:, 1] == 0).all() and co[1, 0] == 0 and co[0, 0] >= 0
    _same_table((eo[0, 0], vo[0, 0], co[0, 0]), ar.table(*ar.cut_graph(mixed[0][0], mixed[1][0], group[0, 0], g), 10), "mixed")


def test_argument_errors_launch_nothing(torch_cuda):
    """Every GCS_EINVAL case of the header (the list of tests/test_region_adjacency.py) with real buffers: nothing is written."""
    import test_region_adjacency as cpu
    torch, lib = torch_cuda, _lib()
    ls = torch.zeros((1, 4, 4), dtype=torch.int32, device="cuda")
    bufs = dict(ws=_ab(torch, 2 ** 16), eo=_ab(torch, 2 ** 12), vo=_ab(torch, 2 ** 12), co=_ab(torch, 64), ed=_ab(torch, 2 ** 12),
                vd=_ab(torch, 2 ** 12), cd=_ab(torch, 64), gd=_ab(torch, 2 ** 12))
    ptrs = {name: t.data_ptr() for name, t in bufs.items()}
    n = cpu.argument_errors(lib, ls.data_ptr(), ptrs, torch.cuda.current_stream().cuda_stream)
    assert n >= 30
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xAB).all() for t in bufs.values()) and int(ls.abs().sum()) == 0


# ---- the tree and the public graph

def _fixture_image(shape=(481, 321)):
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    i = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == shape][0]
    return val["img_" + i].copy()


@pytest.mark.parametrize("nodes", ["superpixels", "components"])
def test_every_merge_row_joins_two_adjacent_regions(torch_cuda, nodes):
    """One val image, colour bank, 300 superpixels. For every written merge row t, (a_t, b_t) is an edge of the cut with t rows
    applied (R = alive - t); the group table of that cut is made on the host (every leaf's current rep: any relabelling is a group
    table). With strength = U (the contour map): every leaf edge's strength is the sum of the restated U over its crossings, at
    least 2 length s(a, b), and exactly that for an edge whose s(a, b) is the largest of any edge at a or b (U on both sides of its
    crossings is then s(a, b) itself: U(p) is the largest s between p's label and a neighbour's). SPEC.md §20's worked example shows
    why the equality cannot hold for every edge: edge (0, 2) there has strength 5 at length 2 and s = 1. In "components" mode the
    graph is planar: count <= 3 nodes - 6."""
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    img = _fixture_image()
    kw = dict(n_superpixels=300, n_iter=4, **COLOUR)
    if nodes == "components":
        kw["tree_nodes"] = "components"
    seg = Segmenter(**kw)
    dev = torch.from_numpy(img[None]).cuda()
    labels, merges, _, alive = seg.region_tree_device(dev)
    u = seg.contour_map_device(labels, merges, alive)
    k = int(merges.shape[1]) + 1
    edges, vals, count = seg.region_adjacency_device(labels, K=k, imgs=dev, strength=u)
    lab, mg, al, un = labels[0].cpu().numpy(), merges[0].cpu().numpy(), int(alive[0]), u[0].cpu().numpy()
    n = int(count[0])
    assert n > 0
    e, v = edges[0, :n].cpu().numpy(), vals[0, :n].cpu().numpy().view(np.uint64)
    we, wv = ar.leaf_graph(lab, k, img, cm.contour_map(lab, mg, al))
    assert np.array_equal(un, cm.contour_map(lab, mg, al)) and np.array_equal(e, we) and np.array_equal(v, wv)
    s = cm.strengths(mg, k, al)
    s_ab = s[e[:, 0], e[:, 1]].astype(np.uint64)
    assert (v[:, 2] >= 2 * v[:, 0] * s_ab).all()
    top = np.zeros(k, np.uint64)
    np.maximum.at(top, e[:, 0], s_ab)
    np.maximum.at(top, e[:, 1], s_ab)
    dominant = (s_ab >= top[e[:, 0]]) & (s_ab >= top[e[:, 1]])
    assert dominant.sum() >= 1 and (v[dominant, 2] == 2 * v[dominant, 0] * s_ab[dominant]).all()
    if nodes == "components":
        used = len(np.unique(lab[(lab >= 0) & (lab < k)]))
        assert n <= max(1, 3 * used - 6)
    written = [t for t in range(k - 1) if mg[t, 0] >= 0]
    assert written == list(range(len(written))) and len(written) >= 1
    root = np.arange(k, dtype=np.int32)
    groups = []
    for t in written:
        groups.append(root.copy())
        a, b = mg[t]
        assert root[a] == a and root[b] == b and a < b
        root[root == b] = a
    for lo in range(0, len(groups), 64):
        chunk = np.stack(groups[lo:lo + 64])[:, None, :]
        ce, _, cc = seg.cut_adjacency_device(edges, vals, count, torch.from_numpy(chunk).cuda())
        ce, cc = ce.cpu().numpy(), cc.cpu().numpy()
        for j in range(chunk.shape[0]):
            t = lo + j
            assert cc[j, 0] >= 1 and mg[t].tolist() in ce[j, 0, :cc[j, 0]].tolist(), (t, mg[t].tolist())


def test_segment_regions_with_adjacency_and_unchanged_calls(torch_cuda):
    """segment_regions(adjacency=True) on a fixture image against the restatement on the returned labels; segment_regions without
    the flag and region_props_device return the same bytes before and after an adjacency call on the same plan."""
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd.segmenter import _plan
    torch = torch_cuda
    img = _fixture_image()
    kw = dict(n_superpixels=300, n_regions=8, n_iter=4, **COLOUR)
    labels0, table0 = pkg.segment_regions(img, **kw)
    assert "adjacency" not in table0
    seg = _plan(dict(kw))
    dev, lab_d = torch.from_numpy(img[None]).cuda(), torch.from_numpy(labels0[None]).cuda()
    props0 = [t.cpu().numpy() for t in seg.region_props_device(dev, lab_d)]
    labels, table = pkg.segment_regions(img, adjacency=True, **kw)
    assert np.array_equal(labels, labels0) and set(table) == set(table0) | {"adjacency"}
    k = int(labels.max()) + 1
    assert k == 8
    we, wv = ar.leaf_graph(labels, k, img)
    adj = table["adjacency"]
    assert set(adj) == {"pairs", "length", "mean_contrast", "mean_strength", "degree", "neighbours"}
    assert np.array_equal(adj["pairs"], we) and np.array_equal(adj["length"], wv[:, 0].astype(np.int64))
    assert np.array_equal(adj["mean_contrast"], wv[:, 1].astype(np.float64) / wv[:, 0].astype(np.float64))
    assert (adj["mean_strength"] == 0).all() and adj["degree"].sum() == 2 * len(we)
    edges, vals, count = seg.region_adjacency_device(lab_d, imgs=dev)          # K and capacity from the map
    assert tuple(edges.shape) == (1, min(64, k * (k - 1) // 2), 2) and int(count[0]) == len(we)
    assert np.array_equal(vals[0, :len(we)].cpu().numpy().view(np.uint64), wv)
    labels1, table1 = pkg.segment_regions(img, **kw)
    props1 = [t.cpu().numpy() for t in seg.region_props_device(dev, lab_d)]
    assert labels1.tobytes() == labels0.tobytes() and set(table1) == set(table0)
    assert all(table1[name].tobytes() == table0[name].tobytes() for name in table0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(props0, props1))
    with pytest.raises(ValueError):
        seg.region_adjacency_device(lab_d.to(torch.int64))
    with pytest.raises(ValueError):
        seg.region_adjacency_device(lab_d, capacity=16385)
    tiny = seg.region_adjacency_device(lab_d, capacity=1)
    with pytest.raises(ValueError, match="capacity="):
        pkg.adjacency_table(tiny[0][0].cpu().numpy(), tiny[1][0].cpu().numpy(), int(tiny[2][0]))


def test_both_calls_inside_a_captured_graph(torch_cuda):
    """The header promises "capturable": the leaf call and the cuts call captured into one graph, replayed twice on changed inputs."""
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    seg = Segmenter(n_iter=2)
    ops, k, cap, b, h, w = seg.ops, 9, 36, 2, 19, 23
    rng = np.random.default_rng(50)
    lab = torch.empty((b, h, w), dtype=torch.int32, device="cuda")
    img = torch.empty((b, h, w, 3), dtype=torch.uint8, device="cuda")
    plane = torch.empty((b, h, w), dtype=torch.int32, device="cuda")
    group = torch.from_numpy(np.stack([np.arange(k) % 4, np.arange(k) // 5]).astype(np.int32)[:, None].repeat(b, 1)).cuda()
    edges = torch.empty((b, cap, 2), dtype=torch.int32, device="cuda")
    vals = torch.empty((b, cap, 3), dtype=torch.int64, device="cuda")
    count = torch.empty((b,), dtype=torch.int32, device="cuda")
    ce = torch.empty((2, b, cap, 2), dtype=torch.int32, device="cuda")
    cv = torch.empty((2, b, cap, 3), dtype=torch.int64, device="cuda")
    cc = torch.empty((2, b), dtype=torch.int32, device="cuda")
    ws, cws = ops.adjacency_buffers(b, cap), ops.adjacency_buffers(2 * b, cap)

    def both():
        ops.region_adjacency(lab, img, plane, b, h, w, k, ws, edges, vals, count)
        ops.region_adjacency_cuts(edges, vals, count, group, b, k, 4, cws, ce, cv, cc)

    def fresh(seed):
        r = np.random.default_rng(seed)
        return r.integers(0, k, (b, h, w)).astype(np.int32), _rand_img(seed, b, h, w), _rand_plane(seed + 1, b, h, w)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for t, a in zip((lab, img, plane), fresh(60)):
            t.copy_(torch.from_numpy(a))
        both()                                                     # (warm-up outside the capture)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            both()
    for seed in (61, 62):
        want = fresh(seed)
        for t, a in zip((lab, img, plane), want):
            t.copy_(torch.from_numpy(a))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for i in range(b):
            we, wv = ar.leaf_graph(want[0][i], k, want[1][i], want[2][i])
            _same_table((edges[i].cpu().numpy(), vals[i].cpu().numpy().view(np.uint64), int(count[i])), ar.table(we, wv, cap), (seed, i))
            for c in range(2):
                _same_table((ce[c, i].cpu().numpy(), cv[c, i].cpu().numpy().view(np.uint64), int(cc[c, i])),
                            ar.table(*ar.cut_graph(we, wv, group[c, i].cpu().numpy(), 4), cap), (seed, c, i))
