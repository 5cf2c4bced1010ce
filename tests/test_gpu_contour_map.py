"""GPU contour map of the region tree and the sweep over all its cuts (SPEC.md §15): gcs_region_tree_contours and
gcs_boundary_sweep_resident against the restatement (tests/contour_map_ref.py), everything ``==``, no tolerance anywhere: hand-made
trees through both table paths, trees of gcs_region_tree itself, odd shapes, the edge cases of K and of the labels, the defining
property against gcs_region_tree_cut on the device, the three histograms, the scores against the per-cut scorer, the host paths,
and the existing paths before and after."""
import os

import numpy as np
import pytest

import contour_map_ref as cm
import region_tree_ref as rt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
TREES = {"chain": cm.chain, "star": cm.star, "balanced": cm.balanced}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _gpu_map(torch, lab, merges, alive, k):
    """lab (B, H, W), merges (B, k - 1, 2) or None (k = 1: a NULL pointer), alive (B,) -> U (B, H, W) host array. Workspace and output
    start out as garbage."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    lab = np.ascontiguousarray(lab, np.int32)
    b, h, w = lab.shape
    ls = torch.from_numpy(lab).cuda()
    ms = None if merges is None else torch.from_numpy(np.ascontiguousarray(merges, np.int32).reshape(b, k - 1, 2)).cuda()
    al = torch.from_numpy(np.ascontiguousarray(alive, np.int32).reshape(b)).cuda()
    need = lib.gcs_region_tree_contours_workspace_bytes(b, k)
    assert need > 0
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full((b, h, w), -9, dtype=torch.int32, device="cuda")
    rc = lib.gcs_region_tree_contours(ls.data_ptr(), None if ms is None else ms.data_ptr(), al.data_ptr(), b, h, w, k, ws.data_ptr(),
                                      out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy()


def _check_map(torch, lab, merges, alive, k):
    lab = np.asarray(lab)
    got = _gpu_map(torch, lab, merges, alive, k)
    for i in range(lab.shape[0]):
        m = np.zeros((0, 2), np.int32) if merges is None else np.asarray(merges).reshape(lab.shape[0], k - 1, 2)[i]
        want = cm.contour_map(lab[i], m, int(np.asarray(alive).reshape(-1)[i]))
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()), got[i].ravel()[:8].tolist(), want.ravel()[:8].tolist())
    return got


# ---- the map

@pytest.mark.parametrize("tree", sorted(TREES))
def test_hand_made_trees_on_4096_one_pixel_labels(torch_cuda, tree):
    """K = 4096 on 64 x 64: the deepest forest (chain), the widest group (star), the table's top level (balanced); pos and the table
    are read from the workspace."""
    lab = np.arange(4096, dtype=np.int32).reshape(1, 64, 64)
    got = _check_map(torch_cuda, lab, TREES[tree](4096)[None], [4096], 4096)
    assert got.max() == 4095 and got.min() >= 1


@pytest.mark.parametrize("tree", sorted(TREES))
def test_hand_made_trees_at_k_40(torch_cuda, tree):
    """K = 40 on 19 x 23 noise labels: pos and the table sit in LDS."""
    lab = np.random.default_rng(40).integers(0, 40, (2, 19, 23)).astype(np.int32)
    merges = np.stack([TREES[tree](40)] * 2)
    _check_map(torch_cuda, lab, merges, [40, 40], 40)


def _gpu_tree(torch, x, lab, k):
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    b, d, h, w = x.shape
    xs = torch.from_numpy(np.ascontiguousarray(x).astype(np.uint16).view(np.int16)).cuda()
    ls = torch.from_numpy(np.ascontiguousarray(lab, np.int32)).cuda()
    ws = torch.empty(lib.gcs_region_tree_workspace_bytes(b, h, w, d, k), dtype=torch.uint8, device="cuda")
    merges = torch.empty((b, k - 1, 2), dtype=torch.int32, device="cuda")
    alive = torch.empty((b,), dtype=torch.int32, device="cuda")
    rc = lib.gcs_region_tree(xs.data_ptr(), ls.data_ptr(), b, h, w, d, k, ws.data_ptr(), merges.data_ptr(), None, alive.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    return ls, merges, alive


def test_tree_of_the_library_on_1961_one_pixel_labels(torch_cuda):
    """37 x 53 one-pixel labels, features up to 46 339: the tree gcs_region_tree builds, K = 1961 (no side a multiple of a tile)."""
    rng = np.random.default_rng(7)
    x = rng.integers(0, 46340, (1, 12, 37, 53)).astype(np.uint16)
    lab = np.arange(37 * 53, dtype=np.int32).reshape(1, 37, 53)
    ls, merges, alive = _gpu_tree(torch_cuda, x, lab, 1961)
    m, a = merges.cpu().numpy(), alive.cpu().numpy()
    assert a.tolist() == [1961] and (m >= 0).all()
    _check_map(torch_cuda, lab, m, a, 1961)


_BSD = {}


def _bsd(torch, shape):
    """One val fixture image of ``shape`` through the plan: (id, segmenter, labels, merges, alive, contours) device tensors, once."""
    if shape not in _BSD:
        from gabor_color_image_segmentation_amd import Segmenter
        val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
        i = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == shape][0]
        seg = Segmenter(n_superpixels=300, n_iter=4, **COLOUR)
        lab, merges, _, alive = seg.region_tree_device(torch.from_numpy(val["img_" + i][None]).cuda())
        _BSD[shape] = (i, seg, lab, merges, alive, seg.contour_map_device(lab, merges, alive))
    return _BSD[shape]


@pytest.mark.parametrize("shape", [(481, 321), (321, 481)])
def test_bsd_fixture_image(torch_cuda, shape):
    i, seg, lab, merges, alive, contours = _bsd(torch_cuda, shape)
    want = cm.contour_map(lab[0].cpu().numpy(), merges[0].cpu().numpy(), int(alive[0]))
    got = contours[0].cpu().numpy()
    assert contours.dtype == torch_cuda.int32 and np.array_equal(got, want), (i, int((got != want).sum()))
    assert got.max() == int(alive[0]) - 1 and 0.02 < (got > 0).mean() < 0.5


@pytest.mark.parametrize("shape", [(1, 4), (4, 1), (1, 4096), (37, 53)])
def test_shapes(torch_cuda, shape):
    lab = np.random.default_rng(shape[1]).integers(0, 40, (2,) + shape).astype(np.int32)
    _check_map(torch_cuda, lab, np.stack([cm.balanced(40), cm.chain(40)]), [40, 40], 40)


def test_worked_example_and_the_smallest_k(torch_cuda):
    got = _check_map(torch_cuda, np.arange(4).reshape(1, 1, 4), np.array([[[1, 2], [0, 1], [0, 3]]]), [4], 4)
    assert got.tolist() == [[[2, 2, 3, 3]]]
    # K = 1: no rows, a NULL merges pointer; the map is 0 wherever no out-of-range label is involved
    lab = np.zeros((1, 9, 13), np.int32)
    lab[0, 4, 6] = 1
    lab[0, 0, 0] = -1
    got = _check_map(torch_cuda, lab, None, [1], 1)
    assert int((got != 0).sum()) == 5 + 3 and set(np.unique(got).tolist()) == {0, 1}
    assert not _check_map(torch_cuda, np.zeros((2, 9, 13), np.int32), None, [1, 1], 1).any()
    # K = 2
    lab = (np.random.default_rng(2).integers(0, 2, (1, 9, 13))).astype(np.int32)
    assert _check_map(torch_cuda, lab, np.array([[[0, 1]]]), [2], 2).max() == 1
    assert _check_map(torch_cuda, lab, np.array([[[-1, -1]]]), [2], 2).max() == 2          # never joined: alive


def _edge_batch():
    """Three 19 x 23 images at K = 40 whose alive differ: noise with unused labels; a label in two pieces among six; out-of-range
    labels, negative and >= K, among noise."""
    rng = np.random.default_rng(23)
    a = rng.integers(0, 40, (19, 23)).astype(np.int32)
    a[a == 17] = 3
    a[a == 30] = 31
    b = np.full((19, 23), 7, np.int32)
    b[:, :3] = 3
    b[:, 20:] = 3
    b[5:9, 8:14] = 12
    b[12:15, 5:18] = np.arange(20, 33)[None, :] % 3 + 20
    c = rng.integers(0, 40, (19, 23)).astype(np.int32)
    c[3, :] = 40
    c[10, 4] = -1
    c[11, 11] = 2 ** 31 - 1
    c[12, 12] = -2 ** 31
    lab = np.stack([a, b, c])
    x = rng.integers(0, 46340, (3, 4, 19, 23))
    trees = [rt.build_tree(x[i], lab[i], 40) for i in range(3)]
    return lab, np.stack([t[0] for t in trees]), np.array([t[2] for t in trees], np.int32)


def test_label_edge_cases(torch_cuda):
    lab, merges, alive = _edge_batch()
    assert alive.tolist()[0] == 38 and alive[1] == 6 and len(set(alive.tolist())) == 3
    _check_map(torch_cuda, lab, merges, alive, 40)
    # an out-of-range column cuts the graph apart: 28 written rows, alive = 30; the two sides never join
    big = np.arange(30, dtype=np.int32).reshape(5, 6).repeat(4, axis=0).repeat(4, axis=1)[:19, :23].copy()
    big[:, 11] = 4096
    m, _, a = rt.build_tree(np.random.default_rng(1).integers(0, 999, (2, 19, 23)), big, 30)
    assert a == 30 and int((m[:, 0] >= 0).sum()) == 28
    got = _check_map(torch_cuda, big[None], m[None], [a], 30)
    assert (got[0][:, 10:13] == 30).all()


def _thick(torch, lab):
    """find_boundaries of a (B, H, W) device label batch with torch."""
    bd = torch.zeros_like(lab, dtype=torch.bool)
    d = lab[:, :, 1:] != lab[:, :, :-1]
    bd[:, :, 1:] |= d
    bd[:, :, :-1] |= d
    d = lab[:, 1:, :] != lab[:, :-1, :]
    bd[:, 1:, :] |= d
    bd[:, :-1, :] |= d
    return bd


def test_thresholds_are_the_boundaries_of_the_library_cuts(torch_cuda):
    """On the device: contours > max(0, alive - R) == the thick boundary of gcs_region_tree_cut's output."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    lab, merges, alive = _edge_batch()
    seg = Segmenter(n_superpixels=64, n_iter=3)
    ls, ms, al = (torch.from_numpy(v).cuda() for v in (lab, merges, alive))
    u = seg.contour_map_device(ls, ms, al)
    for i in range(3):
        for r in sorted({1, 2, 8, int(alive[i]) - 1, int(alive[i]), int(alive[i]) + 2}):
            cut = seg.cut_regions_device(ls, ms, al, r)
            tau = (al - r).clamp(min=0)[:, None, None]
            assert torch.equal((u > tau)[i], _thick(torch, cut)[i]), (i, r)
    for shape in ((481, 321), (321, 481)):
        i, seg, ls, ms, al, u = _bsd(torch, shape)
        a = int(al[0])
        for r in (1, 2, 8, a - 1, a, a + 2):
            assert torch.equal(u > max(0, a - r), _thick(torch, seg.cut_regions_device(ls, ms, al, r))), (shape, r)


# ---- the sweep

def _truth(torch, counts, shape, seed):
    """Ragged synthetic annotator maps -> (list of lists of (H, W) uint16 maps, DeviceTruth)."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth
    rng = np.random.default_rng(seed)
    maps = []
    for n in counts:
        group = []
        for _ in range(n):
            t = np.zeros(shape, np.uint16)
            t[rng.integers(2, shape[0] - 2):, :] += 1
            t[:, rng.integers(2, shape[1] - 2):] += 2
            t[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = 9
            group.append(t)
        maps.append(group)
    flat = np.stack([t for g in maps for t in g])
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    img_of = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    return maps, DeviceTruth(flat, first, img_of, [int(t.max()) + 1 for t in flat])


def _gpu_sweep(torch, u, dt, k):
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    us = torch.from_numpy(np.ascontiguousarray(u, np.int32)).cuda()
    b, h, w = us.shape
    hist = torch.full((b + 2 * dt.t, k + 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda")       # the call zeroes it itself
    rc = lib.gcs_boundary_sweep_resident(us.data_ptr(), dt.planes.data_ptr(), dt.img_of_d.data_ptr(), b, dt.t, h, w, k,
                                         hist.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    raw = hist.cpu().numpy().view(np.uint32)
    ann = raw[b:].reshape(dt.t, 2, k + 1)
    return raw[:b], ann[:, 0], ann[:, 1]


def _check_sweep(torch, u, maps, dt, k):
    hm, hr, hp = _gpu_sweep(torch, u, dt, k)
    t = 0
    for i, group in enumerate(maps):
        wm, wr, wp = cm.histograms(u[i], group, k)
        assert np.array_equal(hm[i], wm), (i, hm[i][:8], wm[:8])
        assert np.array_equal(hr[t:t + len(group)], wr) and np.array_equal(hp[t:t + len(group)], wp), i
        t += len(group)
    return hm, hr, hp


@pytest.mark.parametrize("k", [40, 4096])
def test_sweep_histograms(torch_cuda, k):
    """19 x 23, three images with 1, 3 and 2 annotators: K = 40 counts in LDS, K = 4096 with global atomics."""
    lab, merges, alive = _edge_batch()
    u = np.stack([cm.contour_map(lab[i], merges[i], alive[i]) for i in range(3)])
    maps, dt = _truth(torch_cuda, [1, 3, 2], (19, 23), 5)
    if k == 4096:                                         # the levels of a large tree, up to the last bin
        rng = np.random.default_rng(9)
        u = np.where(rng.random(u.shape) < 0.3, rng.integers(1, 4097, u.shape), 0).astype(np.int32)
        u[0, 0, 0] = 4096
    hm, hr, hp = _check_sweep(torch_cuda, u, maps, dt, k)
    assert hm.sum() == int((u > 0).sum()) and hr.sum() > 0 and hp.sum() > 0
    # an all-zero map; a map holding a value above K and a negative one: counted nowhere
    zero = _check_sweep(torch_cuda, np.zeros_like(u), maps, dt, k)
    assert not any(h.any() for h in zero)
    odd = np.zeros_like(u)
    odd[0, 5, 5], odd[1, 9, 9], odd[2, 3, 20], odd[2, 15, 2] = k + 1, -7, k, 1
    hm, hr, hp = _check_sweep(torch_cuda, odd, maps, dt, k)
    assert hm.sum() == 2 and hm[2][k] == 1 and hm[2][1] == 1 and not hm[:2].any()


@pytest.mark.parametrize("shape", [(481, 321), (321, 481)])
def test_sweep_scores_equal_the_per_cut_scorer(torch_cuda, shape):
    """A BSD fixture image with its real DeviceTruth: the counts as integers and recall / precision / F as floats, ``==``."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import _lib
    from gabor_color_image_segmentation_amd.evaluate_gpu import (all_scores_batch_resident, boundary_sweep_resident, sweep_counts,
                                                                  sweep_scores)
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    lib = _lib.load()
    i, seg, ls, ms, al, u = _bsd(torch, shape)
    dt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz")).to_device([i])
    a = int(al[0])
    regions = [1, 2, 8, a - 1, a, a + 2]
    hists = boundary_sweep_resident(u, al, dt)
    assert hists[0].shape == (1, a + 1) and hists[1].shape == (dt.t, a + 1)
    bd_counts = dt.bd_counts.cpu().numpy()
    counts = sweep_counts(hists, [a], bd_counts, dt.first, regions)
    scratch = torch.empty(lib.gcs_bit_planes_bytes(1, *shape), dtype=torch.uint8, device="cuda")
    for j, r in enumerate(regions):
        cut = seg.cut_regions_device(ls, ms, al, r)
        want = torch.empty(1 + 3 * dt.t, dtype=torch.int64, device="cuda")
        assert lib.gcs_boundary_counts_resident(cut.data_ptr(), dt.planes.data_ptr(), dt.bd_counts.data_ptr(), dt.img_of_d.data_ptr(), 1,
                                                dt.t, shape[0], shape[1], scratch.data_ptr(), want.data_ptr(), None,
                                                torch.cuda.current_stream().cuda_stream) == 0
        assert counts[j].tolist() == want.cpu().numpy().tolist(), (i, r)
        if r == 1:                                        # one region: no boundary pixel, the reference divides by zero
            with pytest.raises(ZeroDivisionError):
                all_scores_batch_resident(cut, dt)
            with pytest.raises(ZeroDivisionError):
                sweep_scores(hists, [a], bd_counts, dt.first, [1])
            continue
        ref = all_scores_batch_resident(cut, dt)[0]
        got = sweep_scores(hists, [a], bd_counts, dt.first, [r])[0][0]
        print(i, r, got)
        for key in ("recall", "precision", "fmeasure"):
            assert got[key] == ref[key], (i, r, key, got[key], ref[key])
    assert dt._uncollected() is None                      # the sweep used buffers of its own


# ---- host paths

def test_host_paths_graph_replay_and_a_side_stream(torch_cuda):
    torch = torch_cuda
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(2, 72, 104, seed=6)
    dev = torch.from_numpy(imgs).cuda()
    kw = dict(n_superpixels=64, n_iter=3)
    seg = Segmenter(**kw)
    contours, alive = seg.contours_device(dev)
    lab, merges, _, alive2 = seg.region_tree_device(dev)
    assert torch.equal(alive, alive2)
    want = np.stack([cm.contour_map(lab[i].cpu().numpy(), merges[i].cpu().numpy(), int(alive[i])) for i in range(2)])
    assert np.array_equal(contours.cpu().numpy(), want)
    soft = pkg.segment_contours(imgs[1], **kw)
    assert soft.dtype == np.float32 and soft.shape == (72, 104) and soft.min() == 0.0 and soft.max() <= 1.0
    assert np.array_equal(soft, want[1].astype(np.float32) / np.float32(int(alive[1])))
    assert np.array_equal(pkg.segment_contours(imgs[0], **kw), want[0].astype(np.float32) / np.float32(int(alive[0])))
    # a plan on a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c2, a2 = Segmenter(**kw).contours_device(dev)
    side.synchronize()
    assert torch.equal(c2, contours) and torch.equal(a2, alive)
    # the contour call captured once and replayed on other labels
    ops = seg.ops
    k = merges.shape[1] + 1
    ws, out = ops.contour_buffers(2, k), torch.empty_like(lab)
    src = lab.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.region_tree_contours(src, merges, alive, 2, 72, 104, k, ws, out)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.region_tree_contours(src, merges, alive, 2, 72, 104, k, ws, out)
    side.synchronize()
    src.copy_(lab.flip(0))
    out.fill_(-1)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    flipped = np.stack([cm.contour_map(lab[1 - i].cpu().numpy(), merges[i].cpu().numpy(), int(alive[i])) for i in range(2)])
    assert np.array_equal(out.cpu().numpy(), flipped)
    with pytest.raises(ValueError):
        ops.region_tree_contours(lab, merges, alive, 2, 72, 104, k, ws, lab)


def test_existing_paths_are_what_they_were(torch_cuda):
    """One label map of the default plan and one tree, before and after the new calls ran in the same process."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import boundary_sweep_resident
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(2, 72, 104, seed=12)
    dev = torch.from_numpy(imgs).cuda()
    plain, tree = Segmenter(n_iter=4), Segmenter(n_superpixels=64, n_iter=3, n_regions=5)
    before = plain.segment_device(dev).clone(), tree.segment_device(dev).clone(), [t.clone() for t in tree.region_tree_device(dev)]
    contours, alive = tree.contours_device(dev)
    maps, dt = _truth(torch, [2, 1], (72, 104), 3)
    hists = boundary_sweep_resident(contours, alive, dt)
    assert hists[0].sum() == int((contours > 0).sum())
    after = plain.segment_device(dev), tree.segment_device(dev), tree.region_tree_device(dev)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert all(torch.equal(x, y) for x, y in zip(before[2], after[2]))
