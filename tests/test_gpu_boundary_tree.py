"""Segmenter(merge_cost="boundary") (SPEC.md §23) on the GPU against tests/boundary_tree_ref.py, bit for bit and never against the
GPU's own output: 64 x 96 crops of two val fixture images (and a mirrored one: a batch of three) in all three ``tree_nodes`` modes
- node map, merges, costs, alive, contour map, cuts, the cost of a row from the cut's own edge table, the small call (captured,
replayed) against eager launches and the restatement -, ``merge_cost="features"`` against the plan without the option, two synthetic
45 x 77 images (no multiple of a tile) in the three modes, and one full 481 x 321 fixture image with ``tree_nodes="clusters"`` at
k = 8."""
import os

import numpy as np
import pytest

import boundary_tree_ref as bt
import cluster_tree_ref as cl
import component_tree_ref as ct
import contour_map_ref as cm
import position_ref as pr
import region_tree_ref as rt
import superpixel_ref as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
H, W, R = 64, 96, 5
MODES = {"superpixels": dict(n_superpixels=48, n_iter=3), "components": dict(n_superpixels=48, n_iter=3, tree_nodes="components"),
         "clusters": dict(tree_nodes="clusters", k=6, n_iter=3)}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_CACHE = {}


def _images():
    if "imgs" not in _CACHE:
        val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
        keys = sorted(k for k in val.files if k.startswith("img_"))
        a, b = val[keys[0]], val[keys[1]]
        crops = [a[40:40 + H, 100:100 + W], b[120:120 + H, 60:60 + W]]
        _CACHE["imgs"] = np.ascontiguousarray(np.stack(crops + [crops[0][:, ::-1]]))
    return _CACHE["imgs"]


def _leaf(mode, i):
    """(G, leaf map, its own K) of the restatements for crop i, computed once."""
    key = (mode, i)
    if key not in _CACHE:
        if ("x", i) not in _CACHE:
            x = pr.features(_images()[i])
            _CACHE[("x", i)] = (x, bt.gradient(x, 4, 6))
        x, g = _CACHE[("x", i)]
        if mode == "clusters":
            lab = ct.nodes(cl.kmeans_maps(x[None], 6, 3)[0], 0)
            k = int(lab.max()) + 1
        else:
            lab = sr.superpixels(x, 48, n_iter=3)
            _, ny, nx = sr.grid(H, W, 48)
            k = ny * nx
            if mode == "components":
                lab = ct.nodes(lab, 0)
                k = int(lab.max()) + 1
        _CACHE[key] = (g, np.ascontiguousarray(lab, np.int32), k)
    return _CACHE[key]


def _tree(mode, i, K):
    key = (mode, i, K)
    if key not in _CACHE:
        g, lab, _ = _leaf(mode, i)
        _CACHE[key] = bt.build_tree(lab, K, g)
    return _CACHE[key]


def _want(mode, r):
    out = []
    for i in range(3):
        g, lab, k = _leaf(mode, i)
        merges, _, alive = _tree(mode, i, k)
        out.append(rt.cut(lab, merges, alive, r))
    return np.stack(out)


def _plan(mode, **kw):
    from gabor_color_image_segmentation_amd import Segmenter
    return Segmenter(merge_cost="boundary", **MODES[mode], **kw)


def _thick(d):
    bd = np.zeros(d.shape, bool)
    e = d[:, 1:] != d[:, :-1]
    bd[:, 1:] |= e
    bd[:, :-1] |= e
    e = d[1:, :] != d[:-1, :]
    bd[1:, :] |= e
    bd[:-1, :] |= e
    return bd


def _groups(merges, t, K):
    """The group (= rep) of every leaf in front of row t."""
    parent = np.arange(K, dtype=np.int64)
    for a, b in merges[:t]:
        parent[b] = a
    root = parent.copy()
    for q in range(K):
        root[q] = root[parent[q]]
    return root.astype(np.int32)


@pytest.mark.parametrize("mode", list(MODES))
def test_tree_cuts_contours_and_costs(torch_cuda, mode):
    torch = torch_cuda
    imgs = _images()
    dev = torch.from_numpy(imgs).cuda()
    seg = _plan(mode)
    n_map, merges, costs, alive = seg.region_tree_device(dev)
    K = merges.shape[1] + 1
    counts = [_leaf(mode, i)[2] for i in range(3)]
    assert K == (counts[0] if mode == "superpixels" else min(4096, -(-max(counts) // 64) * 64))
    plane = seg.edges_device(dev)
    contours = seg.contour_map_device(n_map, merges, alive)
    both, al = seg.contours_device(dev)
    assert torch.equal(both, contours) and torch.equal(al, alive)
    got_map, got_m, got_c = n_map.cpu().numpy(), merges.cpu().numpy(), costs.cpu().numpy().view(np.uint64)
    trees = []
    for i in range(3):
        g, lab, _ = _leaf(mode, i)
        wm, wc, wa = _tree(mode, i, K)
        trees.append((wm, wc, wa))
        assert np.array_equal(plane[i].cpu().numpy(), g) and np.array_equal(got_map[i], lab), i
        assert int(alive[i]) == wa and np.array_equal(got_m[i], wm) and np.array_equal(got_c[i], wc), i
        assert np.array_equal(contours[i].cpu().numpy(), cm.contour_map(lab, wm, wa)), i
    assert all(wa > R for _, _, wa in trees)
    for r in (1, 2, R, 4096):
        cut = seg.cut_regions_device(n_map, merges, alive, r).cpu().numpy()
        for i in range(3):
            wm, _, wa = trees[i]
            assert np.array_equal(cut[i], rt.cut(_leaf(mode, i)[1], wm, wa, r)), (r, i)
            assert np.array_equal(contours[i].cpu().numpy() > max(0, wa - r), _thick(cut[i])), (r, i)
    # the cost of a row, from the edge table of the cut in front of it: three steps per image
    n_rows = [int((wm[:, 0] >= 0).sum()) for wm, _, _ in trees]
    steps = [[0, n // 2, n - 1] for n in n_rows]
    group = np.stack([np.stack([_groups(trees[i][0], steps[i][c], K) for i in range(3)]) for c in range(3)])
    edges, vals, count = seg.region_adjacency_device(n_map, K=K, strength=plane, capacity=16384)
    assert (count.cpu().numpy() >= 0).all()
    ce, cv, cc = seg.cut_adjacency_device(edges, vals, count, torch.from_numpy(group).cuda(), G=K, capacity=16384)
    ce, cv, cc = ce.cpu().numpy(), cv.cpu().numpy().view(np.uint64), cc.cpu().numpy()
    for c in range(3):
        for i in range(3):
            t = steps[i][c]
            a, b = trees[i][0][t]
            rows = ce[c, i, :cc[c, i]]
            hit = np.flatnonzero((rows[:, 0] == a) & (rows[:, 1] == b))
            assert len(hit) == 1, (c, i, t)
            l, _, s = (int(v) for v in cv[c, i, hit[0]])
            assert (128 * s) // l == int(trees[i][1][t]) == int(got_c[i][t]), (c, i, t)


@pytest.mark.parametrize("mode", list(MODES))
def test_host_paths_graph_replay_and_eager(torch_cuda, mode):
    imgs = _images()
    dev = torch_cuda.from_numpy(imgs).cuda()
    want = _want(mode, R)
    seg = _plan(mode, n_regions=R)
    first = seg(imgs[0])                                 # the small call: captured (its warm-up image is all zeros: the chain)
    assert first.dtype == np.int32 and np.array_equal(first, want[0]), int((first != want[0]).sum())
    assert np.array_equal(seg(imgs[0]), want[0]) and np.array_equal(seg(imgs[1]), want[1])          # replayed
    assert any(e["graph"] is not None and e["rt"] is not None and "grad" in e["rt"][0] for e in seg._graphs.values())
    eager = seg.segment_device(dev)                      # eager launches, a batch of three
    assert np.array_equal(eager.cpu().numpy(), want)
    assert np.array_equal(seg.segment_batch(imgs), want)
    assert np.array_equal(seg.segment_batch(imgs[::-1].copy()), want[::-1])
    if mode != "superpixels":                            # exactly min(nodes, R) connected regions
        from scipy import ndimage
        assert all(len(np.unique(w)) == R and all(ndimage.label(w == v)[1] == 1 for v in range(R)) for w in want)


@pytest.mark.parametrize("mode", list(MODES))
def test_features_given_explicitly_is_the_plan_without_the_option(torch_cuda, mode):
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    imgs = _images()
    dev = torch.from_numpy(imgs).cuda()
    a, b = Segmenter(n_regions=R, **MODES[mode]), Segmenter(n_regions=R, merge_cost="features", **MODES[mode])
    assert np.array_equal(a.segment_batch(imgs), b.segment_batch(imgs)) and np.array_equal(a(imgs[0]), b(imgs[0]))
    ta, tb = a.region_tree_device(dev), b.region_tree_device(dev)
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))


def test_segment_regions_and_the_one_shot_rules(torch_cuda):
    import gabor_color_image_segmentation_amd as pkg
    img = _images()[0]
    kw = dict(n_regions=R, merge_cost="boundary", **MODES["clusters"])
    labels, table = pkg.segment_regions(img, adjacency=True, gradient=True, **kw)
    assert np.array_equal(labels, _want("clusters", R)[0]) and np.array_equal(pkg.segment(img, **kw), labels)
    import region_adjacency_ref as ra
    e, v = ra.leaf_graph(labels, R, img, _leaf("clusters", 0)[0])
    adj = table["adjacency"]
    assert np.array_equal(adj["pairs"], e) and np.array_equal(adj["length"], v[:, 0].astype(np.int64))
    assert adj["mean_strength"].tolist() == (v[:, 2].astype(np.float64) / (2.0 * v[:, 0].astype(np.float64))).tolist()
    c = pkg.segment_contours(img, merge_cost="boundary", **MODES["clusters"])
    g, lab, k = _leaf("clusters", 0)
    merges, _, alive = _tree("clusters", 0, k)
    assert np.array_equal(c, (cm.contour_map(lab, merges, alive).astype(np.float32) / np.float32(alive)).astype(np.float32))
    for bad in (dict(merge_cost="boundary", **MODES["clusters"]), dict(merge_cost="boundary", k=6), dict(kw, merge_cost="Boundary")):
        with pytest.raises(ValueError):
            pkg.segment(img, **bad)


SYNTH = {"superpixels": dict(n_superpixels=24, n_iter=3), "components": dict(n_superpixels=24, n_iter=3, tree_nodes="components"),
         "clusters": dict(tree_nodes="clusters", k=5, n_iter=3)}


@pytest.mark.parametrize("mode", list(SYNTH))
def test_synthetic_images(torch_cuda, mode):
    """Two synthetic 45 x 77 images (ragged tiles on both axes): node map, merges, costs, alive, contour map and the delivered labels at
    R = 4 against the restatements."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    torch = torch_cuda
    h, w, r = 45, 77, 4
    imgs = synthetic_batch(2, h, w, seed=7)
    dev = torch.from_numpy(imgs).cuda()
    seg = Segmenter(merge_cost="boundary", **SYNTH[mode])
    n_map, merges, costs, alive = seg.region_tree_device(dev)
    contours = seg.contour_map_device(n_map, merges, alive)
    delivered = Segmenter(merge_cost="boundary", n_regions=r, **SYNTH[mode]).segment_batch(imgs)
    K = merges.shape[1] + 1
    for i in range(2):
        x = pr.features(imgs[i])
        if mode == "clusters":
            lab = ct.nodes(cl.kmeans_maps(x[None], 5, 3)[0], 0)
        else:
            lab = sr.superpixels(x, 24, n_iter=3)
            if mode == "components":
                lab = ct.nodes(lab, 0)
            else:
                assert K == np.prod(sr.grid(h, w, 24)[1:])
        wm, wc, wa = bt.build_tree(lab, K, bt.gradient(x, 4, 6))
        assert wa > r and np.array_equal(n_map[i].cpu().numpy(), lab) and int(alive[i]) == wa, i
        assert np.array_equal(merges[i].cpu().numpy(), wm) and np.array_equal(costs[i].cpu().numpy().view(np.uint64), wc), i
        assert np.array_equal(contours[i].cpu().numpy(), cm.contour_map(lab, wm, wa)), i
        assert np.array_equal(delivered[i], rt.cut(lab, wm, wa, r)), i


def test_one_full_fixture_image_on_clusters(torch_cuda):
    """481 x 321, the default bank, k = 8: the node map, the whole tree and the cut at 8."""
    torch = torch_cuda
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    img = val["img_102061"]                              # (the portrait image with the fewest nodes: the plain-Python tree is quick)
    assert img.shape == (481, 321, 3)
    x = pr.features(img)
    lab = ct.nodes(cl.kmeans_maps(x[None], 8, 10)[0], 0)
    g = bt.gradient(x, 4, 6)
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(tree_nodes="clusters", k=8, merge_cost="boundary")
    n_map, merges, costs, alive = seg.region_tree_device(torch.from_numpy(img[None]).cuda())
    K = merges.shape[1] + 1
    info = {}
    wm, wc, wa = bt.build_tree(lab, K, g, info=info)
    assert np.array_equal(n_map[0].cpu().numpy(), lab) and int(alive[0]) == wa == int(lab.max()) + 1 and info["rounds"] > 3
    assert np.array_equal(merges[0].cpu().numpy(), wm) and np.array_equal(costs[0].cpu().numpy().view(np.uint64), wc)
    got = Segmenter(tree_nodes="clusters", k=8, n_regions=8, merge_cost="boundary").segment_batch(img[None])[0]
    assert np.array_equal(got, rt.cut(lab, wm, wa, 8)) and len(np.unique(got)) == 8
