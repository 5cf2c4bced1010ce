"""The region tree merged by boundary strength (SPEC.md §23) on the CPU: the two worked examples of the section, the restatement
(tests/boundary_tree_ref.py) against a brute force that relabels the map and rebuilds the table of §20 from the pixels before every
round, the cuts and the contour map of its trees, the edge-table cases, the option's argument rules, and the step through the
stand-in ops (tests/boundary_tree_ops.py) in all three ``tree_nodes`` modes. No GPU."""
import numpy as np
import pytest
from scipy import ndimage

import boundary_tree_ref as bt
import component_tree_ref as ct
import contour_map_ref as cm
import region_adjacency_ref as ra
import region_tree_ref as rt


def _connected(lab):
    return all(ndimage.label(lab == v)[1] == 1 for v in np.unique(lab))


def _thick(d):
    bd = np.zeros(d.shape, bool)
    e = d[:, 1:] != d[:, :-1]
    bd[:, 1:] |= e
    bd[:, :-1] |= e
    e = d[1:, :] != d[:-1, :]
    bd[1:, :] |= e
    bd[:-1, :] |= e
    return bd


def test_worked_examples_of_the_section():
    """SPEC.md §23. One row of four one-pixel labels; then three rows in which the edges (0,2) and (1,2) become parallel: their summed
    mean (3968) lies above the tail's 3840, either edge alone would not say so (1408 lies below it, 5248 above)."""
    lab = np.array([[0, 1, 2, 3]])
    g = np.array([[0, 10, 11, 30]], np.int32)
    e, v = ra.leaf_graph(lab, 4, None, g)
    assert e.tolist() == [[0, 1], [1, 2], [2, 3]] and v[:, 0].tolist() == [1, 1, 1] and v[:, 2].tolist() == [10, 21, 41]
    assert [bt.cost(l, s) for l, s in zip(v[:, 0], v[:, 2])] == [1280, 2688, 5248]
    info = {}
    merges, costs, alive = bt.build_tree(lab, 4, g, info=info)
    assert alive == 4 and merges.tolist() == [[0, 1], [0, 2], [0, 3]] and costs.tolist() == [1280, 2688, 5248]
    assert info["rounds"] == 3 and info["edges"] == [3, 2, 1]

    lab = np.array([[0, 1, 1],
                    [2, 2, 2],
                    [3, 3, 3]])
    g = np.array([[1, 1, 1],
                  [10, 40, 40],
                  [0, 0, 0]], np.int32)
    e, v = ra.leaf_graph(lab, 4, None, g)
    assert e.tolist() == [[0, 1], [0, 2], [1, 2], [2, 3]]
    assert v[:, 0].tolist() == [1, 1, 2, 3] and v[:, 2].tolist() == [2, 11, 82, 90]
    assert [bt.cost(l, s) for l, s in zip(v[:, 0], v[:, 2])] == [256, 1408, 5248, 3840]
    merges, costs, alive = bt.build_tree(lab, 4, g)
    # round 1: 0 <-> 1. The edge (0,2) then has l = 3, sigma = 93: floor(128 * 93 / 3) = 3968 > 3840, so 2 picks 3
    assert merges.tolist() == [[0, 1], [2, 3], [0, 2]] and costs.tolist() == [256, 3840, 3968]
    # what keeping one of two parallel edges would give
    assert bt.cost(1, 11) < 3840 < bt.cost(3, 93) < bt.cost(2, 82)


def _brute(lab, k, plane):
    """The definition, with no edge bookkeeping: before every round the map is relabelled by reps and §20's table is made from its
    pixels (the loop form)."""
    cur = np.asarray(lab).astype(np.int64).copy()
    ok = (cur >= 0) & (cur < k)
    alive = len(np.unique(cur[ok]))
    rows, costs = [], []
    while True:
        e, v = ra.leaf_graph_loops(cur, k, None, plane)
        if len(e) == 0:
            break
        pick = {}
        for (a, b), (l, _, s) in zip(e.tolist(), v.tolist()):
            c = (128 * int(s)) // int(l)
            for p, q in ((a, b), (b, a)):
                pick[p] = min(pick.get(p, (c, q)), (c, q))
        pairs = sorted((c, a, b) for a, (c, b) in pick.items() if a < b and pick[b][1] == a)
        assert pairs
        for c, a, b in pairs:
            rows.append((a, b))
            costs.append(c)
        for _, a, b in pairs:
            cur[cur == b] = a
    merges = np.full((k - 1, 2), -1, np.int32)
    merges[:len(rows)] = np.array(rows, np.int32).reshape(-1, 2)
    out = np.zeros(k - 1, np.uint64)
    out[:len(costs)] = costs
    return merges, out, alive


def _random_case(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(2, 13)), int(rng.integers(2, 13))
    k = int(rng.integers(2, 41))
    side = int(rng.integers(1, 4))
    lab = rng.integers(0, k, size=(-(-h // side), -(-w // side))).repeat(side, axis=0).repeat(side, axis=1)[:h, :w]
    plane = rng.choice(np.array([0, 0, 0, 1, 2, 2, 5, 7, 7, 100, -3], np.int32), size=(h, w))     # many ties and zeros, a negative
    return lab, k, plane


@pytest.mark.parametrize("seed", range(40))
def test_restatement_equals_the_brute_force_on_random_maps(seed):
    lab, k, plane = _random_case(seed)
    info = {}
    merges, costs, alive = bt.build_tree(lab, k, plane, info=info)
    bm, bc, ba = _brute(lab, k, plane)
    assert alive == ba and np.array_equal(merges, bm) and np.array_equal(costs, bc)
    assert info["edges"] == sorted(info["edges"], reverse=True)                # contraction never adds an edge
    n = int((merges[:, 0] >= 0).sum())
    assert (merges[:n, 0] < merges[:n, 1]).all() and (merges[n:] == -1).all() and not costs[n:].any()


@pytest.mark.parametrize("seed", range(12))
def test_cuts_are_nested_counted_and_connected_and_the_contour_map_knows_them(seed):
    lab, k, plane = _random_case(100 + seed)
    n_map = ct.nodes(lab, 0)                                                   # connected nodes, as "components" / "clusters" have
    kk = int(n_map.max()) + 1
    merges, costs, alive = bt.build_tree(n_map, kk, plane)
    assert alive == kk and (merges[:alive - 1, 0] >= 0).all()                  # a connected map merges down to one region
    u = cm.contour_map(n_map, merges, alive)
    prev = None
    for r in range(alive + 2, 0, -1):
        cut = rt.cut(n_map, merges, alive, r)
        assert len(np.unique(cut)) == min(alive, r) == cut.max() + 1 and _connected(cut), r
        assert np.array_equal(u > max(0, alive - r), _thick(cut)), r           # SPEC.md §15
        if prev is not None:                                                   # nested: a region of the finer cut lies in one of this
            assert all(len(np.unique(cut[prev == v])) == 1 for v in np.unique(prev)), r
        prev = cut
    # the raw map (labels need not be connected): the count holds for the labels that can reach each other
    merges, _, alive = bt.build_tree(lab, k, plane)
    for r in (1, 2, alive, alive + 1):
        assert len(np.unique(rt.cut(lab, merges, alive, r))) == max(min(alive, r), alive - int((merges[:, 0] >= 0).sum()))


def test_edge_table_cases():
    lab = np.array([[0, 0, 5, 5], [2, 2, 5, 5], [2, 2, 7, 7]])
    plane = np.array([[3, 3, 9, 9], [1, 1, 9, 9], [1, 1, 4, 4]], np.int32)
    used = bt.used_labels(lab, 9)
    assert used.tolist() == [1, 0, 1, 0, 0, 1, 0, 1, 0]
    e, v = ra.leaf_graph(lab, 9, None, plane)
    want = bt.build_tree(lab, 9, plane)
    assert want[2] == 4 and (want[0][:3] >= 0).all() and (want[0][3:] == -1).all()         # unused labels: rows past alive - 1
    # count = -1 (more edges than the capacity): alive as defined, no row
    eo, vo, n = ra.table(e, v, 2)
    assert n == -1
    m, c, a = bt.tree_of_table(eo, vo, n, used, 9)
    assert a == 4 and (m == -1).all() and not c.any()
    m, c, a = bt.build_tree(lab, 9, plane, cap=2)
    assert a == 4 and (m == -1).all() and not c.any()
    # a node without edges never merges; K = 1
    m, c, a = bt.tree_of_table(*ra.table(e, v, 8), np.array([1, 1, 1, 0, 0, 1, 0, 1, 1]), 9)
    assert a == 6 and np.array_equal(m, want[0]) and np.array_equal(c, want[1])
    m, c, a = bt.build_tree(np.zeros((3, 3), int), 1, np.ones((3, 3), np.int32))
    assert a == 1 and m.shape == (0, 2) and c.shape == (0,)
    # out-of-range walls cut the graph in two: each side merges, nothing joins them
    lab = np.array([[0, 1, 99, 2, 3], [0, 1, -1, 2, 3]])
    plane = np.array([[1, 1, 50, 2, 2], [1, 1, 50, 2, 2]], np.int32)
    m, c, a = bt.build_tree(lab, 4, plane)
    assert a == 4 and m.tolist() == [[0, 1], [2, 3], [-1, -1]] and c.tolist() == [256, 512, 0]
    assert len(np.unique(rt.cut(lab, m, a, 1))) == 3                                           # two regions and -1
    # rows of one pair add up; rows with a label outside 0 .. K-1, with a = b or with a label not in use are ignored
    edges = np.array([[0, 1], [1, 0], [1, 2], [2, 2], [1, 7], [3, 1], [-1, 0]], np.int32)
    vals = np.array([[1, 0, 10], [1, 0, 30], [1, 9, 30], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]], np.uint64)
    m, c, a = bt.tree_of_table(edges, vals, 7, [1, 1, 1, 0], 4)
    assert a == 3 and m.tolist() == [[0, 1], [0, 2], [-1, -1]] and c.tolist() == [128 * 40 // 2, 128 * 30, 0]
    # the overflow-free division: strengths near 2^32 per crossing
    big = 2 ** 32 - 2
    edges = np.array([[0, 1], [1, 2]], np.int32)
    vals = np.array([[1, 0, big], [3000, 0, 3000 * big - 1]], np.uint64)
    m, c, a = bt.tree_of_table(edges, vals, 2, [1, 1, 1], 3)
    assert m.tolist() == [[1, 2], [0, 1]] and int(c[0]) == (128 * (3000 * big - 1)) // 3000 < 128 * big
    assert int(c[1]) == 128 * big < 2 ** 40


# ---- the option's rules

def _ops(cls=None, **bank_kw):
    from gabor_color_image_segmentation_amd import make_bank
    from boundary_tree_ops import BoundaryTreeOps
    return (cls or BoundaryTreeOps)(make_bank(**bank_kw))


def test_option_rules():
    import gabor_color_image_segmentation_amd as pkg
    from gabor_color_image_segmentation_amd import Segmenter
    from cluster_tree_ops import ClusterTreeOps
    seg = Segmenter(ops=_ops(), n_superpixels=24, n_regions=4, merge_cost="boundary")
    assert seg.merge_cost == "boundary" and seg._opt.boundary
    assert Segmenter(ops=_ops(), n_superpixels=24, n_regions=4).merge_cost == "features"
    assert not Segmenter(ops=_ops(), n_superpixels=24, merge_cost="features")._opt.boundary and not Segmenter(ops=_ops())._opt.boundary
    for kw in (dict(n_superpixels=24), dict(n_superpixels=24, tree_nodes="components"), dict(tree_nodes="clusters")):
        assert Segmenter(ops=_ops(), merge_cost="boundary", **kw)._opt.boundary    # a plan for the tree calls needs no n_regions
    for bad in ("Boundary", "ucm", None, 1, b"boundary"):
        with pytest.raises(ValueError):
            Segmenter(ops=_ops(), n_superpixels=24, n_regions=4, merge_cost=bad)
    with pytest.raises(ValueError):                                                # no tree can exist
        Segmenter(ops=_ops(), merge_cost="boundary")
    with pytest.raises(ValueError):                                                # ops without the stages of §23
        Segmenter(ops=_ops(ClusterTreeOps), tree_nodes="clusters", n_regions=4, merge_cost="boundary")
    img = np.zeros((16, 16, 3), np.uint8)
    for call in (lambda kw: pkg.segment(img, **kw), lambda kw: pkg.segment_batch(img[None], **kw),
                 lambda kw: list(pkg.segment_images([img], **kw)), lambda kw: pkg.segment_regions(img, **kw)):
        for kw in (dict(n_superpixels=24, merge_cost="boundary"), dict(tree_nodes="clusters", merge_cost="boundary"),
                   dict(n_superpixels=24, n_regions=0, merge_cost="boundary"), dict(n_superpixels=24, n_regions=4, merge_cost="x")):
            with pytest.raises(ValueError):
                call(kw)
    import torch
    dev = torch.from_numpy(np.zeros((1, 24, 40, 3), np.uint8))
    for kw in (dict(n_superpixels=24), dict(tree_nodes="clusters")):               # strips and groups keep raising
        seg = Segmenter(ops=_ops(), n_regions=4, merge_cost="boundary", **kw)
        with pytest.raises(ValueError):
            seg.segment_device(dev, dist_group=object())
        with pytest.raises(ValueError):
            seg.segment_rows_sharded_device(dev, 0, 24, 0, 24)


# ---- the step through the stand-in ops

def _names(calls):
    out = []
    for c in calls:
        if not out or not (c[0] == "assign" and out[-1] == "assign"):
            out.append(c[0])
    return out


@pytest.fixture(scope="module")
def fake(built):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = synthetic_batch(2, 24, 40, seed=5)

    def run(cls=None, **more):
        ops = _ops(cls)
        seg = Segmenter(ops=ops, n_iter=3, **more)
        return seg, ops, seg.segment_device(torch.from_numpy(imgs)).numpy()
    return dict(imgs=imgs, run=run)


MODES = {"superpixels": dict(n_superpixels=24), "components": dict(n_superpixels=24, tree_nodes="components"),
         "clusters": dict(tree_nodes="clusters", k=6)}
TAIL = ["gradient", "used", "adjacency", "tree_edges"]


def _leaf_map(imgs, i, mode):
    """(features, node map, K) of the restatements for image i in a mode."""
    import cluster_tree_ref as cl
    import position_ref as pr
    import superpixel_ref as sr
    x = pr.features(imgs[i])
    if mode == "clusters":
        return x, ct.nodes(cl.kmeans_maps(x[None], 6, 3)[0], 0), 4096
    lab = sr.superpixels(x, 24, n_iter=3)
    _, ny, nx = sr.grid(24, 40, 24)
    return (x, ct.nodes(lab, 0), 4096) if mode == "components" else (x, lab, ny * nx)


@pytest.mark.parametrize("mode", list(MODES))
def test_the_step_through_the_fake_ops(fake, mode):
    import torch
    imgs = fake["imgs"]
    seg, ops, got = fake["run"](n_regions=4, merge_cost="boundary", **MODES[mode])
    head = {"superpixels": ["gabor", "unpack", "superpixels"], "components": ["gabor", "unpack", "superpixels", "nodes"],
            "clusters": ["gabor", "assign", "widen", "nodes"]}[mode]
    assert _names(ops.calls) == head + TAIL + ["cut"]
    assert not {"tree", "tree_slab"} & {c[0] for c in ops.calls}               # no statistics, no merge kernel of §14
    assert ("adjacency", 2, _leaf_map(imgs, 0, mode)[2], True) in ops.calls    # the plane is the table's strength, no image
    for i in range(2):
        x, n_map, K = _leaf_map(imgs, i, mode)
        merges, costs, alive = bt.build_tree(n_map, K, bt.gradient(x, 4, 6))
        want = rt.cut(n_map, merges, alive, 4)
        assert np.array_equal(got[i], want), (mode, i)
        assert mode == "superpixels" or (_connected(want) and len(np.unique(want)) == min(alive, 4))
    assert np.array_equal(seg.segment_batch(imgs), got)
    # the tree, its cuts and its contour map through the device API
    ops.calls.clear()
    n_map_d, merges_d, costs_d, alive_d = seg.region_tree_device(torch.from_numpy(imgs))
    assert _names(ops.calls) == head + TAIL
    K = merges_d.shape[1] + 1
    for i in range(2):
        x, n_map, _ = _leaf_map(imgs, i, mode)
        merges, costs, alive = bt.build_tree(n_map, K, bt.gradient(x, 4, 6))
        assert np.array_equal(n_map_d[i].numpy(), n_map) and int(alive_d[i]) == alive
        assert np.array_equal(merges_d[i].numpy(), merges) and np.array_equal(costs_d[i].numpy().view(np.uint64), costs)
    assert np.array_equal(seg.cut_regions_device(n_map_d, merges_d, alive_d, 4).numpy(), got)


def test_features_is_the_plan_of_today(fake):
    for mode, kw in MODES.items():
        _, ops0, got0 = fake["run"](n_regions=4, **kw)
        _, ops1, got1 = fake["run"](n_regions=4, merge_cost="features", **kw)
        assert ops0.calls == ops1.calls and np.array_equal(got0, got1), mode
        assert not set(TAIL) & {c[0] for c in ops0.calls}
        _, ops2, got2 = fake["run"](n_regions=4, merge_cost="boundary", **kw)
        assert got2.shape == got0.shape and [len(np.unique(g)) for g in got2] == [len(np.unique(g)) for g in got0]


def test_segment_regions_computes_the_plane_once(fake):
    import gabor_color_image_segmentation_amd as pkg
    img = fake["imgs"][0]
    ops = _ops()
    labels, table = pkg.segment_regions(img, adjacency=True, gradient=True, ops=ops, n_iter=3, n_regions=4, merge_cost="boundary",
                                        **MODES["components"])
    assert [c[0] for c in ops.calls].count("gradient") == 1 and [c[0] for c in ops.calls].count("gabor") == 1
    x, n_map, K = _leaf_map(fake["imgs"], 0, "components")
    g = bt.gradient(x, 4, 6)
    merges, _, alive = bt.build_tree(n_map, K, g)
    assert np.array_equal(labels, rt.cut(n_map, merges, alive, 4))
    e, v = ra.leaf_graph(labels, 4, img, g)
    adj = table["adjacency"]
    assert len(e) > 0 and np.array_equal(adj["pairs"], e) and np.array_equal(adj["length"], v[:, 0].astype(np.int64))
    assert adj["mean_strength"].tolist() == (v[:, 2].astype(np.float64) / (2.0 * v[:, 0].astype(np.float64))).tolist()
