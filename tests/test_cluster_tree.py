"""The region tree on k-means clusters (SPEC.md §21) on the CPU: the worked example of the section, the restatement
(tests/cluster_tree_ref.py), the option's argument rules with nothing built or launched before they raise, the call sequence of the
step through the stand-in ops (tests/cluster_tree_ops.py: no "unpack"), the region count and connectivity of every cut, and the
per-image scores of tools/cluster_tree_quality.py. No GPU."""
import json
import os

import numpy as np
import pytest
from scipy import ndimage

import cluster_tree_ref as cl
import component_tree_ref as ct
import region_tree_ref as rt

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
QUALITY = os.path.join(HERE, "..", "profiles", "cluster_tree_quality.json")


def _connected(lab):
    return all(ndimage.label(lab == v)[1] == 1 for v in np.unique(lab))


def _raster_numbered(lab):
    _, first = np.unique(lab.ravel(), return_index=True)
    return np.array_equal(np.unique(lab), np.arange(len(first))) and (np.diff(first) > 0).all()


def test_worked_example_of_the_section():
    """SPEC.md §21: a two-cluster L on 4 x 6, one feature plane with the value 10 on cluster 0's pixels of the left piece, 12 on the
    right piece, 40 on the upper piece of cluster 1 and 90 on its lower piece."""
    lab = np.array([[0, 0, 1, 1, 0, 0],
                    [0, 0, 1, 1, 0, 0],
                    [0, 0, 0, 0, 0, 0],
                    [1, 1, 1, 1, 1, 1]])
    x = np.array([[[10, 10, 40, 40, 12, 12],
                   [10, 10, 40, 40, 12, 12],
                   [10, 10, 10, 12, 12, 12],
                   [90, 90, 90, 90, 90, 90]]])
    info = {}
    n_map, merges, costs, alive = cl.tree(x, lab, info=info)
    assert n_map.tolist() == [[0, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0], [2, 2, 2, 2, 2, 2]]
    assert info["components"] == 3 and info["nodes"] == 3 and alive == 3
    # node 0: 14 pixels, sum 7 * 10 + 7 * 12 = 154, mean 11; node 1: 4 pixels of 40; node 2: 6 pixels of 90
    assert (2 * 154 + 14) // 28 == 11
    # costs: (0,1) = 29^2 * 4 = 3364, (0,2) = 79^2 * 6 = 37446; 1 and 2 are not adjacent. 0 <-> 1 is the mutual pair of round 1.
    assert merges.tolist() == [[0, 1], [0, 2]] and int(costs[0]) == 3364
    m01 = (2 * (154 + 160) + 18) // 36                   # = 17
    assert m01 == 17 and int(costs[1]) == (90 - 17) ** 2 * 6 == 31974
    assert cl.regions(x, lab, 2).tolist() == [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]]
    assert np.array_equal(cl.regions(x, lab, 3), n_map) and np.array_equal(cl.regions(x, lab, 0), n_map)
    assert not cl.regions(x, lab, 1).any()
    # min_region_size = 5 joins the 4-pixel node to its neighbour first: two nodes
    assert cl.regions(x, lab, 0, m=5).tolist() == cl.regions(x, lab, 2).tolist()


@pytest.mark.parametrize("seed,h,w,k", [(0, 9, 11, 3), (1, 16, 12, 5), (2, 12, 17, 8), (3, 8, 8, 2), (4, 13, 29, 16)])
def test_every_cut_has_min_nodes_r_connected_regions(seed, h, w, k):
    """The k-means map of random features (C oracle), its node map, every cut of the tree."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4000, size=(4, -(-h // 2), -(-w // 2))).repeat(2, axis=1).repeat(2, axis=2)[:, :h, :w]
    x = (x + rng.integers(0, 300, size=x.shape)).astype(np.uint16)
    lab = cl.kmeans_maps(x[None], k, 4)[0]
    assert lab.shape == (h, w) and lab.max() < k
    info = {}
    n_map, merges, costs, alive = cl.tree(x, lab, info=info)
    assert alive == info["nodes"] >= len(np.unique(lab)) and _connected(n_map) and _raster_numbered(n_map)
    for r in list(range(1, min(alive, 12) + 3)) + [alive, 4096]:
        cut = cl.regions(x, lab, r)
        assert len(np.unique(cut)) == min(alive, r) == cut.max() + 1, r
        assert _connected(cut) and _raster_numbered(cut), r
    assert np.array_equal(cl.regions(x, lab, [2, 0, 3])[1], n_map)


# ---- the option's rules

class _Ops:
    """What Segmenter needs to build a plan; no stage is reached."""
    smoothing, chroma_gain = 0.0, 0

    def __init__(self, bank):
        self.bank = bank
        self.built = []

    def _never(self, *a, **kw):
        self.built.append(a)
        raise AssertionError("the argument checks come before any buffer or launch")

    feature_slab = label_slab = partial_slab = gabor_features = region_tree_buffers = region_tree_slab = region_tree_cut = _never
    region_nodes_buffers = region_nodes = superpixels = region_tree = _never


def _plan(**kw):
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    return Segmenter(ops=_Ops(make_bank()), **kw)


def test_argument_rules_raise_before_anything_is_built():
    import torch
    seg = _plan(tree_nodes="clusters", n_regions=8, k=16)
    assert seg.tree_nodes == "clusters" and seg._opt.clusters and not seg._opt.components and seg.n_regions == 8
    assert _plan(tree_nodes="clusters")._opt.n_regions == 0 and not _plan()._opt.clusters
    for bad in (dict(tree_nodes="clusters", n_superpixels=300), dict(tree_nodes="clusters", n_superpixels=300, n_regions=8),
                dict(n_regions=8), dict(n_regions=8, tree_nodes="superpixels"), dict(tree_nodes="components"),
                dict(tree_nodes="components", n_regions=8), dict(tree_nodes="nodes"), dict(tree_nodes=None),
                dict(tree_nodes="clusters", n_regions=4097), dict(tree_nodes="clusters", n_regions=-1),
                dict(tree_nodes="clusters", n_regions=2.5)):
        with pytest.raises(ValueError):
            _plan(**bad)
    imgs = np.zeros((1, 72, 104, 3), np.uint8)
    dev = torch.from_numpy(imgs)
    with pytest.raises(ValueError):
        seg.segment_device(dev, dist_group=object())
    with pytest.raises(ValueError):
        seg.segment_rows_sharded_device(dev, 0, 72, 0, 72)
    with pytest.raises(ValueError):
        seg.segment_owned_rows_device(dev, 72)
    with pytest.raises(ValueError):
        seg.segment_batch(np.zeros((1, 4100, 16, 3), np.uint8))
    for kw in (dict(), dict(n_regions=257), dict(min_region_size=5)):               # uint8: only with 1 <= R <= 256
        plan = _plan(tree_nodes="clusters", **kw)
        with pytest.raises(ValueError):
            plan.segment_batch(imgs, out_dtype=np.uint8)
        with pytest.raises(ValueError):
            list(plan.segment_images([imgs[0]], out_dtype=np.uint8))
        with pytest.raises(ValueError):
            list(plan.segment_stream([imgs], out_dtype=np.uint8))
        assert not plan.ops.built and not plan._ws and not plan._graphs
    assert not seg.ops.built and not seg._ws and not seg._graphs
    assert seg._check_args(imgs, "global", np.uint8) == np.uint8                  # one rank's global codebook is allowed
    assert not seg._post_passes and not _plan(tree_nodes="clusters", connectivity=True, min_region_size=4)._post_passes

    from gabor_color_image_segmentation_amd import Segmenter, make_bank

    class NoSlabTree:                                    # the tree of §14 and the node map, but no tree from the slab
        smoothing, chroma_gain, bank = 0.0, 0, make_bank()
        region_tree_buffers = region_tree = region_tree_cut = region_nodes_buffers = region_nodes = None
    assert Segmenter(ops=NoSlabTree(), tree_nodes="clusters").n_regions == 0
    with pytest.raises(ValueError):
        Segmenter(ops=NoSlabTree(), tree_nodes="clusters", n_regions=4)

    class NoNodes:
        smoothing, chroma_gain, bank = 0.0, 0, make_bank()
    with pytest.raises(ValueError):
        Segmenter(ops=NoNodes(), tree_nodes="clusters")


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
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from cluster_tree_ops import ClusterTreeOps
    imgs = synthetic_batch(2, 24, 40, seed=5)

    def run(**more):
        ops = ClusterTreeOps(make_bank())
        seg = Segmenter(ops=ops, n_iter=3, **more)
        return seg, ops, seg.segment_device(torch.from_numpy(imgs)).numpy()
    return dict(imgs=imgs, run=run)


def test_call_sequence_and_result_through_the_fake_ops(fake):
    import torch
    imgs = fake["imgs"]
    seg, ops, got = fake["run"](tree_nodes="clusters", n_regions=4, k=6)
    assert _names(ops.calls) == ["gabor", "assign", "widen", "nodes", "tree_slab", "cut"]
    assert "unpack" not in [c[0] for c in ops.calls] and "connected" not in [c[0] for c in ops.calls]
    assert ops.calls[-3:] == [("nodes", 0), ("tree_slab", 2, 4096), ("cut", 2, 4096, 4)]
    assert ("widen", "torch.int32") in ops.calls
    want = cl.segment_batch(imgs, 4, k=6, n_iter=3)
    assert np.array_equal(got, want) and sorted(np.unique(got[0]).tolist()) == [0, 1, 2, 3]
    assert np.array_equal(seg.segment_batch(imgs), want)
    u8 = seg.segment_batch(imgs, out_dtype=np.uint8)
    assert u8.dtype == np.uint8 and np.array_equal(u8, want)
    # post-pass options join the node map (m) or do nothing (connectivity): nothing runs behind the cut
    seg, ops, got = fake["run"](tree_nodes="clusters", n_regions=4, k=6, min_region_size=6, connectivity=True)
    assert _names(ops.calls) == ["gabor", "assign", "widen", "nodes", "tree_slab", "cut"] and ("nodes", 6) in ops.calls
    assert np.array_equal(got, cl.segment_batch(imgs, 4, k=6, n_iter=3, m=6))
    # n_regions = 0: the node map itself, no tree
    seg, ops, got = fake["run"](tree_nodes="clusters", k=6)
    assert _names(ops.calls) == ["gabor", "assign", "widen", "nodes"]
    assert np.array_equal(got, cl.segment_batch(imgs, 0, k=6, n_iter=3))
    # one rank's global codebook
    seg, ops, _ = fake["run"](tree_nodes="clusters", n_regions=3, k=6)
    glob = seg.segment_device(torch.from_numpy(imgs), mode="global").numpy()
    assert np.array_equal(glob, cl.segment_batch(imgs, 3, k=6, n_iter=3, mode="global"))
    # the tree and its cuts through the device API: K = the node count rounded up to a multiple of 64
    ops.calls.clear()
    n_map, merges, costs, alive = seg.region_tree_device(torch.from_numpy(imgs))
    assert _names(ops.calls) == ["gabor", "assign", "widen", "nodes", "tree_slab"]
    K = merges.shape[1] + 1
    assert K % 64 == 0 and K - 64 < int(alive.max()) <= K and ops.calls[-1] == ("tree_slab", 2, K)
    assert np.array_equal(n_map.numpy(), cl.segment_batch(imgs, 0, k=6, n_iter=3))
    assert np.array_equal(seg.cut_regions_device(n_map, merges, alive, 3).numpy(), cl.segment_batch(imgs, 3, k=6, n_iter=3))


def test_the_option_unset_gives_the_calls_of_today(fake):
    _, ops0, got0 = fake["run"](k=6)
    _, ops1, got1 = fake["run"](k=6, tree_nodes="superpixels")
    assert ops0.calls == ops1.calls and _names(ops0.calls) == ["gabor", "assign", "widen"]
    assert np.array_equal(got0, got1)
    from oracle import spec_oracle as so
    assert np.array_equal(got0[0], so.segment(fake["imgs"][0], k=6, n_iter=3))


# ---- quality (profiles/cluster_tree_quality.json, written by tools/cluster_tree_quality.py)

def test_quality_table_counts_and_means():
    doc = json.load(open(QUALITY))
    assert doc["images"] == 24 and doc["regions"] == [4, 6, 8, 12, 16, 32]
    for row in doc["rows"]:
        assert row["exact_counts"] and row["regions"] == row["n_regions"], row
    r8 = [r for r in doc["rows"] if r["setting"] == "colour" and r["k"] == 16 and r["n_regions"] == 8]
    assert len(r8) == 1
    per = doc["per_image"]["colour_k16"]
    keys = list(per[doc["ids"][0]]["8"])                 # the means are the tool's: of the per-image rows (24 x 12, axis 0)
    mean = np.array([[per[i]["8"][k] for k in keys] for i in doc["ids"]]).mean(axis=0)
    for key, m in zip(keys, mean):
        assert r8[0][key] == float(m), key
    for t in doc["tree"]["colour_k16"].values():
        assert t["nodes"] <= 4096 and t["guard"] == (t["components"] > 4096)


def test_quality_scores_of_two_val_images_are_reproduced():
    """The per-image R = 8 scores of the k = 16 colour rows, from the restatement alone, on the image of either orientation with the
    fewest nodes (the plain-Python tree takes a second per thousand nodes and round)."""
    import position_ref as pr
    from gabor_color_image_segmentation_amd.evaluate import metrics, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(QUALITY))
    bank = doc["settings"]["colour"]
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    trees = doc["tree"]["colour_k16"]
    for shape in ((321, 481), (481, 321)):
        i = min((i for i in doc["ids"] if val["img_" + i].shape[:2] == shape), key=lambda i: trees[i]["nodes"])
        x = pr.features(val["img_" + i], bank["color_weight"], bank["chroma_gain"], bank["position_weight"], 4, bank["n_orient"])
        lab = cl.kmeans_maps(x[None], 16, doc["n_iter"])[0]
        info = {}
        n_map, merges, _, alive = cl.tree(x, lab, info=info)
        assert (info["nodes"], info["components"], info["rounds"]) == tuple(trees[i][k] for k in ("nodes", "components", "rounds"))
        cut = np.ascontiguousarray(rt.cut(n_map, merges, alive, 8), dtype=np.int32)
        assert len(np.unique(cut)) == 8 and _connected(cut) and _raster_numbered(cut)
        m = metrics(None, cut, truth[i])
        m.set_metrics()
        got = dict(m.get_metrics(), **region_agreement(cut, truth[i]))
        for key in ("recall", "precision", "fmeasure", "PRI", "VoI", "covering", "regions"):
            assert float(got[key]) == doc["per_image"]["colour_k16"][i]["8"][key], (i, key)
