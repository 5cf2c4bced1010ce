"""The region tree on connected regions (SPEC.md §18) on the CPU: the node map of tests/component_tree_ref.py and its guard, the
worked example of the section, the cuts of the tree on it (exactly min(nodes, R) labels, each 4-connected, numbered in raster order
of first pixel), the per-image scores of tools/component_tree_quality.py, and the option's argument rules that need no device."""
import json
import os

import numpy as np
import pytest
from scipy import ndimage

import component_tree_ref as ct
import region_tree_ref as rt
from oracle import spec_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _connected(lab):
    """Is every label of ``lab`` one 4-connected piece?"""
    return all(ndimage.label(lab == v)[1] == 1 for v in np.unique(lab))


def _raster_numbered(lab):
    """Are the labels 0 .. n-1 in raster order of their first pixel?"""
    _, first = np.unique(lab.ravel(), return_index=True)
    return np.array_equal(np.unique(lab), np.arange(len(first))) and (np.diff(first) > 0).all()


def _random_map(rng, h, w, n_labels):
    """Labels whose pieces are scattered: a coarse random map with single pixels flipped."""
    lab = rng.integers(0, n_labels, size=(-(-h // 3), -(-w // 3))).repeat(3, axis=0).repeat(3, axis=1)[:h, :w]
    flip = rng.random((h, w)) < 0.15
    lab[flip] = rng.integers(0, n_labels, size=int(flip.sum()))
    return lab


WORKED = np.array([[0, 0, 1, 1, 0, 0],
                   [0, 2, 1, 3, 3, 0],
                   [4, 4, 1, 3, 5, 5],
                   [4, 4, 4, 6, 6, 5]])


def test_worked_example_of_the_section():
    """SPEC.md §18's example: label 0 lies in two pieces, C = 8; no guard at K_cap >= 8; m = 3; the guard at K_cap = 7."""
    info = {}
    cc = np.array([[0, 0, 1, 1, 2, 2], [0, 3, 1, 4, 4, 2], [5, 5, 1, 4, 6, 6], [5, 5, 5, 7, 7, 6]])
    assert np.array_equal(ct.nodes(WORKED, 0, 4096, info), cc) and info == dict(components=8, min_size=0, nodes=8)
    assert np.array_equal(ct.nodes(WORKED, 0, 8, info), cc) and info["min_size"] == 0
    assert np.array_equal(ct.nodes(WORKED, 3, 4096, info),
                          [[0, 0, 1, 1, 2, 2], [0, 3, 1, 4, 4, 2], [3, 3, 1, 4, 5, 5], [3, 3, 3, 3, 3, 5]])
    assert info == dict(components=8, min_size=3, nodes=6)
    for m in (0, 2, 4):                                  # ceil(24 / 7) = 4 takes over from any smaller m
        assert np.array_equal(ct.nodes(WORKED, m, 7, info),
                              [[0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 0, 1]])
        assert info == dict(components=8, min_size=4, nodes=2)
    assert ct.nodes(WORKED, 5, 7, info).max() == 0 and info["min_size"] == 5      # a larger m stays


@pytest.mark.parametrize("h,w,n_labels", [(8, 8, 3), (13, 29, 5), (1, 40, 4), (40, 1, 4), (24, 24, 50)])
def test_node_map_properties(h, w, n_labels):
    from merge_ref import merge_small_regions
    rng = np.random.default_rng(h * 100 + w)
    lab = _random_map(rng, h, w, n_labels)
    cc = so.connected_regions(lab)
    c = int(cc.max()) + 1
    for k_cap in sorted({1, 2, max(1, c // 3), max(1, c - 1), c, c + 1, 4096}):
        for m in (0, 1, 2, 7):
            info = {}
            n_map = ct.nodes(lab, m, k_cap, info)
            guard = -(-h * w // k_cap)
            assert info["components"] == c
            assert info["min_size"] == (max(m, guard) if c > k_cap else m)          # the guard triggers exactly when C > k_cap
            assert info["nodes"] <= k_cap and info["nodes"] == len(np.unique(n_map))
            assert _connected(n_map) and _raster_numbered(n_map)
            assert np.array_equal(n_map, merge_small_regions(lab, info["min_size"]))
            if m <= 1 and c <= k_cap:
                assert np.array_equal(n_map, cc)                                    # §7 as it is


@pytest.mark.parametrize("seed,h,w,d,k_cap", [(0, 9, 11, 3, 4096), (1, 16, 12, 2, 4096), (2, 12, 17, 4, 20), (3, 1, 30, 1, 4096)])
def test_every_cut_has_exactly_min_nodes_r_connected_labels(seed, h, w, d, k_cap):
    rng = np.random.default_rng(seed)
    lab = _random_map(rng, h, w, 6)
    x = rng.integers(0, 46340, size=(d, h, w))
    info = {}
    n_map, merges, costs, alive = ct.tree(x, lab, 0, k_cap, info=info)
    assert alive == info["nodes"] <= k_cap and (seed != 2 or info["components"] > k_cap)
    for r in range(1, alive + 3):
        cut = rt.cut(n_map, merges, alive, r)
        assert len(np.unique(cut)) == min(alive, r), r
        assert _connected(cut) and _raster_numbered(cut), r
    assert np.array_equal(rt.cut(n_map, merges, alive, alive), n_map)
    # the tree does not depend on K beyond capacity: a larger K appends unused rows
    big, big_costs, big_alive = rt.build_tree(x, n_map, alive + 37)
    assert big_alive == alive and np.array_equal(big[:alive - 1], merges) and (big[alive - 1:] == -1).all()
    assert np.array_equal(big_costs[:alive - 1], costs) and not big_costs[alive - 1:].any()


def test_quality_scores_of_two_val_images_are_reproduced():
    """The per-image R = 8 scores tools/component_tree_quality.py wrote, from the restatement alone, on one image of either
    orientation (the two with the fewest nodes: the plain-Python tree takes a second per thousand nodes and round)."""
    import position_ref as pr
    import superpixel_ref as sr
    from gabor_color_image_segmentation_amd.evaluate import metrics, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(os.path.join(HERE, "..", "profiles", "component_tree_quality.json")))
    sp = doc["superpixels"]
    assert (sp["n_superpixels"], sp["n_orient"], doc["per_image_n_regions"]) == (300, 5, 8)
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = []
    for shape in ((321, 481), (481, 321)):
        ids.append(min((i for i in doc["ids"] if val["img_" + i].shape[:2] == shape), key=lambda i: doc["tree"][i]["nodes"]))
    for i in ids:
        x = pr.features(val["img_" + i], sp["color_weight"], sp["chroma_gain"], 0, 4, sp["n_orient"])
        info = {}
        n_map, merges, _, alive = ct.tree(x, sr.superpixels(x, 300, sp["spatial_weight"], doc["n_iter"]), info=info)
        assert (info["nodes"], info["components"], info["rounds"]) == tuple(doc["tree"][i][k] for k in ("nodes", "components",
                                                                                                          "component_rounds"))
        cut = np.ascontiguousarray(rt.cut(n_map, merges, alive, 8), dtype=np.int32)
        assert len(np.unique(cut)) == 8 and _connected(cut) and _raster_numbered(cut)
        m = metrics(None, cut, truth[i])
        m.set_metrics()
        got = dict(m.get_metrics(), **region_agreement(cut, truth[i]))
        for key in ("recall", "precision", "fmeasure", "PRI", "VoI", "covering", "regions"):
            assert float(got[key]) == doc["per_image"][i][key], (i, key, got[key], doc["per_image"][i][key])


def test_every_table_cut_had_exactly_r_labels():
    doc = json.load(open(os.path.join(HERE, "..", "profiles", "component_tree_quality.json")))
    assert doc["images"] == 24 and all(t["exact_counts"] and t["nodes"] <= 4096 for t in doc["tree"].values())
    for row in doc["rows"]:
        if row["tree_nodes"] == "components":
            assert row["regions"] == row["used"] == row["n_regions"]


def test_option_rules_that_need_no_device():
    """The checks of ``tree_nodes`` come before the first use of the device: they hold with the stand-in ops too."""
    from fake_ops import OracleOps
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.bank import make_bank
    ops = OracleOps(make_bank())
    assert Segmenter(ops=ops).tree_nodes == "superpixels" and Segmenter(ops=ops, tree_nodes="superpixels")._opt.components is False
    for bad in ("components", "pixels", None, 1):        # n_superpixels = 0; not one of the two strings
        with pytest.raises(ValueError):
            Segmenter(ops=ops, tree_nodes=bad)
    with pytest.raises(ValueError):                      # (the stand-in has no superpixel stage: as n_superpixels > 0 alone)
        Segmenter(ops=ops, n_superpixels=64, tree_nodes="components")
