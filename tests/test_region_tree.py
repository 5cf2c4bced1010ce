"""Region tree (SPEC.md §14) on the CPU: the restatement (tests/region_tree_ref.py) against what §14 says on cases small enough to
check by hand, the argument checks and the call order of the host API through the stand-in ops (tests/region_tree_ops.py), and the
quality conditions of the committed table (profiles/region_tree_quality.json). No GPU."""
import json
import os

import numpy as np
import pytest

import region_tree_ref as rt

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
QUALITY = os.path.join(HERE, "..", "profiles", "region_tree_quality.json")


def _one_pixel_labels(h, w):
    return np.arange(h * w, dtype=np.int32).reshape(h, w)


# ---- the rule

def test_worked_example_of_the_spec():
    x = np.array([[[0, 10, 11, 30]]])
    lab = _one_pixel_labels(1, 4)
    info = {}
    merges, costs, alive = rt.build_tree(x, lab, 4, info)
    assert merges.dtype == np.int32 and costs.dtype == np.uint64
    assert merges.tolist() == [[1, 2], [0, 1], [0, 3]] and costs.tolist() == [1, 121, 529] and alive == 4 and info["rounds"] == 3
    assert (2 * 21 + 3) // 6 == 7                        # the mean of {0, 10, 11} under §4's rule
    assert rt.cut(lab, merges, alive, 2).tolist() == [[0, 0, 0, 1]]
    assert rt.cut(lab, merges, alive, 3).tolist() == [[0, 1, 1, 2]]
    assert rt.cut(lab, merges, alive, 1).tolist() == [[0, 0, 0, 0]]
    assert rt.cut(lab, merges, alive, 4).tolist() == [[0, 1, 2, 3]]


def test_tie_rule_on_a_constant_3x3_map():
    """Every cost is 0, so the rep decides: a node picks its adjacent node of smallest rep. Round 1: 0 <-> 1 is the only mutual pair
    (1 picks 0, 0 picks 1; 3 picks 0, 2 picks 1, 4 picks 1, ...). Every later round merges exactly one node into group 0: the
    adjacent node of smallest rep (0's pick; that node picks 0, the smallest rep there is)."""
    x = np.full((2, 3, 3), 9)
    info = {}
    merges, costs, alive = rt.build_tree(x, _one_pixel_labels(3, 3), 9, info)
    assert merges.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [0, 5], [0, 6], [0, 7], [0, 8]]
    assert not costs.any() and alive == 9 and info["rounds"] == 8


def test_constant_24x24_one_pixel_labels_take_575_rounds():
    """alive - 1 rounds is reached: with every cost 0, one pair per round."""
    info = {}
    merges, costs, alive = rt.build_tree(np.full((1, 24, 24), 5), _one_pixel_labels(24, 24), 576, info)
    assert info["rounds"] == 575 and alive == 576 and not costs.any()
    assert (merges[:, 0] == 0).all() and sorted(merges[:, 1].tolist()) == list(range(1, 576))


def test_costs_use_the_whole_64_bits():
    """Two labels of 32 769 and 32 767 pixels with values 0 and 46 339 on 207 planes: one merge whose cost is odd and above 2^53."""
    lab = np.zeros((256, 256), np.int32)
    lab.ravel()[32769:] = 1
    x = np.broadcast_to(np.where(lab == 0, 0, 46339).astype(np.uint16), (207, 256, 256))
    merges, costs, alive = rt.build_tree(x, lab, 2)
    assert merges.tolist() == [[0, 1]] and alive == 2
    assert int(costs[0]) == 207 * 46339 ** 2 * 32767 == 14564659686168249 and int(costs[0]) > 2 ** 53 and int(costs[0]) % 2 == 1
    assert 207 * 46340 ** 2 < 2 ** 39 and 2 ** 39 * 2 ** 23 <= 2 ** 62          # the bounds SPEC.md §14 states


def test_cuts_are_nested_and_have_min_alive_r_labels():
    rng = np.random.default_rng(4)
    lab = rng.integers(0, 40, (20, 31)).astype(np.int32)
    lab[lab == 17] = 3                                   # label 17 unused
    x = rng.integers(0, 46340, (5, 20, 31))
    merges, costs, alive = rt.build_tree(x, lab, 40)
    assert alive == 39 and (merges[:38] >= 0).all() and merges[38].tolist() == [-1, -1] and costs[38] == 0
    assert (merges[:38, 0] < merges[:38, 1]).all() and len(set(merges[:38, 1].tolist())) == 38         # every rep dies once
    prev = None
    for r in range(1, 45):
        cut = rt.cut(lab, merges, alive, r)
        assert cut.dtype == np.int32 and sorted(np.unique(cut).tolist()) == list(range(min(alive, r)))
        if prev is not None and r <= alive:                                  # the cut at r refines the cut at r - 1
            assert len(set(zip(cut.ravel().tolist(), prev.ravel().tolist()))) == r
        prev = cut
    # R >= alive only renumbers: the same partition, numbered in increasing order of the label
    full = rt.cut(lab, merges, alive, 4096)
    assert np.array_equal(full, np.unique(lab, return_inverse=True)[1].reshape(lab.shape))
    assert np.array_equal(full, rt.cut(lab, merges, alive, alive))
    with pytest.raises(ValueError):
        rt.cut(lab, merges, alive, 0)


def test_unused_labels_and_a_label_in_two_pieces():
    """K = 16 with only 3, 7 and 12 in use; label 3 lies in two far-apart pieces and is adjacent through either."""
    lab = np.full((8, 12), 7, np.int32)
    lab[:, :2] = 3
    lab[:, 10:] = 3
    lab[3:5, 4:8] = 12
    x = np.zeros((1, 8, 12), np.int64)
    x[0][lab == 3] = 100
    x[0][lab == 7] = 90
    x[0][lab == 12] = 10
    merges, costs, alive = rt.build_tree(x, lab, 16)
    assert alive == 3 and merges[:2].tolist() == [[3, 7], [3, 12]] and (merges[2:] == -1).all()
    n3, n7, n12 = 32, 56, 8
    assert int(costs[0]) == 10 ** 2 * n3 and not costs[2:].any()
    m37 = (2 * (100 * n3 + 90 * n7) + (n3 + n7)) // (2 * (n3 + n7))
    assert int(costs[1]) == (m37 - 10) ** 2 * n12
    assert np.array_equal(rt.cut(lab, merges, alive, 2), np.where(lab == 12, 1, 0))
    assert rt.adjacency(lab, 16) == {3: {7}, 7: {3, 12}, 12: {7}}


def test_out_of_range_labels_become_minus_one():
    lab = _one_pixel_labels(2, 3).copy()                 # 0 1 2 / 3 4 5
    lab[0, 1] = 99
    lab[1, 1] = -4
    x = np.array([[[0, 7, 50], [1, 7, 60]]])
    merges, costs, alive = rt.build_tree(x, lab, 6)      # the out-of-range column cuts {0, 3} from {2, 5}
    assert alive == 4 and merges[:2].tolist() == [[0, 3], [2, 5]] and costs[:2].tolist() == [1, 100] and (merges[2:] == -1).all()
    assert rt.cut(lab, merges, alive, 1).tolist() == [[0, -1, 1], [0, -1, 1]]           # nothing joins the two sides
    assert rt.cut(lab, merges, alive, 3).tolist() == [[0, -1, 1], [0, -1, 2]]
    assert rt.cut(lab, merges, alive, 6).tolist() == [[0, -1, 1], [2, -1, 3]]
    n, s = rt.node_stats(x, lab, 6)
    assert n.tolist() == [1, 0, 1, 1, 0, 1] and s[:, 0].tolist() == [0, 0, 50, 1, 0, 60]


def test_domain_of_the_restatement():
    with pytest.raises(ValueError):
        rt.build_tree(np.zeros((1, 4, 4)), np.zeros((4, 4), int), 4097)
    with pytest.raises(ValueError):
        rt.build_tree(np.zeros((208, 4, 4)), np.zeros((4, 4), int), 4)
    merges, costs, alive = rt.build_tree(np.zeros((1, 4, 4)), np.zeros((4, 4), int), 1)
    assert merges.shape == (0, 2) and costs.shape == (0,) and alive == 1
    assert not rt.cut(np.zeros((4, 4), int), merges, alive, 3).any()


# ---- the host API (no GPU): argument checks, call order

class _Ops:
    """What Segmenter needs to build a plan; no stage is reached."""
    smoothing, chroma_gain = 0.0, 0

    def __init__(self, bank):
        self.bank = bank

    def superpixels(self, *a, **kw):
        raise AssertionError("the argument checks come before any launch")

    region_tree_buffers = region_tree = region_tree_cut = superpixels


def _plan(**kw):
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    return Segmenter(ops=_Ops(make_bank()), **kw)


def test_value_errors_of_the_host_api():
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    for r in (-1, 4097, 2.5, True, "3", None):
        with pytest.raises(ValueError):
            _plan(n_superpixels=300, n_regions=r)
    with pytest.raises(ValueError):
        _plan(n_regions=8)                               # only on top of the superpixel stage
    assert _plan(n_superpixels=300, n_regions=8).n_regions == 8 and _plan(n_superpixels=300).n_regions == 0 and _plan().n_regions == 0
    assert _plan(n_superpixels=64, n_regions=1).n_regions == 1 and _plan(n_superpixels=64, n_regions=4096).n_regions == 4096

    class NoTree:
        smoothing, chroma_gain, bank = 0.0, 0, make_bank()

        def superpixels(self):
            pass
    assert Segmenter(ops=NoTree(), n_superpixels=64).n_superpixels == 64
    with pytest.raises(ValueError):                      # the stage needs ops that have it
        Segmenter(ops=NoTree(), n_superpixels=64, n_regions=8)
    imgs = np.zeros((1, 72, 104, 3), np.uint8)
    dev = torch.from_numpy(imgs)
    seg = _plan(n_superpixels=300, n_regions=8)
    with pytest.raises(ValueError):
        seg.segment_device(dev, mode="global")
    with pytest.raises(ValueError):
        seg.segment_device(dev, dist_group=object())
    with pytest.raises(ValueError):                      # row strips keep raising, as for §13
        seg.segment_rows_sharded_device(dev, 0, 72, 0, 72)
    with pytest.raises(ValueError):
        seg.segment_owned_rows_device(dev, 72)
    # the uint8 rule: min(K, R) <= 256 (n = 300 on 72 x 104 is a 14 x 21 grid: K = 294)
    many = _plan(n_superpixels=300, n_regions=257)
    with pytest.raises(ValueError):
        many.segment_batch(imgs, out_dtype=np.uint8)
    with pytest.raises(ValueError):
        next(iter(many.segment_images([imgs[0]], out_dtype=np.uint8)))
    with pytest.raises(ValueError):
        _plan(n_superpixels=300).segment_batch(imgs, out_dtype=np.uint8)
    assert seg._superpixel_check(72, 104, "per_image", np.uint8) == (14, 21)            # K = 294 > 256, R = 8: allowed
    assert _plan(n_superpixels=64, n_regions=4096)._superpixel_check(72, 104, "per_image", np.uint8) == (7, 9)
    with pytest.raises(ValueError):
        _plan().region_tree_device(dev)
    for r in (0, -2, 4097, 1.5, True):
        with pytest.raises(ValueError):
            seg.cut_regions_device(torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1, 3, 2), dtype=torch.int32),
                                   torch.zeros(1, dtype=torch.int32), r)


@pytest.fixture(scope="module")
def fake(built):
    """One small batch through the stand-in ops, with and without the option, and the references it should equal."""
    import torch
    import superpixel_ref as sr
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from region_tree_ops import RegionTreeOps
    imgs = synthetic_batch(2, 24, 40, seed=5)
    kw = dict(n_superpixels=24, n_iter=3)
    sp = np.stack([sr.segment(im, 24, n_iter=3) for im in imgs])

    def run(**more):
        ops = RegionTreeOps(make_bank())
        seg = Segmenter(ops=ops, **kw, **more)
        return seg, ops, seg.segment_device(torch.from_numpy(imgs)).numpy()
    return dict(imgs=imgs, sp=sp, run=run, grid=sr.grid(24, 40, 24))


def test_call_order_through_the_fake_ops(fake):
    import position_ref as pr
    from merge_ref import merge_small_regions
    _, ny, nx = fake["grid"]
    k = ny * nx
    seg, ops, got = fake["run"](n_regions=4, min_region_size=6)
    assert [c[0] for c in ops.calls] == ["gabor", "unpack", "superpixels", "tree", "cut", "merge"]
    assert ops.calls[3] == ("tree", 2, k) and ops.calls[4] == ("cut", 2, k, 4) and ops.calls[5] == ("merge", 6)
    for i, im in enumerate(fake["imgs"]):
        want = rt.regions(pr.features(im), fake["sp"][i], k, 4)
        assert sorted(np.unique(want).tolist()) == [0, 1, 2, 3]
        assert np.array_equal(got[i], merge_small_regions(want, 6)), i
    seg, ops, got = fake["run"](n_regions=4, connectivity=True)
    assert [c[0] for c in ops.calls] == ["gabor", "unpack", "superpixels", "tree", "cut", "connected"]
    # segment_batch takes the same path on stand-in ops; the tree and its cuts through the device API
    seg, ops, got = fake["run"](n_regions=3)
    assert np.array_equal(seg.segment_batch(fake["imgs"]), got)
    import torch
    lab, merges, costs, alive = seg.region_tree_device(torch.from_numpy(fake["imgs"]))
    assert np.array_equal(lab.numpy(), fake["sp"]) and merges.shape == (2, k - 1, 2) and costs.dtype == torch.int64
    assert np.array_equal(seg.cut_regions_device(lab, merges, alive, 3).numpy(), got)
    assert np.array_equal(lab.numpy(), fake["sp"])       # the cut went into a fresh tensor


def test_n_regions_zero_gives_the_calls_of_today(fake):
    _, ops0, got0 = fake["run"]()
    _, ops1, got1 = fake["run"](n_regions=0)
    assert ops0.calls == ops1.calls and [c[0] for c in ops0.calls] == ["gabor", "unpack", "superpixels"]
    assert np.array_equal(got0, got1) and np.array_equal(got0, fake["sp"])


# ---- quality (profiles/region_tree_quality.json, written by tools/region_tree_quality.py)

def _row(doc, **want):
    rows = [r for r in doc["rows"] if all(r.get(k) == v for k, v in want.items())]
    assert len(rows) == 1, want
    return rows[0]


def test_quality_conditions_of_the_committed_table():
    doc = json.load(open(QUALITY))
    assert doc["images"] == 24 and len(doc["rows"]) == 1 + 6 * 2 and doc["per_image_n_regions"] == 8
    km, r8 = _row(doc, setting="kmeans"), _row(doc, setting="region_tree", n_regions=8, merge=0)
    assert km["regions"] == 8.0 and r8["regions"] == 8.0 and r8["used"] == 8.0
    assert r8["covering"] > km["covering"] and r8["VoI"] < km["VoI"] and r8["fmeasure"] > km["fmeasure"]
    assert round(r8["covering"], 4) == 0.4346 and round(km["covering"], 4) == 0.3867           # the figures the docs quote
    assert round(r8["VoI"], 3) == 2.469 and round(km["VoI"], 3) == 2.645
    for r in (4, 6, 8, 12, 16, 32):
        assert _row(doc, setting="region_tree", n_regions=r, merge=0)["regions"] == float(r)
    per = doc["per_image"]["raw"]                         # the means are the tool's means of the per-image rows (24 x 12, axis 0)
    keys = list(per[doc["ids"][0]])
    mean = np.array([[per[i][k] for k in keys] for i in doc["ids"]]).mean(axis=0)
    for key, m in zip(keys, mean):
        assert r8[key] == float(m), key


def test_the_restatement_reproduces_three_images_of_the_table(built):
    """tests/region_tree_ref.py on three val images == the per-image scores at R = 8 that the tool wrote."""
    import superpixel_ref as sr
    from gabor_color_image_segmentation_amd.evaluate import metrics, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(QUALITY))
    sp = doc["superpixels"]
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    for i in doc["ids"][:3]:
        lab = rt.segment(val["img_" + i], sp["n_superpixels"], 8, lam=sp["spatial_weight"], w=sp["color_weight"], g=sp["chroma_gain"],
                         n_orient=sp["n_orient"])
        m = metrics(None, lab, pt[i])
        m.set_metrics()
        got, want = m.get_metrics(), doc["per_image"]["raw"][i]
        got.update(region_agreement(lab, pt[i]))
        for key in ("recall", "precision", "fmeasure", "PRI", "VoI", "covering", "regions"):
            assert float(got[key]) == want[key], (i, key, got[key], want[key])
