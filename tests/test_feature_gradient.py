"""The texture-gradient edge map (SPEC.md §22) on the CPU: the two worked examples of the section, the restatement
(tests/feature_gradient_ref.py) on its edge cases, ``evaluate.edge_scores`` against one dilation per threshold, the zero rule, the
host calls (``segment_edges``, ``segment_regions(gradient=True)``, ``Segmenter.edges_device``) through the stand-in ops
(tests/feature_gradient_ops.py) and the per-image scores of tools/feature_gradient_quality.py. No GPU."""
import json
import math
import os

import numpy as np
import pytest

import feature_gradient_ref as fg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
QUALITY = os.path.join(HERE, "..", "profiles", "feature_gradient_quality.json")


def _one_plane(rows, n_scales=1):
    """Canonical features (3 n_scales, H, W) with ``rows[s]`` as channel 0 of scale s (one slot per scale) and zeros elsewhere."""
    rows = [np.asarray(r, np.int64) for r in rows]
    x = np.zeros((3 * n_scales,) + rows[0].shape, np.int64)
    for s, r in enumerate(rows):
        x[s] = r
    return x


# ---- the definition

def test_worked_example_one_level():
    """SPEC.md §22: one row of four pixels, one plane, one level."""
    x = _one_plane([[[0, 10, 11, 30]]])
    assert fg.energy(x, 1, 1).tolist() == [[100, 121, 400, 361]]
    assert fg.gradient(x, 1, 1).tolist() == [[10, 11, 20, 19]]


def test_worked_example_two_levels():
    """SPEC.md §22: the same row on level 0 and a level-1 plane [8, 21] (replicated [8, 8, 21, 21]): the level's 13^2 = 169 counts
    as 169 >> 2 = 42 on each of its pixels' children."""
    x = _one_plane([[[0, 10, 11, 30]], [[0, 0, 0, 0]], [[8, 8, 21, 21]]], n_scales=3)
    (dx0, dy0), (dx1, dy1) = fg.level_terms(x, 3, 1)
    assert dx0.tolist() == [[100, 121, 400, 361]] and dx1.tolist() == [[169, 169]] and not dy0.any() and not dy1.any()
    assert fg.energy(x, 3, 1).tolist() == [[142, 163, 442, 403]]
    assert fg.gradient(x, 3, 1).tolist() == [[11, 12, 21, 20]]
    # without the shift the map would be [16, 17, 23, 23]
    assert [int(np.sqrt(v + 169)) for v in (100, 121, 400, 361)] == [16, 17, 23, 23]


def test_constant_features_give_zero_everywhere():
    for ns, slots, shape in ((4, 6, (9, 13)), (8, 2, (17, 5)), (1, 1, (1, 1))):
        x = np.full((3 * ns * slots,) + shape, 1234, np.uint16)
        assert not fg.gradient(x, ns, slots).any()


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1)])
def test_degenerate_shapes(shape):
    rng = np.random.default_rng(sum(shape))
    ns, slots = 4, 2
    x = rng.integers(0, 46340, size=(3 * ns * slots,) + shape).astype(np.uint16)
    for lv in (1,):                                          # level-1 planes are block-replicated (SPEC.md §3)
        pl = [d for d in range(x.shape[0]) if fg.level_of_plane(d, ns, slots) == lv]
        x[pl] = x[pl][:, ::2, ::2].repeat(2, 1).repeat(2, 2)[:, :shape[0], :shape[1]]
    g = fg.gradient(x, ns, slots)
    assert g.shape == shape and g.dtype == np.int32
    if shape == (1, 1):
        assert g.tolist() == [[0]]                           # every neighbour clamps onto the pixel itself
        return
    # a line: only the differences along it count, the ends use the one-sided difference over ONE step (clamped)
    line = x.astype(np.int64).reshape(x.shape[0], -1)
    want = np.zeros(line.shape[1], np.int64)
    for lv in (0, 1):
        pl = [d for d in range(x.shape[0]) if fg.level_of_plane(d, ns, slots) == lv]
        v = line[pl][:, ::1 << lv]
        n = v.shape[1]
        idx = np.arange(n)
        e = ((v[:, np.minimum(idx + 1, n - 1)] - v[:, np.maximum(idx - 1, 0)]) ** 2).sum(0) >> (2 * lv)
        want += e[np.arange(line.shape[1]) >> lv]
    assert g.ravel().tolist() == [math.isqrt(int(v)) for v in want]


def test_clamping_is_symmetric():
    """Transposing the planes transposes the map (every level); mirroring them mirrors it on a bank of one level (a mirrored
    level-1 grid of an odd-sized image is another grid)."""
    rng = np.random.default_rng(5)
    ns, slots, h, w = 4, 1, 7, 10
    x = rng.integers(0, 5000, size=(3 * ns * slots, -(-h // 2), -(-w // 2))).repeat(2, 1).repeat(2, 2)[:, :h, :w]
    x[[d for d in range(x.shape[0]) if fg.level_of_plane(d, ns, slots) == 0]] = rng.integers(0, 5000, size=(6, h, w))
    g = fg.gradient(x, ns, slots)
    assert np.array_equal(fg.gradient(x.transpose(0, 2, 1), ns, slots), g.T)
    y = rng.integers(0, 46340, size=(6, h, w))
    g1 = fg.gradient(y, 2, 1)
    assert np.array_equal(fg.gradient(y[:, :, ::-1], 2, 1), g1[:, ::-1]) and np.array_equal(fg.gradient(y[:, ::-1], 2, 1), g1[::-1])


def test_the_largest_energy_has_an_exact_root():
    """E = 2 * 207 * 46340^2 - the bound of the section - and its neighbours: floor(sqrt) by Python integers."""
    x = np.zeros((207, 3, 3), np.int64)
    x[:, 0, 1] = x[:, 1, 0] = 46340                          # the centre pixel sees 46340 across both axes on every plane
    e = fg.energy(x, 1, 69)
    assert int(e[1, 1]) == 2 * 207 * 46340 ** 2 < 2 ** 40
    g = int(fg.gradient(x, 1, 69)[1, 1])
    assert g * g <= int(e[1, 1]) < (g + 1) * (g + 1) and g < 2 ** 20


# ---- the scores

def _direct_scores(edges, truth, thresholds):
    """``evaluate.metrics``' boundary arithmetic with ``edges > theta`` as the boundary map: one dilation per threshold."""
    from gabor_color_image_segmentation_amd.evaluate import _dilate, find_boundaries
    out = []
    for th in thresholds:
        bd = edges > th
        if not bd.any():
            out.append((0.0, 0.0, 0.0))
            continue
        img_truth = [find_boundaries(s) for s in truth]
        dil = _dilate(bd, 5)
        recall = 0
        for t in img_truth:
            recall += float(np.sum(dil & t)) / float(np.sum(t))
        recall /= len(img_truth)
        precision = 0
        score = float(np.sum(bd))
        for t in img_truth:
            precision += float(np.sum(bd & _dilate(t, 5))) / score
        precision /= len(img_truth)
        s = recall + precision
        out.append((recall, precision, 0.0 if s == 0 else 2.0 * precision * recall / s))
    return np.array(out).T


@pytest.mark.parametrize("seed,h,w", [(0, 12, 17), (1, 30, 21), (2, 5, 40)])
def test_edge_scores_against_one_dilation_per_threshold(seed, h, w):
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    rng = np.random.default_rng(seed)
    edges = (rng.integers(0, 40, size=(h, w)) * (rng.random((h, w)) < 0.3)).astype(np.int32)
    edges[0, 0] = edges[-1, -1] = 39                         # strong pixels in the corners: the dilation's border rule
    truth = [(np.arange(h)[:, None] // (3 + a) + np.arange(w)[None, :] // (4 + a)).astype(np.uint16) for a in range(3)]
    thresholds = [5, 0, 38, 39, 40, 17, -1, 1000]
    got = edge_scores(edges, truth, thresholds)
    want = _direct_scores(edges, truth, thresholds)
    for key, row in zip(("recall", "precision", "fmeasure"), want):
        assert got[key].dtype == np.float64 and got[key].tolist() == row.tolist(), key


def test_the_zero_rule_and_the_reference_error():
    from gabor_color_image_segmentation_amd.evaluate import edge_scores, edge_scores_from_counts
    truth = [np.arange(48).reshape(6, 8) // 24]
    flat = np.zeros((6, 8), np.int32)
    sc = edge_scores(flat, truth, [0, 3])
    assert all(sc[k].tolist() == [0.0, 0.0] for k in ("recall", "precision", "fmeasure"))
    sc = edge_scores(flat + 2, truth, [1, 2])                # theta = 1: every pixel a boundary pixel; theta = 2: none
    assert sc["recall"].tolist() == [1.0, 0.0] and sc["fmeasure"][1] == 0.0 and 0 < sc["precision"][0] <= 1
    assert edge_scores_from_counts(0.0, [0.0, 5.0, 0.0]) == {"recall": 0.0, "precision": 0.0, "fmeasure": 0.0}
    with pytest.raises(ZeroDivisionError):                   # an annotator map without a boundary pixel: as the reference
        edge_scores(flat + 2, [np.zeros((6, 8), np.int32)], [1])
    with pytest.raises(ZeroDivisionError):
        edge_scores(flat, [], [1])
    with pytest.raises(ValueError):
        edge_scores(flat.astype(np.float32), truth, [1])


# ---- the host calls, through the stand-in

@pytest.fixture(scope="module")
def standin(built):
    from gabor_color_image_segmentation_amd import make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from feature_gradient_ops import FeatureGradientOps
    import position_ref as pr
    img = synthetic_batch(1, 24, 40, seed=11)[0]
    ops = FeatureGradientOps(make_bank(n_scales=4, n_orient=2))
    want = fg.gradient(pr.features(img, 0.0, 0, 0, 4, 2), 4, 2)
    return img, ops, want


def test_segment_edges_normalises_the_map(standin):
    import gabor_color_image_segmentation_amd as pkg
    img, ops, want = standin
    kw = dict(n_scales=4, n_orient=2, ops=ops)
    got = pkg.segment_edges(img, **kw)
    assert got.dtype == np.float32 and got.shape == want.shape and want.max() > 0
    assert np.array_equal(got, fg.normalised(want)) and got.max() == 1.0 and got.min() >= 0.0
    assert ("gradient", 1) in ops.calls and not any(c[0] in ("assign", "unpack") for c in ops.calls)    # no clustering, no tensor
    flat = pkg.segment_edges(np.full((16, 16, 3), 77, np.uint8), **kw)
    assert flat.dtype == np.float32 and flat.shape == (16, 16) and not flat.any()
    with pytest.raises(ValueError):
        pkg.segment_edges(img[..., 0], **kw)


def test_edges_device_equals_the_restatement_and_refuses_row_strips(standin):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    img, ops, want = standin
    seg = Segmenter(n_scales=4, n_orient=2, ops=ops)
    dev = torch.from_numpy(img[None])
    got = seg.edges_device(dev)
    assert got.dtype == torch.int32 and np.array_equal(got[0].numpy(), want)
    n = len(ops.calls)
    with pytest.raises(ValueError, match="row strips"):
        seg.edges_device(dev, y0=8)
    with pytest.raises(ValueError):
        seg.edges_device(dev[:, :4])                         # smaller than 8 x 8: the entry points' common rule
    with pytest.raises(ValueError):
        seg.edges_device(dev[..., 0])
    assert len(ops.calls) == n                               # refused before any stage


def test_segment_regions_takes_the_map_as_the_strength_plane(standin):
    import gabor_color_image_segmentation_amd as pkg
    import region_adjacency_ref as ra
    img, ops, want = standin
    kw = dict(n_scales=4, n_orient=2, k=4, n_iter=3, ops=ops)
    labels0, table0 = pkg.segment_regions(img, adjacency=True, **kw)
    labels, table = pkg.segment_regions(img, adjacency=True, gradient=True, **kw)
    assert np.array_equal(labels, labels0)
    k = int(labels.max()) + 1
    edges, vals = ra.leaf_graph(labels, k, img, want)
    adj = table["adjacency"]
    assert len(edges) > 0 and np.array_equal(adj["pairs"], edges) and np.array_equal(adj["length"], vals[:, 0].astype(np.int64))
    assert adj["mean_strength"].tolist() == (vals[:, 2].astype(np.float64) / (2.0 * vals[:, 0].astype(np.float64))).tolist()
    assert adj["mean_strength"].max() > 0 and not table0["adjacency"]["mean_strength"].any()
    for key in ("pairs", "length", "mean_contrast", "degree"):
        assert np.array_equal(adj[key], table0["adjacency"][key]), key
    with pytest.raises(ValueError):
        pkg.segment_regions(img, gradient=True, **kw)


# ---- quality (profiles/feature_gradient_quality.json, written by tools/feature_gradient_quality.py)

def test_quality_table_is_consistent():
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    doc = json.load(open(QUALITY))
    assert doc["images"] == 24 and doc["levels"] == 256 and len(doc["rows"]) == 4
    for row in doc["rows"]:
        per = doc["per_image"][row["setting"]]
        assert row["OIS"] == ods_ois([[per[i]["best_f"]] for i in doc["ids"]], [0])["OIS"]
        assert row["ODS"] == ods_ois([[per[i]["f_at_ods"]] for i in doc["ids"]], [0])["ODS"]
        assert abs(row["ODS"] - max(doc["mean_f_per_level"][row["setting"]])) < 1e-12
        assert row["step"] == -(-(max(per[i]["g_max"] for i in doc["ids"]) + 1) // 256)
        assert (row["ODS_threshold"] + 1) % row["step"] == 0 and row["OIS"] >= row["ODS"] > 0


def test_quality_scores_of_the_first_six_images_are_reproduced():
    """Default bank, no smoothing: the maps from the restatements, the scores from ``evaluate.edge_scores`` at the row's ODS
    threshold and at every image's best one."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    import feature_gradient_quality as tool
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    doc = json.load(open(QUALITY))
    name = tool.setting_name("default", 0.0)
    row = [r for r in doc["rows"] if r["setting"] == name][0]
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    for i in doc["ids"][:6]:
        want = doc["per_image"][name][i]
        g = tool.edge_map(val["img_" + i], "default", 0.0)
        assert int(g.max()) == want["g_max"]
        sc = edge_scores(g, truth[i], [row["ODS_threshold"], want["best_threshold"]])
        for key, got in (("f_at_ods", sc["fmeasure"][0]), ("recall_at_ods", sc["recall"][0]),
                         ("precision_at_ods", sc["precision"][0]), ("best_f", sc["fmeasure"][1])):
            assert abs(got - want[key]) <= 1e-12, (i, key, got, want[key])
