"""Contour map of the region tree (SPEC.md §15) on the CPU: the restatement (tests/contour_map_ref.py) against what §15 says - the
worked example, the defining property against the cuts of tests/region_tree_ref.py for every R, the histogram identities against
``evaluate.metrics`` on those cuts -, ``evaluate.ods_ois``, the host logic and call order through the stand-in ops
(tests/contour_map_ops.py), and the argument checks of the C entry points. No GPU."""
import ctypes as C

import numpy as np
import pytest

import contour_map_ref as cm
import region_tree_ref as rt


def _cases():
    """name -> (labels (H, W), merges, alive): trees of the restatement of §14 on random features."""
    rng = np.random.default_rng(15)
    out = {}
    lab = rng.integers(0, 40, (19, 23)).astype(np.int32)
    out["noise"] = (lab, 40)
    lab2 = lab.copy()
    lab2[lab2 == 17] = 3
    lab2[lab2 == 30] = 31                                 # labels 17 and 30 unused
    out["unused"] = (lab2, 40)
    blocks = np.arange(12, dtype=np.int32).reshape(3, 4).repeat(7, axis=0).repeat(7, axis=1)[:19, :23].copy()
    wall = blocks.copy()
    wall[:, 7] = 99
    wall[4, 7] = -3                                      # an out-of-range wall: the graph is cut in two
    out["wall"] = (wall, 12)
    hole = wall.copy()
    hole[9, 7] = 5                                       # the same wall with a hole: one graph again
    out["hole"] = (hole, 12)
    big = np.arange(30, dtype=np.int32).reshape(5, 6).repeat(4, axis=0).repeat(4, axis=1)[:19, :23].copy()
    big[:, 11] = 4096
    out["cut_apart"] = (big, 30)
    res = {}
    for name, (l, k) in out.items():
        x = rng.integers(0, 46340, (3, 19, 23))
        merges, _, alive = rt.build_tree(x, l, k)
        res[name] = (l, merges, alive)
    return res


CASES = _cases()


def _truths(seed, n, shape=(19, 23)):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        t = np.zeros(shape, np.uint16)
        t[rng.integers(3, shape[0] - 3):, :] += 1
        t[:, rng.integers(3, shape[1] - 3):] += 2
        t[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = 7
        out.append(t)
    return out


def test_worked_example_of_the_spec():
    lab = np.arange(4, dtype=np.int32).reshape(1, 4)
    merges = np.array([[1, 2], [0, 1], [0, 3]], np.int32)
    u = cm.contour_map(lab, merges, 4)
    assert u.dtype == np.int32 and u.tolist() == [[2, 2, 3, 3]]
    assert (u > max(0, 4 - 2)).astype(int).tolist() == [[0, 0, 1, 1]]
    s = cm.strengths(merges, 4, 4)
    assert s[1, 2] == 1 and s[0, 2] == 2 and s[3, 1] == 3 and s[2, 2] == 0 and s[0, 4] == 4 and s[4, 4] == 0


def test_the_cut_apart_case_is_the_one_the_spec_names():
    lab, merges, alive = CASES["cut_apart"]
    assert alive == 30 and int((merges[:, 0] >= 0).sum()) == 28 and (merges[28:] == -1).all()
    lab, merges, alive = CASES["wall"]
    assert alive == 12 and int((merges[:, 0] >= 0).sum()) == 10
    lab, merges, alive = CASES["hole"]
    assert alive == 12 and int((merges[:, 0] >= 0).sum()) == 11
    assert CASES["unused"][2] == 38


@pytest.mark.parametrize("name", sorted(CASES))
def test_thresholds_of_the_map_are_the_boundaries_of_every_cut(built, name):
    from gabor_color_image_segmentation_amd.evaluate import find_boundaries
    lab, merges, alive = CASES[name]
    u = cm.contour_map(lab, merges, alive)
    assert u.min() >= 0 and u.max() <= alive
    for r in range(1, alive + 3):
        want = find_boundaries(rt.cut(lab, merges, alive, r))
        assert np.array_equal(u > max(0, alive - r), want), (name, r)
    assert np.array_equal(u > 0, find_boundaries(np.where((lab >= 0) & (lab < len(merges) + 1), lab, -1)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_suffix_sums_of_the_histograms_are_the_counts_of_every_cut(built, name):
    """The three histograms -> the integer counts and the floats of ``evaluate.metrics`` on the cut at every R."""
    from gabor_color_image_segmentation_amd.evaluate import _dilate, find_boundaries, metrics
    from gabor_color_image_segmentation_amd.evaluate_gpu import sweep_counts, sweep_scores
    lab, merges, alive = CASES[name]
    k = len(merges) + 1
    truths = _truths(3, 3)
    u = cm.contour_map(lab, merges, alive)
    hm, hr, hp = cm.histograms(u, truths, k)
    assert hm[0] == 0 and not hr[:, 0].any() and not hp[:, 0].any() and hm.sum() == int((u > 0).sum())
    bd_counts = [int(find_boundaries(t).sum()) for t in truths]
    regions = list(range(1, alive + 3))
    counts = sweep_counts((hm[None], hr, hp), [alive], bd_counts, [0, 3], regions)
    for j, r in enumerate(regions):
        cut = rt.cut(lab, merges, alive, r)
        bd = find_boundaries(cut)
        want = [int(bd.sum())]
        for t in truths:
            tb = find_boundaries(t)
            want += [int((_dilate(bd, 5) & tb).sum()), int(tb.sum()), int((bd & _dilate(tb, 5)).sum())]
        assert counts[j].tolist() == want, (name, r)
    some = [r for r in regions if find_boundaries(rt.cut(lab, merges, alive, r)).any()]
    scores = sweep_scores((hm[None], hr, hp), [alive], bd_counts, [0, 3], some)[0]
    for r, got in zip(some, scores):
        m = metrics(None, rt.cut(lab, merges, alive, r), truths)
        m.set_boundary_recall()
        m.set_boundary_precision()
        m.set_fmeasure()
        assert (got["recall"], got["precision"], got["fmeasure"]) == (m.recall, m.precision, m.fmeasure), (name, r)
    if len(some) < len(regions):                          # a cut without a boundary pixel: what the reference raises
        with pytest.raises(ZeroDivisionError):
            sweep_scores((hm[None], hr, hp), [alive], bd_counts, [0, 3], [1])


def test_values_outside_the_bins_are_counted_nowhere(built):
    u = np.zeros((9, 11), np.int32)
    u[2, 3], u[5, 5], u[7, 1] = 6, -4, 2
    hm, hr, hp = cm.histograms(u, _truths(1, 1, (9, 11)), 5)
    assert hm.tolist() == [0, 0, 1, 0, 0, 0] and hr[0, 0] == 0 and hr.sum() <= 25 and hp[0].sum() <= 1


def test_hand_made_trees():
    for k in (2, 5, 40, 41):
        for rows in (cm.chain(k), cm.star(k), cm.balanced(k)):
            assert rows.shape == (k - 1, 2) and (rows[:, 0] < rows[:, 1]).all() and len(set(rows[:, 1].tolist())) == k - 1
    s = cm.strengths(cm.chain(5), 5, 5)                   # (3,4), (2,3), (1,2), (0,1): 0 joins everything last
    assert s[0].tolist() == [0, 4, 4, 4, 4, 5] and s[3, 4] == 1 and s[2, 4] == 2
    assert cm.strengths(cm.star(5), 5, 5)[3].tolist() == [3, 3, 3, 0, 4, 5]
    assert cm.strengths(cm.balanced(4), 4, 4)[:4, :4].tolist() == [[0, 1, 3, 3], [1, 0, 3, 3], [3, 3, 0, 2], [3, 3, 2, 0]]


def test_ods_ois():
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    f = [[0.2, 0.5, 0.4], [0.6, 0.3, 0.4], [0.1, 0.2, 0.4]]
    res = ods_ois(f, [4, 8, 16])
    assert res["OIS"] == (0.5 + 0.6 + 0.4) / 3 and res["OIS_regions"] == [8, 4, 16]
    assert res["ODS"] == (0.4 + 0.4 + 0.4) / 3 and res["ODS_regions"] == 16
    # ties: the smallest R wins, wherever it stands in the list
    tie = ods_ois([[0.5, 0.25, 0.5], [0.25, 0.5, 0.25]], [16, 8, 4])
    assert tie["ODS"] == 0.375 and tie["ODS_regions"] == 4 and tie["OIS_regions"] == [4, 8] and tie["OIS"] == 0.5
    assert ods_ois([[0.3]], [8]) == {"OIS": 0.3, "ODS": 0.3, "ODS_regions": 8, "OIS_regions": [8]}
    for bad in (([], [8]), ([[0.1, 0.2]], [8]), ([[0.1]], [])):
        with pytest.raises(ValueError):
            ods_ois(*bad)


# ---- the host API through the stand-in ops

@pytest.fixture(scope="module")
def fake(built):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    from contour_map_ops import ContourMapOps
    imgs = synthetic_batch(2, 24, 40, seed=5)
    ops = ContourMapOps(make_bank())
    seg = Segmenter(ops=ops, n_superpixels=24, n_iter=3)
    return dict(imgs=imgs, ops=ops, seg=seg, dev=torch.from_numpy(imgs))


def test_call_order_and_result_through_the_fake_ops(fake):
    import torch
    import position_ref as pr
    import superpixel_ref as sr
    seg, ops = fake["seg"], fake["ops"]
    del ops.calls[:]
    contours, alive = seg.contours_device(fake["dev"])
    _, ny, nx = sr.grid(24, 40, 24)
    k = ny * nx
    assert [c[0] for c in ops.calls] == ["gabor", "unpack", "superpixels", "tree", "contour_buffers", "contours"]
    assert ops.calls[-1] == ("contours", 2, k) and contours.dtype == torch.int32 and tuple(contours.shape) == (2, 24, 40)
    for i, im in enumerate(fake["imgs"]):
        x = pr.features(im)
        lab = sr.superpixels(x, 24, 576, 3)
        merges, _, a = rt.build_tree(x, lab, k)
        assert int(alive[i]) == a and np.array_equal(contours[i].numpy(), cm.contour_map(lab, merges, a)), i
    # from a tree that is already there, into a tensor of the caller's
    lab, merges, _, alive = seg.region_tree_device(fake["dev"])
    del ops.calls[:]
    out = torch.full_like(lab, -1)
    assert seg.contour_map_device(lab, merges, alive, out=out) is out and torch.equal(out, contours)
    assert [c[0] for c in ops.calls] == ["contour_buffers", "contours"]
    # a plan with n_regions keeps its own output: the map is a call of its own
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    from contour_map_ops import ContourMapOps
    ops8 = ContourMapOps(make_bank())
    seg.segment_device(fake["dev"])
    Segmenter(ops=ops8, n_superpixels=24, n_iter=3, n_regions=4).segment_device(fake["dev"])
    assert "contours" not in [c[0] for c in ops8.calls]


def test_value_errors_come_before_any_launch(fake):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, make_bank, segment_contours
    from region_tree_ops import RegionTreeOps
    seg, ops = fake["seg"], fake["ops"]
    lab = torch.zeros((2, 8, 8), dtype=torch.int32)
    merges, alive = torch.zeros((2, 3, 2), dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    del ops.calls[:]
    for bad in ((lab.to(torch.int64), merges, alive), (lab[0], merges, alive), (lab, merges[:1], alive), (lab, merges[:, :, :1], alive),
                (lab, merges, alive[:1]), (lab, torch.zeros((2, 4096, 2), dtype=torch.int32), alive)):
        with pytest.raises(ValueError):
            seg.contour_map_device(*bad)
    assert ops.calls == []
    old = Segmenter(ops=RegionTreeOps(make_bank()), n_superpixels=24)       # ops without the contour map
    with pytest.raises(ValueError):
        old.contour_map_device(lab, merges, alive)
    with pytest.raises(ValueError):
        old.contours_device(fake["dev"])
    assert old.ops.calls == []
    with pytest.raises(ValueError):                       # only on top of the superpixel stage
        Segmenter(ops=ContourOpsNoStage(make_bank())).contours_device(fake["dev"])
    with pytest.raises(ValueError):
        segment_contours(np.zeros((24, 40), np.uint8), n_superpixels=24)
    with pytest.raises(ValueError):
        segment_contours(np.zeros((24, 40, 3), np.float32), n_superpixels=24)
    with pytest.raises(ValueError):
        segment_contours(np.zeros((24, 40, 3), np.uint8))


class ContourOpsNoStage:
    smoothing, chroma_gain = 0.0, 0

    def __init__(self, bank):
        self.bank = bank

    def region_tree_contours(self, *a, **kw):
        raise AssertionError("the argument checks come before any launch")

    region_tree = superpixels = contour_buffers = region_tree_contours


# ---- C ABI: host-only checks

def test_contour_entries_validate_before_launching(built):
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 18 and lib.gcs_abi_version() == 18
    p = [C.c_void_p(q << 24) for q in range(1, 8)]        # non-NULL dummies far apart, never dereferenced
    lab, mer, ali, ws, out = p[:5]
    good = dict(lab=lab, mer=mer, ali=ali, B=2, H=19, W=23, K=40, ws=ws, out=out)

    def contours(**bad):
        a = dict(good, **bad)
        return lib.gcs_region_tree_contours(a["lab"], a["mer"], a["ali"], a["B"], a["H"], a["W"], a["K"], a["ws"], a["out"], None)
    for bad in (dict(lab=None), dict(mer=None), dict(ali=None), dict(ws=None), dict(out=None)):
        assert contours(**bad) == 1, bad
        assert b"NULL" in lib.gcs_last_error()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(K=0), dict(K=4097)):
        assert contours(**bad) == 1, bad
        assert b"shape" in lib.gcs_last_error()
    for off in (0, 4, 2 * 19 * 23 * 4 - 1, -(2 * 19 * 23 * 4 - 1)):
        assert contours(out=C.c_void_p((1 << 24) + off)) == 1, off
        assert b"overlaps" in lib.gcs_last_error()
    assert lib.gcs_region_tree_contours_workspace_bytes(2, 40) >= 2 * 2 * 40 * (1 + 6)
    assert lib.gcs_region_tree_contours_workspace_bytes(1, 4096) >= 2 * 4096 * 13
    assert lib.gcs_region_tree_contours_workspace_bytes(1, 1) > 0
    for args in ((0, 40), (65536, 40), (2, 0), (2, 4097)):
        assert lib.gcs_region_tree_contours_workspace_bytes(*args) == 0
    u, planes, img_of, hist = p[:4]
    good = dict(u=u, planes=planes, img_of=img_of, B=2, T=5, H=19, W=23, K=40, hist=hist)

    def sweep(**bad):
        a = dict(good, **bad)
        return lib.gcs_boundary_sweep_resident(a["u"], a["planes"], a["img_of"], a["B"], a["T"], a["H"], a["W"], a["K"], a["hist"], None)
    for bad in (dict(u=None), dict(planes=None), dict(img_of=None), dict(hist=None)):
        assert sweep(**bad) == 1, bad
        assert b"NULL" in lib.gcs_last_error()
    for bad in (dict(B=0), dict(B=65536), dict(T=0), dict(T=1000001), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(K=0),
                dict(K=4097)):
        assert sweep(**bad) == 1, bad
        assert b"shape" in lib.gcs_last_error()
    assert sweep(T=1000000, K=4096) == 1 and b"2^31" in lib.gcs_last_error()


def test_header_declares_the_new_entry_points():
    import os
    from gabor_color_image_segmentation_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gcs.h")).read()
    for name in ("gcs_region_tree_contours_workspace_bytes", "gcs_region_tree_contours", "gcs_boundary_sweep_resident"):
        assert name + "(" in text and name in _lib.SIGNATURES
    assert "#define GCS_ABI_VERSION 18" in text
