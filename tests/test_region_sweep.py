"""SPEC.md §16 without a GPU: the restatement (tests/region_sweep_ref.py: leaf table, row additions, §8's terms per cut) against
``evaluate.region_agreement`` of the relabelled cut (tests/region_tree_ref.py) for every R, PRI ``==`` and VoI / covering within
1e-12 (the bound every test of §8 uses between two summation orders); the edge cases of the merge list; ``ods_ois(best="min")``;
the host finishing step; the argument checks of gcs_region_sweep, which launch nothing."""
import ctypes as C

import numpy as np
import pytest

import contour_map_ref as cm
import region_sweep_ref as rs
import region_tree_ref as rt
from gabor_color_image_segmentation_amd import evaluate as ev

TREES = {"chain": cm.chain, "star": cm.star, "balanced": cm.balanced}
TOL = 1e-12


def check_against_relabelled_cuts(lab, merges, alive, truths, regions, k=None):
    """The rule of the issue for one image: per R, the restatement's finished scores against region_agreement of the cut map."""
    sums, terms = rs.sweep(lab, merges, alive, truths, regions, k=k)
    worst = 0.0
    for j, r in enumerate(regions):
        got = ev.agreement_from_sums(sums[j], terms[j], [0, len(truths)], np.asarray(lab).size)[0]
        want = ev.region_agreement(rt.cut(lab, merges, alive, r), truths)
        assert got["PRI"] == want["PRI"], (r, got, want)
        for key in ("VoI", "covering"):
            worst = max(worst, abs(got[key] - want[key]))
            assert abs(got[key] - want[key]) <= TOL, (r, key, got[key], want[key])
    return sums, terms, worst


@pytest.mark.parametrize("tree", sorted(TREES))
def test_k_40_every_r(tree):
    lab, truths = rs.noise_case()
    _, _, worst = check_against_relabelled_cuts(lab, TREES[tree](40), 40, truths, list(range(1, 43)))
    print(tree, "largest difference", worst)


@pytest.mark.parametrize("tree", sorted(TREES))
def test_k_4096_one_pixel_labels(tree):
    lab, truths = rs.one_pixel_case()
    sums, _, worst = check_against_relabelled_cuts(lab, TREES[tree](4096), 4096, truths, [1, 2, 3, 8, 64, 1000, 4095, 4096, 5000])
    print(tree, "largest difference", worst)
    assert (sums[:, :, 0] == 4096).all()
    assert sums[0, 0, 1] == 4096 ** 2 and sums[7, 0, 1] == 4096 and sums[8, 0, 1] == 4096      # one region; the leaves, twice


def test_bsd_sized_blocks():
    lab, truths = rs.block_case()
    x = np.random.default_rng(3).integers(0, 999, (2,) + lab.shape)
    merges, _, alive = rt.build_tree(x, lab, 294)
    assert alive == 294 and (merges >= 0).all()
    _, _, worst = check_against_relabelled_cuts(lab, merges, alive, truths, [1, 2, 4, 6, 8, 12, 16, 32, 293, 294, 300])
    print("largest difference", worst)


def test_unused_labels_and_a_label_in_two_pieces():
    rng = np.random.default_rng(23)
    a = rng.integers(0, 40, (19, 23)).astype(np.int32)
    a[a == 17] = 3
    a[a == 30] = 31                                          # 38 of 40 labels own a pixel
    b = np.full((19, 23), 7, np.int32)
    b[:, :3] = 3
    b[:, 20:] = 3                                            # label 3 in two pieces
    b[5:9, 8:14] = 12
    b[12:15, 5:18] = np.arange(20, 33)[None, :] % 3 + 20
    _, truths = rs.noise_case(seed=5)
    x = rng.integers(0, 46340, (2, 4, 19, 23))
    for i, lab in enumerate((a, b)):
        merges, _, alive = rt.build_tree(x[i], lab, 40)
        assert alive == (38, 6)[i] and (merges[alive - 1:] == -1).all()
        check_against_relabelled_cuts(lab, merges, alive, truths, list(range(1, alive + 3)))


def test_skipped_rows():
    """(-1, -1) rows among the written ones are skipped as the cut skips them; a row that is not (a < b, both reps) changes nothing."""
    lab, truths = rs.noise_case(seed=8, k=6, shape=(9, 11))
    holes = np.array([[1, 2], [-1, -1], [0, 1], [-1, -1], [3, 4]], np.int32)
    check_against_relabelled_cuts(lab, holes, 6, truths, [1, 2, 3, 4, 5, 6, 7])
    clean = np.array([[1, 2], [0, 1], [3, 4], [0, 3], [0, 5]], np.int32)
    #            ok      b = 2 is dead  a = 2 is dead  a > b    a == b   b >= K   ok
    bad = [[1, 2], [0, 2], [2, 3], [4, 3], [3, 3], [0, 6], [0, 1]]
    assert rs.written_rows(bad, 6, 7) == [(1, 2), (0, 1)]
    leaf = rs.leaf_table(lab, truths[0], 6)
    want = leaf.copy()
    want[0] = leaf[0] + leaf[1] + leaf[2]
    want[1] = want[2] = 0
    assert np.array_equal(rs.cut_table(leaf, bad, 7), want)
    assert np.array_equal(rs.cut_table(leaf, bad, 7), rs.cut_table(leaf, clean, 2))
    assert np.array_equal(rs.cut_table(leaf, bad, 1), rs.cut_table(leaf, bad, 6))              # rows 1 .. 5 change nothing
    # a row whose absorber was dead is skipped, so its b stays a rep and a later row may still take it
    later = [[0, 1], [1, 2], [0, 2]]
    assert rs.written_rows(later, 6, 3) == [(0, 1), (0, 2)]


def test_k_1():
    lab = np.zeros((5, 7), np.int32)
    _, truths = rs.noise_case(seed=2, shape=(5, 7))
    sums, terms, _ = check_against_relabelled_cuts(lab, np.zeros((0, 2), np.int32), 1, truths, [1, 2, 9])
    assert np.array_equal(sums[0], sums[2]) and np.array_equal(terms[0], terms[2])


def test_worked_example_of_the_spec():
    lab = np.arange(4).reshape(1, 4)
    merges = np.array([[1, 2], [0, 1], [0, 3]])
    g = np.array([[0, 0, 1, 1]])
    sums, terms = rs.sweep(lab, merges, 4, [g], [4, 3, 2, 1])
    assert sums[:, 0].tolist() == [[4, 4, 8, 4], [4, 6, 8, 4], [4, 10, 8, 6], [4, 16, 8, 8]]
    assert terms[:, 0].tolist() == [[0.0, 4.0, 0.0, 2.0], [2.0, 4.0, 0.0, 2.0], [3 * np.log2(3.0), 4.0, 2.0, 2 * (2 / 3) + 1.0],
                                    [8.0, 4.0, 4.0, 2.0]]
    got = [ev.agreement_from_sums(sums[j], terms[j], [0, 1], 4)[0] for j in range(4)]
    assert [d["PRI"] for d in got] == [1 - 4 / 12, 1 - 6 / 12, 1 - 6 / 12, 1 - 8 / 12]
    assert [d["VoI"] for d in got] == [1.0, 1.5, (3 * np.log2(3.0) + 4.0 - 4.0) / 4, 1.0]
    assert [d["covering"] for d in got] == [0.5, 0.5, (2 * (2 / 3) + 1.0) / 4, 0.5]
    check_against_relabelled_cuts(lab, merges, 4, [g], [1, 2, 3, 4, 5])


# ---- ods_ois(best=...)

def test_ods_ois_min():
    table = [[1.0, 0.5, 0.5, 2.0], [3.0, 0.25, 1.0, 0.25]]
    regions = [16, 8, 4, 2]
    got = ev.ods_ois(table, regions, best="min")
    # image 0: 0.5 at R = 8 and R = 4 -> 4; image 1: 0.25 at R = 8 and R = 2 -> 2; means [2, .375, .75, 1.125] -> R = 8
    assert got == {"OIS": (0.5 + 0.25) / 2, "ODS": 0.375, "ODS_regions": 8, "OIS_regions": [4, 2]}
    tie = ev.ods_ois([[1.0, 1.0, 1.0]], [6, 2, 4], best="min")
    assert tie["ODS_regions"] == 2 and tie["OIS_regions"] == [2]
    assert ev.ods_ois([[1.0, 1.0, 1.0]], [6, 2, 4])["ODS_regions"] == 2
    with pytest.raises(ValueError):
        ev.ods_ois(table, regions, best="lowest")


def test_ods_ois_default_is_unchanged():
    rng = np.random.default_rng(1)
    for _ in range(20):
        table = np.round(rng.random((5, 6)), 1).tolist()                    # one decimal: ties occur
        regions = rng.permutation(np.arange(1, 40))[:6].tolist()
        plain, named = ev.ods_ois(table, regions), ev.ods_ois(table, regions, best="max")
        assert plain == named
        order = sorted(range(6), key=lambda j: regions[j])
        means = [sum(row[j] for row in table) / 5 for j in range(6)]
        jd = max(order, key=lambda q: means[q])
        assert plain["ODS"] == means[jd] and plain["ODS_regions"] == regions[jd]
        assert plain["OIS_regions"] == [regions[max(order, key=lambda q: row[q])] for row in table]
        low = ev.ods_ois([[-v for v in row] for row in table], regions, best="min")
        assert low["ODS_regions"] == plain["ODS_regions"] and low["OIS_regions"] == plain["OIS_regions"] and low["ODS"] == -plain["ODS"]
    # the examples of tests/test_contour_map.py, with and without the keyword
    for kw in ({}, {"best": "max"}):
        res = ev.ods_ois([[0.2, 0.5, 0.4], [0.6, 0.3, 0.4], [0.1, 0.2, 0.4]], [4, 8, 16], **kw)
        assert res["OIS"] == (0.5 + 0.6 + 0.4) / 3 and res["OIS_regions"] == [8, 4, 16]
        assert res["ODS"] == (0.4 + 0.4 + 0.4) / 3 and res["ODS_regions"] == 16
        tie = ev.ods_ois([[0.5, 0.25, 0.5], [0.25, 0.5, 0.25]], [16, 8, 4], **kw)
        assert tie["ODS"] == 0.375 and tie["ODS_regions"] == 4 and tie["OIS_regions"] == [4, 8] and tie["OIS"] == 0.5
        assert ev.ods_ois([[0.3]], [8], **kw) == {"OIS": 0.3, "ODS": 0.3, "ODS_regions": 8, "OIS_regions": [8]}


# ---- the host finishing step

def test_sweep_agreement_orders_and_checks():
    from gabor_color_image_segmentation_amd.evaluate_gpu import sweep_agreement
    lab, truths = rs.noise_case()
    merges = cm.balanced(40)
    regions = [8, 40, 2]
    s0, t0 = rs.sweep(lab, merges, 40, truths[:2], regions)
    s1, t1 = rs.sweep(lab[::-1], merges, 40, truths[2:], regions)
    sums, terms = np.concatenate([s0, s1], axis=1), np.concatenate([t0, t1], axis=1)
    got = sweep_agreement(sums, terms, [0, 2, 3], lab.size, regions)
    assert len(got) == 2 and all(len(row) == 3 for row in got)
    for j, r in enumerate(regions):
        assert got[0][j] == ev.agreement_from_sums(s0[j], t0[j], [0, 2], lab.size)[0]
        assert got[1][j] == ev.agreement_from_sums(s1[j], t1[j], [0, 1], lab.size)[0]
        assert got[0][j]["PRI"] == ev.region_agreement(rt.cut(lab, merges, 40, r), truths[:2])["PRI"]
    broken = sums.copy()
    broken[1, 2, 0] -= 1                                      # one cut of one map did not count every pixel
    with pytest.raises(ValueError):
        sweep_agreement(broken, terms, [0, 2, 3], lab.size, regions)
    with pytest.raises(ValueError):
        sweep_agreement(sums, terms, [0, 2, 3], lab.size, regions[:2])
    with pytest.raises(ValueError):
        sweep_agreement(sums, terms, [0, 2], lab.size, regions)


# ---- the C entry points: bad arguments launch nothing

@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def test_region_sweep_validates_before_launching(lib):
    one = C.c_void_p(16)                                      # non-NULL dummy, never dereferenced

    def call(hist=one, merges=one, alive=one, img_of=one, regions=one, b=2, t=5, k=40, stride=7, n_cuts=3, ws=one, sums=one,
             terms=one):
        return lib.gcs_region_sweep(hist, merges, alive, img_of, regions, b, t, k, stride, n_cuts, ws, sums, terms, None)

    for name in ("hist", "merges", "alive", "img_of", "regions", "ws", "sums", "terms"):
        assert call(**{name: None}) == 1, name
        assert b"NULL" in lib.gcs_last_error()
    assert call(hist=None, merges=None, k=1) == 1             # K = 1 excuses a NULL merges pointer only
    for bad in (dict(n_cuts=0), dict(n_cuts=65), dict(n_cuts=-1), dict(k=0), dict(k=4097), dict(t=0), dict(t=1000001), dict(stride=0),
                dict(t=1 << 13, k=1 << 12, stride=1 << 6), dict(t=1000, k=4096, stride=1000)):
        assert call(**bad) == 1, bad
        size = dict(t=5, k=40, stride=7, n_cuts=3)
        size.update(bad)
        assert lib.gcs_region_sweep_workspace_bytes(size["t"], size["k"], size["stride"], size["n_cuts"]) == 0, bad
    assert call(b=0) == 1 and call(b=65536) == 1
    assert lib.gcs_region_sweep_workspace_bytes(5, 40, 7, 3) == 5 * (40 + 7) * 4
    assert lib.gcs_region_sweep_workspace_bytes(1, 1, 1, 1) == 8
    assert lib.gcs_region_sweep_workspace_bytes(1, 4096, 1, 64) > 0
    assert lib.gcs_region_sweep_workspace_bytes((1 << 13) - 1, 1 << 12, 1 << 6, 1) > 0         # just below 2^31 counters


def test_region_sweep_resident_refuses_a_list_that_cannot_be_made_decreasing():
    """The C call reads ``regions_dev`` on the device, so only the host wrapper can refuse a bad list: before anything else runs."""
    import torch
    from gabor_color_image_segmentation_amd.evaluate_gpu import region_sweep_resident

    class Truth:                                              # what the checks read of a DeviceTruth
        b, h, w, t, stride, u8, a_max = 1, 4, 5, 2, 3, True, 2
        device = torch.device("cpu")
    lab = torch.zeros((1, 4, 5), dtype=torch.int32)
    merges = torch.zeros((1, 3, 2), dtype=torch.int32)
    alive = torch.ones(1, dtype=torch.int32)
    for regions in ([4, 4], [], list(range(1, 66)), [0], [4097], [2.5], ["a"], 7):
        with pytest.raises(ValueError):
            region_sweep_resident(lab, merges, alive, Truth, regions)
    for bad in (dict(lab=lab.long()), dict(lab=lab[0]), dict(lab=torch.zeros((1, 4, 6), dtype=torch.int32)),
                dict(merges=merges.long()), dict(merges=merges[:, :, :1]), dict(merges=torch.zeros((2, 3, 2), dtype=torch.int32)),
                dict(alive=alive.long()), dict(alive=torch.ones(2, dtype=torch.int32))):
        args = dict(lab=lab, merges=merges, alive=alive)
        args.update(bad)
        with pytest.raises(ValueError):
            region_sweep_resident(args["lab"], args["merges"], args["alive"], Truth, [4, 2])
