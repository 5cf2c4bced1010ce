"""SPEC.md §19 without a GPU: the restatement (tests/region_props_ref.py) against scipy.ndimage and np.bincount, the tables of the
cuts by adding rows against tabulating the relabelled map, ``region_table``'s rounding, the SPEC's worked example, and the ABI's
list of entry points with their argument checks (which launch nothing)."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage as ndi

import contour_map_ref as cm
import region_props_ref as rp
import region_tree_ref as rt

NAMES = ("gcs_region_props", "gcs_region_props_cuts", "gcs_region_paint")


def _random_case(seed, h, w, k, d):
    rng = np.random.default_rng(seed)
    lab = rng.integers(-1, k + 1, (h, w)).astype(np.int32)        # -1 and k: out of range
    lab[lab == 3] = 4                                              # an unused label
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    feats = rng.integers(0, 46341, (d, h, w)).astype(np.uint16)
    return lab, img, feats


@pytest.mark.parametrize("seed,h,w,k,d", [(1, 19, 23, 12, 3), (2, 1, 70, 5, 0), (3, 40, 9, 7, 1)])
def test_restatement_against_scipy_and_bincount(seed, h, w, k, d):
    lab, img, feats = _random_case(seed, h, w, k, d)
    sums, bbox = rp.leaf_table(lab, k, img, feats)
    assert sums.shape == (k, 6 + d) and sums.dtype == np.uint64 and bbox.shape == (k, 4)
    ok = (lab >= 0) & (lab < k)
    n = np.bincount(lab[ok], minlength=k)
    assert np.array_equal(sums[:, 0], n) and n[3] == 0
    index = np.arange(k)
    safe = np.where(ok, lab, k)                                    # scipy: every out-of-range pixel in a label of its own
    yy, xx = np.mgrid[0:h, 0:w]
    for col, values in [(1, yy), (2, xx)] + [(3 + c, img[..., c]) for c in range(3)] + [(6 + p, feats[p]) for p in range(d)]:
        want = ndi.sum(values.astype(np.float64), safe, index)     # (below 2^53: exact)
        assert np.array_equal(sums[:, col], want.astype(np.uint64)), col
    for q, sl in enumerate(ndi.find_objects(safe + 1, max_label=k)):
        if sl is None:
            assert q == 3 or n[q] == 0
            assert tuple(bbox[q]) == (h, w, -1, -1)
        else:
            assert tuple(bbox[q]) == (sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1)
    com = ndi.center_of_mass(np.ones((h, w)), safe, [q for q in index if n[q]])
    got = sums[n > 0][:, 1:3].astype(np.float64) / n[n > 0, None]
    assert np.allclose(got, np.array(com), rtol=0, atol=1e-9)


def _tree_case(seed=5, h=17, w=21, k=20, d=4):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    lab = ((yy // 4) * 4 + xx // 6).astype(np.int32)               # 5 x 4 blocks = 20 labels
    lab[lab == 7] = 6                                              # label 7 unused: alive = 19
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    feats = (rng.integers(0, 2000, (d, h, w)) + 300 * (lab % 5)).astype(np.uint16)
    merges, _, alive = rt.build_tree(feats, lab, k)
    return lab, img, feats, merges, alive


def _both_routes(lab, img, feats, merges, alive, regions, k):
    want = rp.cut_tables(lab, merges, alive, regions, k, img, feats)
    sums, bbox = rp.leaf_table(lab, k, img, feats)
    got = rp.cut_tables_by_rows(sums, bbox, merges, alive, regions, lab.shape)
    for name, g, w in zip(("group", "sums", "bbox", "offsets"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, regions)
    return want


def test_cut_tables_by_adding_rows_equal_tabulating_the_relabelled_map():
    lab, img, feats, merges, alive = _tree_case()
    assert alive == 19
    for r in range(1, alive + 3):
        group, sums, bbox, offsets = _both_routes(lab, img, feats, merges, alive, [r], 20)
        assert len(sums) == min(20, r) and group[0, 7] == -1 and group[0].max() + 1 == min(alive, r)
        assert np.array_equal(group[0][lab], rt.cut(lab, merges, alive, r))
        assert sums[:, 0].sum() == lab.size and (sums[min(alive, r):] == 0).all()
        assert all(tuple(b) == (17, 21, -1, -1) for b in bbox[min(alive, r):])
    _both_routes(lab, img, feats, merges, alive, [19, 8, 8, 12, 3, 1], 20)       # entries that are not below their predecessor


@pytest.mark.parametrize("make", [cm.chain, cm.star, cm.balanced])
def test_hand_made_lists_and_a_list_with_rows_that_do_not_count(make):
    k = 13
    lab, img, feats = _random_case(9, 11, 14, k, 2)
    lab = np.clip(lab, 0, k - 1)
    merges = make(k)
    alive = len(np.unique(lab))
    _both_routes(lab, img, feats, merges, alive, [13, 7, 4, 2, 1], k)
    bad = merges.copy()
    bad[2] = (5, 5)                                                # a = b
    bad[4] = (3, k)                                                # b past the labels
    bad[6] = bad[0]                                                # b already absorbed
    bad[8] = (-1, -1)
    clean = rp.counted(bad, k)
    assert (clean[[2, 4, 6, 8]] == -1).all() and (clean >= 0).any()
    _both_routes(lab, img, feats, bad, alive, [13, 7, 4, 2, 1], k)


def test_region_table_rounds_as_the_kmeans_update_does():
    from gabor_color_image_segmentation_amd import region_table
    #            n   sy  sx   R    G     B   x0
    sums = np.array([[2, 1, 3, 255 * 2, 1, 3, 7],                  # means 255, 1 / 2 -> 1 (half rounds up), 3 / 2 -> 2, 7 / 2 -> 4
                     [0, 0, 0, 0, 0, 0, 0],
                     [3, 4, 5, 4, 5, 1, 46340 * 3],                # 4 / 3 -> 1, 5 / 3 -> 2, 1 / 3 -> 0
                     [2 ** 24, 0, 0, 255 * 2 ** 24, 0, 2 ** 23 - 1, 46340 * 2 ** 24]], np.uint64)
    bbox = np.array([[0, 1, 1, 2], [9, 9, -1, -1], [0, 0, 2, 2], [0, 0, 4095, 4095]], np.int32)
    t = region_table(sums, bbox)
    assert t["area"].tolist() == [2, 0, 3, 2 ** 24] and t["used"].tolist() == [True, False, True, True]
    assert t["mean_rgb"].dtype == np.uint8 and t["mean_rgb"].tolist() == [[255, 1, 2], [0, 0, 0], [1, 2, 0], [255, 0, 0]]
    assert t["mean_features"].dtype == np.uint16 and t["mean_features"].ravel().tolist() == [4, 0, 46340, 46340]
    assert t["centroid"][0].tolist() == [0.5, 1.5] and np.isnan(t["centroid"][1]).all() and t["centroid"][2].tolist() == [4 / 3, 5 / 3]
    assert np.array_equal(t["bbox"], bbox)
    for q in range(4):
        for c in range(3):
            assert t["mean_rgb"][q, c] == rp.mean(sums[q, 3 + c], sums[q, 0])
    t64 = region_table(sums.view(np.int64)[None], bbox[None])      # the int64 tensor that carries the bits; a leading batch axis
    assert np.array_equal(t64["mean_rgb"][0], t["mean_rgb"]) and t64["area"].shape == (1, 4)
    with pytest.raises(ValueError):
        region_table(sums[:, :5], bbox)


def test_the_worked_example_of_the_spec():
    """SPEC.md §19's example: a 2 x 3 map with K = 4 (label 3 unused), merges (0, 2), (0, 1), the cut at R = 2."""
    lab = np.array([[0, 0, 1], [2, 0, 1]], np.int32)
    img = np.zeros((2, 3, 3), np.uint8)
    img[..., 0] = [[10, 20, 200], [90, 31, 201]]
    img[..., 2] = 255
    sums, bbox = rp.leaf_table(lab, 4, img)
    assert sums.tolist() == [[3, 1, 2, 61, 0, 765], [2, 1, 4, 401, 0, 510], [1, 1, 0, 90, 0, 255], [0, 0, 0, 0, 0, 0]]
    assert bbox.tolist() == [[0, 0, 1, 1], [0, 2, 1, 2], [1, 0, 1, 0], [2, 3, -1, -1]]
    merges = np.array([[0, 2], [0, 1], [-1, -1]], np.int32)
    group, csums, cbox, offsets = _both_routes(lab, img, None, merges, 3, [2], 4)
    assert group.tolist() == [[0, 1, 0, -1]] and offsets.tolist() == [0, 2]
    assert csums.tolist() == [[4, 2, 2, 151, 0, 1020], [2, 1, 4, 401, 0, 510]]
    assert cbox.tolist() == [[0, 0, 1, 1], [0, 2, 1, 2]]
    from gabor_color_image_segmentation_amd import region_table
    t = region_table(csums, cbox)
    assert t["mean_rgb"].tolist() == [[38, 0, 255], [201, 0, 255]] and t["centroid"].tolist() == [[0.5, 0.5], [0.5, 2.0]]
    assert region_table(sums, bbox)["mean_rgb"].tolist() == [[20, 0, 255], [201, 0, 255], [90, 0, 255], [0, 0, 0]]
    pic = rp.paint(lab, csums, group[0])
    assert pic[..., 0].tolist() == [[38, 38, 201], [38, 38, 201]] and (pic[..., 1] == 0).all() and (pic[..., 2] == 255).all()
    assert rp.paint(lab, sums)[..., 0].tolist() == [[20, 20, 201], [90, 20, 201]]


def test_the_abi_lists_the_three_entry_points(built):
    from gabor_color_image_segmentation_amd import _lib
    assert all(n in _lib.SIGNATURES for n in NAMES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.gcs_abi_version() == 18


def test_argument_errors_launch_nothing(built):
    """Every GCS_EINVAL case of SPEC.md §19, with dummy pointers that are never dereferenced (so this runs without a GPU)."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)
    props = lambda labels=one, img=one, feats=one, b=1, h=4, w=4, d=1, k=3, sums=one, bbox=one: \
        lib.gcs_region_props(labels, img, feats, b, h, w, d, k, sums, bbox, None)
    for kw in (dict(labels=None), dict(sums=None), dict(bbox=None), dict(b=0), dict(b=65536), dict(h=0), dict(w=0), dict(h=4097),
               dict(w=4097), dict(d=-1), dict(d=208), dict(k=0), dict(feats=None), dict(d=0), dict(b=64, k=2 ** 22, d=2),
               dict(k=2 ** 31 // 7 + 1)):
        assert props(**kw) == 1, kw
        assert b"gcs_region_props" in lib.gcs_last_error()
    cuts = lambda sums=one, bbox=one, merges=one, alive=one, regions=one, b=1, h=4, w=4, k=3, c=6, n=2, rsum=5, group=one, so=one, \
        bo=one: lib.gcs_region_props_cuts(sums, bbox, merges, alive, regions, b, h, w, k, c, n, rsum, group, so, bo, None)
    for kw in (dict(sums=None), dict(bbox=None), dict(merges=None), dict(alive=None), dict(regions=None), dict(group=None),
               dict(so=None), dict(bo=None), dict(b=0), dict(b=65536), dict(h=0), dict(w=4097), dict(k=0), dict(k=4097), dict(c=5),
               dict(c=214), dict(n=0), dict(n=65), dict(rsum=0), dict(rsum=7), dict(b=65535, k=4096, c=213),
               dict(b=65535, k=4096, n=64, rsum=1), dict(b=65535, k=4096, c=6, n=64, rsum=64 * 4096)):
        assert cuts(**kw) == 1, kw
        assert b"gcs_region_props_cuts" in lib.gcs_last_error()
    paint = lambda labels=one, group=one, sums=one, b=1, h=4, w=4, k=3, g=2, c=6, stride=2, out=one: \
        lib.gcs_region_paint(labels, group, sums, b, h, w, k, g, c, stride, out, None)
    for kw in (dict(labels=None), dict(sums=None), dict(out=None), dict(b=0), dict(b=65536), dict(h=0), dict(h=4097), dict(w=0),
               dict(k=0), dict(g=0), dict(c=5), dict(c=214), dict(group=None), dict(stride=1), dict(b=65535, g=2 ** 20, stride=2 ** 20, c=213),
               dict(b=65535, k=2 ** 20)):
        assert paint(**kw) == 1, kw
        assert b"gcs_region_paint" in lib.gcs_last_error()
