"""Superpixels (SPEC.md §13) on the CPU: the restatement (tests/superpixel_ref.py) against what §13 says on cases small enough to
check by other means, the quality pin of the recommended setting on six val fixture images, and the argument checks of the host
API (no GPU: the plan is built on a stand-in whose stage is never reached)."""
import json
import os

import numpy as np
import pytest

import superpixel_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


# ---- grid, init, domain

def test_grid_rule_and_round_half_even():
    assert sr.grid(481, 321, 300) == (23, 21, 14) and sr.grid(321, 481, 300) == (23, 14, 21)
    assert sr.grid(37, 53, 2) == (31, 1, 2) and sr.grid(37, 53, 1200) == (1, 37, 53)
    assert sr.grid(9, 9, 36) == (2, 4, 4)               # sqrt(81 / 36) = 1.5 -> 2 (half to even); 9 / 2 = 4.5 -> 4 (half to even)
    assert sr.grid(10, 10, 16) == (2, 5, 5)             # sqrt(100 / 16) = 2.5 -> 2
    assert sr.grid(16, 16, 2) == (11, 1, 1)             # K = 1 is a grid too
    from gabor_color_image_segmentation_amd import superpixel_grid
    rng = np.random.default_rng(1)
    for _ in range(500):
        h, w, n = int(rng.integers(1, 700)), int(rng.integers(1, 700)), int(rng.integers(2, 4097))
        s = max(1, int(np.rint(np.sqrt(np.float64(h * w) / n))))
        want = (s, max(1, int(np.rint(h / s))), max(1, int(np.rint(w / s))))
        assert superpixel_grid(h, w, n) == want
        if want[1] * want[2] <= 4096:
            assert sr.grid(h, w, n) == want


def test_domain_of_the_restatement():
    for n in (0, 1, 4097, 2.0):
        with pytest.raises(ValueError):
            sr.grid(64, 64, n)
    with pytest.raises(ValueError):
        sr.grid(90, 90, 4096)                            # S = 1: 8100 centres
    with pytest.raises(ValueError):
        sr.grid(4097, 8, 2)
    x = np.zeros((3, 16, 16), np.uint16)
    for lam in (0, 65536, 1.5):
        with pytest.raises(ValueError):
            sr.superpixels(x, 4, lam)
    with pytest.raises(ValueError):
        sr.superpixels(x, 4, 576, n_iter=0)
    with pytest.raises(ValueError):
        sr.superpixels(np.zeros((208, 8, 8), np.uint16), 4)
    # the bound SPEC.md §13 states: the largest distance of the domain is below 2^63
    assert 207 * 46340 ** 2 + 65535 * 2 * 4095 ** 2 < 2 ** 63


def test_init_positions_and_centres():
    cy, cx = sr.init_positions(481, 321, 21, 14)
    assert cy[0] == 481 // 42 and cx[0] == 321 // 28 and cy[14] == (3 * 481) // 42 and cx[13] == (27 * 321) // 28
    assert cy.max() < 481 and cx.max() < 321 and len(cy) == 21 * 14
    rng = np.random.default_rng(2)
    x = rng.integers(0, 46340, (5, 40, 56)).astype(np.uint16)
    lab, cen = sr.superpixels(x, 12, 576, n_iter=1, return_centres=True)
    _, ny, nx = sr.grid(40, 56, 12)
    cy, cx = sr.init_positions(40, 56, ny, nx)
    assert np.array_equal(cen[:, :5], x[:, cy, cx].T) and np.array_equal(cen[:, 5], cy) and np.array_equal(cen[:, 6], cx)


# ---- assign

def _nearest(h, w, cy, cx, lowest=True):
    """Brute force over ALL centres: the index of the nearest centre of every pixel, the lowest index among equals."""
    y, x = np.mgrid[0:h, 0:w]
    d = (y[..., None] - cy) ** 2 + (x[..., None] - cx) ** 2
    return d.argmin(axis=-1)                             # (argmin returns the first = lowest index of the minimum)


def test_tie_rule_on_a_constant_image():
    """A constant image: the feature term is the same for every centre, so the spatial term decides, and a pixel as far from one
    candidate centre as from another is a tie: it takes the LOWEST centre index q = i nx + j among them - the upper one of two
    rows, the left one of two columns, the upper left of four. 16 x 16, n = 4: centres at rows / columns 4 and 12; row 8 and
    column 8 are 4 from either, so row 8 belongs to the upper centres, column 8 to the left ones and pixel (8, 8) to centre 0."""
    x = np.full((3, 16, 16), 777, np.uint16)
    for lam in (1, 576, 65535):
        lab = sr.superpixels(x, 4, lam, n_iter=1)
        assert sr.grid(16, 16, 4) == (8, 2, 2)
        assert lab[8, 8] == 0 and set(lab[8, :8]) == {0} and set(lab[8, 9:]) == {1} and set(lab[:8, 8]) == {0} and set(lab[9:, 8]) == {2}
        assert np.array_equal(lab, _nearest(16, 16, *sr.init_positions(16, 16, 2, 2)))


@pytest.mark.parametrize("h,w,n", [(48, 64, 12), (37, 53, 64), (60, 60, 300), (16, 200, 8), (37, 53, 2)])
def test_huge_lambda_on_a_constant_image_gives_the_voronoi_cells(h, w, n):
    """lambda = 65535 on a constant image: every pass labels a pixel with the nearest of ALL its centres (brute force, lowest index
    among equals) - the Voronoi cells of the grid centres in pass 0, of the moved centres afterwards."""
    x = np.full((4, h, w), 123, np.uint16)
    _, ny, nx = sr.grid(h, w, n)
    assert np.array_equal(sr.superpixels(x, n, 65535, n_iter=1), _nearest(h, w, *sr.init_positions(h, w, ny, nx)))
    lab, cen = sr.superpixels(x, n, 65535, n_iter=3, return_centres=True)
    assert np.array_equal(lab, _nearest(h, w, cen[:, 4], cen[:, 5]))
    assert (cen[:, :4] == 123).all()


def test_one_pass_is_the_init_assign_and_labels_stay_candidates():
    rng = np.random.default_rng(3)
    for h, w, n, lam in ((40, 56, 12, 576), (37, 53, 300, 1), (64, 48, 64, 65535), (37, 53, 1200, 144)):
        x = rng.integers(0, 46340, (6, h, w)).astype(np.uint16)
        _, ny, nx = sr.grid(h, w, n)
        cy, cx = sr.init_positions(h, w, ny, nx)
        cand = sr.candidates(h, w, ny, nx)
        one = sr.superpixels(x, n, lam, n_iter=1)
        assert np.array_equal(one, sr.assign(x.astype(np.int64), x[:, cy, cx].T.astype(np.int64), cy, cx, ny, nx, lam))
        for n_iter in (1, 2, 5):
            lab = sr.superpixels(x, n, lam, n_iter=n_iter)
            assert lab.dtype == np.int32 and lab.min() >= 0 and lab.max() < ny * nx
            assert (cand == lab[None]).any(axis=0).all()          # always one of the (existing) 3 x 3 candidates
        # brute force of one assign on a few pixels: every existing candidate, 64-bit Python integers
        xi = x.astype(object)
        for y0, x0 in ((0, 0), (h - 1, w - 1), (h // 2, w // 3), (5, w - 2)):
            best = None
            for q in sorted(set(int(c) for c in cand[:, y0, x0] if c >= 0)):
                d = sum(int((int(xi[p, y0, x0]) - int(xi[p, cy[q], cx[q]])) ** 2) for p in range(6)) \
                    + lam * ((y0 - int(cy[q])) ** 2 + (x0 - int(cx[q])) ** 2)
                if best is None or d < best[0]:
                    best = (d, q)
            assert one[y0, x0] == best[1]


def test_update_rule_and_empty_centres():
    """floor((2 S + n) / (2 n)) on features and positions; a centre without pixels keeps features and position."""
    x = np.zeros((2, 8, 8), np.int64)
    x[0] = np.arange(64).reshape(8, 8)
    x[1, :, :] = 7
    lab = np.zeros((8, 8), np.int64)
    lab[:, 4:] = 2                                       # centre 1 stays empty
    cent = np.array([[1, 1], [500, 600], [3, 3]], np.int64)
    new, cy, cx = sr.update(x, lab, cent, np.array([0, 5, 0]), np.array([0, 6, 0]))
    left = x[0][:, :4].ravel()
    assert new[0, 0] == (2 * left.sum() + 32) // 64 and new[0, 1] == 7
    assert list(new[1]) == [500, 600] and cy[1] == 5 and cx[1] == 6
    assert cy[0] == (2 * (np.arange(8).sum() * 4) + 32) // 64 == 4 and cx[0] == (2 * (0 + 1 + 2 + 3) * 8 + 32) // 64 == 2 and cx[2] == 6


# ---- quality pin

# the recommended setting (colour bank 5, 1/8, 4; n = 300, lambda = 576, 10 passes, min_region_size = S^2 / 4) on the first six val
# fixture images, as tools/superpixel_quality.py scored them: (boundary recall, underseg)
PIN = {"101085": (0.9394756249707289, 0.0535281507244124), "101087": (0.9268199189971561, 0.049445275613499914),
       "102061": (0.857153872772739, 0.030462237938873447), "103070": (0.8931648465752322, 0.055599812609158396),
       "105025": (0.8973253062039301, 0.03126059200825556), "106024": (0.9181028466530206, 0.029122683328290804)}


def test_quality_pin_of_the_recommended_setting(built):
    """Boundary recall and underseg of the recommended setting on six val images, pinned; every image beats the map
    skimage.segmentation.slic(n_segments=300) gave for the same id (bsd_val_scores.json) on boundary recall."""
    from merge_ref import merge_small_regions
    from gabor_color_image_segmentation_amd.evaluate import metrics
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    slic = json.load(open(os.path.join(GOLD, "bsd_val_scores.json")))["per_id"]
    ids = [str(i) for i in val["ids"][:6]]
    assert ids == list(PIN)
    shared = 0
    for i in ids:
        img = val["img_" + i]
        s = sr.grid(img.shape[0], img.shape[1], 300)[0]
        lab = merge_small_regions(sr.segment(img, 300, lam=576, w=0.125, g=4, n_orient=5), s * s // 4)
        m = metrics(None, lab.astype(np.int32), pt[i])
        m.set_metrics()
        got = m.get_metrics()
        assert abs(got["recall"] - PIN[i][0]) <= 1e-12 and abs(got["underseg"] - PIN[i][1]) <= 1e-12, (i, got)
        if i in slic:
            shared += 1
            assert got["recall"] > slic[i]["slic"]["recall"], (i, got["recall"], slic[i]["slic"]["recall"])
    assert shared == 6


def test_quality_table_is_the_tools_output_and_slic_rows_are_beside_it():
    doc = json.load(open(os.path.join(HERE, "..", "profiles", "superpixel_quality.json")))
    assert doc["images"] == 24 and len(doc["rows"]) == 2 * 3 * 3 * 2
    rec = doc["recommended_per_image"]["merged"]
    for i, (recall, under) in PIN.items():
        assert rec[i]["recall"] == recall and rec[i]["underseg"] == under
    slic = json.load(open(os.path.join(GOLD, "superpixel_slic_scores.json")))
    assert slic["skimage"] == "0.18.3" and slic["ids"] == doc["ids"] and [r["n_segments"] for r in slic["rows"]] == [300, 360, 420]
    row = [r for r in doc["rows"] if (r["bank"], r["n_superpixels"], r["spatial_weight"], r["merge"]) == ("colour", 300, 576, 1)][0]
    for s in slic["rows"]:                               # the claim of DESIGN.md §7, at the slot's setting and at matching region counts
        assert row["recall"] > s["recall"] and row["underseg"] < s["underseg"] and row["undersegNP"] < s["undersegNP"]


# ---- the host API's argument checks (no GPU)

class _Ops:
    """What Segmenter needs to build a plan; the stage itself is never reached by these tests."""
    smoothing, chroma_gain = 0.0, 0

    def __init__(self, bank):
        self.bank = bank

    def superpixels(self, *a, **kw):
        raise AssertionError("the argument checks come before any launch")


def _plan(**kw):
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    return Segmenter(ops=_Ops(make_bank()), **kw)


def test_value_errors_of_the_host_api():
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, make_bank
    for n in (1, -1, 4097, 2.5, True, "3", None):
        with pytest.raises(ValueError):
            _plan(n_superpixels=n)
    for lam in (0, 65536, 1.5, -3, None):
        with pytest.raises(ValueError):
            _plan(n_superpixels=300, spatial_weight=lam)
    with pytest.raises(ValueError):
        _plan(spatial_weight=0)                          # checked even when the stage is off
    seg = _plan(n_superpixels=300)
    assert (seg.n_superpixels, seg.spatial_weight) == (300, 576) and _plan().n_superpixels == 0
    imgs = np.zeros((1, 72, 104, 3), np.uint8)
    dev = torch.from_numpy(imgs)
    for mode in ("global", "per-image"):
        with pytest.raises(ValueError):
            seg.segment_device(dev, mode=mode)
    with pytest.raises(ValueError):
        seg.segment_batch(imgs, mode="global")
    with pytest.raises(ValueError):
        next(iter(seg.segment_stream([imgs], mode="global")))
    with pytest.raises(ValueError):
        seg.segment_device(dev, dist_group=object())
    with pytest.raises(ValueError):
        seg.segment_batch(imgs, out_dtype=np.uint8)      # 300 -> 16 x 23 centres, more than 256 labels
    with pytest.raises(ValueError):
        next(iter(seg.segment_images([imgs[0]], out_dtype=np.uint8)))
    with pytest.raises(ValueError):
        seg.segment_rows_sharded_device(dev, 0, 72, 0, 72)
    with pytest.raises(ValueError):
        seg.segment_owned_rows_device(dev, 72)
    with pytest.raises(ValueError):
        _plan(n_superpixels=4096).segment_batch(np.zeros((1, 90, 90, 3), np.uint8))      # S = 1: 8100 centres
    with pytest.raises(ValueError):
        _plan(n_superpixels=2).segment_batch(np.zeros((1, 8, 4100, 3), np.uint8))        # a side beyond 4096
    with pytest.raises(ValueError):                      # the stage needs ops that have it
        Segmenter(ops=type("NoStage", (), dict(bank=make_bank(), smoothing=0.0, chroma_gain=0))(), n_superpixels=64)
    with pytest.raises(ValueError):                      # D = 216 > 207
        Segmenter(n_scales=6, n_orient=12, ops=_Ops(make_bank(6, 12)), n_superpixels=64)
