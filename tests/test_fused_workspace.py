"""The workspace of the self-updating Lloyd passes without a GPU: the model of tests/fused_workspace.py (the reference of
tests/test_gpu_self_updating_stages.py) chained into whole loops against the NumPy oracle, and the two host-side pieces of the
entry points: gcs_kmeans_fused_workspace_bytes (a pure host function) and the argument checks of gcs_kmeans_pass_fused, which
return before any launch."""
import numpy as np
import pytest

import fused_workspace as fw
from gabor_color_image_segmentation_amd import _lib
from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
from oracle import spec_oracle as so

GCS_EINVAL = 1


@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


# ------------------------------------------------------------------------------------------ the model against the oracle
@pytest.fixture(scope="module")
def batch():
    """A small synthetic batch and the default bank's features (B, P, D) int64 from the NumPy oracle."""
    imgs = synthetic_batch(3, 24, 40, seed=11)
    tapq, shift = so.bank()
    x = np.stack([so.gabor_features(im, tapq, shift, 6).reshape(72, -1).T for im in imgs]).astype(np.int64)
    return imgs, x


@pytest.mark.parametrize("mode", ["per_image", "global"])
@pytest.mark.parametrize("n_iter", [1, 2, 3, 4, 7])
def test_the_model_chained_into_a_loop_equals_the_oracle(batch, mode, n_iter):
    """n passes of expected_pass on a zeroed workspace give the labels of so.segment / so.segment_batch and end on all-zero sum
    buffers and ticket; a second loop on the buffer the first one left does too (rows = 1 and rows = 4 hold the same totals)."""
    imgs, x = batch
    b, p, d = x.shape
    k = 8
    n_sets = b if mode == "per_image" else 1
    want = so.segment_batch(imgs, mode=mode, k=k, n_iter=n_iter).reshape(b, p)
    for rows in (1, 4) if mode == "global" else (1,):
        buf = np.zeros(fw.workspace_bytes(n_sets, rows, k, d), np.uint8)
        for loop in range(2):
            dirty = 0
            for t in range(n_iter):
                buf, cent, lab = fw.expected_pass(buf, x, t, t == n_iter - 1, mode, k, rows)
                dirty += not fw.is_as_found(buf, n_sets, rows, k, d)
            assert np.array_equal(lab, want), (rows, loop)
            assert fw.is_as_found(buf, n_sets, rows, k, d), (rows, loop)
            assert dirty == n_iter - 1                      # ... and every pass but the last left sums behind
            assert cent.shape == (n_sets, k, d)
        again, cent2, lab2 = fw.expected_loop(buf, x, n_iter, mode, k, rows)
        assert np.array_equal(lab2, want) and np.array_equal(cent2, cent) and fw.is_as_found(again, n_sets, rows, k, d)


def test_the_model_reads_the_rows_total_and_keeps_empty_clusters(batch):
    """The update of the model: shares spread over the rows of a set fold to the same centroids; an empty cluster keeps the
    centroid of the array the pass does not write; padding bytes are never touched."""
    _, x = batch
    b, p, d = x.shape
    k, rows, t = 5, 3, 2
    buf = np.zeros(fw.workspace_bytes(1, rows, k, d), np.uint8)
    v = fw.views(buf, 1, rows, k, d)
    for piece in v.sum_pad + v.cent_pad:
        piece[...] = 0xA5
    v.cents[(t - 1) & 1][...] = np.arange(k * d).reshape(1, k, d) + 7
    v.cents[t & 1][...] = 0xFFFF
    v.sums[(t - 1) % 3][0, :, 0, :] = [[3], [0], [5]]                    # cluster 0: S = 8 in every feature, n = 8: centroid 1
    v.sums[(t - 1) % 3][0, :, 2, :] = [[1], [1], [1]]                    # cluster 2: S = 3, n = 3
    v.sums[(t - 1) % 3][0, 1, 2, 0] = 2                                  # ... but feature 0: S = 4 -> floor(11 / 6) = 1
    v.sums[(t - 1) % 3][0, 0, 2, 1] = 0                                  # ... and feature 1: S = 2 -> floor(7 / 6) = 1
    v.sums[(t - 1) % 3][0, 2, 2, 2] = 3                                  # ... and feature 2: S = 5 -> floor(13 / 6) = 2
    after, cent, _ = fw.expected_pass(buf, x, t, False, "global", k, rows)
    want = np.arange(k * d).reshape(1, k, d) + 7
    want[0, 0] = 1
    want[0, 2] = 1
    want[0, 2, 2] = 2
    assert np.array_equal(cent, want)
    va = fw.views(after, 1, rows, k, d)
    assert np.array_equal(va.cents[t & 1], want) and np.array_equal(va.cents[(t - 1) & 1], v.cents[(t - 1) & 1])
    assert np.array_equal(va.sums[(t - 1) % 3], v.sums[(t - 1) % 3]) and not va.sums[(t + 1) % 3].any()
    assert int(fw.totals(va.sums[t % 3])[0, :, d].sum()) == b * p
    assert all((piece == 0xA5).all() for piece in va.sum_pad + va.cent_pad)


# ------------------------------------------------------------------------------------------ gcs_kmeans_fused_workspace_bytes
def tile_slots(ns, no):
    """S of csrc/common.h: 16-bit slots of one tile (4 blocks of 8 x 8 pixels) - level L (scales 2L, 2L + 1) keeps 256 >> 2L values
    of each of its 3 * n_orient * (scales on it) planes."""
    return sum(3 * no * min(2, ns - 2 * lv) * (256 >> (2 * lv)) for lv in range((ns + 1) // 2))


FUSED_BANKS = [(4, 6), (2, 6), (2, 8), (1, 16), (3, 7), (4, 5), (2, 5), (1, 1)]
SHAPES = [(321, 481), (81, 121), (64, 96), (9, 10)]            # both packed strips, both, none, one tile


def _bytes(lib, b, h, w, ns, no, k, n_sets):
    parts = lib.gcs_kmeans_parts_per_image(b, h, w)
    return fw.workspace_bytes(n_sets, fw.fold_rows(b, parts, n_sets, fw.env_fold_rows()), k, 3 * ns * no)


@pytest.mark.parametrize("ns,no", FUSED_BANKS, ids=lambda v: str(v))
def test_workspace_bytes_of_every_bank_with_a_self_updating_pass(lib, ns, no):
    assert tile_slots(ns, no) <= 12288 and 3 * ns * no <= 79 and ns <= 4
    n = 0
    for k in range(1, 9):
        for b in (1, 5, 64):
            for n_sets in {1, b}:
                for h, w in SHAPES:
                    got = lib.gcs_kmeans_fused_workspace_bytes(b, h, w, ns, no, k, n_sets)
                    assert got == _bytes(lib, b, h, w, ns, no, k, n_sets) and got % 256 == 0 and got > 0, (k, b, n_sets, h, w, got)
                    n += 1
    assert n == 8 * 5 * len(SHAPES)


def test_workspace_bytes_is_zero_where_there_is_no_such_pass(lib):
    f = lib.gcs_kmeans_fused_workspace_bytes
    h, w = 321, 481
    assert f(5, h, w, 4, 6, 8, 1) == _bytes(lib, 5, h, w, 4, 6, 8, 1) > 0
    for k in (9, 16, 0, -1):
        assert f(5, h, w, 4, 6, k, 1) == 0, k
    # the boundary of the three staging rounds: 2x8 and 1x16 fill them exactly, 3x8 (a split slab too) is one level-1 plane set over
    assert tile_slots(2, 8) == tile_slots(1, 16) == 12288 and (12288 >> 4) == 3 * 256
    assert tile_slots(3, 8) == 13824 and 3 * 3 * 8 <= 79
    assert f(5, h, w, 2, 8, 8, 1) > 0 and f(5, h, w, 1, 16, 8, 5) > 0
    assert f(5, h, w, 3, 8, 8, 1) == 0
    assert 3 * 4 * 7 == 84 and f(5, h, w, 4, 7, 8, 1) == 0               # D > 79: the wide slab
    assert 3 * 26 == 78 and tile_slots(1, 26) == 19968 and f(5, h, w, 1, 26, 8, 1) == 0
    assert f(5, h, w, 5, 1, 8, 1) == 0                                   # three levels
    for n_sets in (0, 2, 4, 6, -1):
        assert f(5, h, w, 4, 6, 8, n_sets) == 0, n_sets
    for b in (0, -3, 65536):
        assert f(b, h, w, 4, 6, 8, 1) == 0 and f(b, h, w, 4, 6, 8, b) == 0, b
    assert f(65535, 9, 10, 4, 6, 8, 1) > 0
    assert f(5, 0, w, 4, 6, 8, 1) == 0 and f(5, h, w, 0, 6, 8, 1) == 0


# ------------------------------------------------------------------------------------------ gcs_kmeans_pass_fused: argument checks
def test_pass_fused_refuses_bad_arguments_before_any_launch(lib):
    """Every call here fails validation (made-up non-null integers stand for the pointers; nothing is dereferenced, nothing is
    launched): NULL pointers, a last pass without a label map, a negative pass index, and banks / k / n_sets with no such pass."""
    F, WS, CENT, OUT = 0x10000, 0x20000, 0x30000, 0x40000

    def call(feats=F, b=5, h=64, w=96, ns=4, no=6, k=8, n_sets=1, t=1, last=0, ws=WS, cent=CENT, out=OUT):
        rc = lib.gcs_kmeans_pass_fused(feats, b, h, w, ns, no, k, n_sets, 0, t, last, ws, cent, out, 0, None)
        return rc, lib.gcs_last_error().decode()

    for kw in (dict(feats=None), dict(ws=None), dict(cent=None), dict(out=None, last=1)):
        rc, msg = call(**kw)
        assert rc == GCS_EINVAL and "gcs_kmeans_pass_fused" in msg and "NULL" in msg, (kw, rc, msg)
    rc, msg = call(t=-1)
    assert rc == GCS_EINVAL and "pass must be >= 0" in msg, (rc, msg)
    rc, msg = call(t=-1, last=1)
    assert rc == GCS_EINVAL and "pass must be >= 0" in msg, (rc, msg)
    for kw in (dict(k=9), dict(k=16), dict(k=0), dict(ns=3, no=8), dict(ns=4, no=7), dict(ns=1, no=26), dict(ns=5, no=1),
               dict(n_sets=2), dict(n_sets=0), dict(b=65536)):
        rc, msg = call(**kw)
        assert rc == GCS_EINVAL and "no self-updating pass" in msg, (kw, rc, msg)
    for kw in (dict(b=0), dict(h=0), dict(ns=0), dict(ns=9)):
        rc, msg = call(**kw)
        assert rc == GCS_EINVAL and "gcs_kmeans_pass_fused" in msg, (kw, rc, msg)
