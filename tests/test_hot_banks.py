"""The hot banks of tests/hot_banks.py on the CPU: gcs_bank_pack accepts them (and refuses their neighbours outside the bounds),
both oracles agree on them bit for bit, the responses stay in |a| <= 32767, and - what makes the GPU cases of
tests/test_gpu_value_range.py mean something - the oracle's features really cover the range the default banks never reach:
every TOP nibble, values above 46 000, bit 15 set in features and centroids, flagged next to unflagged tiles."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import hot_banks as hb
from gabor_color_image_segmentation_amd import _lib
from oracle import c_oracle as co
from oracle import spec_oracle as so
from slab_layout import tile_of_pixels

BANKS = [(4, 6, 13, 8), (4, 6, 13, 7), (8, 8, 15, 8), (2, 3, 7, 7)]
H, W = 64, 96


@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


def _pack(lib, tapq, ns, no, ks):
    packed = np.zeros(lib.gcs_bank_packed_bytes(ns, no), np.int8)
    bias = np.zeros(lib.gcs_bank_bias_count(ns, no), np.int32)
    tq = np.ascontiguousarray(tapq, np.int16)
    return lib.gcs_bank_pack(tq.ctypes.data, ns, no, ks, packed.ctypes.data, bias.ctypes.data)


_FEATS = {}


def _features(cfg):
    """C-oracle features of the eight image kinds at 64x96 -> (imgs, (8, D, H, W) uint16)."""
    if cfg not in _FEATS:
        bank = hb.hot_bank(*cfg)
        imgs = hb.hot_images(8, H, W, seed=1)
        _FEATS[cfg] = imgs, np.stack([co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient) for im in imgs])
    return _FEATS[cfg]


@pytest.mark.parametrize("cfg", BANKS + [(2, 6, 13, 8), (5, 6, 13, 7), (4, 7, 13, 7), (6, 8, 15, 7), (3, 23, 9, 8)])
def test_hot_banks_are_legal(lib, cfg):
    """gcs_bank_pack returns GCS_OK; the tap sums sit at the bounds the recipe states."""
    ns, no, ks, shift = cfg
    bank = hb.hot_bank(*cfg)
    assert bank.tapq.dtype == np.int16 and bank.shift == shift and bank.exponent == shift + 7
    t = bank.tapq.astype(np.int64)
    assert np.all(t[:, 1].sum(axis=(1, 2)) == 0) and np.abs(t).max() <= 32639
    assert np.abs(t).sum(axis=(2, 3)).max() <= 32896
    assert np.abs(t[:, 0]).sum(axis=(1, 2)).max() > (32896 if shift == 8 else 16448) * 0.99
    assert _pack(lib, bank.tapq, ns, no, ks) == 0, lib.gcs_last_error()


def test_banks_outside_the_bounds_are_refused(lib):
    """One tap over sum|tapq| = 32 896, and imaginary taps that do not sum to zero."""
    t = np.zeros((24, 2, 13, 13), np.int16)
    t[:, 0, :4, :8] = 1028                                    # 32 taps of 1028: sum|tapq_re| = 32 896 exactly
    t[:, 1, 0, 0], t[:, 1, 12, 12] = 16448, -16448            # sum|tapq_im| = 32 896, sums to zero
    assert _pack(lib, t, 4, 6, 13) == 0, lib.gcs_last_error()
    over = t.copy()
    over[5, 0, 12, 12] = 1                                    # one filter at 32 897
    assert _pack(lib, over, 4, 6, 13) == 1 and b"32896" in lib.gcs_last_error()
    over = t.copy()
    over[23, 1, 6, 6], over[23, 1, 6, 7] = 1, -1              # imaginary part at 32 898, still summing to zero
    assert _pack(lib, over, 4, 6, 13) == 1 and b"32896" in lib.gcs_last_error()
    bad = hb.hot_bank(4, 6, 13, 7).tapq.copy()
    bad[7, 1, 0, 0] += 1
    assert _pack(lib, bad, 4, 6, 13) == 1 and b"sum to zero" in lib.gcs_last_error()


@pytest.mark.parametrize("cfg", BANKS)
def test_responses_stay_inside_16_bits(cfg):
    """max |a_re|, |a_im| <= 32767 recomputed in int64 on every pyramid level of every image kind (SPEC.md §3: n < 2^31)."""
    ns, no, ks, shift = cfg
    tapq = hb.hot_bank(*cfg).tapq.astype(np.int64)
    worst = 0
    for img in hb.hot_images(8, H, W, seed=1):
        for lv, im in enumerate(so.pyramid(img, (ns + 1) // 2)):
            for f in range(ns * no):
                if so.level_of(f, no) != lv:
                    continue
                for part in range(2):
                    for c in range(3):
                        a = ndi.correlate(im[:, :, c].astype(np.int64), tapq[f, part], mode="reflect") >> shift
                        worst = max(worst, int(np.abs(a).max()))
    assert 32000 <= worst <= 32767, worst


@pytest.mark.parametrize("cfg", BANKS)
def test_both_oracles_agree_on_features_and_labels(cfg):
    ns, no, ks, shift = cfg
    bank = hb.hot_bank(*cfg)
    imgs = hb.hot_images(3, 40, 56, seed=2)
    tapq = bank.tapq.astype(np.int64)
    feats = []
    for im in imgs:
        ref = so.gabor_features(im, tapq, shift, no)
        assert np.array_equal(co.gabor_features(im, bank.tapq, shift, no), ref)
        feats.append(ref)
    feats = np.stack(feats)
    assert feats.max() >= 32768
    x = feats.reshape(3, feats.shape[1], -1)
    for k in (8, 16):
        got, cent = co.kmeans(x, k, 4)
        xs = [x[i].T for i in range(3)]
        want, c = so.kmeans(np.concatenate(xs), k, 4, init_from=xs[0])
        assert np.array_equal(got.ravel(), want) and np.array_equal(cent.astype(np.int64), c)
    for i in range(3):
        assert np.array_equal(co.kmeans(x[i:i + 1], 8, 4)[0].ravel(), so.kmeans(x[i].T, 8, 4)[0])


@pytest.mark.parametrize("cfg", BANKS)
def test_features_cover_the_range(cfg):
    """Every TOP nibble 0..8 (shift 8) / 0..11 (shift 7), a largest value >= 36 000 / >= 46 000, and at least 1 % of the values
    of every stripe image with bit 15 set."""
    shift = cfg[3]
    _, f = _features(cfg)
    assert set(np.unique(f >> 12).tolist()) == set(range(9 if shift == 8 else 12))
    assert int(f.max()) >= (36000 if shift == 8 else 46000) and int(f.max()) <= hb.G_MAX
    for i in hb.STRIPE_KINDS:
        assert (f[i] >= 32768).mean() >= 0.01, (i, float((f[i] >= 32768).mean()))
    assert (f >= 4096).mean() >= 0.7


@pytest.mark.parametrize("cfg", [(4, 6, 13, 8), (4, 6, 13, 7), (2, 3, 7, 7)])
def test_black_region_image_has_flagged_and_unflagged_tiles(cfg):
    _, f = _features(cfg)
    tile = tile_of_pixels(H, W)
    flagged = np.zeros(tile.max() + 1, bool)
    flagged[np.unique(tile[(f[hb.BLACK_REGION] >= 4096).any(axis=0)])] = True
    assert flagged.any() and not flagged.all(), int(flagged.sum())


def test_global_codebooks_hold_centroids_with_bit_15_set():
    """One codebook over the eight image kinds at 81x121, 6 passes: every label is used for k = 8 and k = 16, and the centroids
    end with entries >= 32768 (4x6 shift-7 bank; the high digit of a centroid leaves [-128, -1]). Per image every label is used
    except on the white image (all its init centroids are equal: the tie and empty-cluster rules decide) and on the black-region
    image (two init centroids are the zero vector: one cluster stays empty)."""
    bank = hb.hot_bank(4, 6, 13, 7)
    imgs = hb.hot_images(8, 81, 121, seed=3)
    x = np.stack([co.gabor_features(im, bank.tapq, bank.shift, 6) for im in imgs]).reshape(8, 72, -1)
    for k in (8, 16):
        lab, cent = co.kmeans(x, k, 6)
        assert len(np.unique(lab)) == k
        assert (cent >= 32768).sum() >= 1, k
    for i, kind in enumerate(hb.IMAGE_KINDS):
        used = len(np.unique(co.kmeans(x[i:i + 1], 8, 6)[0]))
        assert used == {"white": 1, "black_region": 7}.get(kind, 8), (kind, used)
