"""tests/slab_codec.py against itself and against the library's pure host functions: sizes, injective slot tables, pixel and
no-pixel bits that tile the value bytes, pack / unpack round trips on every 16-bit value, and fillers that touch no-pixel bits only.
(tests/test_gpu_crafted_slabs.py then holds the codec to gcs_features_unpack and to the Gabor writer on the device.)"""
import numpy as np
import pytest

import slab_codec as sc
from slab_layout import tile_of_pixels

SHAPES = [(1, 1), (1, 9), (5, 9), (8, 8), (9, 10), (16, 17), (17, 16), (13, 21), (33, 41), (481, 321)]
# (n_scales, n_orient): the six banks of tests/test_gpu_kmeans_model.py BANKS, and D = 207
BANKS = {"split_4x6": (4, 6), "split_2x3": (2, 3), "wide_3x9": (3, 9), "deep_7x1": (7, 1), "deep_8x8": (8, 8), "generic_6x12": (6, 12),
         "d207_3x23": (3, 23)}


@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def _random_levels(geo, b, rng):
    return [rng.integers(0, 65536, (b, len(geo.planes[lev]), geo.hl[lev], geo.wl[lev]), dtype=np.uint16) for lev in range(geo.n_levels)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bank", list(BANKS))
def test_geometry_and_round_trip(lib, bank, shape):
    h, w = shape
    ns, no = BANKS[bank]
    geo = sc.geometry(h, w, ns, no)
    # sizes: the library's host functions
    assert geo.img_bytes == lib.gcs_feature_slab_bytes(1, h, w, ns, no)
    assert geo.pass_bytes == lib.gcs_feature_pass_bytes(1, h, w, ns, no)
    assert geo.split == (bank in ("split_4x6", "split_2x3")) and geo.d == 3 * ns * no == sum(len(p) for p in geo.planes)
    assert sorted(np.concatenate(geo.planes).tolist()) == list(range(geo.d))
    # the slot tables are injective and stay inside the value bytes
    n_values = 0
    seen = np.zeros(geo.value_bytes, np.uint8)
    nib = np.zeros(geo.value_bytes, np.uint8)
    for lev in range(geo.n_levels):
        idx = geo.index(lev).reshape(-1)
        n_values += len(idx)
        assert idx.min() >= 0
        if geo.split:
            assert idx.max() < geo.mid_off
            byte, shift = geo.nibble_of(lev, idx)
            assert byte.max() < geo.top_off - geo.mid_off and set(np.unique(shift).tolist()) <= {0, 4}
            np.add.at(nib, 2 * byte + shift // 4, 1)
            np.add.at(seen, idx, 1)
        else:
            assert idx.max() + 1 < geo.value_bytes and not (idx & 1).any()
            np.add.at(seen, idx, 1)
    assert seen.max() == 1 and int(seen.sum()) == n_values and nib.max() <= 1 and int(nib.sum()) == (n_values if geo.split else 0)
    assert n_values == sum(len(geo.planes[lev]) * geo.hl[lev] * geo.wl[lev] for lev in range(geo.n_levels))
    # pixel bits and no-pixel bits tile the value bytes exactly: 16 bits per value, nothing shared, nothing behind the values
    pix, nop = geo.pixel_bits(), geo.no_pixel_bits()
    assert not (pix & nop).any() and ((pix | nop)[:geo.value_bytes] == 0xFF).all()
    assert not pix[geo.value_bytes:].any() and not nop[geo.value_bytes:].any()
    assert int(np.unpackbits(pix).sum()) == 16 * n_values
    if geo.n_levels <= 2:
        assert np.array_equal(geo.tile[0], tile_of_pixels(h, w)) and geo.tile[0].max() + 1 == geo.ntiles
    # round trip on every 16-bit value, two fillers
    b = 1 if h * w > 10000 else 2
    rng = np.random.default_rng(h * 1000 + w + ns)
    levels = _random_levels(geo, b, rng)
    a = geo.pack(levels, filler=0x00)
    z = geo.pack(levels, filler=0xFF)
    assert a.shape == (b, geo.img_bytes) and a.dtype == np.uint8
    for raw in (a, z):
        back = geo.unpack_levels(raw)
        assert all(np.array_equal(back[lev], levels[lev]) for lev in range(geo.n_levels))
    assert np.array_equal(a ^ z, np.broadcast_to(nop[None], a.shape))       # the fillers differ on no-pixel bits, and on all of them
    canon = geo.unpack(a)
    assert canon.shape == (b, geo.d, h, w) and all(np.array_equal(x, y) for x, y in zip(geo.levels_of(canon), levels))
    if h * w >= 64:
        assert int(canon.max()) > 46340 and (canon >> 12 == 15).any()
    if geo.split:
        assert (geo.flags(a)[:, :, :geo.n_levels] != 0).any() and not geo.flags(a)[:, :, geo.n_levels:].any()


def test_flag_bytes_follow_the_top_nibbles_level_by_level():
    """Values >= 4096 confined to one level of one tile set exactly that flag byte; without the flag unpack reads the TOP nibble as 0."""
    geo = sc.geometry(33, 41, 4, 6)
    rng = np.random.default_rng(1)
    levels = [rng.integers(0, 4096, (1, len(geo.planes[lev]), geo.hl[lev], geo.wl[lev]), dtype=np.uint16) for lev in range(2)]
    y, x = np.argwhere(geo.tile[1] == 3)[0]
    levels[1][0, 5, y, x] = 0xF123
    raw = geo.pack(levels)
    want = np.zeros((1, geo.ntiles, 4), bool)
    want[0, 3, 1] = True
    assert np.array_equal(geo.flags(raw) != 0, want)
    assert np.array_equal(geo.unpack_levels(raw)[1], levels[1])
    raw[:, geo.flag_off:] = 0
    levels[1][0, 5, y, x] = 0x0123
    assert np.array_equal(geo.unpack_levels(raw)[1], levels[1])


def test_no_pixel_slots_are_where_the_prose_puts_them():
    """13 x 21 on the split 4 x 6 bank: nothing packed, six main blocks (two tiles, the last holds two blocks): of a level-0 plane's
    512 slots 273 hold a pixel; 9 x 10: one main block, one right and one bottom strip block (18 + 8 level-0 pixels)."""
    geo = sc.geometry(13, 21, 4, 6)
    assert (geo.pack_r, geo.pack_b, geo.nblk, geo.ntiles) == (False, False, 6, 2)
    assert int((geo.no_pixel_bits()[:geo.mid_off] != 0).sum()) == 2 * geo.s - 36 * 13 * 21 - 36 * 7 * 11
    geo = sc.geometry(9, 10, 4, 6)
    assert (geo.pack_r, geo.pack_b, geo.nmain, geo.n_r, geo.n_b, geo.ntiles) == (True, True, 1, 1, 1, 1)
    assert [int((geo.tile[0] == 0).sum()), int((geo.base[0][:, 8:] >= 0).sum()), int((geo.base[0][8, :8] >= 0).sum())] == [90, 18, 8]
    # by hand from the prose: pixel (8, 8) is the corner, the right strip's: block 1, parent q = 4 -> slot (2, 0), split slot
    # 2 * 32 + 1 * 8 + 0; pixel (8, 0) is the bottom strip's: block 2, parent 0 -> slot (0, 0), split slot 2 * 8
    assert (geo.base[0][8, 8], geo.base[0][8, 0], geo.base[0][0, 0], geo.base[0][1, 0]) == (72, 16, 0, 32)
