"""What tests/test_gpu_large_offsets.py and its CPU companion (tests/test_large_offset_geometry.py) share: the batch whose feature
slab crosses byte offsets 2^31 and 2^32, built by replication of a few distinct images, and the host assertions about it. No GPU
here: only the byte-count entry points of the library are called.

The shape, 81 x 130: 81 = 8 * 10 + 1 packs a one-row bottom strip and 130 = 8 * 16 + 2 a two-column right strip (csrc/common.h), the
main blocks make 10 block rows of 16, i.e. 4 tiles per block row and 42 tiles per image on banks of at most two levels (47 on deeper
ones, which pack no strips), the last of them not full; one image's slab is 0.9 to 1.9 MB, so B stays between 2 300 and 4 600 and
an image is far smaller than the 2^27 bytes the slab reaches past 2^32."""
import numpy as np

from slab_layout import tile_geometry

LINE31, LINE32 = 1 << 31, 1 << 32
MARGIN = 1 << 27                     # the slab ends at least this far behind 2^32: larger than any img_bytes used here
H, W = 81, 130
N_BASE = 16                          # two images of each of the eight kinds of tests/hot_banks.py
# id -> (n_scales, n_orient, ksize, shift): one bank per Gabor store path and per tile-addressing path of the Lloyd passes
BANKS = {"split_4x6": (4, 6, 13, 7),           # split slab (LO / MID / TOP / FLAG arrays), two levels
         "wide_3x9": (3, 9, 15, 7),            # wide slab at two levels, packed strips
         "deep_8x8": (8, 8, 15, 7),            # wide slab at four levels (the deep-bank pass)
         "generic_7x10": (7, 10, 13, 7)}       # D = 210: the generic pass


def batch_order(b):
    """The fixed pseudo-random sequence over the base images: a walk with steps 1 .. 7 modulo 16, so that any three consecutive
    images are three different base images (two steps add up to 2 .. 14)."""
    steps = np.random.default_rng(4242).integers(1, N_BASE // 2, b)
    return np.cumsum(steps) % N_BASE


def batch_geometry(lib, ns, no):
    """(img_bytes, B, idx, straddlers): B the smallest count with B * img_bytes >= 2^32 + 2^27, straddlers the image that holds byte
    2^31 and the one that holds 2^32. Asserts on the host that the slab crosses both lines, that an image straddles each, that the
    base images below, across and above each line differ, and that the batch is inside the entry points' own limits."""
    img_bytes = lib.gcs_feature_slab_bytes(1, H, W, ns, no)
    assert 0 < img_bytes < MARGIN
    b = -(-(LINE32 + MARGIN) // img_bytes)
    assert (b - 1) * img_bytes < LINE32 + MARGIN <= b * img_bytes
    assert lib.gcs_feature_slab_bytes(b, H, W, ns, no) == b * img_bytes > LINE32 > LINE31          # the slab crosses both lines
    idx = batch_order(b)
    assert idx.min() == 0 and idx.max() == N_BASE - 1 and np.bincount(idx).min() > b // (2 * N_BASE)
    straddlers = []
    for line in (LINE31, LINE32):
        i = line // img_bytes
        assert 1 <= i < b - 1 and i * img_bytes < line < (i + 1) * img_bytes                       # image i straddles the line
        assert len({int(idx[i - 1]), int(idx[i]), int(idx[i + 1])}) == 3                           # below, across, above: distinct
        straddlers.append(int(i))
    # the entry points' own limits (include/gcs.h; csrc/lloyd_pass.h: kp_batch_fits, kp_image_fits; gabor.hip: gabor_refuses)
    ntiles = tile_geometry(lib, H, W, ns, no)[0]
    assert b <= 65535 and b * ntiles <= 0x1fffffff and b * img_bytes <= 0x7fffffffffff and img_bytes < 1 << 32
    assert ntiles >= 8
    return img_bytes, b, idx, straddlers


def multiplicity(idx):
    return np.bincount(idx, minlength=N_BASE).astype(np.int64)
