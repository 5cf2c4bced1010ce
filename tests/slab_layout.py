"""What the tests know of the SPLIT feature slab's layout (csrc/common.h), in one place: the tile of every pixel and the
flag words behind the value runs. Test helper only; the package treats the slab as opaque bytes."""
import numpy as np


def tile_of_pixels(h, w):
    """(H, W) int array: the slab tile of every pixel for banks of at most two levels (csrc/common.h: main 8x8 blocks in raster
    order, then the virtual blocks of a packed right edge of 1 - 2 columns and a packed bottom edge of 1 - 2 rows)."""
    pack_r = h >= 8 and w >= 8 and (w & 7) in (1, 2)
    pack_b = h >= 8 and w >= 8 and (h & 7) in (1, 2)
    bx_n = w // 8 if pack_r else (w + 7) // 8
    by_n = h // 8 if pack_b else (h + 7) // 8
    wm = 8 * bx_n if pack_r else 1 << 29
    hm = 8 * by_n if pack_b else 1 << 29
    n_r = ((h + 1) // 2 + 15) // 16 if pack_r else 0
    nmain = bx_n * by_n
    y, x = np.mgrid[0:h, 0:w]
    blk = (y >> 3) * bx_n + (x >> 3)
    blk = np.where(x >= wm, nmain + ((y >> 1) >> 4), np.where(y >= hm, nmain + n_r + ((x >> 1) >> 4), blk))
    return blk >> 2


def flag_bytes(seg, feats, b, h, w):
    """The flag words of a split slab -> (uint8 [b][ntiles][4], ntiles): byte L of a tile's word belongs to pyramid level L
    (tests may know the layout: tile_bytes = 2 S, flags behind 2 S ntiles)."""
    lib = seg.ops.lib
    ns, no = seg.bank.n_scales, seg.bank.n_orient
    img_bytes = lib.gcs_feature_slab_bytes(1, h, w, ns, no)
    assert lib.gcs_feature_pass_bytes(1, h, w, ns, no) * 4 < img_bytes * 3 + 4, "this bank does not take the split slab"
    levels = [(3 * min(2, ns - 2 * L) * no, 256 >> (2 * L)) for L in range((ns + 1) // 2)]
    s = sum(d * n for d, n in levels)
    ntiles = img_bytes // (2 * s)
    raw = feats[:b * img_bytes].reshape(b, img_bytes)[:, 2 * s * ntiles:2 * s * ntiles + 4 * ntiles]     # (only the words travel)
    return raw.cpu().numpy().view(np.uint8).reshape(b, ntiles, 4), ntiles


def tile_geometry(lib, h, w, ns, no):
    """(ntiles, tile_bytes, split) of one image's slab from the bank's shape and the byte-count entry points: a tile holds, per
    pyramid level L, 3 * min(2, ns - 2 L) * no planes of 256 >> 2 L values of 16 bits, every level rounded up to 16 bytes
    (csrc/common.h). The split slab (a pass streams 3/4 of it: gcs_feature_pass_bytes) carries 4 flag bytes per tile behind the
    value runs, rounded up to 256 bytes per image; the wide slab is tiles and nothing else."""
    tile_bytes = sum(-(-3 * min(2, ns - 2 * L) * no * (256 >> (2 * L)) * 2 // 16) * 16 for L in range((ns + 1) // 2))
    img_bytes = lib.gcs_feature_slab_bytes(1, h, w, ns, no)
    pass_bytes = lib.gcs_feature_pass_bytes(1, h, w, ns, no)
    assert img_bytes > 0 and pass_bytes > 0, (h, w, ns, no)
    split = pass_bytes != img_bytes
    if split:
        ntiles = pass_bytes // (tile_bytes // 4 * 3)
        assert pass_bytes == ntiles * (tile_bytes // 4 * 3) and img_bytes == ntiles * tile_bytes + -(-4 * ntiles // 256) * 256
    else:
        ntiles = img_bytes // tile_bytes
        assert img_bytes == ntiles * tile_bytes
    return ntiles, tile_bytes, split
