// slab_slots.h — the slab seen slot by slot at a level's own resolution: what the kernels that rewrite planes of a filled slab in
// place share (smooth.hip: SPEC.md §10, position.hip: SPEC.md §12), and the plane-after-plane reader of the kernels that only read
// it (SlabTap below). Layout and names: common.h.
#pragma once
#include "common.h"

// gcs_split_nibble with the group size as a shift: byte (relative to the MID / TOP array) and bit shift of a slot's nibble
__device__ __forceinline__ void sm_nibble(int L, unsigned slot, unsigned &byte, int &shift) {
    const int gsh = L < 2 ? 3 - L : 1;
    const unsigned h = 1u << (gsh - 1), gi = slot & ((1u << gsh) - 1u), second = gi >= h ? 1u : 0u;
    byte = (slot >> gsh) * h + gi - second * h;
    shift = 4 * (int)second;
}

// Level-L pixel (yl, xl) -> value of physical plane r (plain uint16) in the slab `img` of one image.
__device__ __forceinline__ unsigned sm_decode(const GcsLayout &lo, const unsigned char *img, int L, int r, int yl, int xl) {
    const int y = yl << L, x = xl << L;      // any full-resolution pixel of the level pixel's block holds its value
    int blk, iy, ix;
    gcs_locate(lo, y, x, blk, iy, ix);
    const int side = 8 >> L, npl = KP_TP >> (2 * L);
    if (!lo.split) {
        const size_t off = (size_t)(blk >> 2) * lo.tile_bytes + lo.off[L] +
                           ((size_t)(r - lo.row0[L]) * npl + (blk & 3) * side * side + (iy >> L) * side + (ix >> L)) * 2;
        return *reinterpret_cast<const uint16_t *>(img + off) ^ 0x8080u;
    }
    const unsigned tile = (unsigned)(blk >> 2);
    const unsigned slot = tile * (unsigned)lo.S + (unsigned)(lo.sl0[L] + (r - lo.row0[L]) * npl + (iy >> L) * 4 * side +
                                                             (blk & 3) * side + (ix >> L));
    unsigned nb;
    int sh;
    sm_nibble(L, slot, nb, sh);
    unsigned v = (img[slot] ^ 0x80u) | (((unsigned)img[lo.mid_off + nb] >> sh & 15u) << 8);
    if (img[lo.flag_off + 4u * tile + (unsigned)L]) v |= ((unsigned)img[lo.top_off + nb] >> sh & 15u) << 12;
    return v;
}

// ---- a level pixel read plane after plane (feature_gradient.hip: SPEC.md §22, kmeans_model.hip: SPEC.md §28): the pixel is located
// once, then every plane of its level is one constant stride on.
// Where the pixel's value of the level's first plane sits in the slab of its image.
struct SlabTap {
    const unsigned char *p;           // wide slab: the value's address
    unsigned slot, nb;                // split slab: slot (LO byte index) and nibble byte (relative to MID / TOP)
    int sh;                           // split slab: the nibble's shift
    bool top;                         // split slab: the tile's level flag (some TOP nibble of the level is non-zero)
};

__device__ __forceinline__ SlabTap slab_tap(const GcsLayout &lo, const unsigned char *img, int L, int yl, int xl) {
    int blk, iy, ix;
    gcs_locate(lo, yl << L, xl << L, blk, iy, ix);      // any full-resolution pixel of the level pixel's block holds its value
    const unsigned tile = (unsigned)(blk >> 2), q = (unsigned)(blk & 3), side = 8u >> L;
    const unsigned sy = (unsigned)iy >> L, sx = (unsigned)ix >> L;
    SlabTap t{};
    if (lo.split) {
        t.slot = tile * (unsigned)lo.S + (unsigned)lo.sl0[L] + sy * 4u * side + q * side + sx;
        sm_nibble(L, t.slot, t.nb, t.sh);
        t.top = img[lo.flag_off + 4u * tile + (unsigned)L] != 0;
    } else {
        t.p = img + (size_t)tile * lo.tile_bytes + lo.off[L] + (size_t)(q * side * side + sy * side + sx) * 2;
    }
    return t;
}

// The tap's value of the plane it stands on (plain uint16), then one plane on.
template <bool SPLIT>
__device__ __forceinline__ int slab_next(const GcsLayout &lo, const unsigned char *img, SlabTap &t, unsigned npl) {
    unsigned v;
    if (SPLIT) {
        v = (img[t.slot] ^ 0x80u) | (((unsigned)img[lo.mid_off + t.nb] >> t.sh & 15u) << 8);
        if (t.top) v |= ((unsigned)img[lo.top_off + t.nb] >> t.sh & 15u) << 12;
        t.slot += npl, t.nb += npl >> 1;              // (a plane is a multiple of the nibble group: same shift)
    } else {
        v = (unsigned)*reinterpret_cast<const uint16_t *>(t.p) ^ 0x8080u;
        t.p += 2 * npl;
    }
    return (int)v;
}

// Slot (sy, sx) of level L in block blk -> the level pixel it holds; false: the slot holds no pixel.
// by / bx: the block's row and column when it is a main block (the callers divide once per tile, not per slot).
__device__ __forceinline__ bool sm_slot_pixel(const GcsLayout &lo, int blk, int by, int bx, int L, int sy, int sx, int &yl, int &xl) {
    if (blk >= lo.nblk) return false;
    if (blk < lo.nmain) {
        yl = ((8 * by) >> L) + sy;
        xl = ((8 * bx) >> L) + sx;
        return yl < lo.HL[L] && xl < lo.WL[L];
    }
    // virtual blocks of the packed edge strips (banks of at most two levels): csrc/common.h
    const bool right = blk < lo.nmain + lo.nR;
    const int v = blk - lo.nmain - (right ? 0 : lo.nR);
    if (L == 0) {
        const int s = 32 * v + 8 * (sy >> 1) + 2 * (sx >> 1);
        yl = right ? s + (sy & 1) : lo.Hm + (sy & 1);
        xl = right ? lo.Wm + (sx & 1) : s + (sx & 1);
        return yl < lo.H && xl < (right ? lo.W : lo.Wb);
    }
    const int q = 16 * v + 4 * sy + sx;      // the strip's level-1 parent
    yl = right ? q : lo.Hm >> 1;
    xl = right ? lo.Wm >> 1 : q;
    return right ? 2 * q < lo.H : 2 * q < lo.Wb;
}
