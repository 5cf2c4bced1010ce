// position.hip — SPEC.md §12: the coordinate slot of every scale, written in place on a filled feature slab (gfx950 only).
//
// The bank's last slot of every scale has zero taps: the Gabor stage (and the smoothing of §10) leave zeros in its three planes.
// One launch, one workgroup per slab tile, covering every level, then fills channel 0 of that slot with weight * (global row) and
// channel 1 with weight * (column) of the level pixel a slot holds, at the level's resolution: 2 n_scales planes of the 3 F (8 of
// 72, 11 % of a tile's bytes, for the recommended bank), so the launch streams stores and reads nothing but its arguments where a
// run of slots is full.
//   split slab  a work item is eight consecutive slots of one plane: 8 LO bytes and the whole MID / TOP words of their nibbles, the
//               ownership smooth_pack_kernel uses (the nibble pairing of csrc/common.h). The tile's flag byte of level L is SET when
//               a TOP nibble written on that level is non-zero (one byte store by one lane; the bytes the Gabor stage set stay).
//   wide slab   a work item is a 16-byte run of offset-binary u16 of one plane (a level-3 plane of a tile is one 8-byte run).
// Slots that hold no pixel (image edge, last tile, packed strips) keep their bytes: such runs are read, merged and written back.
// No atomics, no workspace, no allocation, no host synchronisation: the launch sits on the caller's stream (and inside a captured graph).
#include "common.h"
#include "slab_slots.h"

namespace {

constexpr int PF_VALUE_MAX = 46340;          // SPEC.md §3 value range

struct PositionArgs {
    GcsLayout lo;
    int item0[GCS_LEVELS_MAX + 1];           // first work item of level L inside a tile; [n_levels] = items per tile
    int weight, y0;
    unsigned char *feats;
};

// Work item `it` of level L -> the physical plane (in level) it belongs to, the channel (0: row, 1: column) and the run inside it.
__device__ __forceinline__ void pf_item(const GcsLayout &lo, int L, int it, int &p, int &c, int &run) {
    const int rsh = L < 3 ? 5 - 2 * L : 0;   // runs per plane: 256 >> 2L values in runs of eight (one run of four on level 3)
    const int scales = lo.FL[L] / lo.n_orient, j = it >> rsh;
    run = it & ((1 << rsh) - 1);
    c = j >= scales ? 1 : 0;
    p = c * lo.FL[L] + (j - c * scales) * lo.n_orient + lo.n_orient - 1;
}

__global__ __launch_bounds__(256) void position_kernel(PositionArgs A) {
    const GcsLayout &lo = A.lo;
    const int tile = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    unsigned char *img = A.feats + (size_t)b * lo.img_bytes;
    const int n_items = A.item0[lo.n_levels];
    int bys[4], bxs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bys[i] = (4 * tile + i) / lo.bx_n;
        bxs[i] = 4 * tile + i - bys[i] * lo.bx_n;
    }
    if (!lo.split) {
        unsigned char *tb = img + (size_t)tile * lo.tile_bytes;
        for (int it = tid; it < n_items; it += 256) {
            int L = 0;
            while (L + 1 < lo.n_levels && it >= A.item0[L + 1]) ++L;
            int p, c, run;
            pf_item(lo, L, it - A.item0[L], p, c, run);
            const int ssh = 3 - L, nsh = 8 - 2 * L, n = L < 3 ? 8 : 4;      // side 8 >> L, 256 >> 2L values per plane
            unsigned short val[8];
            unsigned valid = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int w = 8 * run + i, bi = w >> (2 * ssh), rem = w & ((1 << (2 * ssh)) - 1);
                int yl = 0, xl = 0;
                val[i] = 0;
                if (i < n && sm_slot_pixel(lo, 4 * tile + bi, bys[bi & 3], bxs[bi & 3], L, rem >> ssh, rem & ((1 << ssh) - 1), yl, xl)) {
                    const unsigned v = (unsigned)A.weight * (unsigned)(c ? xl << L : A.y0 + (yl << L));
                    val[i] = (unsigned short)(v ^ 0x8080u);
                    valid |= 1u << i;
                }
            }
            if (!valid) continue;
            unsigned char *dst = tb + lo.off[L] + (((size_t)p << nsh) + 8 * run) * 2;
            if (n == 4) {                                                 // a level-3 plane: four values, 8 bytes
                v2i o = *reinterpret_cast<const v2i *>(dst);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (!(valid >> i & 1)) val[i] = (unsigned short)((unsigned)o[i >> 1] >> (16 * (i & 1)));
                *reinterpret_cast<v2i *>(dst) = v2i{(int)(val[0] | (unsigned)val[1] << 16), (int)(val[2] | (unsigned)val[3] << 16)};
                continue;
            }
            v4i o = valid == 0xffu ? v4i{0, 0, 0, 0} : *reinterpret_cast<const v4i *>(dst);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (!(valid >> i & 1)) val[i] = (unsigned short)((unsigned)o[i >> 1] >> (16 * (i & 1)));
            *reinterpret_cast<v4i *>(dst) = v4i{(int)(val[0] | (unsigned)val[1] << 16), (int)(val[2] | (unsigned)val[3] << 16),
                                                (int)(val[4] | (unsigned)val[5] << 16), (int)(val[6] | (unsigned)val[7] << 16)};
        }
        return;
    }
    unsigned any[2] = {0u, 0u};
    for (int it = tid; it < n_items; it += 256) {
        const int L = lo.n_levels > 1 && it >= A.item0[1] ? 1 : 0;
        int p, c, run;
        pf_item(lo, L, it - A.item0[L], p, c, run);
        const int ssh = 3 - L, nsh = 8 - 2 * L;                           // side 8 >> L, 256 >> 2L slots per plane
        const unsigned slot0 = (unsigned)tile * (unsigned)lo.S + (unsigned)(lo.sl0[L] + (p << nsh) + 8 * run);
        unsigned nb0;
        int sh0;
        sm_nibble(L, slot0, nb0, sh0);
        unsigned lo_w[2] = {0u, 0u}, mid = 0u, top = 0u, nmask = 0u, valid = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int w = 8 * run + i;
            const int sy = w >> (ssh + 2), rem = w & ((4 << ssh) - 1), bi = rem >> ssh, sx = rem & ((1 << ssh) - 1);
            int yl = 0, xl = 0;
            if (!sm_slot_pixel(lo, 4 * tile + bi, bys[bi], bxs[bi], L, sy, sx, yl, xl)) continue;
            const unsigned h = (unsigned)A.weight * (unsigned)(c ? xl << L : A.y0 + (yl << L));
            unsigned nb;
            int sh;
            sm_nibble(L, slot0 + (unsigned)i, nb, sh);
            const int pos = 8 * (int)(nb - nb0) + sh;
            lo_w[i >> 2] |= ((h & 0xffu) ^ 0x80u) << (8 * (i & 3));
            mid |= (h >> 8 & 15u) << pos;
            top |= (h >> 12 & 15u) << pos;
            nmask |= 15u << pos;
            valid |= 1u << i;
        }
        if (!valid) continue;
        any[L] |= top;
        unsigned *lo_dst = reinterpret_cast<unsigned *>(img + slot0);
        unsigned *mid_dst = reinterpret_cast<unsigned *>(img + lo.mid_off + nb0);
        unsigned *top_dst = reinterpret_cast<unsigned *>(img + lo.top_off + nb0);
        if (valid != 0xffu) {                                             // slots without a pixel keep their bytes
            unsigned bmask[2] = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (valid >> i & 1) bmask[i >> 2] |= 0xffu << (8 * (i & 3));
            const v2i old = *reinterpret_cast<const v2i *>(lo_dst);
            lo_w[0] |= (unsigned)old[0] & ~bmask[0];
            lo_w[1] |= (unsigned)old[1] & ~bmask[1];
            mid |= *mid_dst & ~nmask;
            top |= *top_dst & ~nmask;
        }
        *reinterpret_cast<v2i *>(lo_dst) = v2i{(int)lo_w[0], (int)lo_w[1]};
        *mid_dst = mid;
        *top_dst = top;
    }
    // set, never clear: the other planes of the tile may have raised the flag already (one lane per byte, a plain byte store)
    const int f0 = __syncthreads_or(any[0] != 0u), f1 = __syncthreads_or(any[1] != 0u);
    if (tid == 0 && f0) img[lo.flag_off + 4u * (unsigned)tile] = 1;
    if (tid == 1 && f1) img[lo.flag_off + 4u * (unsigned)tile + 1u] = 1;
}

}  // namespace

extern "C" int gcs_position_features(uint16_t *feats, int B, int H, int W, int n_scales, int n_orient, int weight, int y0,
                                     gcs_stream_t stream) {
    if (!feats) return gcs_fail(GCS_EINVAL, "gcs_position_features: NULL pointer");
    PositionArgs A{};
    if (B <= 0 || B > 65535 || H < 8 || W < 8 || !gcs_make_layout(H, W, n_scales, n_orient, &A.lo) || A.lo.ntiles > 0x7fffffff)
        return gcs_fail(GCS_EINVAL, "gcs_position_features: bad shape (1 <= B <= 65535, H, W >= 8)");
    if (weight < 1 || weight > 255) return gcs_fail(GCS_EINVAL, "gcs_position_features: weight outside 1..255");
    if (y0 < 0 || y0 & ((1 << (A.lo.n_levels - 1)) - 1))
        return gcs_fail(GCS_EINVAL, "gcs_position_features: y0 negative or not a multiple of 2^(levels - 1)");
    const long long reach = (long long)y0 + H > W ? (long long)y0 + H : W;
    if ((long long)weight * (reach - 1) > PF_VALUE_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_position_features: weight * (max(y0 + H, W) - 1) exceeds 46340 (SPEC.md 3 value range)");
    int items = 0;
    for (int L = 0; L < A.lo.n_levels; ++L) {
        A.item0[L] = items;
        const int runs = L < 3 ? (KP_TP >> (2 * L)) / 8 : 1;
        items += 2 * (A.lo.FL[L] / n_orient) * runs;                     // two channels of one slot per scale of the level
    }
    A.item0[A.lo.n_levels] = items;
    A.weight = weight;
    A.y0 = y0;
    A.feats = reinterpret_cast<unsigned char *>(feats);
    hipLaunchKernelGGL(position_kernel, dim3(A.lo.ntiles, B), dim3(256), 0, stream, A);
    GCS_CHECK_LAUNCH("gcs_position_features");
    return GCS_OK;
}
