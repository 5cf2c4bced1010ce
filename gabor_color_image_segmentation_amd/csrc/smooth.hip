// smooth.hip — SPEC.md §10: Gaussian smoothing of the feature levels, in place on the feature slab (gfx950 only).
//
// Two launches, each covering every level of the bank in one grid:
//   smooth_planes_kernel  slab -> level planes: one workgroup per 64 x 16 tile of one plane of one level. It decodes the tile and
//                         an R-wide apron from the slab (SPEC.md §3 reflect rule at any distance; the TOP nibble only where the
//                         source tile's flag for the level is set, as the Lloyd pass does), runs the row sums in LDS (32 bits:
//                         sum w g <= 4096 * 46340 < 2^28) and the column sums on the 16-bit halves of the row sums (each below
//                         2^28 in 32 bits, joined once in 64 bits), rounds and writes h to the plane-major scratch
//                         [B][D_L][H_L][W_L] u16 of its level.
//   smooth_pack_kernel    level planes -> slab: one workgroup per slab tile, which owns every byte of the tile. Split slab: LO
//                         bytes and whole MID / TOP bytes of eight slots per lane (the nibble pairing of csrc/common.h), then the
//                         tile's FLAG word in one store, byte L = some TOP nibble written on level L is non-zero. Wide slab: 16-byte
//                         runs of offset-binary u16. Slots that hold no pixel keep their bytes.
// No atomics, no allocation, no host synchronisation: both launches sit on the caller's stream (and inside a captured graph).
#include "common.h"
#include "slab_slots.h"      // sm_nibble, sm_decode, sm_slot_pixel: shared with position.hip

namespace {

constexpr int SM_R_MAX = 24;                 // largest radius SPEC.md §10 allows
constexpr int SM_TAPS = 2 * SM_R_MAX + 1;    // taps per scale in the ABI array (centred)
constexpr int SM_TW = 64, SM_TH = 16;        // output tile of smooth_planes_kernel
constexpr int SM_AW = SM_TW + 2 * SM_R_MAX, SM_AH = SM_TH + 2 * SM_R_MAX;

struct SmoothLevel {
    int tx_n, ty_n;                          // tiles of a plane
    unsigned wg_end;                         // workgroups per image up to and including this level (planes kernel)
    size_t plane_off;                        // byte offset of the level's planes [B][D_L][H_L][W_L] in the workspace
};

struct SmoothArgs {
    GcsLayout lo;
    SmoothLevel lv[GCS_LEVELS_MAX];
    int B;
    const int32_t *taps;                     // [n_scales][49], centred
    const int32_t *radius;                   // [n_scales]
    unsigned char *feats;
    unsigned char *ws;
};

__device__ __forceinline__ int sm_reflect(int i, int n) {     // SPEC.md §3 reflect, any distance
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

__global__ __launch_bounds__(256) void smooth_planes_kernel(SmoothArgs A) {
    __shared__ uint16_t in[SM_AH][SM_AW];
    __shared__ uint32_t rs[SM_AH][SM_TW];
    __shared__ int wt[SM_TAPS];
    const GcsLayout &lo = A.lo;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    unsigned wg = blockIdx.x;
    int L = 0;
    while (L + 1 < lo.n_levels && wg >= A.lv[L].wg_end) ++L;
    if (L > 0) wg -= A.lv[L - 1].wg_end;
    const SmoothLevel lv = A.lv[L];
    const int per_plane = lv.tx_n * lv.ty_n;
    const int p = (int)(wg / (unsigned)per_plane), t = (int)(wg % (unsigned)per_plane);
    const int ty0 = (t / lv.tx_n) * SM_TH, tx0 = (t % lv.tx_n) * SM_TW;
    const int HL = lo.HL[L], WL = lo.WL[L];
    const int s = 2 * L + (p % lo.FL[L]) / lo.n_orient;          // filter scale of the plane
    // the scale's taps; a radius outside 1..24 or taps that are negative or do not sum to 4096 leave the plane as it is (R = 0)
    int R = A.radius[s];
    bool ok = R >= 1 && R <= SM_R_MAX;
    if (ok) {
        int sum = 0;
        for (int i = -R; i <= R; ++i) {
            const int w = A.taps[s * SM_TAPS + SM_R_MAX + i];
            ok = ok && w >= 0 && w <= 4096;
            sum += w;
        }
        ok = ok && sum == 4096;
    }
    if (!ok) R = 0;
    if (tid < SM_TAPS) wt[tid] = R ? (tid <= 2 * R ? A.taps[s * SM_TAPS + SM_R_MAX - R + tid] : 0) : (tid == 0 ? 4096 : 0);

    const unsigned char *img = A.feats + (size_t)b * lo.img_bytes;
    const int r = lo.row0[L] + p, AW = SM_TW + 2 * R, AH = SM_TH + 2 * R;
    const int ax = tid & 127;                                    // AW <= 112: one column per lane, two rows per step
    if (ax < AW) {
        const int xl = sm_reflect(tx0 + ax - R, WL);
        for (int ay = tid >> 7; ay < AH; ay += 2)
            in[ay][ax] = (uint16_t)sm_decode(lo, img, L, r, sm_reflect(ty0 + ay - R, HL), xl);
    }
    __syncthreads();
    const int n = 2 * R + 1;
    for (int i = tid; i < AH * SM_TW; i += 256) {
        const int ay = i >> 6, x = i & (SM_TW - 1);
        unsigned acc = 0;
        for (int j = 0; j < n; ++j) acc += (unsigned)wt[j] * in[ay][x + j];
        rs[ay][x] = acc;
    }
    __syncthreads();
    const int x = tid % SM_TW;
    uint16_t *out = reinterpret_cast<uint16_t *>(A.ws + lv.plane_off) + ((size_t)b * lo.DL[L] + p) * HL * WL;
#pragma unroll
    for (int k = 0; k < SM_TH / 4; ++k) {
        const int y = tid / SM_TW + 4 * k;
        unsigned lo16 = 0, hi16 = 0;                       // sum w (rs & 0xffff) < 2^28, sum w (rs >> 16) < 2^24
        for (int j = 0; j < n; ++j) {
            const unsigned v = rs[y + j][x], w = (unsigned)wt[j];
            lo16 += w * (v & 0xffffu);
            hi16 += w * (v >> 16);
        }
        const unsigned long long acc = ((unsigned long long)hi16 << 16) + lo16;
        if (ty0 + y < HL && tx0 + x < WL) out[(size_t)(ty0 + y) * WL + tx0 + x] = (uint16_t)((acc + (1ull << 23)) >> 24);
    }
}

__device__ __forceinline__ const uint16_t *sm_plane(const SmoothArgs &A, int L, int b, int p) {
    const GcsLayout &lo = A.lo;
    return reinterpret_cast<const uint16_t *>(A.ws + A.lv[L].plane_off) + ((size_t)b * lo.DL[L] + p) * lo.HL[L] * lo.WL[L];
}

__global__ __launch_bounds__(256) void smooth_pack_kernel(SmoothArgs A) {
    const GcsLayout &lo = A.lo;
    const int tile = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    unsigned char *img = A.feats + (size_t)b * lo.img_bytes;
    int bys[4], bxs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bys[i] = (4 * tile + i) / lo.bx_n;
        bxs[i] = 4 * tile + i - bys[i] * lo.bx_n;
    }
    if (!lo.split) {
        unsigned char *tb = img + (size_t)tile * lo.tile_bytes;
        for (int u = tid; u < lo.tile_bytes / 16; u += 256) {
            int L = 0;
            while (L + 1 < lo.n_levels && 16 * u >= lo.off[L + 1]) ++L;
            const int ssh = 3 - L, nsh = 8 - 2 * L, v0 = (16 * u - lo.off[L]) / 2;      // side 8 >> L, 256 >> 2L per plane
            unsigned short val[8];
            unsigned valid = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = v0 + i, p = v >> nsh, w = v & ((1 << nsh) - 1);
                const int bi = w >> (2 * ssh), rem = w & ((1 << (2 * ssh)) - 1);
                int yl = 0, xl = 0;
                val[i] = 0;
                if (p < lo.DL[L] && sm_slot_pixel(lo, 4 * tile + bi, bys[bi], bxs[bi], L, rem >> ssh, rem & ((1 << ssh) - 1), yl, xl)) {
                    val[i] = (unsigned short)(sm_plane(A, L, b, p)[(size_t)yl * lo.WL[L] + xl] ^ 0x8080u);
                    valid |= 1u << i;
                }
            }
            if (!valid) continue;
            v4i *dst = reinterpret_cast<v4i *>(tb + 16 * u);
            v4i o = valid == 0xffu ? v4i{0, 0, 0, 0} : *dst;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (!(valid >> i & 1)) val[i] = (unsigned short)((unsigned)o[i >> 1] >> (16 * (i & 1)));
            *dst = v4i{(int)(val[0] | (unsigned)val[1] << 16), (int)(val[2] | (unsigned)val[3] << 16),
                       (int)(val[4] | (unsigned)val[5] << 16), (int)(val[6] | (unsigned)val[7] << 16)};
        }
        return;
    }
    unsigned any[2] = {0u, 0u};
    for (int u = tid; u < lo.S / 8; u += 256) {
        const int s0 = 8 * u;
        const int L = lo.n_levels > 1 && s0 >= lo.sl0[1] ? 1 : 0;
        const int ssh = 3 - L, nsh = 8 - 2 * L, q0 = s0 - lo.sl0[L];   // side 8 >> L, 256 >> 2L slots per plane
        if (q0 >= lo.DL[L] << nsh) continue;                      // level padding: no plane
        const unsigned slot0 = (unsigned)tile * (unsigned)lo.S + (unsigned)s0;
        unsigned nb0;
        int sh0;
        sm_nibble(L, slot0, nb0, sh0);
        unsigned lo_w[2] = {0u, 0u}, mid = 0u, top = 0u, nmask = 0u, valid = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = q0 + i, p = q >> nsh, w = q & ((1 << nsh) - 1);
            const int sy = w >> (ssh + 2), rem = w & ((4 << ssh) - 1), bi = rem >> ssh, sx = rem & ((1 << ssh) - 1);
            int yl = 0, xl = 0;
            if (!sm_slot_pixel(lo, 4 * tile + bi, bys[bi], bxs[bi], L, sy, sx, yl, xl)) continue;
            const unsigned h = sm_plane(A, L, b, p)[(size_t)yl * lo.WL[L] + xl];
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
        if (valid != 0xffu) {                                     // slots without a pixel keep their bytes
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
    const int f0 = __syncthreads_or(any[0] != 0u), f1 = __syncthreads_or(any[1] != 0u);
    if (tid == 0) *reinterpret_cast<unsigned *>(img + lo.flag_off + 4u * (unsigned)tile) = (f0 ? 1u : 0u) | (f1 ? 0x100u : 0u);
}

bool sm_geometry(int B, int H, int W, int n_scales, int n_orient, GcsLayout &lo, SmoothLevel lv[GCS_LEVELS_MAX], size_t &bytes) {
    if (B <= 0 || H < 8 || W < 8 || !gcs_make_layout(H, W, n_scales, n_orient, &lo)) return false;
    bytes = 0;
    unsigned long long wg = 0;
    for (int L = 0; L < lo.n_levels; ++L) {
        lv[L].tx_n = (lo.WL[L] + SM_TW - 1) / SM_TW;
        lv[L].ty_n = (lo.HL[L] + SM_TH - 1) / SM_TH;
        wg += (unsigned long long)lo.DL[L] * lv[L].tx_n * lv[L].ty_n;
        if (wg > 0x7fffffffULL) return false;
        lv[L].wg_end = (unsigned)wg;
        lv[L].plane_off = bytes;
        bytes += ((size_t)B * lo.DL[L] * lo.HL[L] * lo.WL[L] * 2 + 255) / 256 * 256;
    }
    return B <= 65535 && lo.ntiles <= 0x7fffffff;
}

}  // namespace

extern "C" size_t gcs_smooth_workspace_bytes(int B, int H, int W, int n_scales, int n_orient) {
    GcsLayout lo;
    SmoothLevel lv[GCS_LEVELS_MAX];
    size_t bytes = 0;
    return sm_geometry(B, H, W, n_scales, n_orient, lo, lv, bytes) ? bytes : 0;
}

extern "C" int gcs_smooth_features(uint16_t *feats, int B, int H, int W, int n_scales, int n_orient, const int32_t *taps,
                                   const int32_t *radius, void *workspace, gcs_stream_t stream) {
    if (!feats || !taps || !radius || !workspace) return gcs_fail(GCS_EINVAL, "gcs_smooth_features: NULL pointer");
    SmoothArgs A{};
    size_t bytes = 0;
    if (!sm_geometry(B, H, W, n_scales, n_orient, A.lo, A.lv, bytes))
        return gcs_fail(GCS_EINVAL, "gcs_smooth_features: bad shape (B >= 1, H, W >= 8)");
    A.B = B;
    A.taps = taps;
    A.radius = radius;
    A.feats = reinterpret_cast<unsigned char *>(feats);
    A.ws = static_cast<unsigned char *>(workspace);
    hipLaunchKernelGGL(smooth_planes_kernel, dim3(A.lv[A.lo.n_levels - 1].wg_end, B), dim3(256), 0, stream, A);
    GCS_CHECK_LAUNCH("gcs_smooth_features(planes)");
    hipLaunchKernelGGL(smooth_pack_kernel, dim3(A.lo.ntiles, B), dim3(256), 0, stream, A);
    GCS_CHECK_LAUNCH("gcs_smooth_features(pack)");
    return GCS_OK;
}
