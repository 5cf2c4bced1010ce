// feature_gradient.hip — the texture-gradient edge map of SPEC.md §22, read from the FEATURE SLAB (either format) at every level's
// own resolution: G = floor(sqrt(sum over levels of the level's squared central differences, shifted right by 2L)).
//
//   fg_kernel   one workgroup per 8 x 32 full-resolution pixels (aligned to the 8 x 8 blocks, so the level-L pixels under it are a
//               whole (8 >> L) x (32 >> L) rectangle). First the level >= 1 terms of that rectangle, ONE thread per level pixel
//               (threads 0..63: level 1, 64..79: level 2, 80..83: level 3), into LDS; then a thread per full-resolution pixel adds
//               its level-0 term and the terms of its parents and takes the exact square root. Every thread locates its four clamped
//               neighbours once (slab_tap) and then steps through the level's planes at a constant stride, as rt_slab_walk does.
//               (-DGCS_FG_PER_PIXEL: every pixel recomputes the terms of its parents itself, for same-box A/B runs: DESIGN.md §4.20.)
// No workspace, no allocation, no host synchronisation: one launch (capturable).
#include "slab_slots.h"

namespace {

typedef unsigned long long u64;

constexpr int FG_TW = 32, FG_TH = 8, FG_THREADS = FG_TW * FG_TH;
constexpr int FG_HW_MAX = 4096, FG_D_MAX = 207;

// (DX_L >> 2L) + (DY_L >> 2L) of SPEC.md §22 at level pixel (yl, xl), which lies inside the level image.
template <bool SPLIT>
__device__ __forceinline__ u64 fg_level(const GcsLayout &lo, const unsigned char *img, int L, int yl, int xl) {
    const int HL = lo.HL[L], WL = lo.WL[L];
    SlabTap xm = slab_tap(lo, img, L, yl, max(xl - 1, 0)), xp = slab_tap(lo, img, L, yl, min(xl + 1, WL - 1));
    SlabTap ym = slab_tap(lo, img, L, max(yl - 1, 0), xl), yp = slab_tap(lo, img, L, min(yl + 1, HL - 1), xl);
    const unsigned npl = (unsigned)KP_TP >> (2 * L);
    u64 dx = 0, dy = 0;
    for (int d = lo.DL[L]; d > 0; --d) {
        const int a = slab_next<SPLIT>(lo, img, xp, npl) - slab_next<SPLIT>(lo, img, xm, npl);
        const int c = slab_next<SPLIT>(lo, img, yp, npl) - slab_next<SPLIT>(lo, img, ym, npl);
        dx += (u64)((unsigned)a * (unsigned)a);       // |a| <= 65535: a^2 < 2^32
        dy += (u64)((unsigned)c * (unsigned)c);
    }
    return (dx >> (2 * L)) + (dy >> (2 * L));
}

template <bool SPLIT>
__global__ __launch_bounds__(FG_THREADS) void fg_kernel(const unsigned char *__restrict__ slab, GcsLayout lo, int32_t *__restrict__ out) {
    __shared__ u64 s_term[64 + 16 + 4];                                   // level 1: 4 x 16, level 2: 2 x 8, level 3: 1 x 4
    const int tid = (int)threadIdx.x, b = (int)blockIdx.z;
    const int y0 = (int)blockIdx.y * FG_TH, x0 = (int)blockIdx.x * FG_TW;
    const unsigned char *img = slab + (size_t)b * (size_t)lo.img_bytes;
#ifndef GCS_FG_PER_PIXEL
    {
        const int L = tid < 64 ? 1 : tid < 80 ? 2 : tid < 84 ? 3 : GCS_LEVELS_MAX;
        if (L < lo.n_levels) {
            const int i = tid - (L == 1 ? 0 : L == 2 ? 64 : 80), wl = FG_TW >> L;
            const int yl = (y0 >> L) + i / wl, xl = (x0 >> L) + i % wl;
            s_term[tid] = yl < lo.HL[L] && xl < lo.WL[L] ? fg_level<SPLIT>(lo, img, L, yl, xl) : 0ull;
        }
    }
    __syncthreads();
#endif
    const int ty = tid / FG_TW, tx = tid % FG_TW, y = y0 + ty, x = x0 + tx;
    if (y >= lo.H || x >= lo.W) return;
    u64 e = fg_level<SPLIT>(lo, img, 0, y, x);
    for (int L = 1; L < lo.n_levels; ++L) {
#ifdef GCS_FG_PER_PIXEL
        e += fg_level<SPLIT>(lo, img, L, y >> L, x >> L);
#else
        e += s_term[(L == 1 ? 0 : L == 2 ? 64 : 80) + (ty >> L) * (FG_TW >> L) + (tx >> L)];
#endif
    }
    out[((size_t)b * lo.H + y) * lo.W + x] = fg_isqrt(e);
}

}  // namespace

extern "C" int gcs_feature_gradient(const uint16_t *feats_slab, int B, int H, int W, int n_scales, int n_orient, int32_t *grad_out,
                                    gcs_stream_t stream) {
    if (!feats_slab || !grad_out) return gcs_fail(GCS_EINVAL, "gcs_feature_gradient: NULL pointer");
    GcsLayout lo;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > FG_HW_MAX || W > FG_HW_MAX || !gcs_make_layout(H, W, n_scales, n_orient, &lo) ||
        lo.D > FG_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_feature_gradient: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, a bank of at most 207 features)");
    const dim3 grid((W + FG_TW - 1) / FG_TW, (H + FG_TH - 1) / FG_TH, B);
    const unsigned char *slab = reinterpret_cast<const unsigned char *>(feats_slab);
    if (lo.split)
        hipLaunchKernelGGL(fg_kernel<true>, grid, dim3(FG_THREADS), 0, stream, slab, lo, grad_out);
    else
        hipLaunchKernelGGL(fg_kernel<false>, grid, dim3(FG_THREADS), 0, stream, slab, lo, grad_out);
    GCS_CHECK_LAUNCH("gcs_feature_gradient");
    return GCS_OK;
}
