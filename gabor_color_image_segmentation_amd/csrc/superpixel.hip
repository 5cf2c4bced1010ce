// superpixel.hip — SPEC.md §13: grid-local k-means (superpixels) on the canonical [B][D][H][W] uint16 features (gfx950 only).
//
// K = ny * nx centres per image on a grid; a pixel of cell (gi, gj) is compared with the centres of the 3 x 3 cells around it only,
// with dist = sum_d (x_d - c_d)^2 + lambda ((y - cy)^2 + (x - cx)^2) in 64-bit integers, ties to the lowest centre index. One call
// enqueues the whole schedule: init, then n_iter assigns with an update behind all but the last.
//   sp_init_kernel      centre q of image b := the feature vector of pixel (cy_q, cx_q); its sums := 0.
//   sp_pass_kernel      one workgroup per 8 x 32 pixel tile, one thread per pixel. The centres of every cell the tile's pixels can
//                       see (the tile's cell range grown by one: at most SP_CMAX of them) sit in LDS as uint16 quads, so a thread
//                       reads its D planes once, coalesced along the row, and 9 LDS quads per 4 planes. The squares are 24-bit
//                       multiplies (|x - c| <= 46 340 < 2^16) summed in pairs in 32 bits (2 * 46 340^2 < 2^32), then in 64. An
//                       accumulating pass reads the planes a second time (they are in L2) and adds them, y, x and 1 into uint32 LDS rows
//                       per candidate centre (256 pixels * 46 340 < 2^32), eight lanes that agree on the centre adding one sum; the
//                       rows of centres that received a pixel are flushed into the image's [K][D + 3] uint64 sums with 64-bit vector
//                       atomics (integer sums: any order gives the same bits).
//                       A tile that sees more than SP_CMAX centres (cells of a few pixels) takes the same code without LDS: centres
//                       from global memory, sums straight into the global rows.
//   sp_update_kernel    SPEC.md §4's rule on every feature and on cy, cx: c = floor((2 S + n) / (2 n)), an empty centre keeps its
//                       values; the sums are zeroed for the next pass.
//   sp_export_kernel    centres_out (optional): int32 [B][K][D + 2] = the D features, cy, cx the LAST assign used.
// Reads 2 D bytes per pixel per pass from HBM (the canonical tensor is not compressed like the slab): DESIGN.md §4.10.
// No allocation, no host synchronisation: every launch sits on the caller's stream (and inside a captured graph).
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int SP_TH = 8, SP_TW = 32;         // tile: 8 rows of 32 pixels, 256 threads
constexpr int SP_CMAX = 32;                  // centres a tile holds in LDS
constexpr int SP_D_MAX = 207, SP_K_MAX = 4096, SP_HW_MAX = 4096;

struct SpArgs {
    const uint16_t *feats;                   // [B][D][H][W]
    unsigned long long *cent;                // [B][K][DQ] quads of uint16 (planes 4i .. 4i + 3; planes >= D are zero)
    int *pos;                                // [B][K][2] = cy, cx
    unsigned long long *sums;                // [B][K][D + 3] = the D feature sums, sum y, sum x, count
    int *labels;                             // [B][H][W], written by the last pass
    int *centres_out;                        // [B][K][D + 2] or NULL
    int B, H, W, D, DQ, ny, nx, K, lambda;
};

__host__ __device__ inline size_t sp_align(size_t n) { return (n + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void sp_init_kernel(SpArgs A) {
    const int q = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int i = q / A.nx, j = q - i * A.nx;
    const int cy = (int)(((long long)(2 * i + 1) * A.H) / (2 * A.ny)), cx = (int)(((long long)(2 * j + 1) * A.W) / (2 * A.nx));
    const size_t bq = (size_t)b * A.K + q, hw = (size_t)A.H * A.W;
    const uint16_t *px = A.feats + (size_t)b * A.D * hw + (size_t)cy * A.W + cx;
    for (int dq = tid; dq < A.DQ; dq += 256) {
        unsigned long long v = 0;
        for (int e = 0; e < 4; ++e)
            if (4 * dq + e < A.D) v |= (unsigned long long)px[(size_t)(4 * dq + e) * hw] << (16 * e);
        A.cent[bq * A.DQ + dq] = v;
    }
    for (int e = tid; e < A.D + 3; e += 256) A.sums[bq * (A.D + 3) + e] = 0;
    if (tid == 0) {
        A.pos[2 * bq] = cy;
        A.pos[2 * bq + 1] = cx;
    }
}

__global__ __launch_bounds__(256) void sp_update_kernel(SpArgs A) {
    const int q = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const size_t bq = (size_t)b * A.K + q;
    unsigned long long *s = A.sums + bq * (A.D + 3);
    const unsigned long long n = s[A.D + 2];
    __syncthreads();                                                      // every thread has the count before it is zeroed
    if (n) {
        uint16_t *c = reinterpret_cast<uint16_t *>(A.cent + bq * A.DQ);
        for (int d = tid; d < A.D; d += 256) c[d] = (uint16_t)((2 * s[d] + n) / (2 * n));
        if (tid < 2) A.pos[2 * bq + tid] = (int)((2 * s[A.D + tid] + n) / (2 * n));
    }
    __syncthreads();
    for (int e = tid; e < A.D + 3; e += 256) s[e] = 0;
}

__global__ __launch_bounds__(256) void sp_export_kernel(SpArgs A) {
    const int q = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const size_t bq = (size_t)b * A.K + q;
    const uint16_t *c = reinterpret_cast<const uint16_t *>(A.cent + bq * A.DQ);
    int *o = A.centres_out + bq * (A.D + 2);
    for (int d = tid; d < A.D; d += 256) o[d] = c[d];
    if (tid < 2) o[A.D + tid] = A.pos[2 * bq + tid];
}

__device__ __forceinline__ unsigned sp_sq2(unsigned x01, unsigned c01) {      // (x0 - c0)^2 + (x1 - c1)^2 of two packed uint16 pairs
    const int d0 = (int)(x01 & 0xffffu) - (int)(c01 & 0xffffu), d1 = (int)(x01 >> 16) - (int)(c01 >> 16);
    return (unsigned)__mul24(d0, d0) + (unsigned)__mul24(d1, d1);
}

// LDS: the tile's centres live in dynamic shared memory; otherwise they are read from global memory.
template <bool LDS>
__device__ __forceinline__ void sp_tile(const SpArgs &A, unsigned long long *s_cent, unsigned *s_acc, int *s_pos, int accumulate,
                                        int gi_lo, int gj_lo, int nci, int ncj) {
    const int tid = (int)threadIdx.x, b = (int)blockIdx.z;
    const int ty0 = (int)blockIdx.y * SP_TH, tx0 = (int)blockIdx.x * SP_TW;
    const int D = A.D, DQ = A.DQ, E = D + 3, ncand = nci * ncj;
    const size_t hw = (size_t)A.H * A.W;
    const unsigned long long *g_cent = A.cent + (size_t)b * A.K * DQ;
    const int *g_pos = A.pos + (size_t)b * A.K * 2;
    if (LDS) {
        for (int idx = tid; idx < ncand * DQ; idx += 256) {
            const int s = idx / DQ, dq = idx - s * DQ, q = (gi_lo + s / ncj) * A.nx + gj_lo + s % ncj;
            s_cent[idx] = g_cent[(size_t)q * DQ + dq];
        }
        for (int idx = tid; idx < ncand * 2; idx += 256) {
            const int s = idx >> 1, q = (gi_lo + s / ncj) * A.nx + gj_lo + s % ncj;
            s_pos[idx] = g_pos[2 * q + (idx & 1)];
        }
        if (accumulate)
            for (int idx = tid; idx < ncand * E; idx += 256) s_acc[idx] = 0u;
        __syncthreads();
    }
    const int yy = ty0 + tid / SP_TW, xx = tx0 + tid % SP_TW;
    const bool valid = yy < A.H && xx < A.W;
    const int y = valid ? yy : (yy < A.H ? yy : A.H - 1), x = valid ? xx : (xx < A.W ? xx : A.W - 1);   // clamped: reads stay inside
    const int gi = y * A.ny / A.H, gj = x * A.nx / A.W;
    // the 3 x 3 candidates, clamped to the grid: a clamped duplicate has the same centre and the same distance as the original
    int cq[9], cs[9];
    unsigned long long dist[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        int ci = gi + c / 3 - 1, cj = gj + c % 3 - 1;
        ci = ci < 0 ? 0 : (ci >= A.ny ? A.ny - 1 : ci);
        cj = cj < 0 ? 0 : (cj >= A.nx ? A.nx - 1 : cj);
        cq[c] = ci * A.nx + cj;
        cs[c] = LDS ? (ci - gi_lo) * ncj + (cj - gj_lo) : cq[c];
        const int py = LDS ? s_pos[2 * cs[c]] : g_pos[2 * cq[c]], pxx = LDS ? s_pos[2 * cs[c] + 1] : g_pos[2 * cq[c] + 1];
        const int dy = y - py, dx = x - pxx;
        dist[c] = (unsigned long long)(unsigned)A.lambda * (unsigned long long)(unsigned)(dy * dy + dx * dx);
    }
    const uint16_t *px = A.feats + (size_t)b * D * hw + (size_t)y * A.W + x;
    for (int dq = 0; dq < DQ; ++dq) {
        const int d = 4 * dq;
        const unsigned x0 = px[(size_t)d * hw], x1 = d + 1 < D ? px[(size_t)(d + 1) * hw] : 0u;
        const unsigned x2 = d + 2 < D ? px[(size_t)(d + 2) * hw] : 0u, x3 = d + 3 < D ? px[(size_t)(d + 3) * hw] : 0u;
        const unsigned x01 = x0 | x1 << 16, x23 = x2 | x3 << 16;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const unsigned long long cv = LDS ? s_cent[cs[c] * DQ + dq] : g_cent[(size_t)cs[c] * DQ + dq];
            dist[c] += (unsigned long long)sp_sq2(x01, (unsigned)cv) + (unsigned long long)sp_sq2(x23, (unsigned)(cv >> 32));
        }
    }
    int best = 0;
#pragma unroll
    for (int c = 1; c < 9; ++c)
        if (dist[c] < dist[best] || (dist[c] == dist[best] && cq[c] < cq[best])) best = c;
    int bq = cq[0], bs = cs[0];
#pragma unroll
    for (int c = 1; c < 9; ++c)
        if (best == c) {
            bq = cq[c];
            bs = cs[c];
        }
    if (A.labels && valid) A.labels[(size_t)b * hw + (size_t)y * A.W + x] = bq;
    if (!accumulate) return;
    if (LDS) {
        // eight neighbouring lanes that are all valid and agree on the centre add ONE sum (fewer same-address LDS atomics)
        int same = valid ? 1 : 0;
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {
            const int obs = __shfl_xor(bs, m), osame = __shfl_xor(same, m);
            same = same && osame && obs == bs;
        }
        unsigned *row = s_acc + bs * E;
        const bool lead = (tid & 7) == 0;
        for (int d = 0; d < E; ++d) {
            unsigned v = d < D ? px[(size_t)d * hw] : (d == D ? (unsigned)y : (d == D + 1 ? (unsigned)x : 1u));
            unsigned t = v;
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) t += (unsigned)__shfl_xor((int)t, m);
            if (same) {
                if (lead) atomicAdd(row + d, t);
            } else if (valid) {
                atomicAdd(row + d, v);
            }
        }
        __syncthreads();
        unsigned long long *g_sums = A.sums + (size_t)b * A.K * E;
        for (int idx = tid; idx < ncand * E; idx += 256) {
            const int s = idx / E, e = idx - s * E;
            const unsigned v = s_acc[idx];
            if (v) {
                const int q = (gi_lo + s / ncj) * A.nx + gj_lo + s % ncj;
                atomicAdd(g_sums + (size_t)q * E + e, (unsigned long long)v);
            }
        }
    } else if (valid) {
        unsigned long long *row = A.sums + ((size_t)b * A.K + bq) * E;
        for (int d = 0; d < D; ++d) atomicAdd(row + d, (unsigned long long)px[(size_t)d * hw]);
        atomicAdd(row + D, (unsigned long long)y);
        atomicAdd(row + D + 1, (unsigned long long)x);
        atomicAdd(row + D + 2, 1ull);
    }
}

__global__ __launch_bounds__(256) void sp_pass_kernel(SpArgs A, int accumulate) {
    extern __shared__ unsigned long long sp_smem[];
    const int ty0 = (int)blockIdx.y * SP_TH, tx0 = (int)blockIdx.x * SP_TW;
    const int yl = min(ty0 + SP_TH, A.H) - 1, xl = min(tx0 + SP_TW, A.W) - 1;
    const int gi_lo = max(ty0 * A.ny / A.H - 1, 0), gi_hi = min(yl * A.ny / A.H + 1, A.ny - 1);
    const int gj_lo = max(tx0 * A.nx / A.W - 1, 0), gj_hi = min(xl * A.nx / A.W + 1, A.nx - 1);
    const int nci = gi_hi - gi_lo + 1, ncj = gj_hi - gj_lo + 1;
    if (nci * ncj <= SP_CMAX) {                                           // (uniform over the workgroup)
        unsigned long long *s_cent = sp_smem;                             // [SP_CMAX][DQ]
        unsigned *s_acc = reinterpret_cast<unsigned *>(s_cent + SP_CMAX * A.DQ);   // [SP_CMAX][D + 3]
        int *s_pos = reinterpret_cast<int *>(s_acc + SP_CMAX * (A.D + 3));         // [SP_CMAX][2]
        sp_tile<true>(A, s_cent, s_acc, s_pos, accumulate, gi_lo, gj_lo, nci, ncj);
    } else {
        sp_tile<false>(A, nullptr, nullptr, nullptr, accumulate, 0, 0, A.ny, A.nx);
    }
}

size_t sp_smem_bytes(int D) { return (size_t)SP_CMAX * ((size_t)((D + 3) / 4) * 8 + (size_t)(D + 3) * 4 + 8); }

int sp_rint(double v) { return (int)nearbyint(v); }                       // round-half-even (the default rounding mode)

}  // namespace

extern "C" int gcs_superpixel_grid(int H, int W, int n, int *S_out, int *ny_out, int *nx_out) {
    if (H < 1 || W < 1 || H > SP_HW_MAX || W > SP_HW_MAX || n < 2 || n > SP_K_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_superpixel_grid: needs 1 <= H, W <= 4096 and 2 <= n <= 4096");
    const int S = std::max(1, sp_rint(sqrt((double)((long long)H * W) / (double)n)));
    const int ny = std::max(1, sp_rint((double)H / (double)S)), nx = std::max(1, sp_rint((double)W / (double)S));
    if (S_out) *S_out = S;
    if (ny_out) *ny_out = ny;
    if (nx_out) *nx_out = nx;
    return GCS_OK;
}

extern "C" size_t gcs_superpixel_workspace_bytes(int B, int H, int W, int D, int n) {
    int ny, nx;
    if (B < 1 || B > 65535 || D < 1 || D > SP_D_MAX || gcs_superpixel_grid(H, W, n, nullptr, &ny, &nx) != GCS_OK) return 0;
    const size_t K = (size_t)ny * nx;
    if (K > SP_K_MAX) return 0;
    return (size_t)B * (sp_align(K * ((D + 3) / 4) * 8) + sp_align(K * 8) + sp_align(K * (D + 3) * 8));
}

extern "C" int gcs_superpixel_segment(const uint16_t *feats, int B, int H, int W, int D, int ny, int nx, int lambda, int n_iter,
                                      void *workspace, int32_t *labels_out, int32_t *centres_out, gcs_stream_t stream) {
    if (!feats || !workspace || !labels_out) return gcs_fail(GCS_EINVAL, "gcs_superpixel_segment: NULL pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > SP_HW_MAX || W > SP_HW_MAX || D < 1 || D > SP_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_superpixel_segment: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 1 <= D <= 207)");
    if (ny < 1 || nx < 1 || ny > H || nx > W || (long long)ny * nx > SP_K_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_superpixel_segment: bad grid (1 <= ny <= H, 1 <= nx <= W, ny * nx <= 4096)");
    if (lambda < 1 || lambda > 65535) return gcs_fail(GCS_EINVAL, "gcs_superpixel_segment: lambda outside 1..65535");
    if (n_iter < 1) return gcs_fail(GCS_EINVAL, "gcs_superpixel_segment: n_iter must be >= 1");
    SpArgs A{};
    A.feats = feats;
    A.B = B, A.H = H, A.W = W, A.D = D, A.DQ = (D + 3) / 4, A.ny = ny, A.nx = nx, A.K = ny * nx, A.lambda = lambda;
    const size_t K = (size_t)A.K;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    A.cent = reinterpret_cast<unsigned long long *>(ws);
    ws += (size_t)B * sp_align(K * A.DQ * 8);
    A.pos = reinterpret_cast<int *>(ws);
    ws += (size_t)B * sp_align(K * 8);
    A.sums = reinterpret_cast<unsigned long long *>(ws);
    A.centres_out = centres_out;
    const dim3 per_centre(A.K, B), tiles((W + SP_TW - 1) / SP_TW, (H + SP_TH - 1) / SP_TH, B);
    const size_t smem = sp_smem_bytes(D);
    hipLaunchKernelGGL(sp_init_kernel, per_centre, dim3(256), 0, stream, A);
    GCS_CHECK_LAUNCH("gcs_superpixel_segment (init)");
    for (int t = 0; t < n_iter; ++t) {
        const int last = t == n_iter - 1;
        A.labels = last ? labels_out : nullptr;
        hipLaunchKernelGGL(sp_pass_kernel, tiles, dim3(256), smem, stream, A, last ? 0 : 1);
        GCS_CHECK_LAUNCH("gcs_superpixel_segment (pass)");
        if (!last) {
            hipLaunchKernelGGL(sp_update_kernel, per_centre, dim3(256), 0, stream, A);
            GCS_CHECK_LAUNCH("gcs_superpixel_segment (update)");
        }
    }
    if (centres_out) {
        hipLaunchKernelGGL(sp_export_kernel, per_centre, dim3(256), 0, stream, A);
        GCS_CHECK_LAUNCH("gcs_superpixel_segment (centres)");
    }
    return GCS_OK;
}
