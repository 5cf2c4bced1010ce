// kmeans.hip — SPEC.md §4 on gfx950 over the pyramid feature slab (csrc/common.h): the entry points, lloyd_pass and the small kernels.
// The reference ships no code for this path; slot: /root/reference/BSD_metrics/script.py:30.
//
// Kernels
//   kmeans_pass_mfma_kernel    (csrc/lloyd_mfma.hip) one Lloyd pass (assign + update) on the matrix cores for D <= 207.
//   kmeans_pass_native_kernel  (csrc/lloyd_native.hip) the pass for deep banks (BASELINE config 4): every level at its own resolution.
//   kmeans_assign_kernel     generic pass for D >= 208: exact integer argmin via fp32 byte-digit FMAs (all partial
//                            sums < 2^24, hence exact), LDS-replicated u32 accumulators.
//   kmeans_reduce_kernel     element-major partial sums -> int64 sums (+ the centroid update when single-rank).
//   kmeans_finalize / init / features_gather / labels_widen: small helpers.
// Which pass kernel a (bank, k) takes: gcs_pass_kernel (csrc/lloyd_pass.h).
// Label maps leave every pass in RASTER order ([B][H][W] uint8 or int32): which slot of which block holds a pixel
// (csrc/common.h: main blocks and packed edge strips) is the passes' own business.
// Nothing here allocates, frees or synchronises; every entry point enqueues on the caller's stream.
#include "lloyd_pass.h"

#define LAYOUT_OR_FAIL(lo, who)                                        \
    GcsLayout lo;                                                      \
    if (B <= 0 || !gcs_make_layout(H, W, n_scales, n_orient, &lo))     \
        return gcs_fail(GCS_EINVAL, who ": bad shape or bank")

// ------------------------------------------------------------------------ init / gather
__global__ void kmeans_init_kernel(const unsigned char *__restrict__ feats, GcsLayout lo, int k,
                                   uint16_t *__restrict__ cent) {
    const int set = blockIdx.x; // image index == set index (n_sets == 1 -> image 0)
    const long P = (long)lo.H * lo.W;
    for (int i = threadIdx.x; i < k * lo.D; i += blockDim.x) {
        const int j = i / lo.D, d = i % lo.D;
        const long p = ((2L * j + 1) * P) / (2L * k);
        const int y = (int)(p / lo.W), x = (int)(p % lo.W);
        cent[((size_t)set * k + j) * lo.D + d] = (uint16_t)gcs_slab_value(feats, lo, set, gcs_plane_of_logical(lo, d), y, x);
    }
}

extern "C" int gcs_kmeans_init(const uint16_t *feats, int B, int H, int W, int n_scales, int n_orient, int k,
                               int n_sets, uint16_t *cent, gcs_stream_t stream) {
    if (!feats || !cent) return gcs_fail(GCS_EINVAL, "gcs_kmeans_init: NULL pointer");
    LAYOUT_OR_FAIL(lo, "gcs_kmeans_init");
    if (k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_init: k must be in 1..16");
    if (n_sets != 1 && n_sets != B) return gcs_fail(GCS_EINVAL, "gcs_kmeans_init: n_sets must be 1 or B");
    hipLaunchKernelGGL(kmeans_init_kernel, dim3(n_sets), dim3(256), 0, stream,
                       reinterpret_cast<const unsigned char *>(feats), lo, k, cent);
    GCS_CHECK_LAUNCH("gcs_kmeans_init");
    return GCS_OK;
}

// out[i][d] = feature d of pixel (b, y, x) = byx[i]; b < 0 gives a zero row. Lets a rank publish the
// SPEC.md §4 init centroids it owns when an image is sharded by rows (BASELINE config 5).
__global__ void features_gather_kernel(const unsigned char *__restrict__ feats, GcsLayout lo, int n,
                                       const int32_t *__restrict__ byx, uint16_t *__restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * lo.D; i += gridDim.x * blockDim.x) {
        const int r = i / lo.D, d = i % lo.D;
        const int b = byx[3 * r], y = byx[3 * r + 1], x = byx[3 * r + 2];
        out[i] = b < 0 ? (uint16_t)0 : (uint16_t)gcs_slab_value(feats, lo, b, gcs_plane_of_logical(lo, d), y, x);
    }
}

extern "C" int gcs_features_gather(const uint16_t *feats, int B, int H, int W, int n_scales, int n_orient, int n,
                                   const int32_t *byx, uint16_t *out, gcs_stream_t stream) {
    if (!feats || !byx || !out) return gcs_fail(GCS_EINVAL, "gcs_features_gather: NULL pointer");
    LAYOUT_OR_FAIL(lo, "gcs_features_gather");
    if (n <= 0) return gcs_fail(GCS_EINVAL, "gcs_features_gather: n must be > 0");
    hipLaunchKernelGGL(features_gather_kernel, dim3((n * lo.D + 255) / 256), dim3(256), 0, stream,
                       reinterpret_cast<const unsigned char *>(feats), lo, n, byx, out);
    GCS_CHECK_LAUNCH("gcs_features_gather");
    return GCS_OK;
}

// ---------------------------------------------------------------------------------------
// Generic pass (D >= 208). Exact integer argmin with fp32 digit arithmetic: x = 256*xh + xl, c = 256*ch + cl (bytes);
//   sum_d x*c = 65536*sum xh*ch + 256*sum (xh*cl + xl*ch) + sum xl*cl,
// every partial sum stays below 2^24 over a chunk of <= 128 planes, so fp32 FMA is exact.
// score_j = |c_j|^2 - 2 sum_d x_d c_jd (the |x|^2 term is common to all j). Planes are walked in PHYSICAL order
// (level-major); the centroid digits are permuted to match when they are loaded.
constexpr int KM_CHUNK = 128;

// two horizontally adjacent pixels (x even) of physical plane r: one aligned dword on level 0, the same parent twice above
// (wide slab: feature vectors of 208 or more planes never take the split one)
__device__ __forceinline__ unsigned feature_pair(const unsigned char *feats, const GcsLayout &lo, int b, int r, int y, int x) {
    const unsigned char *p = feats + gcs_slab_offset(lo, b, r, y, x);
    if (r < lo.DL[0]) return *reinterpret_cast<const unsigned *>(p) ^ 0x80808080u;
    const unsigned v = *reinterpret_cast<const uint16_t *>(p) ^ 0x8080u;
    return v | (v << 16);
}

template <int K>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(
    const unsigned char *__restrict__ feats, const uint16_t *__restrict__ cent, GcsLayout lo, int per_image, int parts,
    int R, int row_lo, int row_hi, uint8_t *__restrict__ labels, uint64_t *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // carve: cdig float [D][K][2] | cnorm int64 [K] | acc u32 [K][D+1][R]
    const int D = lo.D, H = lo.H, W = lo.W;
    float *cdig = reinterpret_cast<float *>(smem);
    long long *cnorm = reinterpret_cast<long long *>(smem + (((size_t)D * K * 2 * 4 + 15) & ~(size_t)15));
    unsigned *acc = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned char *>(cnorm) + ((K * 8 + 15) & ~15));

    const int tid = threadIdx.x;
    const int b = blockIdx.y, part = blockIdx.x;
    const uint16_t *cset = cent + (size_t)(per_image ? b : 0) * K * D;
    const int D1 = D + 1;

    for (int i = tid; i < K * D; i += 256) {
        const int j = i / D, r = i % D;                      // r = physical plane
        const unsigned cv = cset[j * D + gcs_logical_of_plane(lo, r)];
        cdig[(r * K + j) * 2 + 0] = (float)(cv & 255u);
        cdig[(r * K + j) * 2 + 1] = (float)(cv >> 8);
    }
    if (tid < K) {
        long long s = 0;
        for (int d = 0; d < D; ++d) {
            const long long cv = cset[tid * D + d];
            s += cv * cv;
        }
        cnorm[tid] = s;
    }
    for (int i = tid; i < K * D1 * R; i += 256) acc[i] = 0u;
    __syncthreads();

    const int ppr = (W + 1) >> 1; // pixel pairs per row
    const long npairs = (long)H * ppr;
    const int rep = tid & (R - 1);

    for (long q = (long)part * 256 + tid; q < npairs; q += (long)parts * 256) {
        const int y = (int)(q / ppr), x = 2 * (int)(q % ppr);
        long long S[2][K];
#pragma unroll
        for (int j = 0; j < K; ++j) S[0][j] = S[1][j] = 0;
        for (int d0 = 0; d0 < D; d0 += KM_CHUNK) {
            const int d1 = min(D, d0 + KM_CHUNK);
            float a0[2][K], a1[2][K], a2[2][K];
#pragma unroll
            for (int j = 0; j < K; ++j) a0[0][j] = a0[1][j] = a1[0][j] = a1[1][j] = a2[0][j] = a2[1][j] = 0.f;
            for (int d = d0; d < d1; ++d) {
                const unsigned u = feature_pair(feats, lo, b, d, y, x);
                const float xl0 = (float)(u & 255u), xh0 = (float)((u >> 8) & 255u);
                const float xl1 = (float)((u >> 16) & 255u), xh1 = (float)(u >> 24);
                const float *cd = cdig + d * K * 2;
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float cl = cd[2 * j], ch = cd[2 * j + 1];
                    a0[0][j] = fmaf(xl0, cl, a0[0][j]);
                    a1[0][j] = fmaf(xh0, cl, fmaf(xl0, ch, a1[0][j]));
                    a2[0][j] = fmaf(xh0, ch, a2[0][j]);
                    a0[1][j] = fmaf(xl1, cl, a0[1][j]);
                    a1[1][j] = fmaf(xh1, cl, fmaf(xl1, ch, a1[1][j]));
                    a2[1][j] = fmaf(xh1, ch, a2[1][j]);
                }
            }
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < K; ++j)
                    S[p][j] += ((long long)(unsigned)a2[p][j] << 16) + ((long long)(unsigned)a1[p][j] << 8) +
                               (long long)(unsigned)a0[p][j];
        }
        int lab[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            long long best = cnorm[0] - 2 * S[p][0];
            int bj = 0;
#pragma unroll
            for (int j = 1; j < K; ++j) {
                const long long sc = cnorm[j] - 2 * S[p][j];
                if (sc < best) {
                    best = sc;
                    bj = j;
                }
            }
            lab[p] = bj;
        }
        if (labels) {   // uint8 raster map [B][H][W]
            uint8_t *lp = labels + ((size_t)b * H + y) * W + x;
            lp[0] = (uint8_t)lab[0];
            if (x + 1 < W) lp[1] = (uint8_t)lab[1];
        }
        // accumulate (second pass over this thread's planes; L2-resident)
        const bool rows_ok = partials && y >= row_lo && y < row_hi;
        const bool v0 = rows_ok && x < W, v1 = rows_ok && x + 1 < W;
        if (v0) {
            unsigned *a_0 = acc + (size_t)lab[0] * D1 * R + rep;
            unsigned *a_1 = acc + (size_t)lab[1] * D1 * R + rep;
            if (v1 && lab[0] == lab[1]) {
                for (int d = 0; d < D; ++d) {
                    const unsigned u = feature_pair(feats, lo, b, d, y, x);
                    atomicAdd(a_0 + d * R, (u & 0xffffu) + (u >> 16));
                }
                atomicAdd(a_0 + D * R, 2u);
            } else {
                for (int d = 0; d < D; ++d) {
                    const unsigned u = feature_pair(feats, lo, b, d, y, x);
                    atomicAdd(a_0 + d * R, u & 0xffffu);
                    if (v1) atomicAdd(a_1 + d * R, u >> 16);
                }
                atomicAdd(a_0 + D * R, 1u);
                if (v1) atomicAdd(a_1 + D * R, 1u);
            }
        }
    }
    __syncthreads();
    if (!partials) return;
    for (int i = tid; i < K * D1; i += 256) {
        const int j = i / D1, e = i % D1;                   // e = logical feature (or D = count)
        const int pe = e < D ? gcs_plane_of_logical(lo, e) : D;
        uint64_t s = 0;
        for (int rr = 0; rr < R; ++rr) s += acc[((size_t)j * D1 + pe) * R + rr];
        partials[partial_index(per_image, b, part, parts, (int)gridDim.y, i, K * D1)] = s;
    }
}

static size_t assign_lds_bytes(int D, int k, int R) {
    size_t a = ((size_t)D * k * 2 * 4 + 15) & ~(size_t)15;
    size_t c = ((size_t)k * 8 + 15) & ~(size_t)15;
    return a + c + (size_t)k * (D + 1) * R * 4;
}

// accumulator replicas per (cluster, element) in LDS: as many (a power of two, at most 32) as 120 KB hold
static int assign_replicas(int D, int k) {
    int R = 32;
    while (R > 1 && assign_lds_bytes(D, k, R) > 120 * 1024) R >>= 1;
    return R;
}
constexpr size_t ASSIGN_LDS_MAX = 160 * 1024;

template <int K>
static int launch_assign(const uint16_t *feats, const uint16_t *cent, int B, const GcsLayout &lo, int n_sets,
                         int row_lo, int row_hi, uint8_t *labels, uint64_t *partials, hipStream_t stream) {
    const int D = lo.D;
    const int parts = (int)gcs_kmeans_parts_per_image(B, lo.H, lo.W);
    const int R = assign_replicas(D, K);
    const size_t lds = assign_lds_bytes(D, K, R);
    if (lds > ASSIGN_LDS_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: k*D too large for LDS");
    // raise the dynamic-LDS cap: per device and cheap, so set on every launch (no process-wide cache to race on)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kmeans_assign_kernel<K>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return gcs_hip_fail(e, "hipFuncSetAttribute(assign)");
    hipLaunchKernelGGL(kmeans_assign_kernel<K>, dim3(parts, B), dim3(256), lds, stream,
                       reinterpret_cast<const unsigned char *>(feats), cent, lo, n_sets == B ? 1 : 0, parts, R, row_lo,
                       row_hi, labels, partials);
    GCS_CHECK_LAUNCH("gcs_kmeans_assign_accumulate");
    return GCS_OK;
}

extern "C" int gcs_labels_widen(const uint8_t *labels, int B, int H, int W, int32_t *out, gcs_stream_t stream);

// One Lloyd pass, whatever it emits: uint8 label map, partial sums, raster label map (any subset, not none).
static int lloyd_pass(const uint16_t *feats, const uint16_t *cent, int B, int H, int W, int n_scales, int n_orient, int k,
                      int n_sets, int row_lo, int row_hi, int reverse, uint8_t *labels, uint64_t *partials, void *raster,
                      int raster_u8, gcs_stream_t stream) {
    if (!feats || !cent || (!labels && !partials && !raster))
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: NULL pointer (labels and partials may not both be NULL)");
    LAYOUT_OR_FAIL(lo, "gcs_kmeans_assign_accumulate");
    if (row_lo < 0 || row_hi > H || row_lo >= row_hi)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: need 0 <= row_lo < row_hi <= H");
    if (B > 65535) return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: B too large for one launch");
    if (!kp_batch_fits(lo, B)) return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: batch too large for one launch");
    if (k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: k must be in 1..16");
    if (n_sets != 1 && n_sets != B)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: n_sets must be 1 or B");
    const GcsPassKernel pk = gcs_pass_kernel(lo, k);
    if (pk != GCS_PASS_GENERIC) {
        if (!kp_image_fits(lo))
            return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: image too large for the split slab's pass");
        // the matrix-core passes have ONE label output, in raster order: the caller's raster map, or its uint8 label map
        // (assign_accumulate with labels: every pixel of the image is labelled, halo rows of a row window included)
        const LloydPassArgs a = {reinterpret_cast<const unsigned char *>(feats), cent, lo, B, k, n_sets,
                                 (int)gcs_kmeans_parts_per_image(B, H, W), reverse, row_lo, row_hi, partials,
                                 raster ? raster : static_cast<void *>(labels), raster ? raster_u8 : 1, stream};
        if (gcs_pass_is_native(pk)) lloyd_native_launch(pk, a);
        else lloyd_mfma_launch(pk, a, nullptr);
        GCS_CHECK_LAUNCH("gcs_kmeans_assign_accumulate");
        return GCS_OK;
    }
    // generic pass: uint8 raster labels only. A uint8 raster map is written directly, an int32 one through the scratch map.
    if (raster && raster_u8) labels = static_cast<uint8_t *>(raster);
    else if (raster && !labels)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_raster: feature vectors of 208 or more planes need the scratch label map for int32 output");
    int rc = GCS_EINVAL;
    switch (k) { // generic VALU pass for wider feature vectors
#define GCS_CASE(KK) \
    case KK:         \
        rc = launch_assign<KK>(feats, cent, B, lo, n_sets, row_lo, row_hi, labels, partials, stream); \
        break;
        GCS_CASE(1) GCS_CASE(2) GCS_CASE(3) GCS_CASE(4) GCS_CASE(5) GCS_CASE(6) GCS_CASE(7) GCS_CASE(8)
        GCS_CASE(9) GCS_CASE(10) GCS_CASE(11) GCS_CASE(12) GCS_CASE(13) GCS_CASE(14) GCS_CASE(15) GCS_CASE(16)
#undef GCS_CASE
    }
    if (rc != GCS_OK || !raster || raster_u8) return rc;
    return gcs_labels_widen(labels, B, H, W, static_cast<int32_t *>(raster), stream);   // uint8 -> int32: one more launch
}

extern "C" int gcs_kmeans_assign_accumulate(const uint16_t *feats, const uint16_t *cent, int B, int H, int W,
                                            int n_scales, int n_orient, int k, int n_sets, int row_lo, int row_hi,
                                            int reverse, uint8_t *labels, uint64_t *partials, gcs_stream_t stream) {
    if (!labels && !partials)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_accumulate: NULL pointer (labels and partials may not both be NULL)");
    return lloyd_pass(feats, cent, B, H, W, n_scales, n_orient, k, n_sets, row_lo, row_hi, reverse, labels, partials, nullptr, 0,
                      stream);
}

extern "C" int gcs_kmeans_assign_raster(const uint16_t *feats, const uint16_t *cent, int B, int H, int W, int n_scales,
                                        int n_orient, int k, int n_sets, int reverse, void *out, int out_u8,
                                        uint8_t *scratch_labels, gcs_stream_t stream) {
    if (!out) return gcs_fail(GCS_EINVAL, "gcs_kmeans_assign_raster: NULL pointer");
    return lloyd_pass(feats, cent, B, H, W, n_scales, n_orient, k, n_sets, 0, H, reverse, scratch_labels, nullptr, out,
                      out_u8 ? 1 : 0, stream);
}

// Test hook (host only): the display name of the pass kernel lloyd_pass takes for this bank and k - split<KT,NR[,L0T]>,
// narrow<KT,NST>, wide<KT,NST>, wide8w<1,5>, native<NL,MINB,N0>, generic -, NULL where it refuses the shape, the bank or k.
extern "C" const char *gcs_selftest_pass_kernel(int H, int W, int n_scales, int n_orient, int k) {
    GcsLayout lo;
    if (!gcs_make_layout(H, W, n_scales, n_orient, &lo) || k < 1 || k > GCS_K_MAX) return nullptr;
    const GcsPassKernel pk = gcs_pass_kernel(lo, k);
    if (pk == GCS_PASS_GENERIC ? assign_lds_bytes(lo.D, k, assign_replicas(lo.D, k)) > ASSIGN_LDS_MAX : !kp_image_fits(lo)) return nullptr;
    return gcs_pass_name(pk);
}

// Test hook (host only): the `nt` limit the launch of one pass over this batch would use (csrc/lloyd_pass.h: gcs_pass_nt_limit) -
// list positions below it are loaded with the nontemporal hint -, 0 for a kernel that loads plain, -1 where lloyd_pass refuses the call.
extern "C" int gcs_selftest_pass_nt_limit(int B, int H, int W, int n_scales, int n_orient, int k, int n_sets) {
    GcsLayout lo;
    if (B <= 0 || B > 65535 || !gcs_make_layout(H, W, n_scales, n_orient, &lo) || !kp_batch_fits(lo, B) || k < 1 || k > GCS_K_MAX ||
        (n_sets != 1 && n_sets != B) || !gcs_selftest_pass_kernel(H, W, n_scales, n_orient, k))
        return -1;
    return gcs_pass_nt_limit(gcs_pass_kernel(lo, k), lo, B, n_sets);
}

// ------------------------------------------------------------------- self-updating passes (single rank, whole images)
// The Lloyd loop as n_iter launches: no init kernel, no reduce launches (GcsFold in csrc/common.h, FUSED in kmeans_pass_mfma_kernel).
// Which banks: gcs_pass_self_updating (csrc/lloyd_pass.h). Everything else keeps the init / pass / reduce launches.
//
// Shared rows per set: a workgroup adds into row (its index) % rows. ONE row is the measured optimum (profiles/r7_notes.md: 768
// workgroups behind every address cost the fold nothing that shows, while every further row is one more dependent read in every
// workgroup's prologue: the 10-pass loop takes 1.25 ms with 1 row, 1.28 with 8, 1.42 with 32, 1.61 with 64 - against 1.32 ms for
// init / pass / reduce). GCS_KP_FOLD_ROWS in the environment (1 .. 64, read once; one global codebook only) repeats that sweep.
#ifndef KP_FOLD_ROWS
#define KP_FOLD_ROWS 1
#endif
static int fold_rows(int B, int parts, int n_sets) {
    if (n_sets == B && B > 1) return 1;
    static const int env = [] {
        const char *e = getenv("GCS_KP_FOLD_ROWS");
        const int v = e ? atoi(e) : 0;
        return v >= 1 && v <= 64 ? v : KP_FOLD_ROWS;
    }();
    const long long wgs = (long long)B * parts;
    return (int)(wgs < env ? wgs : env);
}
// workspace: [3 sum buffers][2 centroid arrays][ticket], every piece a multiple of 256 bytes
static size_t fused_sum_bytes(const GcsLayout &lo, int k, int n_sets, int rows) {
    return ((size_t)n_sets * rows * k * (lo.D + 1) * 8 + 255) & ~(size_t)255;
}
static size_t fused_cent_bytes(const GcsLayout &lo, int k, int n_sets) {
    return ((size_t)n_sets * k * lo.D * 2 + 255) & ~(size_t)255;
}
extern "C" size_t gcs_kmeans_fused_workspace_bytes(int B, int H, int W, int n_scales, int n_orient, int k, int n_sets) {
    GcsLayout lo;
    if (B <= 0 || B > 65535 || !gcs_make_layout(H, W, n_scales, n_orient, &lo) || (n_sets != 1 && n_sets != B) || k < 1 ||
        k > GCS_K_MAX || !gcs_pass_self_updating(gcs_pass_kernel(lo, k)))
        return 0;
    const int rows = fold_rows(B, (int)gcs_kmeans_parts_per_image(B, H, W), n_sets);
    return 3 * fused_sum_bytes(lo, k, n_sets, rows) + 2 * fused_cent_bytes(lo, k, n_sets) + 256;
}

extern "C" int gcs_kmeans_pass_fused(const uint16_t *feats, int B, int H, int W, int n_scales, int n_orient, int k, int n_sets,
                                     int reverse, int pass, int last, void *workspace, uint16_t *cent, void *out, int out_u8,
                                     gcs_stream_t stream) {
    if (!feats || !workspace || !cent || (last && !out))
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_pass_fused: NULL pointer (the last pass needs its label map)");
    LAYOUT_OR_FAIL(lo, "gcs_kmeans_pass_fused");
    if (pass < 0) return gcs_fail(GCS_EINVAL, "gcs_kmeans_pass_fused: pass must be >= 0");
    if (gcs_kmeans_fused_workspace_bytes(B, H, W, n_scales, n_orient, k, n_sets) == 0)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_pass_fused: no self-updating pass for this bank / k / n_sets (gcs_kmeans_fused_workspace_bytes == 0)");
    if (!kp_batch_fits(lo, B) || !kp_image_fits(lo))
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_pass_fused: batch or image too large for one launch");
    const int parts = (int)gcs_kmeans_parts_per_image(B, H, W);
    const int rows = fold_rows(B, parts, n_sets);
    const size_t sb = fused_sum_bytes(lo, k, n_sets, rows), cb = fused_cent_bytes(lo, k, n_sets);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    auto sums = [&](int t) { return reinterpret_cast<unsigned long long *>(ws + (size_t)(t % 3) * sb); };
    auto cents = [&](int t) { return reinterpret_cast<uint16_t *>(ws + 3 * sb + (size_t)(t & 1) * cb); };
    GcsFold fz;
    fz.prev = pass > 0 ? sums(pass - 1) : nullptr;
    fz.clear = sums(pass + 1);
    fz.cent_new = cents(pass);
    fz.cent_out = cent;
    fz.ticket = reinterpret_cast<unsigned *>(ws + 3 * sb + 2 * cb);
    fz.rows = rows;
    uint64_t *acc = last ? nullptr : reinterpret_cast<uint64_t *>(sums(pass));
    const LloydPassArgs a = {reinterpret_cast<const unsigned char *>(feats), cents(pass + 1), lo, B, k, n_sets, parts, reverse, 0, H,
                             acc, last ? out : nullptr, out_u8 ? 1 : 0, stream};
    lloyd_mfma_launch(gcs_pass_kernel(lo, k), a, &fz);
    GCS_CHECK_LAUNCH("gcs_kmeans_pass_fused");
    return GCS_OK;
}

// sums[set][e] = sum over the set's rows of element e (layout: partial_index in common.h). Integer sums: any order gives
// the same bits. One 1024-thread workgroup per chunk of 16 elements: thread (row group rg = t >> 4, element t & 15) adds
// rows rg, rg + 64, ...; a wave reads four whole rows = 512 contiguous bytes per load.
// FIN: the SPEC.md §4 update is applied in the same launch (single-rank case, no all-reduce in between): every thread
// also folds the count element of its element's cluster, so no second kernel and no cross-block dependency is needed.
// RG = row groups per workgroup (threads = 16 * RG): 64 for the long row lists of one global codebook, 16 for the `parts`
// rows of a per-image codebook.
template <bool FIN, int RG>
__global__ __launch_bounds__(16 * RG) void kmeans_reduce_kernel(const uint64_t *__restrict__ partials,
                                                             int rows_per_set, int row_len, int D1,
                                                             long long *__restrict__ sums,
                                                             uint16_t *__restrict__ cent) {
    __shared__ unsigned long long sm_s[RG][KP_PCH], sm_c[RG][KP_PCH];
    const int set = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const int e16 = t & (KP_PCH - 1), rg = t >> 4;
    const int nch = partial_chunks(row_len);
    const int e = chunk * KP_PCH + e16;
    const int ee = e < row_len ? e : row_len - 1;              // padding columns of the last chunk: read a valid one
    const int j = ee / D1, d = ee - j * D1;
    const int ec = j * D1 + (D1 - 1);                          // the count element of this element's cluster
    const uint64_t *p = partials + (((size_t)set * nch + chunk) * rows_per_set) * KP_PCH + (ee - chunk * KP_PCH);
    const uint64_t *pc = partials + (((size_t)set * nch + ec / KP_PCH) * rows_per_set) * KP_PCH + ec % KP_PCH;
    uint64_t s = 0, c = 0;
    int r = rg;
    // the loop is latency-bound: 12 (then 4) rows in flight per thread
    auto burst = [&](auto n_c) {
        constexpr int N = decltype(n_c)::value;
        for (; r + RG * (N - 1) < rows_per_set; r += RG * N) {
            uint64_t a[N], q[N];
#pragma unroll
            for (int u = 0; u < N; ++u) {
                a[u] = p[(size_t)(r + RG * u) * KP_PCH];
                q[u] = FIN ? pc[(size_t)(r + RG * u) * KP_PCH] : 0;
            }
#pragma unroll
            for (int u = 0; u < N; ++u) {
                s += a[u];
                c += q[u];
            }
        }
    };
    burst(std::integral_constant<int, 12>{});
    burst(std::integral_constant<int, 4>{});
    burst(std::integral_constant<int, 1>{});
    sm_s[rg][e16] = s;
    if (FIN) sm_c[rg][e16] = c;
    __syncthreads();
    if (RG == 64) {                                            // 64 -> 16 row groups
        if (t < 256) {
            s = sm_s[4 * rg][e16] + sm_s[4 * rg + 1][e16] + sm_s[4 * rg + 2][e16] + sm_s[4 * rg + 3][e16];
            if (FIN) c = sm_c[4 * rg][e16] + sm_c[4 * rg + 1][e16] + sm_c[4 * rg + 2][e16] + sm_c[4 * rg + 3][e16];
        }
        __syncthreads();
        if (t < 256) {
            sm_s[rg][e16] = s;
            if (FIN) sm_c[rg][e16] = c;
        }
        __syncthreads();
    }
    if (t < KP_PCH && e < row_len) {
        s = 0;
        c = 0;
        for (int q = 0; q < 16; ++q) {
            s += sm_s[q][e16];
            if (FIN) c += sm_c[q][e16];
        }
        if (sums) sums[(size_t)set * row_len + e] = (long long)s;
        if (FIN && d < D1 - 1 && c > 0)
            cent[((size_t)set * (row_len / D1) + j) * (D1 - 1) + d] = (uint16_t)((2 * s + c) / (2 * c));
    }
}

static int reduce_args_ok(const void *partials, int B, int H, int W, int D, int k, int n_sets, const char *who) {
    if (!partials) return gcs_fail(GCS_EINVAL, "gcs_kmeans_reduce: NULL pointer");
    if (B <= 0 || H <= 0 || W <= 0 || D <= 0 || k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, who);
    if (n_sets != 1 && n_sets != B) return gcs_fail(GCS_EINVAL, "gcs_kmeans_reduce: n_sets must be 1 or B");
    return GCS_OK;
}

extern "C" int gcs_kmeans_reduce(const uint64_t *partials, int B, int H, int W, int D, int k, int n_sets,
                                 int64_t *sums, gcs_stream_t stream) {
    if (!sums) return gcs_fail(GCS_EINVAL, "gcs_kmeans_reduce: NULL pointer");
    if (int rc = reduce_args_ok(partials, B, H, W, D, k, n_sets, "gcs_kmeans_reduce: bad shape")) return rc;
    const int parts = (int)gcs_kmeans_parts_per_image(B, H, W);
    const int row_len = k * (D + 1);
    const int rows_per_set = n_sets == B ? parts : B * parts;
    if (rows_per_set > 64)
        hipLaunchKernelGGL((kmeans_reduce_kernel<false, 64>), dim3(partial_chunks(row_len), n_sets), dim3(1024), 0, stream,
                           partials, rows_per_set, row_len, D + 1, reinterpret_cast<long long *>(sums), (uint16_t *)nullptr);
    else
        hipLaunchKernelGGL((kmeans_reduce_kernel<false, 16>), dim3(partial_chunks(row_len), n_sets), dim3(256), 0, stream,
                           partials, rows_per_set, row_len, D + 1, reinterpret_cast<long long *>(sums), (uint16_t *)nullptr);
    GCS_CHECK_LAUNCH("gcs_kmeans_reduce");
    return GCS_OK;
}

extern "C" int gcs_kmeans_reduce_finalize(const uint64_t *partials, int B, int H, int W, int D, int k, int n_sets,
                                          int64_t *sums, uint16_t *cent, gcs_stream_t stream) {
    if (!cent) return gcs_fail(GCS_EINVAL, "gcs_kmeans_reduce_finalize: NULL pointer");
    if (int rc = reduce_args_ok(partials, B, H, W, D, k, n_sets, "gcs_kmeans_reduce_finalize: bad shape")) return rc;
    const int parts = (int)gcs_kmeans_parts_per_image(B, H, W);
    const int row_len = k * (D + 1);
    const int rows_per_set = n_sets == B ? parts : B * parts;
    if (rows_per_set > 64)
        hipLaunchKernelGGL((kmeans_reduce_kernel<true, 64>), dim3(partial_chunks(row_len), n_sets), dim3(1024), 0, stream,
                           partials, rows_per_set, row_len, D + 1, reinterpret_cast<long long *>(sums), cent);
    else
        hipLaunchKernelGGL((kmeans_reduce_kernel<true, 16>), dim3(partial_chunks(row_len), n_sets), dim3(256), 0, stream,
                           partials, rows_per_set, row_len, D + 1, reinterpret_cast<long long *>(sums), cent);
    GCS_CHECK_LAUNCH("gcs_kmeans_reduce_finalize");
    return GCS_OK;
}

__global__ void kmeans_finalize_kernel(const long long *__restrict__ sums, int n, int k, int D,
                                       uint16_t *__restrict__ cent) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int d = i % D, j = (i / D) % k, set = i / (D * k);
    const long long *row = sums + ((size_t)set * k + j) * (D + 1);
    const long long cnt = row[D];
    if (cnt > 0) cent[i] = (uint16_t)((2 * row[d] + cnt) / (2 * cnt));
}

extern "C" int gcs_kmeans_finalize(const int64_t *sums, int n_sets, int k, int D, uint16_t *cent,
                                   gcs_stream_t stream) {
    if (!sums || !cent) return gcs_fail(GCS_EINVAL, "gcs_kmeans_finalize: NULL pointer");
    if (n_sets <= 0 || D <= 0 || k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_finalize: bad shape");
    const int n = n_sets * k * D;
    hipLaunchKernelGGL(kmeans_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, stream,
                       reinterpret_cast<const long long *>(sums), n, k, D, cent);
    GCS_CHECK_LAUNCH("gcs_kmeans_finalize");
    return GCS_OK;
}

// ----------------------------------------------------------------------------- uint8 label map -> int32
__global__ __launch_bounds__(256) void labels_widen_kernel(const uint8_t *__restrict__ labels, size_t n, int32_t *__restrict__ out) {
    // four labels per thread where the dword is whole (the map starts on an allocation boundary: aligned)
    const size_t i4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 + 3 < n) {
        const unsigned v = *reinterpret_cast<const unsigned *>(labels + i4);
        typedef int __attribute__((ext_vector_type(4), aligned(4))) v4i_a4;
        *reinterpret_cast<v4i_a4 *>(out + i4) = v4i_a4{(int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u), (int)(v >> 24)};
    } else {
        for (size_t i = i4; i < n; ++i) out[i] = labels[i];
    }
}

extern "C" int gcs_labels_widen(const uint8_t *labels, int B, int H, int W, int32_t *out, gcs_stream_t stream) {
    if (!labels || !out || B <= 0 || H <= 0 || W <= 0) return gcs_fail(GCS_EINVAL, "gcs_labels_widen: bad argument");
    if ((reinterpret_cast<uintptr_t>(labels) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return gcs_fail(GCS_EINVAL, "gcs_labels_widen: pointers must be 4-byte aligned");
    const size_t n = (size_t)B * H * W;
    const size_t blocks = (n / 4 + 1 + 255) / 256;
    if (blocks > 0x7fffffffull) return gcs_fail(GCS_EINVAL, "gcs_labels_widen: map too large for one launch");
    hipLaunchKernelGGL(labels_widen_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, labels, n, out);
    GCS_CHECK_LAUNCH("gcs_labels_widen");
    return GCS_OK;
}
