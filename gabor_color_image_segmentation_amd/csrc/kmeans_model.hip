// kmeans_model.hip — the k-means model of SPEC.md §28: a FEATURE SLAB (either format) measured against given codebooks, every
// level at its own resolution, in exact integers: labels (the assignment of SPEC.md §4), the squared distance to the nearest and
// to the second nearest centroid, and the count and inertia of every cluster.
//
//   ke_kernel   one workgroup per 8 x 32 full-resolution pixels, cut as fg_kernel cuts them (csrc/feature_gradient.hip): aligned to
//               the 8 x 8 blocks, so the level-L pixels under it are a whole (8 >> L) x (32 >> L) rectangle. The centroids of the
//               workgroup's set go to LDS once, permuted to physical plane order ([plane][KB] uint16: the k values of a plane are
//               one broadcast read). A thread per full-resolution pixel sums the k distances over its level-0 planes and over the
//               planes of its parents on every level - d_j(p) = sum over L of partial_{L,j}(parent_L(p)) - and takes the minimum
//               and the runner-up in one sweep over j. A thread locates a (level) pixel once (slab_tap) and then steps through
//               the level's planes at a constant stride. Counts and inertias: 64-bit LDS counters per workgroup, then one atomic
//               add per counter, cluster and workgroup into the caller's table (integer sums: any order, same bits).
//               KB = k rounded up to 2, 4, 8 or 16: the distances live in registers, the padding centroids are never compared.
//               (-DGCS_KE_SHARED_LEVELS: the level >= 1 pixels of the rectangle first, ONE thread per level pixel - threads 0..63:
//               level 1, 64..79: level 2, 80..83: level 3 - sum their partial distances once each into LDS, [j][84], and the pixels
//               add their parents' words: fg_kernel's form. It does a quarter of the level-1 loads with a quarter of the lanes
//               and was the slower one in the same-box A/B run: DESIGN.md §4.26.)
// No workspace, no allocation, no host synchronisation: the table's zeroing (ke_zero_kernel) and one launch (capturable).
#include "kmeans_level.h"
#include "gcs_model.h"

namespace {

template <bool SPLIT, int KB>
__global__ __launch_bounds__(KE_THREADS) void ke_kernel(const unsigned char *__restrict__ slab, const uint16_t *__restrict__ cent,
                                                        GcsLayout lo, int k, int per_image, int32_t *__restrict__ labels,
                                                        long long *__restrict__ best_out, long long *__restrict__ second_out,
                                                        u64 *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *s_cent = reinterpret_cast<uint16_t *>(smem);                 // [D][KB], physical plane order
#ifdef GCS_KE_SHARED_LEVELS
    __shared__ u64 s_part[KB * KE_LP];                                     // [j][level pixel]
#endif
    __shared__ u64 s_stat[2 * GCS_K_MAX];                                  // counts, then inertias
    const int tid = (int)threadIdx.x, b = (int)blockIdx.z;
    const int y0 = (int)blockIdx.y * KE_TH, x0 = (int)blockIdx.x * KE_TW;
    const unsigned char *img = slab + (size_t)b * (size_t)lo.img_bytes;
    const int set = per_image ? b : 0;
    const uint16_t *cset = cent + (size_t)set * k * lo.D;
    for (int i = tid; i < lo.D * KB; i += KE_THREADS) {
        const int r = i / KB, j = i % KB;
        s_cent[i] = j < k ? cset[(size_t)j * lo.D + gcs_logical_of_plane(lo, r)] : (uint16_t)0;
    }
    if (tid < 2 * GCS_K_MAX) s_stat[tid] = 0ull;
    __syncthreads();
#ifdef GCS_KE_SHARED_LEVELS
    {
        const int L = tid < 64 ? 1 : tid < 80 ? 2 : tid < KE_LP ? 3 : GCS_LEVELS_MAX;
        if (L < lo.n_levels) {
            const int i = tid - (L == 1 ? 0 : L == 2 ? 64 : 80), wl = KE_TW >> L;
            const int yl = (y0 >> L) + i / wl, xl = (x0 >> L) + i % wl;
            u64 d[KB];
#pragma unroll
            for (int j = 0; j < KB; ++j) d[j] = 0ull;
            if (yl < lo.HL[L] && xl < lo.WL[L]) ke_level<SPLIT, KB>(lo, img, s_cent, L, yl, xl, d);
#pragma unroll
            for (int j = 0; j < KB; ++j) s_part[j * KE_LP + tid] = d[j];
        }
    }
    __syncthreads();
#endif
    const int ty = tid / KE_TW, tx = tid % KE_TW, y = y0 + ty, x = x0 + tx;
    const bool inside = y < lo.H && x < lo.W;
    if (inside) {
        u64 d[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) d[j] = 0ull;
        ke_level<SPLIT, KB>(lo, img, s_cent, 0, y, x, d);
        for (int L = 1; L < lo.n_levels; ++L) {
#ifndef GCS_KE_SHARED_LEVELS
            ke_level<SPLIT, KB>(lo, img, s_cent, L, y >> L, x >> L, d);
#else
            const int at = (L == 1 ? 0 : L == 2 ? 64 : 80) + (ty >> L) * (KE_TW >> L) + (tx >> L);
#pragma unroll
            for (int j = 0; j < KB; ++j) d[j] += s_part[j * KE_LP + at];
#endif
        }
        u64 best = d[0], second = ~0ull;
        int lab = 0;
#pragma unroll
        for (int j = 1; j < KB; ++j) {
            if (j < k) {
                if (d[j] < best) {                      // strictly: ties stay with the lowest j
                    second = best;
                    best = d[j];
                    lab = j;
                } else if (d[j] < second) {
                    second = d[j];
                }
            }
        }
        if (k == 1) second = best;
        const size_t p = ((size_t)b * lo.H + y) * lo.W + x;
        if (labels) labels[p] = lab;
        if (best_out) best_out[p] = (long long)best;
        if (second_out) second_out[p] = (long long)second;
        if (stats) {
            atomicAdd(&s_stat[lab], 1ull);
            atomicAdd(&s_stat[GCS_K_MAX + lab], best);
        }
    }
    if (!stats) return;                                 // (uniform: no thread waits at the barrier below)
    __syncthreads();
    if (tid < 2 * k) {
        const int j = tid >> 1, what = tid & 1;
        const u64 v = s_stat[what * GCS_K_MAX + j];
        if (v) atomicAdd(&stats[((size_t)set * k + j) * 2 + what], v);
    }
}

// The table's zeroing as a launch of its own: a kernel node replays in a captured graph like any other.
__global__ void ke_zero_kernel(u64 *__restrict__ stats, int n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) stats[i] = 0ull;
}

template <bool SPLIT, int KB>
void ke_launch(const unsigned char *slab, const uint16_t *cent, const GcsLayout &lo, int B, int k, int n_sets, int32_t *labels,
               int64_t *best, int64_t *second, int64_t *stats, hipStream_t stream) {
    const dim3 grid((lo.W + KE_TW - 1) / KE_TW, (lo.H + KE_TH - 1) / KE_TH, B);
    hipLaunchKernelGGL((ke_kernel<SPLIT, KB>), grid, dim3(KE_THREADS), (size_t)lo.D * KB * 2, stream, slab, cent, lo, k,
                       n_sets == B ? 1 : 0, labels, reinterpret_cast<long long *>(best), reinterpret_cast<long long *>(second),
                       reinterpret_cast<u64 *>(stats));
}

}  // namespace

extern "C" int gcs_kmeans_evaluate(const uint16_t *feats_slab, const uint16_t *centroids, int B, int H, int W, int n_scales,
                                   int n_orient, int k, int n_sets, int32_t *labels_out, int64_t *best_out, int64_t *second_out,
                                   int64_t *stats_out, gcs_stream_t stream) {
    if (!feats_slab || !centroids) return gcs_fail(GCS_EINVAL, "gcs_kmeans_evaluate: NULL pointer");
    if (!labels_out && !best_out && !second_out && !stats_out)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_evaluate: NULL pointer (at least one output must be given)");
    if (k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_evaluate: k must be in 1..16");
    if (B >= 1 && n_sets != 1 && n_sets != B) return gcs_fail(GCS_EINVAL, "gcs_kmeans_evaluate: n_sets must be 1 or B");
    GcsLayout lo;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > KE_HW_MAX || W > KE_HW_MAX || !gcs_make_layout(H, W, n_scales, n_orient, &lo) ||
        lo.D > KE_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_evaluate: bad shape or bank (1 <= B <= 65535, 1 <= H, W <= 4096, a bank of at most 1536 features)");
    const long long p_set = (long long)H * W * (n_sets == 1 ? B : 1);
    if (p_set * lo.D >= (1LL << 31))
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_evaluate: a set of P pixels needs P * D < 2^31 (its inertia could pass 2^63)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (stats_out) {
        const int n = n_sets * k * 2;
        hipLaunchKernelGGL(ke_zero_kernel, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<u64 *>(stats_out), n);
    }
    const unsigned char *slab = reinterpret_cast<const unsigned char *>(feats_slab);
#define GCS_KE_GO(KB)                                                                                                   \
    do {                                                                                                                \
        if (lo.split) ke_launch<true, KB>(slab, centroids, lo, B, k, n_sets, labels_out, best_out, second_out, stats_out, s); \
        else ke_launch<false, KB>(slab, centroids, lo, B, k, n_sets, labels_out, best_out, second_out, stats_out, s);   \
    } while (0)
    if (k <= 2) GCS_KE_GO(2);
    else if (k <= 4) GCS_KE_GO(4);
    else if (k <= 8) GCS_KE_GO(8);
    else GCS_KE_GO(16);
#undef GCS_KE_GO
    GCS_CHECK_LAUNCH("gcs_kmeans_evaluate");
    return GCS_OK;
}
