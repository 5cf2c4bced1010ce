// label_relax.hip — SPEC.md §30: the cost volume of a feature slab under given codebooks, and a Potts prior on a label map
// minimised by iterated conditional modes (ICM), in exact integers.
//
//   kc_kernel     gcs_kmeans_costs: ke_kernel's workgroup (csrc/kmeans_model.hip: 8 x 32 pixels, centroids in LDS in physical plane
//                 order, a thread per pixel walking its own and its parents' planes through ke_level of kmeans_level.h) with the k
//                 distances stored instead of reduced: per j a row of 32 threads writes 256 contiguous bytes.
//   lr_pass_kernel  one launch per SUB-PASS (class c = 2 (y & 1) + (x & 1)) on the output map in place: a thread per pixel of the
//                 class reads its k costs (KB = k rounded up to 2, 4, 8, 16, all loads issued before the first use), its 4 or 8
//                 neighbours' labels and its own, and writes its label only when it changes. No two pixels of a class are
//                 neighbours, so a sub-pass reads only labels it does not write: in place is exact, and the launch boundary is
//                 the ordering between the classes. A sweep is four launches and pulls every second 16 bytes of every second row
//                 of a cost plane per launch, so each cache line of the volume about twice (DESIGN.md §4.28 weighs this against
//                 a tile-with-halo form, one launch per sweep, which was not built). `workspace` is therefore not used here.
//   lr_energy_kernel  unary and pairs of the delivered map: a thread per pixel counts the pairs it forms with its right, lower
//                 and (8 neighbours) two lower diagonal neighbours; wave shuffle, LDS, one atomic add per workgroup and counter.
//   lr_copy_kernel, lr_zero_kernel  the start map into the output, and the counters' zeroing as a launch of its own (replays in
//                 a captured graph like any other kernel node).
// No allocation, no host synchronisation (capturable).
#include "kmeans_level.h"
#include "gcs_model.h"
#include "gcs_relax.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- costs
template <bool SPLIT, int KB>
__global__ __launch_bounds__(KE_THREADS) void kc_kernel(const unsigned char *__restrict__ slab, const uint16_t *__restrict__ cent,
                                                        GcsLayout lo, int k, int per_image, long long *__restrict__ costs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *s_cent = reinterpret_cast<uint16_t *>(smem);                 // [D][KB], physical plane order
    const int tid = (int)threadIdx.x, b = (int)blockIdx.z;
    const int y0 = (int)blockIdx.y * KE_TH, x0 = (int)blockIdx.x * KE_TW;
    const unsigned char *img = slab + (size_t)b * (size_t)lo.img_bytes;
    const uint16_t *cset = cent + (size_t)(per_image ? b : 0) * k * lo.D;
    for (int i = tid; i < lo.D * KB; i += KE_THREADS) {
        const int r = i / KB, j = i % KB;
        s_cent[i] = j < k ? cset[(size_t)j * lo.D + gcs_logical_of_plane(lo, r)] : (uint16_t)0;
    }
    __syncthreads();
    const int y = y0 + tid / KE_TW, x = x0 + tid % KE_TW;
    if (y >= lo.H || x >= lo.W) return;
    u64 d[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) d[j] = 0ull;
    ke_level<SPLIT, KB>(lo, img, s_cent, 0, y, x, d);
    for (int L = 1; L < lo.n_levels; ++L) ke_level<SPLIT, KB>(lo, img, s_cent, L, y >> L, x >> L, d);
    const size_t plane = (size_t)lo.H * lo.W;
    long long *o = costs + (size_t)b * k * plane + (size_t)y * lo.W + x;
#pragma unroll
    for (int j = 0; j < KB; ++j)
        if (j < k) o[(size_t)j * plane] = (long long)d[j];
}

template <bool SPLIT, int KB>
void kc_launch(const unsigned char *slab, const uint16_t *cent, const GcsLayout &lo, int B, int k, int n_sets, int64_t *costs,
               hipStream_t stream) {
    const dim3 grid((lo.W + KE_TW - 1) / KE_TW, (lo.H + KE_TH - 1) / KE_TH, B);
    hipLaunchKernelGGL((kc_kernel<SPLIT, KB>), grid, dim3(KE_THREADS), (size_t)lo.D * KB * 2, stream, slab, cent, lo, k,
                       n_sets == B ? 1 : 0, reinterpret_cast<long long *>(costs));
}

// ---------------------------------------------------------------------------------------------------------------- relax
constexpr int LR_TW = 64, LR_TH = 4, LR_THREADS = LR_TW * LR_TH;           // a wave per row of the workgroup
constexpr long long LR_BETA_MAX = (1LL << 58) - 1;
constexpr int LR_NONE = -1, LR_ABSENT = -2;                                // "no label"; a neighbour outside the image

__device__ __forceinline__ int lr_norm(int l, int k) { return (unsigned)l < (unsigned)k ? l : LR_NONE; }

__device__ __forceinline__ u64 lr_beta(const long long *beta, int b) {
    const long long v = beta[b];
    return (u64)(v < 0 ? 0 : v > LR_BETA_MAX ? LR_BETA_MAX : v);
}

// One sub-pass: the pixels (cy + 2 i, cx + 2 j) of every image, in place on `labels`.
template <int KB>
__global__ __launch_bounds__(LR_THREADS) void lr_pass_kernel(const long long *__restrict__ costs, const long long *__restrict__ beta,
                                                             int H, int W, int k, int eight, int cy, int cx, int32_t *labels,
                                                             int32_t *__restrict__ changed, int changed_stride) {
    const int b = (int)blockIdx.z;
    const int x = cx + 2 * ((int)blockIdx.x * LR_TW + (int)threadIdx.x), y = cy + 2 * ((int)blockIdx.y * LR_TH + (int)threadIdx.y);
    int moved = 0;
    if (y < H && x < W) {
        const size_t plane = (size_t)H * W;
        const long long *c = costs + (size_t)b * k * plane + (size_t)y * W + x;
        u64 e[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) e[j] = j < k ? (u64)c[(size_t)j * plane] : 0ull;
        int32_t *lab = labels + (size_t)b * plane + (size_t)y * W + x;
        const bool up = y > 0, down = y + 1 < H, left = x > 0, right = x + 1 < W;
        int q[8];                                                          // normalised on the way in: a raw label may be any int
        q[0] = up ? lr_norm(lab[-W], k) : LR_ABSENT;
        q[1] = down ? lr_norm(lab[W], k) : LR_ABSENT;
        q[2] = left ? lr_norm(lab[-1], k) : LR_ABSENT;
        q[3] = right ? lr_norm(lab[1], k) : LR_ABSENT;
        q[4] = eight && up && left ? lr_norm(lab[-W - 1], k) : LR_ABSENT;
        q[5] = eight && up && right ? lr_norm(lab[-W + 1], k) : LR_ABSENT;
        q[6] = eight && down && left ? lr_norm(lab[W - 1], k) : LR_ABSENT;
        q[7] = eight && down && right ? lr_norm(lab[W + 1], k) : LR_ABSENT;
        const int own = lr_norm(*lab, k);
        int n = 0, n_none = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            n += q[i] != LR_ABSENT;
            n_none += q[i] == LR_NONE;
        }
        const u64 bt = lr_beta(beta, b);
        u64 best = ~0ull, e_own = bt * (u64)(n - n_none);                  // (of "no label" until a j turns out to be the own label)
        int arg = 0;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (j < k) {
                int same = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) same += q[i] == j;
                const u64 ej = e[j] + bt * (u64)(n - same);                // < 2^62 + 8 * 2^58
                if (ej < best) {                                           // strictly: the lowest j attaining the minimum
                    best = ej;
                    arg = j;
                }
                if (j == own) e_own = ej;
            }
        }
        const bool stay = own == LR_NONE ? e_own < best : e_own == best;   // the current label wins ties, "no label" never does
        if (!stay) {
            *lab = arg;
            moved = 1;
        }
    }
    const int total = __syncthreads_count(moved);
    if (changed && total && threadIdx.x == 0 && threadIdx.y == 0) atomicAdd(changed + (size_t)b * changed_stride, total);
}

__global__ __launch_bounds__(LR_THREADS) void lr_energy_kernel(const long long *__restrict__ costs, int H, int W, int k, int eight,
                                                               const int32_t *__restrict__ labels, u64 *__restrict__ energy) {
    __shared__ u64 s_sum[2][LR_TH];
    const int b = (int)blockIdx.z;
    const int x = (int)blockIdx.x * LR_TW + (int)threadIdx.x, y = (int)blockIdx.y * LR_TH + (int)threadIdx.y;
    u64 unary = 0ull, pairs = 0ull;
    if (y < H && x < W) {
        const size_t plane = (size_t)H * W;
        const int32_t *lab = labels + (size_t)b * plane + (size_t)y * W + x;
        const int own = lr_norm(*lab, k);
        if (own != LR_NONE) unary = (u64)costs[((size_t)b * k + own) * plane + (size_t)y * W + x];
        const bool down = y + 1 < H, left = x > 0, right = x + 1 < W;
        if (right) pairs += lr_norm(lab[1], k) != own;
        if (down) pairs += lr_norm(lab[W], k) != own;
        if (eight && down && left) pairs += lr_norm(lab[W - 1], k) != own;
        if (eight && down && right) pairs += lr_norm(lab[W + 1], k) != own;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                               // a wave is a row of the workgroup
        unary += __shfl_down(unary, off, 64);
        pairs += __shfl_down(pairs, off, 64);
    }
    if (threadIdx.x == 0) {
        s_sum[0][threadIdx.y] = unary;
        s_sum[1][threadIdx.y] = pairs;
    }
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x < 2) {
        u64 v = 0ull;
#pragma unroll
        for (int i = 0; i < LR_TH; ++i) v += s_sum[threadIdx.x][i];
        if (v) atomicAdd(&energy[(size_t)b * 2 + threadIdx.x], v);
    }
}

__global__ void lr_copy_kernel(const int32_t *__restrict__ in, int32_t *__restrict__ out, size_t n) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) out[i] = in[i];
}

__global__ void lr_zero_kernel(int32_t *__restrict__ changed, int n_changed, u64 *__restrict__ energy, int n_energy) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (changed && i < n_changed) changed[i] = 0;
    if (energy && i < n_energy) energy[i] = 0ull;
}

template <int KB>
void lr_sweeps(const int64_t *costs, const int64_t *beta, int B, int H, int W, int k, int eight, int sweeps, int32_t *labels,
               int32_t *changed, hipStream_t s) {
    for (int t = 0; t < sweeps; ++t) {
        for (int c = 0; c < 4; ++c) {
            const int cy = c >> 1, cx = c & 1, hc = (H - cy + 1) / 2, wc = (W - cx + 1) / 2;
            if (hc < 1 || wc < 1) continue;                                // (a class with no pixel: H or W is 1)
            const dim3 grid((wc + LR_TW - 1) / LR_TW, (hc + LR_TH - 1) / LR_TH, B);
            hipLaunchKernelGGL((lr_pass_kernel<KB>), grid, dim3(LR_TW, LR_TH), 0, s, reinterpret_cast<const long long *>(costs),
                               reinterpret_cast<const long long *>(beta), H, W, k, eight, cy, cx, labels,
                               changed ? changed + t : nullptr, sweeps);
        }
    }
}

}  // namespace

extern "C" int gcs_kmeans_costs(const uint16_t *feats_slab, const uint16_t *centroids, int B, int H, int W, int n_scales, int n_orient,
                                int k, int n_sets, int64_t *costs_out, gcs_stream_t stream) {
    if (!feats_slab || !centroids || !costs_out) return gcs_fail(GCS_EINVAL, "gcs_kmeans_costs: NULL pointer");
    if (k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_costs: k must be in 1..16");
    if (B >= 1 && n_sets != 1 && n_sets != B) return gcs_fail(GCS_EINVAL, "gcs_kmeans_costs: n_sets must be 1 or B");
    GcsLayout lo;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > KE_HW_MAX || W > KE_HW_MAX || !gcs_make_layout(H, W, n_scales, n_orient, &lo) ||
        lo.D > KE_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_costs: bad shape or bank (1 <= B <= 65535, 1 <= H, W <= 4096, a bank of at most 1536 features)");
    const long long p_set = (long long)H * W * (n_sets == 1 ? B : 1);
    if (p_set * lo.D >= (1LL << 31)) return gcs_fail(GCS_EINVAL, "gcs_kmeans_costs: a set of P pixels needs P * D < 2^31");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned char *slab = reinterpret_cast<const unsigned char *>(feats_slab);
#define GCS_KC_GO(KB)                                                                       \
    do {                                                                                    \
        if (lo.split) kc_launch<true, KB>(slab, centroids, lo, B, k, n_sets, costs_out, s); \
        else kc_launch<false, KB>(slab, centroids, lo, B, k, n_sets, costs_out, s);         \
    } while (0)
    if (k <= 2) GCS_KC_GO(2);
    else if (k <= 4) GCS_KC_GO(4);
    else if (k <= 8) GCS_KC_GO(8);
    else GCS_KC_GO(16);
#undef GCS_KC_GO
    GCS_CHECK_LAUNCH("gcs_kmeans_costs");
    return GCS_OK;
}

extern "C" int gcs_label_relax(const int64_t *costs, const int64_t *beta, int B, int H, int W, int k, int neighbours, int sweeps,
                               const int32_t *labels_in, int32_t *labels_out, void *workspace, int32_t *changed_out,
                               int64_t *energy_out, gcs_stream_t stream) {
    if (!costs || !beta || !labels_in || !labels_out) return gcs_fail(GCS_EINVAL, "gcs_label_relax: NULL pointer");
    if (k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, "gcs_label_relax: k must be in 1..16");
    if (neighbours != 4 && neighbours != 8) return gcs_fail(GCS_EINVAL, "gcs_label_relax: neighbours must be 4 or 8");
    if (sweeps < 0 || sweeps > 64) return gcs_fail(GCS_EINVAL, "gcs_label_relax: sweeps must be in 0..64");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 4096 || W > 4096)
        return gcs_fail(GCS_EINVAL, "gcs_label_relax: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096)");
    if (sweeps >= 2 && !workspace) return gcs_fail(GCS_EINVAL, "gcs_label_relax: sweeps >= 2 need the workspace");
    const size_t n = (size_t)B * H * W;
    const uintptr_t a = reinterpret_cast<uintptr_t>(labels_in), o = reinterpret_cast<uintptr_t>(labels_out);
    if (a < o + n * 4 && o < a + n * 4) return gcs_fail(GCS_EINVAL, "gcs_label_relax: labels_out must not overlap labels_in");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_changed = changed_out ? B * sweeps : 0, n_energy = energy_out ? B * 2 : 0;
    if (n_changed > 0 || n_energy > 0) {
        const int m = n_changed > n_energy ? n_changed : n_energy;
        hipLaunchKernelGGL(lr_zero_kernel, dim3((m + 255) / 256), dim3(256), 0, s, changed_out, n_changed,
                           reinterpret_cast<u64 *>(energy_out), n_energy);
    }
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(lr_copy_kernel, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, s, labels_in,
                       labels_out, n);
    const int eight = neighbours == 8;
    if (k <= 2) lr_sweeps<2>(costs, beta, B, H, W, k, eight, sweeps, labels_out, changed_out, s);
    else if (k <= 4) lr_sweeps<4>(costs, beta, B, H, W, k, eight, sweeps, labels_out, changed_out, s);
    else if (k <= 8) lr_sweeps<8>(costs, beta, B, H, W, k, eight, sweeps, labels_out, changed_out, s);
    else lr_sweeps<16>(costs, beta, B, H, W, k, eight, sweeps, labels_out, changed_out, s);
    if (energy_out) {
        const dim3 grid((W + LR_TW - 1) / LR_TW, (H + LR_TH - 1) / LR_TH, B);
        hipLaunchKernelGGL(lr_energy_kernel, grid, dim3(LR_TW, LR_TH), 0, s, reinterpret_cast<const long long *>(costs), H, W, k, eight,
                           labels_out, reinterpret_cast<u64 *>(energy_out));
    }
    GCS_CHECK_LAUNCH("gcs_label_relax");
    return GCS_OK;
}
