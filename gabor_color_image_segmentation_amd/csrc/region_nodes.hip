// region_nodes.hip — the node map of SPEC.md §18 (gfx950): the connected regions of a label map (§7), merged by §9 with a minimum
// size that each image chooses on the device, so that no image has more than k_cap nodes. Forest and round kernels: region_kernels.h.
// Nothing here allocates, frees or synchronises; the entry point enqueues on the caller's stream.
#include "region_kernels.h"

// The round flags of §9 (region_kernels.h) with one row in front: act[0][b] = "image b runs rounds at all" (m_b > 1), written by
// rn_count_kernel; round r of gcs_region_nodes is round r + 1 of the shared kernels, so an image with m_b <= 1 is idle from its
// first round on and pays the launches' empty blocks only.

// One workgroup per image: the roots of the forest (parent[p] == p) are the regions. n_out == NULL: in front of the rounds, C =
// their count decides m_b (SPEC.md §18), stored for the rounds and, if asked for, for the caller. Else: n_out[b] = their count.
__global__ __launch_bounds__(1024) void rn_count_kernel(int H, int W, int B, const int *__restrict__ parent, int min_size, int k_cap,
                                                        unsigned *__restrict__ m_used, int32_t *__restrict__ m_out,
                                                        int *__restrict__ act, int32_t *__restrict__ n_out) {
    __shared__ int s_total;
    const int P = H * W, b = blockIdx.x;
    const int *par = parent + (size_t)b * P;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    int cnt = 0;
    for (int p = threadIdx.x; p < P; p += blockDim.x) cnt += par[p] == p;
    if (cnt) atomicAdd(&s_total, cnt);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int C = s_total;
    if (n_out) {
        n_out[b] = C;
        return;
    }
    const int m_guard = (P + k_cap - 1) / k_cap;
    const int m_b = C > k_cap && m_guard > min_size ? m_guard : min_size;
    m_used[b] = (unsigned)m_b;
    if (m_out) m_out[b] = m_b;
    act[b] = m_b > 1;
}

// mr_best_kernel with the image's own minimum size
__global__ void rn_best_kernel(int H, int W, int B, int round, const unsigned *__restrict__ m_used, const int *__restrict__ parent,
                               const unsigned *__restrict__ size, unsigned long long *__restrict__ best,
                               const int *__restrict__ act) {
    const int P = H * W, b = blockIdx.y;
    if (mr_idle(act, round, B, b)) return;
    mr_best_image(H, W, m_used[b], parent + (size_t)b * P, size + (size_t)b * P, best + (size_t)b * P);
}

static bool rn_shape_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096; }

extern "C" size_t gcs_region_nodes_scratch_bytes(int B, int H, int W) {
    if (!rn_shape_ok(B, H, W)) return 0;
    // best (u64) | parent | rootid | size per pixel, one flag per (round + 1, image), one minimum size per image
    return (size_t)B * H * W * (sizeof(unsigned long long) + 3 * sizeof(int32_t)) + (size_t)(32 + 1) * B * sizeof(int32_t);
}

extern "C" int gcs_region_nodes(const int32_t *labels, int B, int H, int W, int min_size, int k_cap, void *scratch, int32_t *nodes_out,
                                int32_t *n_nodes_out, int32_t *min_size_used, gcs_stream_t stream) {
    if (!labels || !scratch || !nodes_out || !n_nodes_out) return gcs_fail(GCS_EINVAL, "gcs_region_nodes: NULL pointer");
    if (!rn_shape_ok(B, H, W)) return gcs_fail(GCS_EINVAL, "gcs_region_nodes: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096)");
    if (min_size < 0) return gcs_fail(GCS_EINVAL, "gcs_region_nodes: min_size < 0");
    if (k_cap < 1 || k_cap > 4096) return gcs_fail(GCS_EINVAL, "gcs_region_nodes: k_cap outside 1..4096");
    const int P = H * W;
    const size_t n = (size_t)B * P;
    const uintptr_t l0 = reinterpret_cast<uintptr_t>(labels), o0 = reinterpret_cast<uintptr_t>(nodes_out), bytes = n * sizeof(int32_t);
    if (l0 < o0 + bytes && o0 < l0 + bytes) return gcs_fail(GCS_EINVAL, "gcs_region_nodes: nodes_out overlaps labels");
    unsigned long long *best = static_cast<unsigned long long *>(scratch);
    int *parent = reinterpret_cast<int *>(best + n);
    int *rootid = parent + n;
    unsigned *size = reinterpret_cast<unsigned *>(rootid + n);
    int *act = reinterpret_cast<int *>(size + n);                  // [n_rounds + 1][B]: row 0 = m_b > 1
    unsigned *m_used = reinterpret_cast<unsigned *>(act + (size_t)32 * B);
    // The guard needs C > k_cap, and C <= P: an image of at most k_cap pixels never takes it, so with min_size <= 1 no round is
    // enqueued. Otherwise the rounds of §9's halving bound are: floor(log2(P)) + 1 <= 25, and 26 flag rows fit the 32.
    int n_rounds = 0;
    if (min_size > 1 || P > k_cap)
        for (unsigned v = (unsigned)P; v; v >>= 1) ++n_rounds;
    const dim3 grid(min(1024, (P + 255) / 256), B), block(256);
    hipLaunchKernelGGL(mr_init_kernel, grid, block, 0, stream, H, W, B, n_rounds + 1, parent, size, best, act);
    GCS_CHECK_LAUNCH("gcs_region_nodes(init)");
    hipLaunchKernelGGL(cc_union_kernel, grid, block, 0, stream, labels, H, W, parent);
    GCS_CHECK_LAUNCH("gcs_region_nodes(union)");
    hipLaunchKernelGGL(rn_count_kernel, dim3(B), dim3(1024), 0, stream, H, W, B, parent, min_size, k_cap, m_used, min_size_used, act,
                       static_cast<int32_t *>(nullptr));
    GCS_CHECK_LAUNCH("gcs_region_nodes(count)");
    if (n_rounds > 0) {
        hipLaunchKernelGGL(mr_flatten_kernel, grid, block, 0, stream, H, W, B, 0, parent, act);      // (idle images stay as they are)
        GCS_CHECK_LAUNCH("gcs_region_nodes(flatten)");
    }
    for (int r = 1; r <= n_rounds; ++r) {
        hipLaunchKernelGGL(mr_size_kernel, grid, block, 0, stream, H, W, B, r, parent, size, act);
        GCS_CHECK_LAUNCH("gcs_region_nodes(size)");
        hipLaunchKernelGGL(rn_best_kernel, grid, block, 0, stream, H, W, B, r, m_used, parent, size, best, act);
        GCS_CHECK_LAUNCH("gcs_region_nodes(best)");
        hipLaunchKernelGGL(mr_union_kernel, grid, block, 0, stream, H, W, B, r, parent, size, best, act);
        GCS_CHECK_LAUNCH("gcs_region_nodes(merge)");
        hipLaunchKernelGGL(mr_flatten_kernel, grid, block, 0, stream, H, W, B, r, parent, act);
        GCS_CHECK_LAUNCH("gcs_region_nodes(flatten)");
    }
    hipLaunchKernelGGL(cc_rank_kernel, dim3(B), dim3(1024), 0, stream, H, W, parent, rootid);
    GCS_CHECK_LAUNCH("gcs_region_nodes(rank)");
    hipLaunchKernelGGL(cc_relabel_kernel, grid, block, 0, stream, H, W, parent, rootid, nodes_out);
    GCS_CHECK_LAUNCH("gcs_region_nodes(relabel)");
    hipLaunchKernelGGL(rn_count_kernel, dim3(B), dim3(1024), 0, stream, H, W, B, parent, min_size, k_cap, m_used,
                       static_cast<int32_t *>(nullptr), act, n_nodes_out);
    GCS_CHECK_LAUNCH("gcs_region_nodes");
    return GCS_OK;
}
