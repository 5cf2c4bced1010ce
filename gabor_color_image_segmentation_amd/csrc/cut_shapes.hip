// cut_shapes.hip — area, perimeter and boundary count of every group of every cut of a region tree at once (SPEC.md §17): the
// integer part of the reference's compactness and density (metrics.py:157-201) without relabelling a pixel per cut.
// Nothing here allocates, frees or synchronises; the entry point enqueues on the caller's stream.
//
// A pixel counts towards its region's perimeter when it lies on the image border or a 4-neighbour carries another label; in the cut
// at R an interior pixel has such a neighbour exactly when U > tau, tau = max(0, alive - R), U the contour map of SPEC.md §15. With
// the requested cuts in decreasing R the tau_c are non-decreasing, so a pixel is a perimeter pixel at exactly the cuts c < m,
// m = #{c : tau_c < U} (m = n_cuts on the image border), and a boundary pixel (density) at the cuts c < m', m' the same count from U
// alone. Three launches:
//   zero    the workspace: per image bins [K][n_cuts + 1], area [K], bd [n_cuts + 1]
//   pixels  one pass over (labels, U): bins[label][m] += 1 for m > 0, area[label] += 1, bd[m'] += 1 for m' > 0 (bin 0 is never summed
//           and stays 0). A workgroup owns a run of whole rows of one image; its counters sit in LDS when the K (n_cuts + 2) +
//           n_cuts + 1 of them fit SW_LDS_COUNTERS (the budget of the other sweep's pixel pass) and leave with one vector atomic per
//           non-zero counter, otherwise every count is a global atomic (slow, exact). No neighbour is read: U already holds them.
//   groups  a workgroup per image: rs_absorbers and, per distinct tau, rs_group_reps (tree_cuts.h: the walk every cut kernel shares);
//           every leaf adds its area and the suffix sum of its bins above c into its rep's LDS row, the rows leave densely.
// Both kernels take their tau list from rs_taus (tree_cuts.h). Integer sums only: any order gives the same bits.
#include "common.h"
#include "tree_cuts.h"

constexpr int CS_THREADS = 256, CS_UNROLL = 4;
constexpr int CS_PIXELS_MIN = 4096;                            // pixels a workgroup of the pixel pass takes at least

__global__ __launch_bounds__(256) void cut_shapes_zero_kernel(unsigned *p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

__global__ __launch_bounds__(CS_THREADS) void cut_shapes_pixel_kernel(const int32_t *__restrict__ labels,
                                                                      const int32_t *__restrict__ contours,
                                                                      const int32_t *__restrict__ alive_p,
                                                                      const int32_t *__restrict__ regions, int H, int W, int K,
                                                                      int n_cuts, int rows_per, int use_lds, unsigned *ws) {
    extern __shared__ unsigned cs_tab[];                       // use_lds: [K][n_cuts + 1] bins | [K] area | [n_cuts + 1] bd
    __shared__ int s_tau[RS_CUTS_MAX];
    const int tid = threadIdx.x, b = blockIdx.y, E = n_cuts + 1;
    const int n_tab = K * (E + 1) + E;
    const int y0 = blockIdx.x * rows_per, y1 = min(H, y0 + rows_per);
    if (use_lds)
        for (int i = tid; i < n_tab; i += CS_THREADS) cs_tab[i] = 0u;
    rs_taus(regions, n_cuts, alive_p[b], K - 1, s_tau);        // (and the barrier behind the zeroing)
    unsigned *tab = use_lds ? cs_tab : ws + (size_t)b * n_tab;
    unsigned *t_area = tab + (size_t)K * E, *t_bd = t_area + K;
    const int tau0 = s_tau[0];
    const size_t base = (size_t)b * H * W;
    const int p0 = y0 * W, p1 = y1 * W;                        // (H * W <= 2^24)
    for (int q0 = p0 + tid; q0 < p1; q0 += CS_THREADS * CS_UNROLL) {
        int l[CS_UNROLL], u[CS_UNROLL];
#pragma unroll
        for (int k = 0; k < CS_UNROLL; ++k) {                  // the loads of CS_UNROLL pixels in flight together
            const int p = q0 + k * CS_THREADS;
            l[k] = p < p1 ? labels[base + p] : -1;
            u[k] = p < p1 ? contours[base + p] : 0;
        }
#pragma unroll
        for (int k = 0; k < CS_UNROLL; ++k) {
            const int p = q0 + k * CS_THREADS;
            int m = 0;                                         // #{c : tau_c < U}: the tau_c are non-decreasing
            if (u[k] > tau0) {
                int lo = 1, hi = n_cuts;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_tau[mid] < u[k]) lo = mid + 1; else hi = mid;
                }
                m = lo;
            }
            if (m > 0) atomicAdd(&t_bd[m], 1u);                // (a pixel past p1 has U = 0 <= tau_0)
            if ((unsigned)l[k] >= (unsigned)K) continue;       // outside 0 .. K-1 (or past p1): counted in no area and no perimeter
            const int y = p / W, x = p - y * W;
            if (y == 0 || y == H - 1 || x == 0 || x == W - 1) m = n_cuts;
            atomicAdd(&t_area[l[k]], 1u);
            if (m > 0) atomicAdd(&tab[(size_t)l[k] * E + m], 1u);
        }
    }
    if (!use_lds) return;
    __syncthreads();
    unsigned *g = ws + (size_t)b * n_tab;
    for (int i = tid; i < n_tab; i += CS_THREADS) {
        const unsigned c = cs_tab[i];
        if (c) atomicAdd(&g[i], c);
    }
}

__global__ __launch_bounds__(AG_THREADS) void cut_shapes_group_kernel(const int32_t *__restrict__ merges,
                                                                      const int32_t *__restrict__ alive_p,
                                                                      const int32_t *__restrict__ regions, int B, int K, int n_cuts,
                                                                      const unsigned *__restrict__ ws, unsigned *__restrict__ area_out,
                                                                      unsigned *__restrict__ perim_out,
                                                                      unsigned *__restrict__ boundary_out) {
    __shared__ unsigned s_dk[RS_K_MAX];
    __shared__ unsigned short s_root[RS_K_MAX];
    __shared__ unsigned s_area[RS_K_MAX], s_perim[RS_K_MAX];
    __shared__ int s_tau[RS_CUTS_MAX];
    __shared__ int s_changed;
    const int b = blockIdx.x, tid = threadIdx.x, E = n_cuts + 1;
    const int n_tab = K * (E + 1) + E;
    const unsigned *bins = ws + (size_t)b * n_tab, *leaf_area = bins + (size_t)K * E, *bd = leaf_area + K;
    rs_absorbers(merges + (size_t)b * (K - 1) * 2, K - 1, K, s_dk, &s_changed);   // (merges is not read with K = 1)
    rs_taus(regions, n_cuts, alive_p[b], K - 1, s_tau);
    if (tid == 0) {                                            // boundary[c] = the pixels with m' > c
        unsigned above = 0;
        for (int c = n_cuts - 1; c >= 0; --c) {
            above += bd[c + 1];
            boundary_out[(size_t)c * B + b] = above;
        }
    }
    unsigned mine[RS_PER], above[RS_PER];                      // this thread's leaves: their area, and their bins above the cut in hand
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
        const int q = tid + j * AG_THREADS;
        mine[j] = q < K ? leaf_area[q] : 0u;
        above[j] = 0u;
    }
    for (int c = n_cuts - 1; c >= 0; --c) {                    // from the coarsest cut up: the suffix sums grow by one bin per cut
        if (c == n_cuts - 1 || s_tau[c] != s_tau[c + 1]) rs_group_reps(s_dk, s_root, K, s_tau[c]);
        for (int q = tid; q < K; q += AG_THREADS) s_area[q] = s_perim[q] = 0u;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RS_PER; ++j) {
            const int q = tid + j * AG_THREADS;
            if (q < K) {
                above[j] += bins[(size_t)q * E + c + 1];
                if (mine[j]) {                                 // (an unused label has no pixel in any bin either)
                    atomicAdd(&s_area[s_root[q]], mine[j]);
                    if (above[j]) atomicAdd(&s_perim[s_root[q]], above[j]);
                }
            }
        }
        __syncthreads();
        unsigned *a_out = area_out + ((size_t)c * B + b) * K, *p_out = perim_out + ((size_t)c * B + b) * K;
        for (int q = tid; q < K; q += AG_THREADS) {
            a_out[q] = s_area[q];
            p_out[q] = s_perim[q];
        }
        __syncthreads();                                       // the rows are read before the next cut clears them
    }
}

static bool cut_shapes_ws_ok(int B, int K, int n_cuts) {
    return B >= 1 && B <= 65535 && K >= 1 && K <= RS_K_MAX && n_cuts >= 1 && n_cuts <= RS_CUTS_MAX &&
           (long long)B * ((long long)K * (n_cuts + 2) + n_cuts + 1) < 0x80000000LL;
}

extern "C" size_t gcs_cut_shapes_workspace_bytes(int B, int K, int n_cuts) {
    if (!cut_shapes_ws_ok(B, K, n_cuts)) return 0;
    return (size_t)B * ((size_t)K * (n_cuts + 2) + n_cuts + 1) * sizeof(uint32_t);
}

extern "C" int gcs_cut_shapes(const int32_t *labels, const int32_t *contours, const int32_t *merges, const int32_t *alive,
                              const int32_t *regions, int B, int H, int W, int K, int n_cuts, void *workspace, uint32_t *area_out,
                              uint32_t *perim_out, uint32_t *boundary_out, gcs_stream_t stream) {
    if (!labels || !contours || !alive || !regions || !workspace || !area_out || !perim_out || !boundary_out || (K > 1 && !merges))
        return gcs_fail(GCS_EINVAL, "gcs_cut_shapes: NULL pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 4096 || W > 4096 || K < 1 || K > RS_K_MAX || n_cuts < 1 || n_cuts > RS_CUTS_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_cut_shapes: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 1 <= K <= 4096, 1 <= n_cuts <= 64)");
    if (!cut_shapes_ws_ok(B, K, n_cuts) || (long long)B * H * W >= 0x80000000LL)   // (the outputs are smaller than the workspace)
        return gcs_fail(GCS_EINVAL, "gcs_cut_shapes: B * H * W and B * (K * (n_cuts + 2) + n_cuts + 1) must be below 2^31");
    const int n_tab = K * (n_cuts + 2) + n_cuts + 1;
    const size_t n_ws = (size_t)B * n_tab;
    const unsigned zero_blocks = (unsigned)((n_ws + 1023) / 1024 < 4096 ? (n_ws + 1023) / 1024 : 4096);
    hipLaunchKernelGGL(cut_shapes_zero_kernel, dim3(zero_blocks), dim3(256), 0, stream, static_cast<unsigned *>(workspace), n_ws);
    GCS_CHECK_LAUNCH("gcs_cut_shapes(zero)");
    // a workgroup takes whole rows: about 1024 workgroups over the batch, none below CS_PIXELS_MIN pixels (its counters are zeroed
    // and flushed once per workgroup)
    const long long pixels = (long long)H * W;
    long long per = pixels * B / 1024;
    per = per < CS_PIXELS_MIN ? CS_PIXELS_MIN : per;
    const int rows_per = (int)((per + W - 1) / W < H ? (per + W - 1) / W : H);
    const int use_lds = n_tab <= SW_LDS_COUNTERS;
    hipLaunchKernelGGL(cut_shapes_pixel_kernel, dim3((H + rows_per - 1) / rows_per, B), dim3(CS_THREADS),
                       use_lds ? (size_t)n_tab * sizeof(unsigned) : 0, stream, labels, contours, alive, regions, H, W, K, n_cuts,
                       rows_per, use_lds, static_cast<unsigned *>(workspace));
    GCS_CHECK_LAUNCH("gcs_cut_shapes(pixels)");
    hipLaunchKernelGGL(cut_shapes_group_kernel, dim3(B), dim3(AG_THREADS), 0, stream, merges, alive, regions, B, K, n_cuts,
                       static_cast<const unsigned *>(workspace), area_out, perim_out, boundary_out);
    GCS_CHECK_LAUNCH("gcs_cut_shapes(groups)");
    return GCS_OK;
}
