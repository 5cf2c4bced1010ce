// texton_gradient.hip — the texton gradient of SPEC.md §24: per pixel and direction the chi-square distance between the label
// histograms of the two halves of a disc, the maximum over the directions, optionally joined with an edge map G (§22) as
// floor(sqrt(TG * G)).
//
//   tg_kernel   one workgroup per 8 x 32 output pixels, one thread per pixel. The tile and its halo are (8 + 2r) rows of
//               32 + 2r <= 62 columns, so ONE ROW OF ONE LABEL'S INDICATOR PLANE IS ONE 64-BIT WORD in LDS. Load phase: a wave owns
//               whole halo rows (a lane per column, mirrored through two small index tables), and one ballot per label the row
//               holds is that label's word - no atomics, and the labels the window holds fall out as a bit mask. Count phase: a
//               pixel at tile column c takes window = (word >> c) & (2^(2r+1) - 1) of every row of its disc; a half's count is the
//               sum of popcount(window & mask row), the mask rows being wave-uniform: LDS broadcasts of a copy of the table laid out
//               as the loop walks it. Directions go CH at a time so that their counters are registers; labels absent from the
//               tile's window are skipped for the whole workgroup (-DGCS_TG_NO_SKIP, for same-box A/B runs: every label 0 .. K-1
//               is walked). The steps are texton_tile.h's, shared with cue_gradient.hip; the kernel's own part
//               is the single label load per halo row and the maximum over the chunks.
// The kernel knows no trigonometry: gcs_texton_masks (host) makes §24's table, and any table of 2r + 1 rows of 2r + 1 bits is exact.
// No workspace, no allocation, no host synchronisation: one launch (capturable).
#include <math.h>

#include "common.h"
#include "texton_tile.h"

namespace {

template <int CH>
__global__ __launch_bounds__(TG_THREADS) void tg_kernel(const int32_t *__restrict__ lab, int H, int W, int K, int r, int n,
                                                        const uint32_t *__restrict__ masks, const int32_t *__restrict__ grad,
                                                        int32_t *__restrict__ out, uint8_t *__restrict__ dir_out) {
    __shared__ u64 s_plane[TG_K_MAX * TG_ROWS_MAX];          // [label][halo row]: bit c = halo column c holds the label
    __shared__ int s_my[TG_ROWS_MAX], s_mx[TG_COLS_MAX];     // mirrored image row / column of every halo row / column
    __shared__ u64 s_present[TG_WAVES];                      // labels each wave met
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[2 * TG_N_MAX * (2 * TG_R_MAX + 1)];      // tg_fill_masks
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y0 = (int)blockIdx.y * TG_TH, x0 = (int)blockIdx.x * TG_TW;
    const int R = 2 * r + 1, rows = TG_TH + 2 * r, cols = TG_TW + 2 * r;
    for (int idx = tid; idx < K * rows; idx += TG_THREADS) s_plane[idx] = 0ull;
    if (tid < rows) s_my[tid] = tg_mirror(y0 - r + tid, H);
    if (tid >= 64 && tid < 64 + cols) s_mx[tid - 64] = tg_mirror(x0 - r + tid - 64, W);
    tg_fill_masks<CH>(s_mask, masks, (n + CH - 1) / CH, R, n, tid);
    __syncthreads();

    // ---- load: wave w owns halo rows w, w + 4, ...; a lane per halo column
    const int32_t *img = lab + (size_t)blockIdx.z * (size_t)H * (size_t)W;
    u64 met = 0ull;
    for (int row = wave; row < rows; row += TG_WAVES) {
        int l = -1;
        if (lane < cols) l = img[(size_t)s_my[row] * (size_t)W + (size_t)s_mx[lane]];
        tg_ballot_row(s_plane, l, K, rows, row, lane, met);
    }
    if (lane == 0) s_present[wave] = met;
    __syncthreads();

    // ---- count: a thread per output pixel
    const u64 present = tg_present(s_present, K);
    const int ty = tid / TG_TW, tx = tid % TG_TW;
    unsigned best = 0u;
    int best_dir = 0;
    for (int i0 = 0; i0 < n; i0 += CH) {
        unsigned chi[CH];
        tg_chunk_chi<CH>(chi, s_plane, s_mask + i0 / CH * R * 2 * CH, present, rows, R, ty, tx);
#pragma unroll
        for (int u = 0; u < CH; ++u)
            if (chi[u] > best) best = chi[u], best_dir = i0 + u;     // the lowest direction that attains the maximum
    }
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    tg_store(((size_t)blockIdx.z * (size_t)H + (size_t)y) * (size_t)W + (size_t)x, best, best_dir, grad, out, dir_out);
}

}  // namespace

extern "C" int gcs_texton_masks(int r, int n, uint32_t *masks_out) {
    if (!masks_out) return gcs_fail(GCS_EINVAL, "gcs_texton_masks: NULL pointer");
    if (r < 1 || r > TG_R_MAX || n < 1 || n > TG_N_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_texton_masks: bad argument (1 <= r <= 15, 1 <= n <= 16)");
    const int R = 2 * r + 1;
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
        const int a = (int)floor(1024.0 * cos(pi * i / n) + 0.5), b = (int)floor(1024.0 * sin(pi * i / n) + 0.5);
        for (int dy = -r; dy <= r; ++dy) {
            uint32_t ma = 0u, mb = 0u;
            for (int dx = -r; dx <= r; ++dx) {
                if (dy * dy + dx * dx > r * r) continue;
                const int s = dx * a + dy * b;
                if (s > 0) ma |= 1u << (dx + r);
                if (s < 0) mb |= 1u << (dx + r);
            }
            masks_out[(2 * i) * R + dy + r] = ma;
            masks_out[(2 * i + 1) * R + dy + r] = mb;
        }
    }
    return GCS_OK;
}

extern "C" int gcs_texton_gradient(const int32_t *labels, int B, int H, int W, int K, int r, int n, const uint32_t *masks,
                                   const int32_t *grad, int32_t *out, uint8_t *dir_out, gcs_stream_t stream) {
    if (!labels || !masks || !out) return gcs_fail(GCS_EINVAL, "gcs_texton_gradient: NULL pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > TG_HW_MAX || W > TG_HW_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_texton_gradient: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096)");
    if (K < 1 || K > TG_K_MAX || r < 1 || r > TG_R_MAX || n < 1 || n > TG_N_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_texton_gradient: bad argument (1 <= K <= 64, 1 <= r <= 15, 1 <= n <= 16)");
    const dim3 grid((W + TG_TW - 1) / TG_TW, (H + TG_TH - 1) / TG_TH, B);
    if (n > 4)
        hipLaunchKernelGGL(tg_kernel<8>, grid, dim3(TG_THREADS), 0, stream, labels, H, W, K, r, n, masks, grad, out, dir_out);
    else
        hipLaunchKernelGGL(tg_kernel<4>, grid, dim3(TG_THREADS), 0, stream, labels, H, W, K, r, n, masks, grad, out, dir_out);
    GCS_CHECK_LAUNCH("gcs_texton_gradient");
    return GCS_OK;
}
