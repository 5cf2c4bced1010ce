// cue_gradient.hip — the boundary map of SPEC.md §25: half-disc chi-square distances (§24) of up to four cues - a label map and
// the three channels of a uint8 image quantised to 2 .. 64 bins - added per direction with integer weights before the maximum
// over the directions is taken, optionally joined with an edge map G (§22) as floor(sqrt(PB * G)).
//
//   cg_kernel   tg_kernel's method (texton_gradient.hip) with the cues walked outermost: one workgroup per
//               8 x 32 output pixels, one thread per pixel; one row of one bin's indicator plane is one 64-bit LDS word made by a
//               wave ballot; a half's count is a sum of popcounts against mask rows broadcast from LDS; bins absent from the
//               tile's window are skipped; the division is tg_chi_term - the steps of texton_tile.h, which both kernels call.
//               What differs, and is this kernel's own: the mirror tables and the transposed mask
//               table are built once per tile and serve every cue; a lane loads the three bytes of its halo pixels ONCE, keeps
//               them packed in registers (a wave owns at most 10 halo rows) and ballots one channel of them per cue; ONE set of
//               planes in LDS is re-used cue after cue; and the per-direction sums P_i = sum_c w_c chi_{c,i} live in registers
//               (CH * NCH <= 16 of them) until the last cue, when the maximum and its lowest direction are taken. The weight is
//               applied once per cue and direction, outside the popcount loop. A cue of weight 0 is not read.
// No workspace, no allocation, no host synchronisation: one launch (capturable).
#include "common.h"
#include "gcs_cues.h"
#include "texton_tile.h"

namespace {

constexpr int CG_ROWS_PER_WAVE = (TG_ROWS_MAX + TG_WAVES - 1) / TG_WAVES;      // 10 halo rows of a wave at r = 15
constexpr int CG_W_MAX = 16, CG_SHIFT_MIN = 2, CG_SHIFT_MAX = 7;

// wpack: the four weights, a byte each (cue c in bits 8c .. 8c + 7)
template <int CH, int NCH>
__global__ __launch_bounds__(TG_THREADS) void cg_kernel(const int32_t *__restrict__ lab, const uint8_t *__restrict__ img, int H, int W,
                                                        int K, int shift, unsigned wpack, int r, int n,
                                                        const uint32_t *__restrict__ masks, const int32_t *__restrict__ grad,
                                                        int32_t *__restrict__ out, uint8_t *__restrict__ dir_out) {
    __shared__ u64 s_plane[TG_K_MAX * TG_ROWS_MAX];          // [bin][halo row] of the cue at hand: bit c = halo column c holds the bin
    __shared__ int s_my[TG_ROWS_MAX], s_mx[TG_COLS_MAX];     // mirrored image row / column of every halo row / column
    __shared__ u64 s_present[TG_WAVES];                      // bins each wave met
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[2 * TG_N_MAX * (2 * TG_R_MAX + 1)];      // tg_fill_masks
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y0 = (int)blockIdx.y * TG_TH, x0 = (int)blockIdx.x * TG_TW;
    const int R = 2 * r + 1, rows = TG_TH + 2 * r, cols = TG_TW + 2 * r;
    if (tid < rows) s_my[tid] = tg_mirror(y0 - r + tid, H);
    if (tid >= 64 && tid < 64 + cols) s_mx[tid - 64] = tg_mirror(x0 - r + tid - 64, W);
    tg_fill_masks<CH>(s_mask, masks, NCH, R, n, tid);
    __syncthreads();

    // ---- load: wave w owns halo rows w, w + 4, ...; a lane per halo column; the three bytes of a pixel are read once
    const size_t plane = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    unsigned px[CG_ROWS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < CG_ROWS_PER_WAVE; ++j) {
        const int row = wave + j * TG_WAVES;
        px[j] = 0u;
        if ((wpack >> 8) && row < rows && lane < cols) {
            const uint8_t *p = img + 3 * (plane + (size_t)s_my[row] * (size_t)W + (size_t)s_mx[lane]);
            px[j] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
        }
    }

    const int ty = tid / TG_TW, tx = tid % TG_TW;
    unsigned P[CH * NCH];
#pragma unroll
    for (int i = 0; i < CH * NCH; ++i) P[i] = 0u;

    for (int c = 0; c < 4; ++c) {                            // (every branch on c and wc is workgroup-uniform)
        const unsigned wc = (wpack >> (8 * c)) & 255u;
        if (!wc) continue;
        const int Kc = c ? 256 >> shift : K;
        for (int idx = tid; idx < Kc * rows; idx += TG_THREADS) s_plane[idx] = 0ull;
        __syncthreads();
        u64 met = 0ull;
#pragma unroll
        for (int j = 0; j < CG_ROWS_PER_WAVE; ++j) {
            const int row = wave + j * TG_WAVES;
            if (row >= rows) continue;                       // wave-uniform
            int v = -1;
            if (c == 0) {
                if (lane < cols) v = lab[plane + (size_t)s_my[row] * (size_t)W + (size_t)s_mx[lane]];
            } else if (lane < cols) {
                v = (int)((px[j] >> (8 * (c - 1))) & 255u) >> shift;
            }
            tg_ballot_row(s_plane, v, Kc, rows, row, lane, met);
        }
        if (lane == 0) s_present[wave] = met;
        __syncthreads();

        // ---- count: a thread per output pixel, the bins the window holds only
        const u64 present = tg_present(s_present, Kc);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            unsigned chi[CH];
            tg_chunk_chi<CH>(chi, s_plane, s_mask + ch * R * 2 * CH, present, rows, R, ty, tx);
#pragma unroll
            for (int u = 0; u < CH; ++u) P[ch * CH + u] += wc * chi[u];      // the weight: once per cue and direction
        }
        __syncthreads();                                     // the planes are the next cue's
    }

    unsigned best = 0u;
    int best_dir = 0;
#pragma unroll
    for (int i = 0; i < CH * NCH; ++i)
        if (P[i] > best) best = P[i], best_dir = i;          // the lowest direction that attains the maximum (P_i = 0 past n)
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    tg_store(plane + (size_t)y * (size_t)W + (size_t)x, best, best_dir, grad, out, dir_out);
}

bool cg_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int gcs_cue_gradient(const int32_t *labels, const uint8_t *img, int B, int H, int W, int K, int shift, int w0, int w1,
                                int w2, int w3, int r, int n, const uint32_t *masks, const int32_t *grad, int32_t *out,
                                uint8_t *dir_out, gcs_stream_t stream) {
    if (!masks || !out) return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: NULL pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > TG_HW_MAX || W > TG_HW_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096)");
    if (K < 1 || K > TG_K_MAX || r < 1 || r > TG_R_MAX || n < 1 || n > TG_N_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: bad argument (1 <= K <= 64, 1 <= r <= 15, 1 <= n <= 16)");
    if (shift < CG_SHIFT_MIN || shift > CG_SHIFT_MAX) return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: bad shift (2 <= shift <= 7)");
    const int w[4] = {w0, w1, w2, w3};
    for (int c = 0; c < 4; ++c)
        if (w[c] < 0 || w[c] > CG_W_MAX) return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: bad weight (0 <= w <= 16)");
    if (!(w0 | w1 | w2 | w3)) return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: every weight is 0");
    if ((w0 && !labels) || ((w1 | w2 | w3) && !img))
        return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: a cue of non-zero weight has no plane");
    const size_t px = (size_t)B * (size_t)H * (size_t)W;
    const struct { const void *p; size_t bytes; } ins[4] = {{w0 ? labels : nullptr, 4 * px}, {(w1 | w2 | w3) ? img : nullptr, 3 * px},
                                                            {grad, 4 * px}, {masks, (size_t)n * 2 * (2 * r + 1) * 4}};
    for (const auto &in : ins)
        if (cg_overlap(out, 4 * px, in.p, in.bytes) || cg_overlap(dir_out, px, in.p, in.bytes))
            return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: an output overlaps an input");
    if (cg_overlap(out, 4 * px, dir_out, px)) return gcs_fail(GCS_EINVAL, "gcs_cue_gradient: out overlaps dir_out");
    const unsigned wpack = (unsigned)w0 | (unsigned)w1 << 8 | (unsigned)w2 << 16 | (unsigned)w3 << 24;
    const dim3 grid((W + TG_TW - 1) / TG_TW, (H + TG_TH - 1) / TG_TH, B);
#define CG_LAUNCH(CH, NCH)                                                                                                       \
    hipLaunchKernelGGL((cg_kernel<CH, NCH>), grid, dim3(TG_THREADS), 0, stream, labels, img, H, W, K, shift, wpack, r, n, masks, \
                       grad, out, dir_out)
    if (n > 8)
        CG_LAUNCH(8, 2);
    else if (n > 4)
        CG_LAUNCH(8, 1);
    else
        CG_LAUNCH(4, 1);
#undef CG_LAUNCH
    GCS_CHECK_LAUNCH("gcs_cue_gradient");
    return GCS_OK;
}
