// edge_thin.hip — thin boundary maps, SPEC.md §26: non-maximum suppression of an int32 edge map E along its uint8 direction map,
// by linear interpolation (in integers) of V = max(E, 0) between the two ring neighbours the direction's normal passes between.
//
//   et_kernel   one workgroup per 32 rows of 62 output pixels, 256 threads. With its one-pixel halo a tile row is 64 words: ONE
//               dword load per wave and halo row, lane = halo column (the column clamped once per lane, the row once per wave:
//               §26's "the missing neighbour is the pixel itself"), 34 rows over four waves. Every load of a thread - its nine
//               tile words, its eight dir bytes - is issued before the first is waited for. The tile goes to LDS, so the four
//               dir-dependent taps of a pixel are LDS reads, never scattered global loads. The step table (n <= 16 rows) goes to
//               LDS once per workgroup as one 16-byte entry per direction: the two offsets as tile-index deltas (clamped to
//               -1 .. 1 here), w1 and w2. Lanes 1 .. 62 own an output column, rows wave, wave + 4, ...; there is no branch around
//               the taps (a pixel outside the image, a halo lane or dir >= n reads direction 0's taps and drops the result; the
//               tile has a spare row above and below so that those reads stay inside it), and four rows go through their table
//               reads, their taps and their arithmetic together. The products are 32 x 32 -> 64-bit multiply-adds; the store is
//               one dword per lane, 62 contiguous words per wave.
//               9 bytes per pixel of HBM traffic (4 read + 1 read + 4 written); the halo re-reads are L2 hits (9.7 % more words).
// The kernel knows no trigonometry: gcs_thin_steps (host) makes §26's table from §24's normals, and any table is exact.
// No workspace, no allocation, no host synchronisation: one launch (capturable).
#include "common.h"
#include "gcs_thin.h"

#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int ET_TW = 62, ET_TH = 32, ET_THREADS = 256, ET_WAVES = ET_THREADS / 64;
constexpr int ET_PITCH = ET_TW + 2, ET_ROWS = ET_TH + 2;     // the tile with its halo: 34 rows of 64 words, a lane per column
constexpr int ET_PER_THREAD = ET_TH / ET_WAVES;              // 8 output rows of a lane
constexpr int ET_GROUP = 4;                                  // of them in flight together
constexpr int ET_LOADS = (ET_ROWS + ET_WAVES - 1) / ET_WAVES;      // at most 9 halo rows of a wave
constexpr int ET_N_MAX = 16, ET_HW_MAX = 4096;
static_assert(ET_PITCH == 64, "a halo row is one wave wide");

__device__ __forceinline__ int et_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(ET_THREADS) void et_kernel(const int32_t *__restrict__ edges, const uint8_t *__restrict__ dir, int H, int W,
                                                        int n, const int32_t *__restrict__ steps, int32_t *__restrict__ out) {
    __shared__ int s_v[(ET_ROWS + 2) * ET_PITCH];            // V of the tile and its halo in rows 1 .. 34; rows 0 and 35 are spare
    __shared__ v4i s_step[ET_N_MAX];                         // per direction: q1, q2 as deltas of s_v's index, w1, w2
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y0 = (int)blockIdx.y * ET_TH, x0 = (int)blockIdx.x * ET_TW;
    const size_t plane = (size_t)blockIdx.z * (size_t)H * (size_t)W;      // 64-bit: B H W passes 2^32; inside an image H W <= 2^24
    edges += plane, dir += plane, out += plane;

    // every load of the thread is issued before the first one is waited for: the tile's words, then the dir bytes
    const int gx = et_clamp(x0 - 1 + lane, 0, W - 1);
    int e[ET_LOADS];
#pragma unroll
    for (int k = 0; k < ET_LOADS; ++k) {
        const int row = wave + k * ET_WAVES;                 // wave-uniform
        e[k] = 0;
        if (row < ET_ROWS) e[k] = edges[et_clamp(y0 - 1 + row, 0, H - 1) * W + gx];
    }
    const int x = x0 - 1 + lane;
    const bool column = lane >= 1 && lane <= ET_TW && x < W;      // the lane owns an output column (x >= 0 then)
    int d[ET_PER_THREAD];
#pragma unroll
    for (int j = 0; j < ET_PER_THREAD; ++j) {
        const int y = y0 + wave + j * ET_WAVES;
        d[j] = (column && y < H) ? (int)dir[y * W + x] : 255;
    }
    if (tid < n) {                                           // n <= 16: one thread per direction
        const int32_t *row = steps + tid * 8;
        v4i st;
        st.x = et_clamp(row[0], -1, 1) * ET_PITCH + et_clamp(row[1], -1, 1);
        st.y = et_clamp(row[2], -1, 1) * ET_PITCH + et_clamp(row[3], -1, 1);
        st.z = row[4];
        st.w = row[5];
        s_step[tid] = st;
    }
#pragma unroll
    for (int k = 0; k < ET_LOADS; ++k) {
        const int row = wave + k * ET_WAVES;
        if (row < ET_ROWS) s_v[(row + 1) * ET_PITCH + lane] = e[k] > 0 ? e[k] : 0;
    }
    __syncthreads();

    // no branch around the taps: a lane without a pixel (d = 255) or with dir >= n reads direction 0's taps - at most 65 words
    // from its own word, inside s_v thanks to the spare rows - and drops the result. Four rows at a time in three phases (table
    // entries and centres, taps, arithmetic), so that a wave waits for LDS three times per four pixels, not three times per pixel.
#pragma unroll
    for (int j0 = 0; j0 < ET_PER_THREAD; j0 += ET_GROUP) {
        v4i st[ET_GROUP];
        unsigned v[ET_GROUP], c[ET_GROUP][4];
#pragma unroll
        for (int u = 0; u < ET_GROUP; ++u) {
            st[u] = s_step[d[j0 + u] < n ? d[j0 + u] : 0];
            v[u] = (unsigned)s_v[(wave + (j0 + u) * ET_WAVES + 2) * ET_PITCH + lane];
        }
#pragma unroll
        for (int u = 0; u < ET_GROUP; ++u) {
            const int at = (wave + (j0 + u) * ET_WAVES + 2) * ET_PITCH + lane;
            c[u][0] = (unsigned)s_v[at + st[u].x], c[u][1] = (unsigned)s_v[at + st[u].y];
            c[u][2] = (unsigned)s_v[at - st[u].x], c[u][3] = (unsigned)s_v[at - st[u].y];
        }
#pragma unroll
        for (int u = 0; u < ET_GROUP; ++u) {
            const int y = y0 + wave + (j0 + u) * ET_WAVES;
            const unsigned w1 = (unsigned)st[u].z, w2 = (unsigned)st[u].w;
            const u64 plus = (u64)w1 * c[u][0] + (u64)w2 * c[u][1], minus = (u64)w1 * c[u][2] + (u64)w2 * c[u][3];
            const u64 mv = (u64)(w1 + w2) * v[u];
            const int keep = (int)(d[j0 + u] < n) & (int)(v[u] > 0u) & (int)(mv > minus) & (int)(mv >= plus);
            if (column && y < H) out[y * W + x] = keep ? (int)v[u] : 0;
        }
    }
}

bool et_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

int et_sign(int v) { return (v > 0) - (v < 0); }

}  // namespace

extern "C" int gcs_thin_steps(int n, int32_t *steps_out) {
    if (!steps_out) return gcs_fail(GCS_EINVAL, "gcs_thin_steps: NULL pointer");
    if (n < 1 || n > ET_N_MAX) return gcs_fail(GCS_EINVAL, "gcs_thin_steps: bad argument (1 <= n <= 16)");
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
        const int a = (int)floor(1024.0 * cos(pi * i / n) + 0.5), b = (int)floor(1024.0 * sin(pi * i / n) + 0.5);   // SPEC.md §24
        const int A = abs(a), B = abs(b), sa = et_sign(a), sb = et_sign(b);
        int32_t *s = steps_out + 8 * i;
        if (A >= B) {
            s[0] = 0, s[1] = sa, s[4] = A - B, s[5] = B;
        } else {
            s[0] = sb, s[1] = 0, s[4] = B - A, s[5] = A;
        }
        s[2] = sb, s[3] = sa;
        s[6] = s[7] = 0;
    }
    return GCS_OK;
}

extern "C" int gcs_edge_thin(const int32_t *edges, const uint8_t *dir, int B, int H, int W, int n, const int32_t *steps, int32_t *out,
                             gcs_stream_t stream) {
    if (!edges || !dir || !steps || !out) return gcs_fail(GCS_EINVAL, "gcs_edge_thin: NULL pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > ET_HW_MAX || W > ET_HW_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_edge_thin: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096)");
    if (n < 1 || n > ET_N_MAX) return gcs_fail(GCS_EINVAL, "gcs_edge_thin: bad argument (1 <= n <= 16)");
    const size_t px = (size_t)B * (size_t)H * (size_t)W;
    if (et_overlap(out, 4 * px, edges, 4 * px) || et_overlap(out, 4 * px, dir, px) || et_overlap(out, 4 * px, steps, (size_t)n * 32))
        return gcs_fail(GCS_EINVAL, "gcs_edge_thin: out overlaps an input");
    const dim3 grid((W + ET_TW - 1) / ET_TW, (H + ET_TH - 1) / ET_TH, B);
    hipLaunchKernelGGL(et_kernel, grid, dim3(ET_THREADS), 0, stream, edges, dir, H, W, n, steps, out);
    GCS_CHECK_LAUNCH("gcs_edge_thin");
    return GCS_OK;
}
