// texton_tile.h — what the half-disc histogram kernels share (texton_gradient.hip: SPEC.md §24; cue_gradient.hip: §25): the tile
// geometry and the limits, the mirror of the border, the exact per-bin chi-square term, and the steps of the method both kernels
// follow - the mask table as the count loop reads it, the ballots of one halo row, the bins a tile holds, the popcount loop over
// one chunk of directions, the store. The LDS arrays are the kernels' own; the pieces take pointers. Device code only, no kernel.
#pragma once

#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int TG_TW = 32, TG_TH = 8, TG_THREADS = TG_TW * TG_TH, TG_WAVES = TG_THREADS / 64;
constexpr int TG_R_MAX = 15, TG_N_MAX = 16, TG_K_MAX = 64, TG_HW_MAX = 4096;
constexpr int TG_ROWS_MAX = TG_TH + 2 * TG_R_MAX, TG_COLS_MAX = TG_TW + 2 * TG_R_MAX;      // 38 rows of 62 columns
static_assert(TG_COLS_MAX <= 64, "a halo row must fit one 64-bit word and one wave");

// mir(t, N) of SPEC.md §24: reflection without repeating the edge pixel, any t.
__device__ __forceinline__ int tg_mirror(int t, int N) {
    if (N == 1) return 0;
    const int p = 2 * (N - 1);
    int u = t % p;
    if (u < 0) u += p;
    return u < N ? u : p - u;
}

// floor(64 (g - h)^2 / (g + h)), 0 for g + h = 0. g, h <= 961 (a 31 x 31 frame): the numerator is below 2^26, the quotient below
// 2^17, so the float estimate (conversion, reciprocal and product: relative error below 2^-21) is within one of the quotient and
// the integer steps (two each way) make it exact for any mask table.
__device__ __forceinline__ unsigned tg_chi_term(unsigned g, unsigned h) {
    const unsigned s = g + h, d = g > h ? g - h : h - g;
    const unsigned num = 64u * d * d, den = s ? s : 1u;
    unsigned q = (unsigned)((float)num * __builtin_amdgcn_rcpf((float)den));
    int rem = (int)(num - q * den);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (rem < 0) --q, rem += (int)den;
        if (rem >= (int)den) ++q, rem -= (int)den;
    }
    return q;
}

// The mask rows as the count loop reads them, [chunk of CH directions][row][direction in chunk][side], zeros past direction n.
template <int CH>
__device__ __forceinline__ void tg_fill_masks(uint32_t *s_mask, const uint32_t *__restrict__ masks, int chunks, int R, int n, int tid) {
    for (int idx = tid; idx < chunks * R * 2 * CH; idx += TG_THREADS) {
        const int e = idx % (2 * CH), m = idx / (2 * CH) % R, i = idx / (2 * CH * R) * CH + (e >> 1);
        s_mask[idx] = i < n ? masks[(2 * i + (e & 1)) * R + m] : 0u;
    }
}

// One halo row of a wave, lane = halo column holding bin v (a value outside 0 .. K-1 counts in no bin): one ballot per bin the row
// holds is that bin's word - no atomics - and the bins met are added to `met`. Wave-uniform: one turn per bin of the row.
__device__ __forceinline__ void tg_ballot_row(u64 *s_plane, int v, int K, int rows, int row, int lane, u64 &met) {
    const bool counted = (unsigned)v < (unsigned)K;
    u64 todo = __ballot(counted);
    while (todo) {
        const int v0 = __builtin_amdgcn_readlane(v, __ffsll((long long)todo) - 1);
        const u64 word = __ballot(counted && v == v0);
        if (lane == 0) s_plane[v0 * rows + row] = word;
        met |= 1ull << v0;
        todo &= ~word;
    }
}

// The bins the tile's window holds, wave-uniform (-DGCS_TG_NO_SKIP, for same-box A/B runs: every bin 0 .. K-1).
__device__ __forceinline__ u64 tg_present(const u64 *s_present, int K) {
#ifdef GCS_TG_NO_SKIP
    const u64 present = K == 64 ? ~0ull : (1ull << K) - 1ull;
#else
    const u64 present = s_present[0] | s_present[1] | s_present[2] | s_present[3];
#endif
    return (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)present) |
           (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(present >> 32)) << 32;
}

// chi[u] of one chunk of CH directions at tile pixel (ty, tx), summed over the bins of `present`: the pixel takes window =
// (word >> tx) & (2^R - 1) of every row of its disc, a half's count is the sum of popcount(window & mask row). `mrows`: the chunk's
// R rows of s_mask, read at one address by the whole wave (LDS broadcast). CH directions at a time, so their counters are registers.
template <int CH>
__device__ __forceinline__ void tg_chunk_chi(unsigned (&chi)[CH], const u64 *s_plane, const uint32_t *mrows, u64 present, int rows,
                                             int R, int ty, int tx) {
    const unsigned full = (1u << R) - 1u;                    // R <= 31
#pragma unroll
    for (int u = 0; u < CH; ++u) chi[u] = 0u;
    for (u64 pm = present; pm; pm &= pm - 1ull) {
        const u64 *pl = s_plane + (__ffsll((long long)pm) - 1) * rows + ty;
        unsigned g[CH], h[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) g[u] = h[u] = 0u;
        for (int m = 0; m < R; ++m) {
            const unsigned win = (unsigned)(pl[m] >> tx) & full;
            const uint4 *row = reinterpret_cast<const uint4 *>(mrows + m * 2 * CH);
#pragma unroll
            for (int u = 0; u < CH; u += 2) {
                const uint4 q = row[u >> 1];
                g[u] += (unsigned)__popc(win & q.x), h[u] += (unsigned)__popc(win & q.y);
                g[u + 1] += (unsigned)__popc(win & q.z), h[u + 1] += (unsigned)__popc(win & q.w);
            }
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) chi[u] += tg_chi_term(g[u], h[u]);
    }
}

// best, or floor(sqrt(best * max(grad, 0))), and the direction. The product is inside fg_isqrt's 2^52: TG < 2^17 and G < 2^31
// (below 2^48) in tg_kernel, PB <= 2^23 and G < 2^20 (§22: below 2^43) in cg_kernel.
__device__ __forceinline__ void tg_store(size_t at, unsigned best, int best_dir, const int32_t *__restrict__ grad,
                                         int32_t *__restrict__ out, uint8_t *__restrict__ dir_out) {
    if (grad) {
        const int gv = grad[at];
        out[at] = fg_isqrt((u64)best * (u64)(gv > 0 ? gv : 0));
    } else {
        out[at] = (int32_t)best;
    }
    if (dir_out) dir_out[at] = (uint8_t)best_dir;
}

}  // namespace
