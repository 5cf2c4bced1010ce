// texton_tile.h — what the half-disc histogram kernels share (texton_gradient.hip: SPEC.md §24; cue_gradient.hip: §25): the tile
// geometry and the limits, the mirror of the border and the exact per-bin chi-square term. Device code only, no kernel.
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

}  // namespace
