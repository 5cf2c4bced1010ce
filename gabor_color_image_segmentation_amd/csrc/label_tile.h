// label_tile.h — the tile-local label accumulator of rt_stats_kernel (region_tree.hip) and rp_stats_kernel (region_props.hip): one
// workgroup of LT_THREADS threads per LT_TH x LT_TW pixel tile, one thread per pixel. The labels a tile sees get a row of `width`
// uint32 accumulators in LDS through an LT_SLOTS-slot hash table (256 pixels * 65 535 < 2^32); eight neighbouring lanes (one run of a
// tile row) that agree on the label add ONE sum; touched cells leave with 64-bit vector atomics into rows [K][width]. A tile that
// sees more than LT_SLOTS labels raises *s_over and its kernel adds straight into the global rows instead (slow, exact). The row
// layout, the LDS arrays and whatever else a kernel keeps per slot belong to the caller.
#pragma once
#include "common.h"

constexpr int LT_TH = 8, LT_TW = 32, LT_THREADS = LT_TH * LT_TW;  // statistics tile: 8 rows of 32 pixels, one thread each
constexpr int LT_SLOTS = 32;                                       // labels a tile accumulates in LDS

// At entry: s_acc [LT_SLOTS][width] := 0, every slot free (key -1), no overflow. The caller's __syncthreads() follows.
__device__ __forceinline__ void lt_clear(unsigned *s_acc, int width, int *s_keys, int *s_over) {
    const int tid = (int)threadIdx.x;
    for (int idx = tid; idx < LT_SLOTS * width; idx += LT_THREADS) s_acc[idx] = 0u;
    if (tid < LT_SLOTS) s_keys[tid] = -1;
    if (tid == 0) *s_over = 0;
}

// This thread's pixel of tile (blockIdx.x, blockIdx.y): false past the image's edge, where (y, x) is clamped so reads stay inside.
__device__ __forceinline__ bool lt_pixel(int H, int W, int *y, int *x) {
    const int yy = (int)blockIdx.y * LT_TH + (int)threadIdx.x / LT_TW, xx = (int)blockIdx.x * LT_TW + (int)threadIdx.x % LT_TW;
    *y = yy < H ? yy : H - 1, *x = xx < W ? xx : W - 1;
    return yy < H && xx < W;
}

// The slot of label l (`in`: this pixel is counted), or -1 with *s_over = 1 when every slot holds another label. The slots are
// settled for all only behind the caller's __syncthreads().
__device__ __forceinline__ int lt_claim(int *s_keys, int *s_over, int l, bool in) {
    int slot = -1;
    if (in) {
        const unsigned h = ((unsigned)l * 2654435761u) >> 27;
        for (int p = 0; p < LT_SLOTS; ++p) {
            const int s = (int)((h + p) & (LT_SLOTS - 1));
            const int old = atomicCAS(&s_keys[s], -1, l);
            if (old == -1 || old == l) {
                slot = s;
                break;
            }
        }
        if (slot < 0) *s_over = 1;
    }
    return slot;
}

// Non-zero when this lane and its seven neighbours are all counted and agree on the slot (fewer same-address LDS atomics).
__device__ __forceinline__ int lt_agree(int slot, bool in) {
    int same = in ? 1 : 0;
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        const int os = __shfl_xor(slot, m), osame = __shfl_xor(same, m);
        same = same && osame && os == slot;
    }
    return same;
}

// *cell += v of every counted lane: the eight lanes' sum by their lead lane where they agree, else every lane its own. Called by
// all lanes (the shuffles), counted or not.
__device__ __forceinline__ void lt_add(unsigned *cell, unsigned v, int same, bool in) {
    unsigned t = v;
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) t += (unsigned)__shfl_xor((int)t, m);
    if (same) {
        if ((threadIdx.x & 7) == 0) atomicAdd(cell, t);
    } else if (in) {
        atomicAdd(cell, v);
    }
}

// The non-zero cells of s_acc [LT_SLOTS][width] are added into the rows g_rows [K][width] of their slots' labels (a non-zero cell's
// slot has a label). Behind the caller's __syncthreads().
__device__ __forceinline__ void lt_flush(const unsigned *s_acc, const int *s_keys, int width, unsigned long long *g_rows) {
    for (int idx = (int)threadIdx.x; idx < LT_SLOTS * width; idx += LT_THREADS) {
        const int s = idx / width, e = idx - s * width;
        const unsigned v = s_acc[idx];
        if (v) atomicAdd(g_rows + (size_t)s_keys[s] * width + e, (unsigned long long)v);
    }
}
