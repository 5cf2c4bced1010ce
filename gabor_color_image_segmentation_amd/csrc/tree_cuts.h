// tree_cuts.h — what the kernels that walk the cuts of a region tree share (SPEC.md §14, §16, §17, §19): which rows of a merge list
// count and what absorbs every label (step 1), the non-decreasing tau of a list of cuts, the group rep of every label at one cut
// (pointer jumping), and the dense numbering of the groups of the labels in use. Used by rt_cut_kernel (region_tree.hip:
// gcs_region_tree_cut), region_sweep_kernel (scoring.hip: gcs_region_sweep, gcs_region_sweep_under), cut_shapes_pixel_kernel (the tau
// list alone) and cut_shapes_group_kernel (cut_shapes.hip: gcs_cut_shapes) and rp_cuts_kernel (region_props.hip:
// gcs_region_props_cuts). Except rs_taus, which takes any workgroup, every function is called by ALL AG_THREADS threads of a
// workgroup; the LDS arrays belong to the caller.
#pragma once
#include "common.h"

constexpr int AG_WAVES = 16, AG_THREADS = 64 * AG_WAVES;
constexpr int RS_K_MAX = 4096, RS_CUTS_MAX = 64, RS_PER = RS_K_MAX / AG_THREADS;
constexpr unsigned RS_NONE = 0xffffffffu;                      // never absorbed: its row field is above every row index
constexpr int SW_LDS_COUNTERS = 8192;                          // workgroup-private counters of a sweep's pixel pass (32 KiB of LDS)

// Step 1. s_dk[q] = the row that absorbs label q, with its absorber (one LDS word, (row << 12) | absorber), RS_NONE for a label no
// row absorbs. A row counts when it has 0 <= a < b < K and both are reps at that step; which rows count depends on the rows before
// them only, so the rule is iterated from "every well-formed row counts" until nothing changes (a list gcs_region_tree wrote: the
// first check already agrees; any list: at most K - 1 rounds, row t is settled after round t + 1). No serial walk over the rows.
// rows: int32 [n_rows][2] (not read with n_rows = 0). Ends behind a __syncthreads(): s_dk may be read at once.
__device__ __forceinline__ void rs_absorbers(const int32_t *__restrict__ rows, int n_rows, int K, unsigned *s_dk, int *s_changed) {
    const int tid = threadIdx.x;
    int ra[RS_PER], rc[RS_PER];
    unsigned formed = 0;
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
        const int r = tid + j * AG_THREADS;
        ra[j] = rc[j] = 0;
        if (r < n_rows) {
            ra[j] = rows[2 * r];
            rc[j] = rows[2 * r + 1];
            if (ra[j] >= 0 && ra[j] < rc[j] && rc[j] < K) formed |= 1u << j;
        }
    }
    unsigned counted = formed;
    for (;;) {
        for (int q = tid; q < K; q += AG_THREADS) s_dk[q] = RS_NONE;
        if (tid == 0) *s_changed = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RS_PER; ++j)
            if ((counted >> j) & 1u) atomicMin(&s_dk[rc[j]], ((unsigned)(tid + j * AG_THREADS) << 12) | (unsigned)ra[j]);
        __syncthreads();
        unsigned now = 0;
#pragma unroll
        for (int j = 0; j < RS_PER; ++j) {
            const unsigned r = (unsigned)(tid + j * AG_THREADS);
            if (((formed >> j) & 1u) && (s_dk[ra[j]] >> 12) >= r && (s_dk[rc[j]] >> 12) >= r) now |= 1u << j;
        }
        if (now != counted) *s_changed = 1;                    // (every writer stores the same value)
        counted = now;
        __syncthreads();
        const int changed = *s_changed;
        __syncthreads();                                       // everyone has read the flag before the next round clears it
        if (!changed) break;
    }
}

// tau of the cut at R for a tree of `alive` leaves and n_rows merge rows: max(0, alive - R), never past the list.
__device__ __forceinline__ int rs_tau(int alive, int R, int n_rows) {
    const long long want = (long long)alive - (long long)R;
    return (int)(want < 0 ? 0 : want > n_rows ? n_rows : want);
}

// s_tau[c] = tau of cut c, made non-decreasing (an entry of regions that is not below its predecessor repeats its predecessor's cut,
// as in gcs_region_sweep, which keeps a running tau instead). Called by a whole workgroup of at least n_cuts threads, ends behind
// a __syncthreads().
__device__ __forceinline__ void rs_taus(const int32_t *__restrict__ regions, int n_cuts, int alive, int n_rows, int *s_tau) {
    if ((int)threadIdx.x < n_cuts) s_tau[threadIdx.x] = rs_tau(alive, regions[threadIdx.x], n_rows);
    __syncthreads();
    if (threadIdx.x == 0)
        for (int c = 1; c < n_cuts; ++c) s_tau[c] = max(s_tau[c], s_tau[c - 1]);
    __syncthreads();
}

// The group rep of every label with the rows below tau applied: s_root[q] = s_dk[q] names a row < tau ? its absorber : q, then
// pointer jumping, ceil(log2 K) rounds (a chain has at most K - 1 links). Ends behind a __syncthreads().
__device__ __forceinline__ void rs_group_reps(const unsigned *s_dk, unsigned short *s_root, int K, int tau) {
    const int tid = threadIdx.x;
    const int LV = K > 1 ? 32 - __builtin_clz((unsigned)(K - 1)) : 0;
    for (int q = tid; q < K; q += AG_THREADS) {
        const unsigned d = s_dk[q];
        s_root[q] = (d >> 12) < (unsigned)tau ? (unsigned short)(d & 0xfffu) : (unsigned short)q;
    }
    __syncthreads();
    for (int it = 0; it < LV; ++it) {
        unsigned short pp[RS_PER];
#pragma unroll
        for (int j = 0; j < RS_PER; ++j) {
            const int q = tid + j * AG_THREADS;
            pp[j] = q < K ? s_root[s_root[q]] : (unsigned short)0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RS_PER; ++j) {
            const int q = tid + j * AG_THREADS;
            if (q < K) s_root[q] = pp[j];
        }
        __syncthreads();
    }
}

// The groups of the labels in use (bit row s_used), numbered densely in increasing order of their rep: s_group[q] = the number of
// label q's group, -1 for a label not in use. s_rep (the reps' bit row) and s_pref (reps below each word) are scratch of
// ceil(K / 32) words each, no more than the workgroup has threads (a thread zeroes a word: K <= RS_K_MAX gives 128 <= AG_THREADS).
// Ends behind a __syncthreads().
__device__ __forceinline__ void rs_number_groups(const unsigned *s_used, const unsigned short *s_root, int K, unsigned *s_rep,
                                                 unsigned *s_pref, short *s_group) {
    const int tid = threadIdx.x, KW = (K + 31) >> 5;
    if (tid < KW) s_rep[tid] = 0u;
    __syncthreads();
    for (int q = tid; q < K; q += AG_THREADS)
        if ((s_used[q >> 5] >> (q & 31)) & 1u) {
            const unsigned r = s_root[q];
            atomicOr(&s_rep[r >> 5], 1u << (r & 31));
        }
    __syncthreads();
    if (tid == 0) {
        unsigned acc = 0;
        for (int w = 0; w < KW; ++w) {
            s_pref[w] = acc;
            acc += (unsigned)__popc(s_rep[w]);
        }
    }
    __syncthreads();
    for (int q = tid; q < K; q += AG_THREADS) {
        const unsigned r = s_root[q];
        const bool used = (s_used[q >> 5] >> (q & 31)) & 1u;
        s_group[q] = used ? (short)(s_pref[r >> 5] + (unsigned)__popc(s_rep[r >> 5] & ((1u << (r & 31)) - 1u))) : (short)-1;
    }
    __syncthreads();
}
