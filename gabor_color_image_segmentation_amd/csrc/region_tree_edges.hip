// region_tree_edges.hip — SPEC.md §23: the region tree merged by boundary strength, built from an edge table of §20 (gfx950 only).
//
// Nodes = the labels 0 .. K-1 whose `used` word is not 0; an edge (A, B) between two groups carries l = the crossings and s = the
// strength summed over the leaf edges between them; cost(A, B) = floor(128 s / l), computed as 128 q + floor(128 r / l) with
// s = q l + r. Rounds, ties, merge list and outputs are §14's: every node picks the adjacent node of least (cost, rep), mutual picks
// merge, the round's merges are listed in (cost, smaller rep) order. No node statistics, no features, no float: integer adds and
// minima of packed keys, so any execution order gives the same bits.
//   te_used_kernel   (gcs_label_used) one workgroup per image marks the labels of a map that own a pixel: the `used` table for a
//                    caller that has no per-label count on the device.
//   te_merge_kernel  (gcs_region_tree_edges) ONE workgroup of 1024 threads per image runs every round; only workgroup barriers.
//                    LDS: per node the pick, one packed word cost << 12 | target (a cost is below 2^40, a label below 2^12), taken
//                    with a 64-bit LDS atomic min from a sweep over the live edges; the rep table (a node that died in this round:
//                    who absorbed it); the round's pair list as packed words cost << 12 | smaller rep, whose rank is the pair's row.
//                    Workspace (L2): the live edges in an open-addressing table, key a << 12 | b (32 bits), columns l and s, and
//                    its twin. After a round's merges the table is rebuilt into the twin: every live edge maps its ends through the
//                    rep table, drops itself if they coincide, else claims (32-bit CAS) or finds the slot of its new key and adds
//                    its columns there: parallel edges sum. The twin is cleared and sized for the edges that are live BEFORE the
//                    round (a power of two of at least twice their number, at least 64): contraction never adds an edge, so a
//                    table is never more than half full and a probe never fails; every probe loop is bounded by the table size all
//                    the same. A round costs O(slots of the table) = O(live edges) loads per sweep, two sweeps and one clear, plus
//                    O(pairs^2 / 1024) LDS reads for the ranks: the tables shrink with the graph.
//                    Every access to a table bypasses the CU's L1 (relaxed agent-scope loads and stores, atomics at L2). A phase
//                    that wrote a table ends with te_sync: every wave waits until its own stores and atomics are acknowledged
//                    (s_waitcnt vmcnt(0): a workgroup barrier alone does not wait for them, and a later wave's load could pass an
//                    add that is still on its way), then the barrier; no cache is written back or invalidated.
// No allocation, no host synchronisation: the launches sit on the caller's stream (and inside a captured graph).
#include "common.h"

namespace {

constexpr int TE_T = 1024;                   // threads of the merge workgroup
constexpr int TE_K_MAX = 4096, TE_E_MAX = 16384, TE_HW_MAX = 4096;
constexpr int TE_S_MIN = 64;                 // smallest table

typedef unsigned long long u64;
constexpr unsigned TE_FREE = 0xffffffffu;    // no key (a key is below 2^24)
constexpr u64 TE_NONE = ~0ull;               // no pick
constexpr unsigned TE_UNUSED = 0xffffu;      // rep entry of a label that owns no pixel

__host__ __device__ inline int te_slots(int n) {   // the table of n edges: a power of two >= max(64, 2 n)
    int s = TE_S_MIN;
    while (s < 2 * n) s <<= 1;
    return s;
}
__host__ __device__ inline int te_bits(int s) { return 31 - __builtin_clz((unsigned)s); }

__host__ __device__ inline size_t te_lds_bytes(int K) { return 32 + (size_t)8 * K + (size_t)8 * (K / 2 + 1) + (size_t)2 * K; }

template <class T> __device__ __forceinline__ T te_ld(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> __device__ __forceinline__ void te_st(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the end of a phase that wrote a table (see the head of the file)
__device__ __forceinline__ void te_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

struct TeTable {
    unsigned *keys;                          // [S]
    u64 *len, *str;                          // [S] each
};

__device__ __forceinline__ void te_clear(const TeTable &T, int S, int tid) {
    for (int s = tid; s < S; s += TE_T) {
        te_st(T.keys + s, TE_FREE);
        te_st(T.len + s, 0ull);
        te_st(T.str + s, 0ull);
    }
}

__device__ __forceinline__ unsigned te_hash(unsigned key, int bits) { return (key * 0x9E3779B1u) >> (32 - bits); }

// adds (l, s) into the slot of `key`, claimed if it is new (*claimed counts the keys of the table)
__device__ __forceinline__ void te_insert(const TeTable &T, int S, int bits, unsigned key, u64 l, u64 s, int *claimed) {
    const unsigned mask = (unsigned)S - 1u, h = te_hash(key, bits);
    for (int q = 0; q < S; ++q) {
        const unsigned sl = (h + (unsigned)q) & mask;
        unsigned cur = te_ld(T.keys + sl);
        if (cur == TE_FREE) {
            cur = atomicCAS(T.keys + sl, TE_FREE, key);
            if (cur == TE_FREE) {
                atomicAdd(claimed, 1);
                cur = key;
            }
        }
        if (cur == key) {
            atomicAdd(T.len + sl, l);
            atomicAdd(T.str + sl, s);
            return;
        }
    }
}

// floor(128 s / l) = 128 q + floor(128 r / l), s = q l + r, without overflow (l < 2^57; l = 0, which no table of §20 holds, counts
// as 1): one division, a 32-bit one where both fit (every table of a real image), then seven steps of binary long division
__device__ __forceinline__ u64 te_cost(u64 l, u64 s) {
    if (l == 0) l = 1;
    u64 q, r;
    if (((l | s) >> 32) == 0) {
        const unsigned q32 = (unsigned)s / (unsigned)l;
        q = q32, r = (unsigned)s - q32 * (unsigned)l;
    } else {
        q = s / l, r = s - q * l;
    }
    unsigned f = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        r <<= 1, f <<= 1;
        if (r >= l) r -= l, f |= 1u;
    }
    return (q << 7) | f;
}

constexpr int TE_U = 4;                      // slots a thread has in flight in a sweep

// TE_U slots of a table per thread, all loads issued before the first is used: key (TE_FREE past the end), l, s
__device__ __forceinline__ void te_load(const TeTable &T, int S, int s0, int tid, unsigned *k, u64 *l, u64 *st) {
#pragma unroll
    for (int j = 0; j < TE_U; ++j) {
        const int s = s0 + j * TE_T + tid;
        const int sc = s < S ? s : 0;                                      // (slot 0 exists: a read that is thrown away)
        k[j] = te_ld(T.keys + sc), l[j] = te_ld(T.len + sc), st[j] = te_ld(T.str + sc);
        if (s >= S) k[j] = TE_FREE;
    }
}

__global__ __launch_bounds__(TE_T) void te_merge_kernel(const int32_t *__restrict__ edges, const u64 *__restrict__ vals,
                                                        const int32_t *__restrict__ count, const int32_t *__restrict__ used, int K,
                                                        int E_cap, int S_max, unsigned char *ws, int32_t *merges, u64 *costs,
                                                        int32_t *alive_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char te_lds[];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    int *s_cnt = reinterpret_cast<int *>(te_lds);                          // [0] alive, [1] pairs of the round, [2] keys of the table
                                                                           // being filled, [3] labels in use (largest + 1)
    u64 *s_pick = reinterpret_cast<u64 *>(te_lds + 32);                    // [K] cost << 12 | target
    u64 *s_pkey = s_pick + K;                                              // [K / 2 + 1] cost << 12 | smaller rep of a mutual pair
    uint16_t *s_rep = reinterpret_cast<uint16_t *>(s_pkey + (K / 2 + 1));  // [K] q: live; a node that died in this round: its absorber
    used += (size_t)b * K;
    if (K > 1) merges += (size_t)b * (K - 1) * 2;
    if (costs) costs += (size_t)b * (K - 1);
    TeTable cur, nxt;
    {
        unsigned char *w = ws + (size_t)b * S_max * 40;                    // four uint64 columns, then two key arrays
        cur.len = reinterpret_cast<u64 *>(w), cur.str = cur.len + S_max;
        nxt.len = cur.str + S_max, nxt.str = nxt.len + S_max;
        cur.keys = reinterpret_cast<unsigned *>(nxt.str + S_max), nxt.keys = cur.keys + S_max;
    }

    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    for (int q = tid; q < K; q += TE_T) {
        const bool u = used[q] != 0;
        s_rep[q] = u ? (uint16_t)q : (uint16_t)TE_UNUSED;
        if (u) {
            atomicAdd(&s_cnt[0], 1);
            atomicMax(&s_cnt[3], q + 1);
        }
    }
    int n = count[b];
    const bool table = n >= 0 && n <= E_cap;                               // count = -1: no leaf table (SPEC.md §20 overflow)
    if (!table) n = 0;
    int S = te_slots(n), bits = te_bits(S);
    te_clear(cur, S, tid);
    te_sync();
    int alive = s_cnt[0], base = 0;
    const int Ku = s_cnt[3];
    if (tid == 0) alive_out[b] = alive;
    const int32_t *e = edges + (size_t)b * E_cap * 2;
    const u64 *v = vals + (size_t)b * E_cap * 3;
    for (int i = tid; i < n; i += TE_T) {                                  // the leaf rows: length and strength; contrast is not read
        const int a0 = e[2 * i], b0 = e[2 * i + 1];
        if ((unsigned)a0 >= (unsigned)K || (unsigned)b0 >= (unsigned)K || a0 == b0) continue;
        if (s_rep[a0] == TE_UNUSED || s_rep[b0] == TE_UNUSED) continue;
        const unsigned key = ((unsigned)min(a0, b0) << 12) | (unsigned)max(a0, b0);
        te_insert(cur, S, bits, key, v[3 * (size_t)i], v[3 * (size_t)i + 2], &s_cnt[2]);
    }
    te_sync();
    int n_cur = s_cnt[2];

    while (alive > 1 && n_cur > 0) {
        for (int q = tid; q < Ku; q += TE_T) s_pick[q] = TE_NONE;
        if (tid == 0) s_cnt[1] = 0;
        __syncthreads();
        // pick: every live edge offers itself to both of its ends
        for (int s0 = 0; s0 < S; s0 += TE_U * TE_T) {
            unsigned k[TE_U];
            u64 l[TE_U], st[TE_U];
            te_load(cur, S, s0, tid, k, l, st);
#pragma unroll
            for (int j = 0; j < TE_U; ++j) {
                if (k[j] == TE_FREE) continue;
                const u64 c = te_cost(l[j], st[j]) << 12;
                const unsigned a = k[j] >> 12, bb = k[j] & 0xfffu;
                atomicMin(&s_pick[a], c | bb);
                atomicMin(&s_pick[bb], c | a);
            }
        }
        __syncthreads();
        // mutual pairs, listed by (cost, smaller rep)
        for (int q = tid; q < Ku; q += TE_T) {
            const u64 p = s_pick[q];
            if (p == TE_NONE) continue;
            const unsigned t = (unsigned)(p & 0xfffu);
            if ((unsigned)q < t && (unsigned)(s_pick[t] & 0xfffu) == (unsigned)q) s_pkey[atomicAdd(&s_cnt[1], 1)] = (p & ~0xfffull) | (u64)q;
        }
        __syncthreads();
        const int P = s_cnt[1];
        if (P == 0) break;                                                 // (never with a live edge: the cheapest edge is mutual)
        for (int i = tid; i < P; i += TE_T) {
            const u64 key = s_pkey[i];
            int rank = 0;
            for (int j = 0; j < P; ++j) rank += s_pkey[j] < key ? 1 : 0;
            const unsigned a = (unsigned)(key & 0xfffu), t = (unsigned)(s_pick[a] & 0xfffu);
            merges[2 * (base + rank)] = (int)a;
            merges[2 * (base + rank) + 1] = (int)t;
            if (costs) costs[base + rank] = key >> 12;
            s_rep[t] = (uint16_t)a;
        }
        const int Sn = te_slots(n_cur), bn = te_bits(Sn);                  // the edges live now bound the edges of the next table
        te_clear(nxt, Sn, tid);
        if (tid == 0) s_cnt[2] = 0;
        te_sync();
        // contract: the edges of a dead node move to its rep, parallel edges add up, the pair's own edge disappears
        for (int s0 = 0; s0 < S; s0 += TE_U * TE_T) {
            unsigned k[TE_U];
            u64 l[TE_U], st[TE_U];
            te_load(cur, S, s0, tid, k, l, st);
#pragma unroll
            for (int j = 0; j < TE_U; ++j) {
                if (k[j] == TE_FREE) continue;
                const unsigned a = s_rep[k[j] >> 12], bb = s_rep[k[j] & 0xfffu];
                if (a != bb) te_insert(nxt, Sn, bn, (min(a, bb) << 12) | max(a, bb), l[j], st[j], &s_cnt[2]);
            }
        }
        te_sync();
        n_cur = s_cnt[2];
        const TeTable t = cur;
        cur = nxt, nxt = t;
        S = Sn, bits = bn;
        alive -= P;
        base += P;
    }
    for (int t = base + tid; t < K - 1; t += TE_T) {                       // rows no merge filled
        merges[2 * t] = -1;
        merges[2 * t + 1] = -1;
        if (costs) costs[t] = 0;
    }
}

__global__ __launch_bounds__(TE_T) void te_used_kernel(const int32_t *__restrict__ labels, int H, int W, int K, int32_t *used) {
    __shared__ unsigned s_used[TE_K_MAX / 32];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const size_t hw = (size_t)H * W;
    labels += (size_t)b * hw;
    if (tid < TE_K_MAX / 32) s_used[tid] = 0u;
    __syncthreads();
    for (size_t p = tid; p < hw; p += TE_T) {
        const int l = labels[p];
        if ((unsigned)l < (unsigned)K && !(s_used[l >> 5] & (1u << (l & 31)))) atomicOr(&s_used[l >> 5], 1u << (l & 31));
    }
    __syncthreads();
    for (int q = tid; q < K; q += TE_T) used[(size_t)b * K + q] = (int32_t)((s_used[q >> 5] >> (q & 31)) & 1u);
}

bool te_shape_ok(int B, int K, int E_cap) { return B >= 1 && B <= 65535 && K >= 1 && K <= TE_K_MAX && E_cap >= 1 && E_cap <= TE_E_MAX; }

}  // namespace

extern "C" size_t gcs_region_tree_edges_workspace_bytes(int B, int K, int E_cap) {
    if (!te_shape_ok(B, K, E_cap)) return 0;
    return (size_t)B * te_slots(E_cap) * 40;
}

extern "C" int gcs_region_tree_edges(const int32_t *edges, const uint64_t *vals, const int32_t *count, const int32_t *used, int B, int K,
                                     int E_cap, void *workspace, int32_t *merges_out, uint64_t *costs_out, int32_t *alive_out,
                                     gcs_stream_t stream) {
    if (!edges || !vals || !count || !used || !workspace || !alive_out || (K > 1 && !merges_out))
        return gcs_fail(GCS_EINVAL, "gcs_region_tree_edges: NULL pointer");
    if (!te_shape_ok(B, K, E_cap))
        return gcs_fail(GCS_EINVAL, "gcs_region_tree_edges: bad shape (1 <= B <= 65535, 1 <= K <= 4096, 1 <= E_cap <= 16384)");
    hipLaunchKernelGGL(te_merge_kernel, dim3(B), dim3(TE_T), te_lds_bytes(K), static_cast<hipStream_t>(stream), edges,
                       reinterpret_cast<const u64 *>(vals), count, used, K, E_cap, te_slots(E_cap), static_cast<unsigned char *>(workspace),
                       merges_out, reinterpret_cast<u64 *>(costs_out), alive_out);
    GCS_CHECK_LAUNCH("gcs_region_tree_edges");
    return GCS_OK;
}

extern "C" int gcs_label_used(const int32_t *labels, int B, int H, int W, int K, int32_t *used_out, gcs_stream_t stream) {
    if (!labels || !used_out) return gcs_fail(GCS_EINVAL, "gcs_label_used: NULL pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > TE_HW_MAX || W > TE_HW_MAX || K < 1 || K > TE_K_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_label_used: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 1 <= K <= 4096)");
    hipLaunchKernelGGL(te_used_kernel, dim3(B), dim3(TE_T), 0, static_cast<hipStream_t>(stream), labels, H, W, K, used_out);
    GCS_CHECK_LAUNCH("gcs_label_used");
    return GCS_OK;
}
