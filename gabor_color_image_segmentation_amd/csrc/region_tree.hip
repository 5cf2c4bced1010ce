// region_tree.hip — SPEC.md §14: agglomerative merging of a label map's regions on their adjacency graph (gfx950 only).
//
// Nodes = the labels 0 .. K-1 that own a pixel; state per node = pixel count n, exact feature sums S_d, mean m_d = floor((2 S_d + n) /
// (2 n)); cost(A, B) = sum_d (m_A,d - m_B,d)^2 * min(n_A, n_B) in unsigned 64 bits (< 2^62); per round every node picks the adjacent
// node of least (cost, rep), mutual picks merge, the round's merges are listed in (cost, rep) order. One call enqueues
//   rt_zero_kernel      the [K][D + 1] uint64 sums and the K x K adjacency bit matrix of every image := 0.
//   rt_stats_kernel     one workgroup per 8 x 32 pixel tile, one thread per pixel: ONE read of the canonical tensor and of the label
//                       map. Sums: the tile accumulator of label_tile.h, shared with rp_stats_kernel (region_props.hip), rows
//                       [D sums, n]; a tile that sees more than 32 labels adds straight into the global rows (slow, exact).
//                       Adjacency: a pixel whose right / lower neighbour carries another in-range label sets bits (a, b) and (b, a)
//                       (an atomic OR only when the bit is not seen set: every later pixel of the same border reads and skips).
//   rt_stats_slab_kernel  the same tile, labels, adjacency and accumulator with the values read from the FEATURE SLAB (SPEC.md §21,
//                       gcs_region_tree_slab): a pixel locates its block and slot once (gcs_locate), then steps plane by plane through
//                       its tile, every level at its own resolution (the 2^L x 2^L pixels of a level-L slot read the same bytes and
//                       each adds the value to its own label); sums and bits equal rt_stats_kernel's on gcs_features_unpack of the slab.
//   rt_merge_kernel     ONE workgroup of 1024 threads per image runs every round (the trip count is data, so the loop lives here):
//                       pick (a wave per node whose neighbourhood changed: it walks the node's adjacency row, lanes over the planes of a cost), mutual pairs,
//                       rank of every pair in (cost, rep) order = its row of the merge list, merge (sums, mean, adjacency row OR),
//                       remap (the merged node's neighbours drop the dead label's bit, gain the rep's, and pick again next round).
//                       Picks, costs, pair list and flags sit in LDS, the means too where they fit beside them; sums and adjacency
//                       stay in the workspace (L2). Only workgroup barriers: images are independent.
// and gcs_region_tree_cut one launch: a workgroup per image walks the list as every cut kernel does (tree_cuts.h: rs_absorbers, then
// rs_group_reps at tau = alive - R: a row counts when 0 <= a < b < K and both are still reps), marks the labels in use, numbers
// their groups in increasing order of rep (rs_number_groups) and relabels.
// No allocation, no host synchronisation: every launch sits on the caller's stream (and inside a captured graph).
#include <algorithm>

#include "common.h"
#include "label_tile.h"
#include "slab_slots.h"
#include "tree_cuts.h"

namespace {

constexpr int RT_D_MAX = 207, RT_K_MAX = RS_K_MAX, RT_HW_MAX = 4096;
constexpr int RT_T = 1024, RT_NW = RT_T / 64;   // merge / contour-prepare workgroup
constexpr unsigned RT_NONE = 0xffffu;        // "no adjacent node" (a label is below 4096)
constexpr size_t RT_LDS_MAX = 65536;

typedef unsigned long long u64;

struct RtArgs {
    const uint16_t *feats;                   // [B][D][H][W]
    const int *labels;                       // [B][H][W]
    u64 *sums;                               // [B][K][D + 1] = the D feature sums, count
    unsigned *adj;                           // [B][K][KW] bit (a, b): a and b are adjacent
    uint16_t *mean;                          // [B][K][D] (used when the means do not fit LDS)
    int *merges;                             // [B][K - 1][2]
    u64 *costs;                              // [B][K - 1] or NULL
    int *alive;                              // [B]
    int B, H, W, D, K, KW;
};

__host__ __device__ inline size_t rt_align(size_t n) { return (n + 255) & ~(size_t)255; }

__device__ __forceinline__ unsigned rt_ld(const unsigned *p) {             // a word other waves change with atomics: read it in L2
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void rt_zero_kernel(uint4 *p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ void rt_edge(unsigned *adj, int KW, int a, int b) {
    unsigned *wa = adj + (size_t)a * KW + (b >> 5), *wb = adj + (size_t)b * KW + (a >> 5);
    const unsigned ba = 1u << (b & 31), bb = 1u << (a & 31);
    if (!(rt_ld(wa) & ba)) atomicOr(wa, ba);                               // (read in L2, where the atomics land)
    if (!(rt_ld(wb) & bb)) atomicOr(wb, bb);
}

// What the two statistics kernels do before they read a value: the tile accumulator of label_tile.h cleared, this thread's pixel
// (clamped past the edge) and label, the adjacency bits of its right and lower pair, its label's slot. Returns the slot; the slots
// and *s_over are settled for the workgroup (a __syncthreads() has passed).
struct RtPixel {
    int y, x, l;
    bool in;                                 // inside the image with a label in 0 .. K-1: a label outside is counted nowhere
};
__device__ __forceinline__ int rt_tile_begin(const RtArgs &A, int b, unsigned *s_acc, int *s_keys, int *s_over, RtPixel *px) {
    const int E = A.D + 1, K = A.K;
    lt_clear(s_acc, E, s_keys, s_over);
    __syncthreads();
    const size_t hw = (size_t)A.H * A.W;
    int y, x;
    const bool valid = lt_pixel(A.H, A.W, &y, &x);
    const int *lab = A.labels + (size_t)b * hw + (size_t)y * A.W + x;
    const int l = *lab;
    const bool in = valid && (unsigned)l < (unsigned)K;
    unsigned *adj = A.adj + (size_t)b * K * A.KW;
    if (in) {
        if (x + 1 < A.W) {
            const int r = lab[1];
            if (r != l && (unsigned)r < (unsigned)K) rt_edge(adj, A.KW, l, r);
        }
        if (y + 1 < A.H) {
            const int r = lab[A.W];
            if (r != l && (unsigned)r < (unsigned)K) rt_edge(adj, A.KW, l, r);
        }
    }
    const int slot = lt_claim(s_keys, s_over, l, in);
    __syncthreads();
    px->y = y, px->x = x, px->l = l, px->in = in;
    return slot;
}

__global__ __launch_bounds__(LT_THREADS) void rt_stats_kernel(RtArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned rt_smem[];
    const int b = (int)blockIdx.z, D = A.D, E = D + 1, K = A.K;
    unsigned *s_acc = rt_smem;                                             // [LT_SLOTS][E]
    int *s_keys = reinterpret_cast<int *>(s_acc + LT_SLOTS * E);          // [LT_SLOTS] label of the slot, -1: free
    int *s_over = s_keys + LT_SLOTS;                                       // more labels than slots
    RtPixel p;
    const int slot = rt_tile_begin(A, b, s_acc, s_keys, s_over, &p);
    const int y = p.y, x = p.x, l = p.l;
    const bool in = p.in;
    const size_t hw = (size_t)A.H * A.W;
    const uint16_t *px = A.feats + (size_t)b * D * hw + (size_t)y * A.W + x;
    u64 *g_sums = A.sums + (size_t)b * K * E;
    if (*s_over) {                                                         // (uniform over the workgroup)
        if (in) {
            u64 *row = g_sums + (size_t)l * E;
            for (int d = 0; d < D; ++d) atomicAdd(row + d, (u64)px[(size_t)d * hw]);
            atomicAdd(row + D, 1ull);
        }
        return;
    }
    const int same = lt_agree(slot, in);
    unsigned *row = s_acc + (in ? slot : 0) * E;
    for (int d = 0; d < E; ++d) lt_add(row + d, d < D ? px[(size_t)d * hw] : 1u, same, in);
    __syncthreads();
    lt_flush(s_acc, s_keys, E, g_sums);
}

// The D values of one pixel in the slab of its image, handed to f(column of the sums row = logical feature, value): physical plane
// order (level, channel, filter in level), a plane step inside the tile is a constant per level. Split slab: low byte, MID nibble
// and, in a tile whose level flag is set, TOP nibble (a plane is a multiple of the nibble group: byte += half a plane, same shift).
template <class F>
__device__ __forceinline__ void rt_slab_walk(const GcsLayout &lo, const unsigned char *img, int y, int x, F f) {
    int blk, iy, ix;
    gcs_locate(lo, y, x, blk, iy, ix);
    const unsigned tile = (unsigned)(blk >> 2), q = (unsigned)(blk & 3);
    for (int L = 0; L < lo.n_levels; ++L) {
        const unsigned side = 8u >> L, npl = (unsigned)KP_TP >> (2 * L);
        const int FL = lo.FL[L], col0 = 2 * L * lo.n_orient;
        if (lo.split) {
            unsigned slot = tile * (unsigned)lo.S + (unsigned)lo.sl0[L] + ((unsigned)iy >> L) * 4u * side + q * side + ((unsigned)ix >> L);
            unsigned nb;
            int sh;
            sm_nibble(L, slot, nb, sh);
            const bool top = img[lo.flag_off + 4u * tile + (unsigned)L] != 0;
            for (int c = 0; c < 3; ++c)
                for (int fl = 0; fl < FL; ++fl, slot += npl, nb += npl >> 1) {
                    unsigned v = (img[slot] ^ 0x80u) | (((unsigned)img[lo.mid_off + nb] >> sh & 15u) << 8);
                    if (top) v |= ((unsigned)img[lo.top_off + nb] >> sh & 15u) << 12;
                    f(c * lo.F + col0 + fl, v);
                }
        } else {
            const unsigned char *p = img + (size_t)tile * lo.tile_bytes + lo.off[L] +
                                     (size_t)(q * side * side + ((unsigned)iy >> L) * side + ((unsigned)ix >> L)) * 2;
            for (int c = 0; c < 3; ++c)
                for (int fl = 0; fl < FL; ++fl, p += 2 * npl)
                    f(c * lo.F + col0 + fl, (unsigned)*reinterpret_cast<const uint16_t *>(p) ^ 0x8080u);
        }
    }
}

__global__ __launch_bounds__(LT_THREADS) void rt_stats_slab_kernel(RtArgs A, GcsLayout lo, const unsigned char *slab) {
    extern __shared__ __attribute__((aligned(16))) unsigned rt_smem[];
    const int b = (int)blockIdx.z, D = A.D, E = D + 1, K = A.K;
    unsigned *s_acc = rt_smem;                                             // [LT_SLOTS][E]
    int *s_keys = reinterpret_cast<int *>(s_acc + LT_SLOTS * E);          // [LT_SLOTS] label of the slot, -1: free
    int *s_over = s_keys + LT_SLOTS;                                       // more labels than slots
    RtPixel p;
    const int slot = rt_tile_begin(A, b, s_acc, s_keys, s_over, &p);
    const int y = p.y, x = p.x, l = p.l;
    const bool in = p.in;
    const unsigned char *img = slab + (size_t)b * (size_t)lo.img_bytes;    // (a clamped pixel past the edge reads inside the image)
    u64 *g_sums = A.sums + (size_t)b * K * E;
    if (*s_over) {                                                         // (uniform over the workgroup)
        if (in) {
            u64 *row = g_sums + (size_t)l * E;
            rt_slab_walk(lo, img, y, x, [&](int d, unsigned v) { atomicAdd(row + d, (u64)v); });
            atomicAdd(row + D, 1ull);
        }
        return;
    }
    const int same = lt_agree(slot, in);
    unsigned *row = s_acc + (in ? slot : 0) * E;
    rt_slab_walk(lo, img, y, x, [&](int d, unsigned v) { lt_add(row + d, v, same, in); });
    lt_add(row + D, 1u, same, in);
    __syncthreads();
    lt_flush(s_acc, s_keys, E, g_sums);
}

// LDS of the merge kernel: 16 bytes of counters, then per node the pick's cost (8 bytes) and target (2), a slot of the pair list (2)
// and a flag byte (bit 0: alive, bit 1: picks again), then the means where they fit.
__host__ __device__ inline size_t rt_state_bytes(int K) { return (16 + (size_t)13 * K + 15) & ~(size_t)15; }

// sum_d (ma_d - mb_d)^2 by one wave, the planes spread over its lanes; every lane returns the sum
__device__ __forceinline__ u64 rt_delta(const uint16_t *ma, const uint16_t *mb, int D, int lane) {
    u64 acc = 0;
    if ((D & 1) == 0) {                                                    // rows of an even D start on a 32-bit boundary: two planes per load
        const unsigned *pa = reinterpret_cast<const unsigned *>(ma), *pb = reinterpret_cast<const unsigned *>(mb);
        for (int i = lane; i < (D >> 1); i += 64) {
            const unsigned va = pa[i], vb = pb[i];
            const int d0 = (int)(va & 0xffffu) - (int)(vb & 0xffffu), d1 = (int)(va >> 16) - (int)(vb >> 16);
            acc += (u64)((unsigned)(d0 * d0) + (unsigned)(d1 * d1));      // 2 * 46 340^2 < 2^32 (a mean is at most 46 340)
        }
    } else {
        for (int d = lane; d < D; d += 64) {
            const int df = (int)ma[d] - (int)mb[d];
            acc += (u64)(unsigned)(df * df);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    return acc;
}

__global__ __launch_bounds__(RT_T) void rt_merge_kernel(RtArgs A, int mean_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rt_lds[];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = A.K, D = A.D, E = D + 1, KW = A.KW;
    int *s_cnt = reinterpret_cast<int *>(rt_lds);                          // [0] alive, [1] pairs of the round, [2] labels in use
    u64 *s_cost = reinterpret_cast<u64 *>(rt_lds + 16);                    // [K]
    uint16_t *s_t = reinterpret_cast<uint16_t *>(rt_lds + 16 + (size_t)8 * K);      // [K] the pick; of a dead node: who absorbed it
    uint16_t *s_pair = reinterpret_cast<uint16_t *>(rt_lds + 16 + (size_t)10 * K);  // [K] the smaller rep of every mutual pair
    unsigned char *s_flag = rt_lds + 16 + (size_t)12 * K;                  // [K]
    u64 *sums = A.sums + (size_t)b * K * E;
    unsigned *adj = A.adj + (size_t)b * K * KW;
    uint16_t *mean = mean_in_lds ? reinterpret_cast<uint16_t *>(rt_lds + rt_state_bytes(K)) : A.mean + (size_t)b * K * D;
    int *merges = A.merges + (size_t)b * (K - 1) * 2;
    u64 *costs = A.costs ? A.costs + (size_t)b * (K - 1) : nullptr;

    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    for (int q = tid; q < K; q += RT_T) {
        const u64 n = sums[(size_t)q * E + D];
        s_flag[q] = n ? 3 : 0;
        s_t[q] = (uint16_t)RT_NONE;
        s_cost[q] = 0;
        if (n) {
            atomicAdd(&s_cnt[0], 1);
            atomicMax(&s_cnt[2], q + 1);
        }
    }
    __syncthreads();
    // Labels >= Ku own no pixel: they are never alive, never adjacent (rt_stats_kernel sets bits between labels of pixels only) and
    // never picked, so every walk over nodes or over the words of an adjacency row may stop at Ku / KWu (the rows keep their stride
    // KW). With K at a capacity far above the labels in use (SPEC.md §18: K = 4096 for about 1200 nodes) the rounds cost what the
    // nodes cost; results are the same bits for every input.
    const int Ku = s_cnt[2], KWu = (Ku + 31) >> 5;
    for (int idx = tid; idx < Ku * D; idx += RT_T) {
        const int q = idx / D, d = idx - q * D;
        const u64 n = sums[(size_t)q * E + D];
        mean[idx] = n ? (uint16_t)((2 * sums[(size_t)q * E + d] + n) / (2 * n)) : (uint16_t)0;
    }
    for (int t = tid; t < K - 1; t += RT_T) {
        merges[2 * t] = -1;
        merges[2 * t + 1] = -1;
        if (costs) costs[t] = 0;
    }
    __threadfence();
    __syncthreads();
    int alive = s_cnt[0], base = 0;
    if (tid == 0) A.alive[b] = alive;

    while (alive > 1) {
        // pick: the adjacent node of least (cost, rep), for every node whose neighbourhood changed (all of them in round one)
        for (int q = wave; q < Ku; q += RT_NW) {
            if (s_flag[q] != 3) continue;                                  // (uniform over the wave)
            const u64 nq = sums[(size_t)q * E + D];
            u64 best = ~0ull;
            unsigned bt = RT_NONE;
            for (int w0 = 0; w0 < KWu; w0 += 64) {                         // the row's words, 64 at a time; the wave then walks the set bits
                const unsigned mine = w0 + lane < KWu ? rt_ld(adj + (size_t)q * KW + w0 + lane) : 0u;
                u64 nz = __ballot(mine != 0u);
                while (nz) {
                    const int src = __ffsll((long long)nz) - 1;
                    nz &= nz - 1;
                    unsigned bits = (unsigned)__shfl((int)mine, src);
                    while (bits) {                                         // (uniform: every lane holds the same word)
                        const unsigned r = (unsigned)(32 * (w0 + src) + __ffs((int)bits) - 1);
                        bits &= bits - 1;
                        const u64 nr = sums[(size_t)r * E + D];
                        const u64 c = rt_delta(mean + (size_t)q * D, mean + (size_t)r * D, D, lane) * (nq < nr ? nq : nr);
                        if (c < best || (c == best && r < bt)) {
                            best = c;
                            bt = r;
                        }
                    }
                }
            }
            if (lane == 0) {
                s_cost[q] = best;
                s_t[q] = (uint16_t)bt;
                s_flag[q] = 1;
            }
        }
        __syncthreads();
        // mutual pairs, listed by their smaller rep
        for (int q = tid; q < Ku; q += RT_T) {
            if (!(s_flag[q] & 1)) continue;
            const unsigned t = s_t[q];
            if (t != RT_NONE && (unsigned)q < t && s_t[t] == (unsigned)q) s_pair[atomicAdd(&s_cnt[1], 1)] = (uint16_t)q;
        }
        __syncthreads();
        const int P = s_cnt[1];
        if (P == 0) break;                                                 // out-of-range labels cut the graph apart: nothing is adjacent
        // the round's rows of the merge list: a pair's rank in (cost, smaller rep) order
        for (int i = tid; i < P; i += RT_T) {
            const unsigned a = s_pair[i];
            const u64 c = s_cost[a];
            int rank = 0;
            for (int j = 0; j < P; ++j) {
                const unsigned aj = s_pair[j];
                const u64 cj = s_cost[aj];
                rank += (cj < c || (cj == c && aj < a)) ? 1 : 0;
            }
            merges[2 * (base + rank)] = (int)a;
            merges[2 * (base + rank) + 1] = (int)s_t[a];
            if (costs) costs[base + rank] = c;
        }
        // merge: a wave per pair (a < bq): sums add, the mean follows, a's adjacency row takes bq's bits
        for (int i = wave; i < P; i += RT_NW) {
            const unsigned a = s_pair[i], bq = s_t[a];
            const u64 n = sums[(size_t)a * E + D] + sums[(size_t)bq * E + D];
            for (int e = lane; e < D; e += 64) {
                const u64 s = sums[(size_t)a * E + e] + sums[(size_t)bq * E + e];
                sums[(size_t)a * E + e] = s;
                mean[(size_t)a * D + e] = (uint16_t)((2 * s + n) / (2 * n));
            }
            if (lane == 0) sums[(size_t)a * E + D] = n;
            for (int w = lane; w < KWu; w += 64) {
                const unsigned v = rt_ld(adj + (size_t)bq * KW + w);
                if (v) atomicOr(adj + (size_t)a * KW + w, v);
            }
        }
        __threadfence();
        __syncthreads();
        for (int i = tid; i < P; i += RT_T) {
            const unsigned a = s_pair[i];
            s_flag[s_t[a]] = 0;
            s_flag[a] = 3;
        }
        __syncthreads();
        // remap: every neighbour c of the merged node drops bq's bit, gains a's and picks again; a neighbour that died in this round
        // stands for the node that absorbed it. Rows of living nodes hold bits of living nodes only when the round ends.
        for (int i = wave; i < P; i += RT_NW) {
            const unsigned a = s_pair[i], bq = s_t[a];
            for (int w = lane; w < KWu; w += 64) {
                unsigned bits = rt_ld(adj + (size_t)a * KW + w);
                while (bits) {
                    const unsigned c = (unsigned)(32 * w + __ffs((int)bits) - 1);
                    bits &= bits - 1;
                    if (c == a || c == bq) continue;
                    const unsigned cc = (s_flag[c] & 1) ? c : s_t[c];
                    if (cc == a || cc >= (unsigned)K) continue;
                    atomicAnd(adj + (size_t)cc * KW + (bq >> 5), ~(1u << (bq & 31)));
                    atomicOr(adj + (size_t)cc * KW + (a >> 5), 1u << (a & 31));
                    if (c != cc) {                                         // a's own row: the dead neighbour's bit becomes its rep's
                        atomicAnd(adj + (size_t)a * KW + (c >> 5), ~(1u << (c & 31)));
                        atomicOr(adj + (size_t)a * KW + (cc >> 5), 1u << (cc & 31));
                    }
                    s_flag[cc] = 3;
                }
            }
            if (lane == 0) {
                atomicAnd(adj + (size_t)a * KW + (a >> 5), ~(1u << (a & 31)));
                atomicAnd(adj + (size_t)a * KW + (bq >> 5), ~(1u << (bq & 31)));
            }
        }
        if (tid == 0) s_cnt[1] = 0;
        __threadfence();
        __syncthreads();
        alive -= P;
        base += P;
    }
}

// LDS: the absorber table and the reps of tree_cuts.h, the new number of every label, three bit rows.
__global__ __launch_bounds__(AG_THREADS) void rt_cut_kernel(const int *labels, const int *merges, const int *alive_p, int H, int W,
                                                            int K, int R, int *out) {
    __shared__ unsigned s_dk[RS_K_MAX];
    __shared__ unsigned short s_root[RS_K_MAX];
    __shared__ short s_new[RS_K_MAX];
    __shared__ unsigned s_used[RS_K_MAX / 32], s_rep[RS_K_MAX / 32], s_pref[RS_K_MAX / 32];
    __shared__ int s_changed;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const size_t hw = (size_t)H * W;
    labels += (size_t)b * hw;
    out += (size_t)b * hw;
    if (tid < RS_K_MAX / 32) s_used[tid] = 0u;                             // (the barriers of the walk lie before the pixel pass)
    rs_absorbers(merges + (size_t)b * (K - 1) * 2, K - 1, K, s_dk, &s_changed);   // (merges is not read with K = 1)
    rs_group_reps(s_dk, s_root, K, rs_tau(alive_p[b], R, K - 1));
    for (size_t p = tid; p < hw; p += AG_THREADS) {
        const int l = labels[p];
        if ((unsigned)l < (unsigned)K && !(s_used[l >> 5] & (1u << (l & 31)))) atomicOr(&s_used[l >> 5], 1u << (l & 31));
    }
    __syncthreads();
    rs_number_groups(s_used, s_root, K, s_rep, s_pref, s_new);
    for (size_t p = tid; p < hw; p += AG_THREADS) {                        // (out may be labels: a pixel is read, then written, by one thread)
        const int l = labels[p];
        out[p] = (unsigned)l < (unsigned)K ? (int)s_new[l] : -1;
    }
}

// ---- contour map (SPEC.md §15): the level at which every boundary pixel of the label map disappears from the tree
//   rt_contour_prepare_kernel  ONE workgroup per image turns the merge list into a leaf order in which every group of every step is a
//                       contiguous run: a list per rep (head = the rep, a tail table), row t appends b's list to a's and writes the gap
//                       value t + 1 at the seam (one thread: K - 1 dependent LDS steps); the roots that are left are chained in
//                       increasing order with the gap "never" (RT_NEVER, above every level). Positions by list ranking (pointer
//                       jumping, ceil(log2 K) rounds), then a range-maximum table over the K - 1 gaps, ceil(log2 K) levels of K
//                       uint16 entries: join(p, q) = the maximum gap between pos[p] and pos[q] = two table entries. A row that is
//                       not (a < b, both still reps) is skipped, so any list gives a forest and every position lies in 0 .. K-1.
//   rt_contour_kernel   RT_CP consecutive pixels of an image per workgroup: a pixel that agrees with its four neighbours stores 0; the
//                       others read two positions and two table entries per differing neighbour. pos and the table sit in LDS
//                       where one copy per workgroup costs less than the pixels it serves (RT_CLDS_MAX), else they are read in L2.
constexpr unsigned RT_NEVER = 0xffffu;       // gap between two roots: no row joins them (levels are below 4096)
constexpr int RT_CP = 4096;                  // pixels per workgroup of the pixel kernel
constexpr size_t RT_CLDS_MAX = 16384;        // pos + table bytes a pixel workgroup copies to LDS (4 bytes per pixel it serves)

__host__ __device__ inline int rt_levels(int K) { return K > 1 ? 32 - __builtin_clz((unsigned)(K - 1)) : 0; }   // ceil(log2 K)
__host__ __device__ inline size_t rt_contour_bytes(int K) { return rt_align((size_t)2 * K * (1 + rt_levels(K))); }

__global__ __launch_bounds__(RT_T) void rt_contour_prepare_kernel(const int *merges, int K, unsigned char *ws) {
    __shared__ unsigned short s_tail[RT_K_MAX], s_next[RT_K_MAX], s_gap[RT_K_MAX], s_dist[RT_K_MAX];
    __shared__ unsigned short s_a[RT_K_MAX], s_b[RT_K_MAX];
    __shared__ unsigned s_dead[RT_K_MAX / 32];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x, LV = rt_levels(K);
    unsigned short *pos = reinterpret_cast<unsigned short *>(ws + (size_t)b * rt_contour_bytes(K)), *table = pos + K;
    for (int q = tid; q < K; q += RT_T) {
        s_tail[q] = s_next[q] = (unsigned short)q;
        s_gap[q] = 0;
    }
    if (tid < RT_K_MAX / 32) s_dead[tid] = 0u;
    if (K > 1) {
        const int *rows = merges + (size_t)b * (K - 1) * 2;
        for (int t = tid; t < K - 1; t += RT_T) {
            const int a = rows[2 * t], c = rows[2 * t + 1];
            const bool ok = a >= 0 && a < c && c < K;
            s_a[t] = ok ? (unsigned short)a : (unsigned short)RT_NEVER;
            s_b[t] = ok ? (unsigned short)c : (unsigned short)RT_NEVER;
        }
    }
    __syncthreads();
    if (tid == 0 && K > 1) {                                               // the concatenation: serial, its steps depend on each other
        // One LDS round trip per row: the row after this one is fetched before this one's stores, and a dead rep is one whose tail
        // entry says RT_NEVER (its list has gone to its absorber: the entry is never needed again), so the two tails are all a row reads.
        unsigned a = s_a[0], c = s_b[0];
        for (int t = 0; t < K - 1; ++t) {
            const unsigned an = t + 1 < K - 1 ? s_a[t + 1] : RT_NEVER, cn = t + 1 < K - 1 ? s_b[t + 1] : RT_NEVER;
            if (a != RT_NEVER) {
                const unsigned ta = s_tail[a], tc = s_tail[c];
                if (ta != RT_NEVER && tc != RT_NEVER) {                    // both still reps; a row that is not is skipped
                    s_next[ta] = (unsigned short)c;
                    s_gap[ta] = (unsigned short)(t + 1);
                    s_tail[a] = (unsigned short)tc;
                    s_tail[c] = (unsigned short)RT_NEVER;
                }
            }
            a = an;
            c = cn;
        }
    }
    __syncthreads();
    for (int q = tid; q < K; q += RT_T)
        if (s_tail[q] == RT_NEVER) atomicOr(&s_dead[q >> 5], 1u << (q & 31));
    __syncthreads();
    const int KW = (K + 31) >> 5;
    for (int q = tid; q < K; q += RT_T) {                                  // a root's list goes in front of the next root's
        if ((s_dead[q >> 5] >> (q & 31)) & 1u) continue;
        int nxt = -1;
        for (int w = q >> 5; w < KW && nxt < 0; ++w) {
            unsigned live = ~s_dead[w];
            if (w == (q >> 5)) live &= (q & 31) == 31 ? 0u : ~0u << ((q & 31) + 1);
            if (live) nxt = 32 * w + __ffs((int)live) - 1;
        }
        if (nxt >= 0 && nxt < K) {
            const unsigned tq = s_tail[q];
            s_next[tq] = (unsigned short)nxt;
            s_gap[tq] = (unsigned short)RT_NEVER;
        }
    }
    __syncthreads();
    for (int q = tid; q < K; q += RT_T) s_dist[q] = s_next[q] != q ? 1 : 0;
    __syncthreads();
    for (int it = 0; it < LV; ++it) {                                      // one list of K elements: at most K - 1 <= 2^LV links
        unsigned short nn[RT_K_MAX / RT_T], dd[RT_K_MAX / RT_T];
#pragma unroll
        for (int j = 0; j < RT_K_MAX / RT_T; ++j) {
            const int q = tid + j * RT_T;
            if (q < K) {
                const unsigned n = s_next[q];
                nn[j] = s_next[n];
                dd[j] = (unsigned short)(s_dist[q] + s_dist[n]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RT_K_MAX / RT_T; ++j) {
            const int q = tid + j * RT_T;
            if (q < K) {
                s_next[q] = nn[j];
                s_dist[q] = dd[j];
            }
        }
        __syncthreads();
    }
    // positions; the gaps in position order = level 0 of the table (entry K - 1, behind the last element, is 0)
    unsigned short *lv_a = s_tail, *lv_b = s_next;
    for (int q = tid; q < K; q += RT_T) lv_a[q] = 0;
    __syncthreads();
    for (int q = tid; q < K; q += RT_T) {
        const int d = min((int)s_dist[q], K - 1), p = K - 1 - d;
        pos[q] = (unsigned short)p;
        if (p < K - 1) lv_a[p] = s_gap[q];
    }
    __syncthreads();
    for (int j = 0; j < LV; ++j) {                                         // level j entry i = max of the gaps i .. i + 2^j - 1
        for (int i = tid; i < K; i += RT_T) table[(size_t)j * K + i] = lv_a[i];
        const int half = 1 << j;
        for (int i = tid; i < K; i += RT_T) lv_b[i] = max(lv_a[i], i + half < K ? lv_a[i + half] : (unsigned short)0);
        __syncthreads();
        unsigned short *t = lv_a;
        lv_a = lv_b;
        lv_b = t;
    }
}

// s(p, q) of SPEC.md §15 for two labels already known to differ; q < 0: out of range
__device__ __forceinline__ int rt_strength(const unsigned short *pos, const unsigned short *table, int K, int alive, int p, int q) {
    if (p < 0 || q < 0) return alive;
    int l = pos[p], r = pos[q];
    if (l > r) {
        const int t = l;
        l = r;
        r = t;
    }
    if (l == r) return alive;                                              // (only a list that is no forest order: never read past)
    const int j = 31 - __builtin_clz((unsigned)(r - l));
    const unsigned v = max((unsigned)table[(size_t)j * K + l], (unsigned)table[(size_t)j * K + r - (1 << j)]);
    return v == RT_NEVER ? alive : (int)v;
}

__global__ __launch_bounds__(256) void rt_contour_kernel(const int *labels, const int *alive_p, int H, int W, int K,
                                                         const unsigned char *ws, int in_lds, int *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned short rt_ctab[];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const size_t hw = (size_t)H * W;
    const unsigned short *pos = reinterpret_cast<const unsigned short *>(ws + (size_t)b * rt_contour_bytes(K));
    if (in_lds) {
        const int n = K * (1 + rt_levels(K));
        for (int i = tid; i < n; i += 256) rt_ctab[i] = pos[i];
        __syncthreads();
        pos = rt_ctab;
    }
    const unsigned short *table = pos + K;
    const int alive = alive_p[b];
    labels += (size_t)b * hw;
    out += (size_t)b * hw;
    const size_t p0 = (size_t)blockIdx.x * RT_CP, p1 = p0 + RT_CP < hw ? p0 + RT_CP : hw;
    for (size_t p = p0 + tid; p < p1; p += 256) {
        const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
        int c = labels[p];
        if ((unsigned)c >= (unsigned)K) c = -1;                            // every label outside 0 .. K-1 is the one label -1
        int u = 0;
        const int nb[4] = {x > 0 ? labels[p - 1] : c, x + 1 < W ? labels[p + 1] : c, y > 0 ? labels[p - W] : c,
                           y + 1 < H ? labels[p + W] : c};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q = nb[k];
            if ((unsigned)q >= (unsigned)K) q = -1;
            if (q != c) u = max(u, rt_strength(pos, table, K, alive, c, q));
        }
        out[p] = u;
    }
}

bool rt_shape_ok(int B, int H, int W, int K) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= RT_HW_MAX && W <= RT_HW_MAX && K >= 1 && K <= RT_K_MAX;
}

}  // namespace

extern "C" size_t gcs_region_tree_workspace_bytes(int B, int H, int W, int D, int K) {
    if (!rt_shape_ok(B, H, W, K) || D < 1 || D > RT_D_MAX) return 0;
    const size_t k = (size_t)K, kw = (k + 31) / 32;
    return (size_t)B * (rt_align(k * (D + 1) * 8) + rt_align(k * kw * 4) + rt_align(k * D * 2));
}

// The three launches of SPEC.md §14. `lo`: NULL = statistics from the canonical tensor A.feats, else from the slab `slab` of that layout.
static int rt_enqueue(RtArgs A, const GcsLayout *lo, const unsigned char *slab, void *workspace, gcs_stream_t stream) {
    const int B = A.B, H = A.H, W = A.W, D = A.D, K = A.K;
    A.KW = (K + 31) / 32;
    const size_t k = (size_t)K;
    const size_t sums_b = rt_align(k * (D + 1) * 8), adj_b = rt_align(k * A.KW * 4);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    A.sums = reinterpret_cast<u64 *>(ws);                                  // image b's rows: [b][K][D + 1] (dense; the padding sits behind all)
    A.adj = reinterpret_cast<unsigned *>(ws + (size_t)B * sums_b);
    A.mean = reinterpret_cast<uint16_t *>(ws + (size_t)B * (sums_b + adj_b));
    const size_t n16 = (size_t)B * (sums_b + adj_b) / 16;
    const int zgrid = (int)std::min<size_t>((n16 + 255) / 256, (size_t)gcs_cu_count() * 8);
    hipLaunchKernelGGL(rt_zero_kernel, dim3(zgrid), dim3(256), 0, stream, reinterpret_cast<uint4 *>(ws), n16);
    GCS_CHECK_LAUNCH("gcs_region_tree (zero)");
    const dim3 tiles((W + LT_TW - 1) / LT_TW, (H + LT_TH - 1) / LT_TH, B);
    const size_t tile_lds = (size_t)LT_SLOTS * (D + 1) * 4 + LT_SLOTS * 4 + 16;
    if (lo)
        hipLaunchKernelGGL(rt_stats_slab_kernel, tiles, dim3(LT_THREADS), tile_lds, stream, A, *lo, slab);
    else
        hipLaunchKernelGGL(rt_stats_kernel, tiles, dim3(LT_THREADS), tile_lds, stream, A);
    GCS_CHECK_LAUNCH("gcs_region_tree (statistics)");
    const size_t state = rt_state_bytes(K), with_mean = state + k * D * 2;
    const int mean_in_lds = with_mean <= RT_LDS_MAX ? 1 : 0;
    hipLaunchKernelGGL(rt_merge_kernel, dim3(B), dim3(RT_T), mean_in_lds ? with_mean : state, stream, A, mean_in_lds);
    GCS_CHECK_LAUNCH("gcs_region_tree (merge)");
    return GCS_OK;
}

extern "C" int gcs_region_tree(const uint16_t *feats, const int32_t *labels, int B, int H, int W, int D, int K, void *workspace,
                               int32_t *merges_out, uint64_t *costs_out, int32_t *alive_out, gcs_stream_t stream) {
    if (!feats || !labels || !workspace || !alive_out || (K > 1 && !merges_out))
        return gcs_fail(GCS_EINVAL, "gcs_region_tree: NULL pointer");
    if (!rt_shape_ok(B, H, W, K) || D < 1 || D > RT_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_region_tree: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 1 <= D <= 207, 1 <= K <= 4096)");
    RtArgs A{};
    A.feats = feats, A.labels = labels;
    A.B = B, A.H = H, A.W = W, A.D = D, A.K = K;
    A.merges = merges_out, A.costs = reinterpret_cast<u64 *>(costs_out), A.alive = alive_out;
    return rt_enqueue(A, nullptr, nullptr, workspace, stream);
}

extern "C" int gcs_region_tree_slab(const uint16_t *feats_slab, const int32_t *labels, int B, int H, int W, int n_scales, int n_orient,
                                    int K, void *workspace, int32_t *merges_out, uint64_t *costs_out, int32_t *alive_out,
                                    gcs_stream_t stream) {
    if (!feats_slab || !labels || !workspace || !alive_out || (K > 1 && !merges_out))
        return gcs_fail(GCS_EINVAL, "gcs_region_tree_slab: NULL pointer");
    GcsLayout lo;
    if (!rt_shape_ok(B, H, W, K) || !gcs_make_layout(H, W, n_scales, n_orient, &lo) || lo.D > RT_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_region_tree_slab: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, a bank of at most 207 "
                                    "features, 1 <= K <= 4096)");
    RtArgs A{};
    A.labels = labels;
    A.B = B, A.H = H, A.W = W, A.D = lo.D, A.K = K;
    A.merges = merges_out, A.costs = reinterpret_cast<u64 *>(costs_out), A.alive = alive_out;
    return rt_enqueue(A, &lo, reinterpret_cast<const unsigned char *>(feats_slab), workspace, stream);
}

extern "C" int gcs_region_tree_cut(const int32_t *labels, const int32_t *merges, const int32_t *alive, int B, int H, int W, int K,
                                   int R, int32_t *labels_out, gcs_stream_t stream) {
    if (!labels || !alive || !labels_out || (K > 1 && !merges)) return gcs_fail(GCS_EINVAL, "gcs_region_tree_cut: NULL pointer");
    if (!rt_shape_ok(B, H, W, K)) return gcs_fail(GCS_EINVAL, "gcs_region_tree_cut: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 1 <= K <= 4096)");
    if (R < 1) return gcs_fail(GCS_EINVAL, "gcs_region_tree_cut: R must be >= 1");
    hipLaunchKernelGGL(rt_cut_kernel, dim3(B), dim3(AG_THREADS), 0, stream, labels, merges, alive, H, W, K, R, labels_out);
    GCS_CHECK_LAUNCH("gcs_region_tree_cut");
    return GCS_OK;
}

extern "C" size_t gcs_region_tree_contours_workspace_bytes(int B, int K) {
    if (B < 1 || B > 65535 || K < 1 || K > RT_K_MAX) return 0;
    return (size_t)B * rt_contour_bytes(K);
}

extern "C" int gcs_region_tree_contours(const int32_t *labels, const int32_t *merges, const int32_t *alive, int B, int H, int W, int K,
                                        void *workspace, int32_t *contours_out, gcs_stream_t stream) {
    if (!labels || !alive || !workspace || !contours_out || (K > 1 && !merges))
        return gcs_fail(GCS_EINVAL, "gcs_region_tree_contours: NULL pointer");
    if (!rt_shape_ok(B, H, W, K))
        return gcs_fail(GCS_EINVAL, "gcs_region_tree_contours: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 1 <= K <= 4096)");
    const uintptr_t lo = reinterpret_cast<uintptr_t>(labels), co = reinterpret_cast<uintptr_t>(contours_out);
    const size_t map_bytes = (size_t)B * H * W * sizeof(int32_t);
    if (lo < co + map_bytes && co < lo + map_bytes)
        return gcs_fail(GCS_EINVAL, "gcs_region_tree_contours: contours_out overlaps labels (neighbours are read)");
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    hipLaunchKernelGGL(rt_contour_prepare_kernel, dim3(B), dim3(RT_T), 0, stream, merges, K, ws);
    GCS_CHECK_LAUNCH("gcs_region_tree_contours (prepare)");
    const size_t tab = (size_t)2 * K * (1 + rt_levels(K));
    const int in_lds = tab <= RT_CLDS_MAX ? 1 : 0;
    const size_t hw = (size_t)H * W;
    hipLaunchKernelGGL(rt_contour_kernel, dim3((unsigned)((hw + RT_CP - 1) / RT_CP), B), dim3(256), in_lds ? tab : 0, stream, labels,
                       alive, H, W, K, ws, in_lds, contours_out);
    GCS_CHECK_LAUNCH("gcs_region_tree_contours (pixels)");
    return GCS_OK;
}
