// region_kernels.h — the union-find forest and the round kernels of the label-map passes (SPEC.md §7, §9), shared by regions.hip
// (gcs_connected_regions, gcs_merge_small_regions) and region_nodes.hip (gcs_region_nodes, SPEC.md §18). The kernels are `static`:
// each translation unit that includes this header gets its own copy and launches that one.
#pragma once
#include "common.h"

// ================================================================== connected regions (§8f-4)
// SPEC.md §7: 4-connected components of equal labels, renumbered 0,1,2,... in raster order of each
// component's first pixel (so "Regions" = max+1 at /root/reference/BSD_metrics/metrics.py:51 counts
// connected regions, as it does for the SLIC output the slot holds today). Lock-free union-find:
// parents only ever decrease (atomicMin), a root is the smallest pixel index of its component, and a
// failed link (someone re-parented the node meanwhile) retries from the displaced parent, so no
// equivalence is lost even when a find reads a stale pointer.
__device__ __forceinline__ int cc_find(const int *parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void cc_unite(int *parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }   // link the larger root under the smaller
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;                                          // a was re-parented meanwhile: merge that chain too
    }
}

static __global__ void cc_union_kernel(const int32_t *__restrict__ labels, int H, int W, int *__restrict__ parent) {
    const int P = H * W;
    const int32_t *lab = labels + (size_t)blockIdx.y * P;
    int *par = parent + (size_t)blockIdx.y * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int y = p / W, x = p % W;
        const int32_t l = lab[p];
        if (x + 1 < W && lab[p + 1] == l) cc_unite(par, p, p + 1);
        if (y + 1 < H && lab[p + W] == l) cc_unite(par, p, p + W);
    }
}

static __global__ void cc_local_init_kernel(int H, int W, int *__restrict__ parent) {
    const int P = H * W;
    int *par = parent + (size_t)blockIdx.y * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) par[p] = p;
}

// one workgroup per image: flatten, count roots per contiguous chunk, scan, hand out ids in raster order
static __global__ __launch_bounds__(1024) void cc_rank_kernel(int H, int W, int *__restrict__ parent, int *__restrict__ rootid) {
    __shared__ int s_cnt[1024];
    const int P = H * W;
    int *par = parent + (size_t)blockIdx.x * P;
    int *rid = rootid + (size_t)blockIdx.x * P;
    const int tid = threadIdx.x;
    const int chunk = (P + 1023) / 1024;
    const int lo = min(P, tid * chunk), hi = min(P, lo + chunk);
    int cnt = 0;
    for (int p = lo; p < hi; ++p) cnt += par[p] == p;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {          // Hillis-Steele inclusive scan
        const int v = tid >= off ? s_cnt[tid - off] : 0;
        __syncthreads();
        s_cnt[tid] += v;
        __syncthreads();
    }
    int id = s_cnt[tid] - cnt;                           // exclusive prefix = first id of this chunk
    for (int p = lo; p < hi; ++p)
        if (par[p] == p) rid[p] = id++;
}

static __global__ void cc_relabel_kernel(int H, int W, const int *__restrict__ parent, const int *__restrict__ rootid,
                                  int32_t *__restrict__ out) {
    const int P = H * W;
    const int *par = parent + (size_t)blockIdx.y * P;
    const int *rid = rootid + (size_t)blockIdx.y * P;
    int32_t *o = out + (size_t)blockIdx.y * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        int r = par[p];
        while (par[r] != r) r = par[r];                  // the union kernel has finished: plain loads are current
        o[p] = rid[r];
    }
}

// ================================================================== small-region merging (SPEC.md §9)
// Starts from the union-find forest of the connected regions and keeps it: a region's id is its root, which cc_unite keeps
// at the smallest pixel index of the set, i.e. the region's first pixel. One round = four launches on a flattened forest
// (parent[p] = root of p): sizes by horizontal runs, each absorbable region's best neighbour by 64-bit atomicMax, the union of
// every absorbable root with its pick, a flatten. size[] and best[] are non-zero at roots only; the union kernel clears
// them after use, so the next round starts from zeros. act[r][b] = 1 when round r merged something in image b: a later round
// of an image whose previous round merged nothing returns at once. The rounds the halving bound allows are all enqueued.
__device__ __forceinline__ bool mr_idle(const int *act, int round, int B, int b) {
    return round > 0 && act[(size_t)(round - 1) * B + b] == 0;
}

static __global__ void mr_init_kernel(int H, int W, int B, int n_rounds, int *__restrict__ parent, unsigned *__restrict__ size,
                               unsigned long long *__restrict__ best, int *__restrict__ act) {
    const int P = H * W, b = blockIdx.y;
    int *par = parent + (size_t)b * P;
    unsigned *sz = size + (size_t)b * P;
    unsigned long long *bs = best + (size_t)b * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        par[p] = p;
        sz[p] = 0;
        bs[p] = 0;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < n_rounds) act[(size_t)threadIdx.x * B + b] = 0;
}

static __global__ void mr_flatten_kernel(int H, int W, int B, int round, int *__restrict__ parent, const int *__restrict__ act) {
    const int P = H * W, b = blockIdx.y;
    if (round >= 0 && act[(size_t)round * B + b] == 0) return;     // nothing was united: the forest is still flat
    int *par = parent + (size_t)b * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        int r = par[p];
        while (par[r] != r) r = par[r];                  // concurrent shortcuts only ever point at the same root
        par[p] = r;
    }
}

// the first pixel of each horizontal run of one region adds the run's length: one atomic per run, not per pixel
static __global__ void mr_size_kernel(int H, int W, int B, int round, const int *__restrict__ parent, unsigned *__restrict__ size,
                               const int *__restrict__ act) {
    const int P = H * W, b = blockIdx.y;
    if (mr_idle(act, round, B, b)) return;
    const int *par = parent + (size_t)b * P;
    unsigned *sz = size + (size_t)b * P;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int x = p % W, r = par[p];
        if (x > 0 && par[p - 1] == r) continue;
        int len = 1;
        while (x + len < W && par[p + len] == r) ++len;
        atomicAdd(&sz[r], (unsigned)len);
    }
}

// key of region r as a neighbour: larger size first, then the smaller root (= the earlier first pixel)
__device__ __forceinline__ unsigned long long mr_key(const unsigned *sz, int r) {
    return ((unsigned long long)sz[r] << 32) | (0xFFFFFFFFu - (unsigned)r);
}

// one image's pass of a round's second launch: every absorbable region (fewer than min_size pixels) learns its best neighbour
__device__ __forceinline__ void mr_best_image(int H, int W, unsigned min_size, const int *__restrict__ par,
                                              const unsigned *__restrict__ sz, unsigned long long *__restrict__ bs) {
    const int P = H * W;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int x = p % W, ra = par[p];
        const bool a_small = sz[ra] < min_size;
        #pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const int q = dir == 0 ? p + 1 : p + W;
            if (dir == 0 ? x + 1 >= W : q >= P) continue;
            const int rb = par[q];
            if (rb == ra) continue;
            if (a_small) atomicMax(&bs[ra], mr_key(sz, rb));
            if (sz[rb] < min_size) atomicMax(&bs[rb], mr_key(sz, ra));
        }
    }
}

static __global__ void mr_best_kernel(int H, int W, int B, int round, unsigned min_size, const int *__restrict__ parent,
                               const unsigned *__restrict__ size, unsigned long long *__restrict__ best,
                               const int *__restrict__ act) {
    const int P = H * W, b = blockIdx.y;
    if (mr_idle(act, round, B, b)) return;
    mr_best_image(H, W, min_size, parent + (size_t)b * P, size + (size_t)b * P, best + (size_t)b * P);
}

static __global__ void mr_union_kernel(int H, int W, int B, int round, int *__restrict__ parent, unsigned *__restrict__ size,
                                unsigned long long *__restrict__ best, int *__restrict__ act) {
    const int P = H * W, b = blockIdx.y;
    if (mr_idle(act, round, B, b)) return;
    int *par = parent + (size_t)b * P;
    unsigned *sz = size + (size_t)b * P;
    unsigned long long *bs = best + (size_t)b * P;
    bool merged = false;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        if (sz[p] == 0) continue;                        // not a root
        const unsigned long long k = bs[p];
        sz[p] = 0;
        if (k == 0) continue;                            // not absorbable (big enough, or the whole image)
        bs[p] = 0;
        cc_unite(par, p, (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)));
        merged = true;
    }
    if (merged) act[(size_t)round * B + b] = 1;          // every writer stores the same value
}
