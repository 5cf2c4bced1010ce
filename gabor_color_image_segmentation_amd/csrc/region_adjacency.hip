// region_adjacency.hip — SPEC.md §20: the region adjacency graph of a label map and of every cut of a region tree (gfx950 only).
// An edge (a, b), a < b, carries three uint64 columns: length (crossings), contrast (sum of squared colour differences across the
// crossings) and strength (sum of the clamped values of a plane on both sides). Integer sums and a final sort: any execution order
// gives the same bits. Nothing here allocates, frees or synchronises; every entry point enqueues on the caller's stream.
//
// An image's edges live, while they are being counted, in an open-addressing table in the workspace: S = a power of two of at
// least 2 E_cap slots, a 64-bit key (a << 32 | b) claimed by a 64-bit atomicCAS, three uint64 columns added with vector atomics, and
// a counter of claimed keys that raises the image's overflow flag once it passes E_cap. No probe loop is unbounded and no thread
// waits on another: a probe ends at a free slot, at its key, after S slots or when it sees the flag (it looks every 16th step);
// whatever ends it without a slot raises the flag. The flag is raised exactly when the image has more than E_cap edges (with at
// most E_cap the table is never more than half full and nothing ever ends a probe early; with more, every key is claimed unless a
// probe was ended, and both raise it).
//   gcs_region_adjacency       ra_fill_kernel    keys := free, columns := 0, counters := 0.
//                              ra_pixels_kernel  one workgroup per 8 x 32 pixel tile, a thread per pixel, which owns its right and its
//                                                lower pair (the shape of rp_stats_kernel, restated, not shared): labels, packed colours
//                                                and plane values of the tile and of the pixels right of and below it sit in LDS.
//                                                Crossings go through a 64-slot LDS hash of keys with uint64 columns (a tile's strength
//                                                reaches 512 * 2 * (2^31 - 1)); touched slots leave with one probe and up to three
//                                                64-bit atomics each. A crossing that finds the LDS hash full goes straight to the table.
//                              ra_finish_kernel  a workgroup per image: the claimed keys are compacted into LDS (16 384 keys = 128 KiB),
//                                                sorted there (bitonic, padded to a power of two), looked up again and written as dense
//                                                rows, the sentinel rows behind them and count; count = -1 and sentinel rows only for a
//                                                flagged image.
//   gcs_region_adjacency_cuts  ra_fill_kernel, then ra_cuts_kernel: a workgroup per (cut, image) sends every leaf row whose two groups
//                                                differ through the same LDS hash into the table of that (cut, image); ra_finish_kernel
//                                                with n_cuts * B "images".
#include <algorithm>

#include "common.h"

namespace {

constexpr int RA_TH = 8, RA_TW = 32;         // pixel tile: 8 rows of 32 pixels, 256 threads
constexpr int RA_LW = RA_TW + 1, RA_LH = RA_TH + 1, RA_LN = RA_LW * RA_LH;   // the tile with the column right of and the row below it
constexpr int RA_SLOTS = 64;                 // edges a workgroup accumulates in LDS
constexpr int RA_HW_MAX = 4096, RA_E_MAX = 16384, RA_CUTS_MAX = 64;
constexpr int RA_FT = 1024;                  // threads of the finish kernel

typedef unsigned long long u64;
constexpr u64 RA_FREE = ~0ull;               // no key: a = 2^32 - 1 is no label

struct RaTable {                             // the tables of all images: image t owns keys[t S ..], vals[3 t S ..], ctr[2 t ..]
    u64 *keys;                               // [T][S]
    u64 *vals;                               // [T][S][3]
    int *ctr;                                // [T][2]: claimed keys, overflow flag
    int S, shift, E_cap;                     // S = 1 << (64 - shift)
};

__host__ __device__ __forceinline__ int ra_slots(int E_cap) {
    int s = 2;
    while (s < 2 * E_cap) s <<= 1;
    return s;
}

__device__ __forceinline__ unsigned ra_hash(u64 key, int shift) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> shift); }

__device__ __forceinline__ int ra_flagged(const int *ctr) { return __hip_atomic_load(ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ra_flag(int *ctr) { __hip_atomic_store(ctr + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The slot of `key` in image t's table, claimed if it is new; -1 (and the flag raised) when the probe ends without one.
__device__ int ra_slot_of(const RaTable &T, size_t t, u64 key) {
    u64 *keys = T.keys + t * (size_t)T.S;
    int *ctr = T.ctr + 2 * t;
    const unsigned mask = (unsigned)T.S - 1u, h = ra_hash(key, T.shift);
    for (unsigned q = 0; q <= mask; ++q) {
        // the flag is one word per image: an agent-scope read of it at every probe's first step made that word the hottest address
        // of the pass, so a probe looks at it every 16th step only, which a table that is at most half full rarely reaches
        if ((q & 15u) == 15u && ra_flagged(ctr)) return -1;
        const unsigned s = (h + q) & mask;
        // a plain, cached read first: a slot goes from free to its key once and never changes again, so a stale value can only be
        // "free", and then the atomicCAS decides
        u64 cur = keys[s];
        if (cur == RA_FREE) {
            cur = atomicCAS(keys + s, RA_FREE, key);
            if (cur == RA_FREE) {
                if (atomicAdd(ctr, 1) >= T.E_cap) ra_flag(ctr);            // (the slot is this key's all the same: in bounds, never read)
                return (int)s;
            }
        }
        if (cur == key) return (int)s;
    }
    ra_flag(ctr);
    return -1;
}

__device__ __forceinline__ void ra_table_add(const RaTable &T, size_t t, u64 key, u64 len, u64 con, u64 str) {
    const int s = ra_slot_of(T, t, key);
    if (s < 0) return;
    u64 *row = T.vals + (t * (size_t)T.S + (size_t)s) * 3;
    if (len) atomicAdd(row, len);
    if (con) atomicAdd(row + 1, con);
    if (str) atomicAdd(row + 2, str);
}

// The workgroup's LDS hash: s_keys [RA_SLOTS], s_vals [RA_SLOTS][3]. ra_local_clear, a barrier, any number of ra_local_add, a
// barrier, ra_local_flush. An edge that finds all slots taken by others goes to the table at once.
__device__ __forceinline__ void ra_local_clear(u64 *s_keys, u64 *s_vals, int tid, int nthreads) {
    for (int i = tid; i < RA_SLOTS; i += nthreads) s_keys[i] = RA_FREE;
    for (int i = tid; i < 3 * RA_SLOTS; i += nthreads) s_vals[i] = 0ull;
}

__device__ __forceinline__ void ra_local_add(u64 *s_keys, u64 *s_vals, const RaTable &T, size_t t, u64 key, u64 len, u64 con, u64 str) {
    const unsigned h = ra_hash(key, 64 - 6);
    for (int q = 0; q < RA_SLOTS; ++q) {
        const int s = (int)((h + (unsigned)q) & (RA_SLOTS - 1));
        const u64 old = atomicCAS(s_keys + s, RA_FREE, key);
        if (old == RA_FREE || old == key) {
            if (len) atomicAdd(s_vals + 3 * s, len);
            if (con) atomicAdd(s_vals + 3 * s + 1, con);
            if (str) atomicAdd(s_vals + 3 * s + 2, str);
            return;
        }
    }
    ra_table_add(T, t, key, len, con, str);
}

__device__ __forceinline__ void ra_local_flush(const u64 *s_keys, const u64 *s_vals, const RaTable &T, size_t t, int tid, int nthreads) {
    for (int s = tid; s < RA_SLOTS; s += nthreads)
        if (s_keys[s] != RA_FREE) ra_table_add(T, t, s_keys[s], s_vals[3 * s], s_vals[3 * s + 1], s_vals[3 * s + 2]);
}

__global__ __launch_bounds__(256) void ra_fill_kernel(RaTable T, size_t n_tables) {
    const size_t step = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n_keys = n_tables * (size_t)T.S;
    for (size_t i = first; i < n_keys; i += step) T.keys[i] = RA_FREE;
    for (size_t i = first; i < 3 * n_keys; i += step) T.vals[i] = 0ull;
    for (size_t i = first; i < 2 * n_tables; i += step) T.ctr[i] = 0;
}

__global__ __launch_bounds__(256) void ra_pixels_kernel(const int32_t *__restrict__ labels, const uint8_t *__restrict__ img,
                                                        const int32_t *__restrict__ plane, int H, int W, int K, RaTable T) {
    __shared__ u64 s_keys[RA_SLOTS], s_vals[3 * RA_SLOTS];
    __shared__ int s_lab[RA_LN];
    __shared__ unsigned s_rgb[RA_LN], s_pl[RA_LN];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.z;
    const int y0 = (int)blockIdx.y * RA_TH, x0 = (int)blockIdx.x * RA_TW;
    const size_t hw = (size_t)H * W;
    ra_local_clear(s_keys, s_vals, tid, 256);
    for (int i = tid; i < RA_LN; i += 256) {
        const int y = y0 + i / RA_LW, x = x0 + i % RA_LW;
        int l = -1;                                                        // outside the image: a label that crosses nothing
        unsigned c = 0u, e = 0u;
        if (y < H && x < W) {
            const size_t p = (size_t)b * hw + (size_t)y * W + x;
            l = labels[p];
            if (img) c = (unsigned)img[3 * p] | ((unsigned)img[3 * p + 1] << 8) | ((unsigned)img[3 * p + 2] << 16);
            if (plane) e = (unsigned)max(plane[p], 0);
        }
        s_lab[i] = l, s_rgb[i] = c, s_pl[i] = e;
    }
    __syncthreads();
    const int me = (tid / RA_TW) * RA_LW + tid % RA_TW;
    const int l = s_lab[me];
    if ((unsigned)l < (unsigned)K) {
        const unsigned c = s_rgb[me], e = s_pl[me];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int other = me + (side ? RA_LW : 1);
            const int m = s_lab[other];
            if ((unsigned)m >= (unsigned)K || m == l) continue;
            const unsigned d = s_rgb[other];
            const int dr = (int)(c & 255u) - (int)(d & 255u), dg = (int)((c >> 8) & 255u) - (int)((d >> 8) & 255u),
                      db = (int)(c >> 16) - (int)(d >> 16);
            const u64 key = ((u64)(unsigned)min(l, m) << 32) | (u64)(unsigned)max(l, m);
            ra_local_add(s_keys, s_vals, T, (size_t)b, key, 1ull, (u64)(dr * dr + dg * dg + db * db), (u64)e + (u64)s_pl[other]);
        }
    }
    __syncthreads();
    ra_local_flush(s_keys, s_vals, T, (size_t)b, tid, 256);
}

// A workgroup per (image, cut): the leaf rows of the image under the cut's group table.
__global__ __launch_bounds__(256) void ra_cuts_kernel(const int32_t *__restrict__ edges, const u64 *__restrict__ vals,
                                                      const int32_t *__restrict__ count, const int32_t *__restrict__ group, int B, int K,
                                                      int G, int E_cap, RaTable T) {
    __shared__ u64 s_keys[RA_SLOTS], s_vals[3 * RA_SLOTS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x, c = (int)blockIdx.y;
    const size_t t = (size_t)c * B + b;
    const int n = count[b];
    if (n < 0 || n > E_cap) {                                              // (uniform) no leaf table: no table of the cut
        if (tid == 0) ra_flag(T.ctr + 2 * t);
        return;
    }
    ra_local_clear(s_keys, s_vals, tid, 256);
    __syncthreads();
    const int32_t *g = group + t * (size_t)K;
    const int32_t *e = edges + (size_t)b * E_cap * 2;
    const u64 *v = vals + (size_t)b * E_cap * 3;
    for (int i = tid; i < n; i += 256) {
        const int a0 = e[2 * i], b0 = e[2 * i + 1];
        if ((unsigned)a0 >= (unsigned)K || (unsigned)b0 >= (unsigned)K) continue;
        const int ga = g[a0], gb = g[b0];
        if ((unsigned)ga >= (unsigned)G || (unsigned)gb >= (unsigned)G || ga == gb) continue;
        const u64 key = ((u64)(unsigned)min(ga, gb) << 32) | (u64)(unsigned)max(ga, gb);
        ra_local_add(s_keys, s_vals, T, t, key, v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]);
    }
    __syncthreads();
    ra_local_flush(s_keys, s_vals, T, t, tid, 256);
}

// A workgroup per table: dense sorted rows, sentinel rows, count. Dynamic LDS: cap keys (cap = the power of two at or above E_cap)
// and one counter behind them.
__global__ __launch_bounds__(RA_FT) void ra_finish_kernel(RaTable T, int cap, int32_t *__restrict__ edges_out, u64 *__restrict__ vals_out,
                                                          int32_t *__restrict__ count_out) {
    extern __shared__ __attribute__((aligned(16))) u64 ra_smem[];
    u64 *s_sort = ra_smem;
    int *s_n = reinterpret_cast<int *>(ra_smem + cap);
    const int tid = (int)threadIdx.x, E_cap = T.E_cap;
    const size_t t = blockIdx.x;
    const u64 *keys = T.keys + t * (size_t)T.S;
    const u64 *vals = T.vals + t * (size_t)T.S * 3;
    int32_t *eo = edges_out + t * (size_t)E_cap * 2;
    u64 *vo = vals_out + t * (size_t)E_cap * 3;
    const int claimed = T.ctr[2 * t], flagged = T.ctr[2 * t + 1];
    if (flagged || claimed < 0 || claimed > E_cap) {                       // (uniform)
        for (int i = tid; i < E_cap; i += RA_FT) {
            eo[2 * i] = -1, eo[2 * i + 1] = -1;
            vo[3 * (size_t)i] = 0ull, vo[3 * (size_t)i + 1] = 0ull, vo[3 * (size_t)i + 2] = 0ull;
        }
        if (tid == 0) count_out[t] = -1;
        return;
    }
    if (tid == 0) *s_n = 0;
    __syncthreads();
    for (int s = tid; s < T.S; s += RA_FT) {
        const u64 k = keys[s];
        if (k != RA_FREE) {
            const int pos = atomicAdd(s_n, 1);
            if (pos < cap) s_sort[pos] = k;                                // (pos < claimed <= E_cap <= cap)
        }
    }
    __syncthreads();
    const int n = min(*s_n, E_cap);
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += RA_FT) s_sort[i] = RA_FREE;          // the padding sorts behind every key
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += RA_FT) {
                const int o = i ^ j;
                if (o > i) {
                    const u64 x = s_sort[i], y = s_sort[o];
                    if ((x > y) == ((i & k) == 0)) s_sort[i] = y, s_sort[o] = x;
                }
            }
            __syncthreads();
        }
    const unsigned mask = (unsigned)T.S - 1u;
    for (int i = tid; i < E_cap; i += RA_FT) {
        int a = -1, b = -1;
        u64 len = 0ull, con = 0ull, str = 0ull;
        if (i < n) {
            const u64 key = s_sort[i];
            a = (int)(key >> 32), b = (int)(key & 0xffffffffull);
            const unsigned h = ra_hash(key, T.shift);
            for (unsigned q = 0; q <= mask; ++q) {                         // the key is in the table: the probe that put it there, again
                const unsigned s = (h + q) & mask;
                if (keys[s] == key) {
                    len = vals[3 * (size_t)s], con = vals[3 * (size_t)s + 1], str = vals[3 * (size_t)s + 2];
                    break;
                }
            }
        }
        eo[2 * i] = a, eo[2 * i + 1] = b;
        vo[3 * (size_t)i] = len, vo[3 * (size_t)i + 1] = con, vo[3 * (size_t)i + 2] = str;
    }
    if (tid == 0) count_out[t] = n;
}

bool ra_cap_ok(int E_cap) { return E_cap >= 1 && E_cap <= RA_E_MAX; }

// the workspace of n_tables tables at E_cap: keys, columns, counters
RaTable ra_carve(void *workspace, size_t n_tables, int E_cap) {
    RaTable T{};
    T.S = ra_slots(E_cap);
    int bits = 0;
    while ((1 << bits) < T.S) ++bits;
    T.shift = 64 - bits;
    T.E_cap = E_cap;
    T.keys = static_cast<u64 *>(workspace);
    T.vals = T.keys + n_tables * (size_t)T.S;
    T.ctr = reinterpret_cast<int *>(T.vals + 3 * n_tables * (size_t)T.S);
    return T;
}

int ra_fill(const RaTable &T, size_t n_tables, hipStream_t stream, const char *what) {
    const size_t words = 3 * n_tables * (size_t)T.S;
    const int grid = (int)std::min<size_t>((words + 255) / 256, (size_t)gcs_cu_count() * 8);
    hipLaunchKernelGGL(ra_fill_kernel, dim3(grid), dim3(256), 0, stream, T, n_tables);
    GCS_CHECK_LAUNCH(what);
    return GCS_OK;
}

int ra_finish(const RaTable &T, size_t n_tables, int32_t *edges_out, uint64_t *vals_out, int32_t *count_out, hipStream_t stream,
              const char *what) {
    int cap = 1;
    while (cap < T.E_cap) cap <<= 1;
    const size_t lds = (size_t)cap * 8 + 16;
    // raise the dynamic-LDS cap, always to the largest any call needs: the attribute belongs to the function, not to the launch, so a
    // value of this call's own could be lowered by another host thread's smaller call between this line and the launch
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ra_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       RA_E_MAX * 8 + 16);
    if (e != hipSuccess) return gcs_hip_fail(e, "hipFuncSetAttribute(region adjacency finish)");
    hipLaunchKernelGGL(ra_finish_kernel, dim3((unsigned)n_tables), dim3(RA_FT), lds, stream, T, cap, edges_out,
                       reinterpret_cast<u64 *>(vals_out), count_out);
    GCS_CHECK_LAUNCH(what);
    return GCS_OK;
}

}  // namespace

extern "C" size_t gcs_region_adjacency_workspace_bytes(int B, int E_cap) {
    if (B < 1 || !ra_cap_ok(E_cap)) return 0;
    return (size_t)B * ((size_t)ra_slots(E_cap) * 32 + 8);
}

extern "C" int gcs_region_adjacency(const int32_t *labels, const uint8_t *img, const int32_t *strength, int B, int H, int W, int K,
                                    int E_cap, void *workspace, int32_t *edges_out, uint64_t *vals_out, int32_t *count_out,
                                    gcs_stream_t stream) {
    if (!labels || !workspace || !edges_out || !vals_out || !count_out)
        return gcs_fail(GCS_EINVAL, "gcs_region_adjacency: NULL pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > RA_HW_MAX || W > RA_HW_MAX || K < 1 || !ra_cap_ok(E_cap))
        return gcs_fail(GCS_EINVAL, "gcs_region_adjacency: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, K >= 1, 1 <= E_cap <= 16384)");
    if ((long long)B * H * W >= 0x80000000LL || (long long)B * ra_slots(E_cap) * 4 >= 0x80000000LL)
        return gcs_fail(GCS_EINVAL, "gcs_region_adjacency: B * H * W and the workspace's 8-byte words must be below 2^31");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const RaTable T = ra_carve(workspace, (size_t)B, E_cap);
    int rc = ra_fill(T, (size_t)B, s, "gcs_region_adjacency (fill)");
    if (rc != GCS_OK) return rc;
    const dim3 tiles((W + RA_TW - 1) / RA_TW, (H + RA_TH - 1) / RA_TH, B);
    hipLaunchKernelGGL(ra_pixels_kernel, tiles, dim3(256), 0, s, labels, img, strength, H, W, K, T);
    GCS_CHECK_LAUNCH("gcs_region_adjacency (pixels)");
    return ra_finish(T, (size_t)B, edges_out, vals_out, count_out, s, "gcs_region_adjacency (finish)");
}

extern "C" int gcs_region_adjacency_cuts(const int32_t *edges, const uint64_t *vals, const int32_t *count, const int32_t *group, int B,
                                         int K, int G, int E_cap, int n_cuts, int E_out_cap, void *workspace, int32_t *edges_out,
                                         uint64_t *vals_out, int32_t *count_out, gcs_stream_t stream) {
    if (!edges || !vals || !count || !group || !workspace || !edges_out || !vals_out || !count_out)
        return gcs_fail(GCS_EINVAL, "gcs_region_adjacency_cuts: NULL pointer");
    if (B < 1 || B > 65535 || K < 1 || G < 1 || !ra_cap_ok(E_cap) || !ra_cap_ok(E_out_cap) || n_cuts < 1 || n_cuts > RA_CUTS_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_region_adjacency_cuts: bad shape (1 <= B <= 65535, K >= 1, G >= 1, 1 <= E_cap, E_out_cap <= 16384, "
                                    "1 <= n_cuts <= 64)");
    const long long tables = (long long)n_cuts * B;
    if (tables * K >= 0x80000000LL || (long long)B * E_cap * 3 >= 0x80000000LL || tables * ra_slots(E_out_cap) * 4 >= 0x80000000LL)
        return gcs_fail(GCS_EINVAL, "gcs_region_adjacency_cuts: n_cuts * B * K, B * E_cap * 3 and the workspace's 8-byte words must be "
                                    "below 2^31");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const RaTable T = ra_carve(workspace, (size_t)tables, E_out_cap);
    int rc = ra_fill(T, (size_t)tables, s, "gcs_region_adjacency_cuts (fill)");
    if (rc != GCS_OK) return rc;
    hipLaunchKernelGGL(ra_cuts_kernel, dim3(B, n_cuts), dim3(256), 0, s, edges, reinterpret_cast<const u64 *>(vals), count, group, B, K,
                       G, E_cap, T);
    GCS_CHECK_LAUNCH("gcs_region_adjacency_cuts (rows)");
    return ra_finish(T, (size_t)tables, edges_out, vals_out, count_out, s, "gcs_region_adjacency_cuts (finish)");
}
