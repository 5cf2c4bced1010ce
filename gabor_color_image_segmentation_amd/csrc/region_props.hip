// region_props.hip — SPEC.md §19: descriptors of the regions of a label map and of every cut of a region tree, and the mean-colour
// picture of a map (gfx950 only). Integer sums, minima and maxima only: any execution order gives the same bits. Nothing here
// allocates, frees or synchronises; every entry point enqueues on the caller's stream (and inside a captured graph).
//
// A table row has C = 6 + D uint64 columns  n, sum y, sum x, sum R, sum G, sum B, sum x_0 .. sum x_{D-1}  and a box
// (y0, x0, y1, x1), inclusive, (H, W, -1, -1) for a row without pixels. Rows add and boxes take min / max, so the rows of a
// group of a cut are made from the rows of its leaves: the pixels are read once, for every cut.
//   gcs_region_props       rp_fill_kernel   sums := 0, boxes := empty.
//                          rp_stats_kernel  one workgroup per 8 x 32 pixel tile, one thread per pixel, ONE read of labels, image and
//                                           canonical features. Sums: the tile accumulator of label_tile.h, shared with
//                                           rt_stats_kernel (region_tree.hip), rows [n, y, x, R, G, B, D sums] (256 * 4095 < 2^32).
//                                           Boxes, this kernel's own: a box per slot in LDS, eight lanes that agree add one box,
//                                           atomicMin / atomicMax into the global boxes; a tile of more than 32 labels writes both
//                                           straight to memory. No table indexed by K exists on chip: K is bounded by the output.
//   gcs_region_props_cuts  rp_cuts_kernel   a workgroup per image, all of its walk from tree_cuts.h: rs_absorbers and rs_taus once,
//                                           then per distinct tau rs_group_reps and rs_number_groups (the cut and the numbering
//                                           of gcs_region_tree_cut); a wave per leaf adds its row into its group's dense row.
//   gcs_region_paint       rp_paint_kernel  4096 pixels of an image per workgroup; the packed mean colours of the G rows sit in LDS
//                                           where they fit (RP_PAINT_LDS rows), else every pixel reads its row in L2 and divides.
//                                           A thread paints four consecutive pixels of the batch: 12 bytes, three whole words.
#include <algorithm>

#include "common.h"
#include "label_tile.h"
#include "tree_cuts.h"

namespace {

constexpr int RP_D_MAX = 207, RP_HW_MAX = 4096, RP_FIXED = 6;
constexpr int RP_PP = 4096;                  // pixels per workgroup of the paint kernel
constexpr int RP_PAINT_LDS = 2048;           // rows whose mean colours a paint workgroup keeps in LDS (8 KiB: two per pixel it serves)

typedef unsigned long long u64;

struct RpArgs {
    const int *labels;                       // [B][H][W]
    const uint8_t *img;                      // [B][H][W][3] or NULL
    const uint16_t *feats;                   // [B][D][H][W] or NULL (D = 0)
    u64 *sums;                               // [B][K][C]
    int *bbox;                               // [B][K][4]
    int H, W, D, K;
};

__device__ __forceinline__ int rp_empty_box(size_t i, int H, int W) { return (i & 3) == 0 ? H : (i & 3) == 1 ? W : -1; }

__global__ __launch_bounds__(256) void rp_fill_kernel(u64 *sums, size_t n_sums, int *bbox, size_t n_rows, int H, int W) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_sums; i += step) sums[i] = 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < 4 * n_rows; i += step) bbox[i] = rp_empty_box(i, H, W);
}

__global__ __launch_bounds__(LT_THREADS) void rp_stats_kernel(RpArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned rp_smem[];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.z, D = A.D, C = RP_FIXED + D, K = A.K;
    unsigned *s_acc = rp_smem;                                             // [LT_SLOTS][C]
    int *s_box = reinterpret_cast<int *>(s_acc + LT_SLOTS * C);            // [LT_SLOTS][4]
    int *s_keys = s_box + LT_SLOTS * 4;                                    // [LT_SLOTS] label of the slot, -1: free
    int *s_over = s_keys + LT_SLOTS;                                       // more labels than slots
    lt_clear(s_acc, C, s_keys, s_over);
    if (tid < LT_SLOTS) s_box[4 * tid] = A.H, s_box[4 * tid + 1] = A.W, s_box[4 * tid + 2] = -1, s_box[4 * tid + 3] = -1;
    __syncthreads();
    const size_t hw = (size_t)A.H * A.W;
    int y, x;
    const bool valid = lt_pixel(A.H, A.W, &y, &x);
    const size_t p = (size_t)y * A.W + x;
    const int l = A.labels[(size_t)b * hw + p];
    const bool in = valid && (unsigned)l < (unsigned)K;                    // a label outside 0 .. K-1 is counted nowhere
    unsigned fixed[RP_FIXED] = {1u, (unsigned)y, (unsigned)x, 0u, 0u, 0u};
    if (A.img) {
        const uint8_t *c = A.img + ((size_t)b * hw + p) * 3;
        fixed[3] = c[0], fixed[4] = c[1], fixed[5] = c[2];
    }
    const int slot = lt_claim(s_keys, s_over, l, in);
    __syncthreads();
    const uint16_t *px = D ? A.feats + (size_t)b * D * hw + p : nullptr;
    u64 *g_sums = A.sums + (size_t)b * K * C;
    int *g_box = A.bbox + (size_t)b * K * 4;
    if (*s_over) {                                                         // (uniform over the workgroup)
        if (in) {
            u64 *row = g_sums + (size_t)l * C;
#pragma unroll
            for (int e = 0; e < RP_FIXED; ++e)
                if (fixed[e]) atomicAdd(row + e, (u64)fixed[e]);
            for (int d = 0; d < D; ++d) atomicAdd(row + RP_FIXED + d, (u64)px[(size_t)d * hw]);
            int *box = g_box + (size_t)l * 4;
            atomicMin(box, y), atomicMin(box + 1, x), atomicMax(box + 2, y), atomicMax(box + 3, x);
        }
        return;
    }
    const int same = lt_agree(slot, in);                                   // eight lanes that agree add one sum and one box
    unsigned *row = s_acc + (in ? slot : 0) * C;
    int *box = s_box + (in ? slot : 0) * 4;
    if (same) {
        if ((tid & 7) == 0) atomicMin(box, y), atomicMin(box + 1, x), atomicMax(box + 2, y), atomicMax(box + 3, x + 7);
    } else if (in) {
        atomicMin(box, y), atomicMin(box + 1, x), atomicMax(box + 2, y), atomicMax(box + 3, x);
    }
#pragma unroll
    for (int e = 0; e < RP_FIXED; ++e) lt_add(row + e, fixed[e], same, in);
    for (int d = 0; d < D; ++d) lt_add(row + RP_FIXED + d, px[(size_t)d * hw], same, in);
    __syncthreads();
    lt_flush(s_acc, s_keys, C, g_sums);
    if (tid < LT_SLOTS * 4) {
        const int s = tid >> 2, e = tid & 3, key = s_keys[s];
        if (key >= 0) {
            if (e < 2) atomicMin(g_box + (size_t)key * 4 + e, s_box[tid]);
            else atomicMax(g_box + (size_t)key * 4 + e, s_box[tid]);
        }
    }
}

// Rows of the cuts. LDS: the absorber table and the reps of tree_cuts.h, the new number of every leaf, three bit rows.
__global__ __launch_bounds__(AG_THREADS) void rp_cuts_kernel(const u64 *__restrict__ sums, const int *__restrict__ bbox,
                                                             const int32_t *__restrict__ merges, const int32_t *__restrict__ alive_p,
                                                             const int32_t *__restrict__ regions, int B, int H, int W, int K, int C,
                                                             int n_cuts, int Rsum, int32_t *__restrict__ group_out,
                                                             u64 *__restrict__ sums_out, int *__restrict__ bbox_out) {
    __shared__ unsigned s_dk[RS_K_MAX];
    __shared__ unsigned short s_root[RS_K_MAX];
    __shared__ short s_group[RS_K_MAX];
    __shared__ unsigned s_used[RS_K_MAX / 32], s_rep[RS_K_MAX / 32], s_pref[RS_K_MAX / 32];
    __shared__ int s_tau[RS_CUTS_MAX], s_off[RS_CUTS_MAX + 1];
    __shared__ int s_changed;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 *leaf = sums + (size_t)b * K * C;
    const int *leaf_box = bbox + (size_t)b * K * 4;
    u64 *out = sums_out + (size_t)b * Rsum * C;
    int *out_box = bbox_out + (size_t)b * Rsum * 4;
    rs_absorbers(merges + (size_t)b * (K - 1) * 2, K - 1, K, s_dk, &s_changed);   // (merges is not read with K = 1)
    if (tid < RS_K_MAX / 32) s_used[tid] = 0u;
    rs_taus(regions, n_cuts, alive_p[b], K - 1, s_tau);                    // (and the barrier behind the zeroing)
    if (tid == 0) {                                                        // cut c owns min(K, R_c) rows behind the cuts before it
        int acc = 0;
        for (int c = 0; c < n_cuts; ++c) {
            s_off[c] = acc;
            acc += min(K, max(regions[c], 0));
        }
        s_off[n_cuts] = acc;
    }
    for (int q = tid; q < K; q += AG_THREADS)
        if (leaf[(size_t)q * C]) atomicOr(&s_used[q >> 5], 1u << (q & 31));
    for (size_t i = tid; i < (size_t)Rsum * C; i += AG_THREADS) out[i] = 0ull;
    for (int i = tid; i < 4 * Rsum; i += AG_THREADS) out_box[i] = rp_empty_box((size_t)i, H, W);
    __threadfence();                                                       // the rows are in L2 before the atomics that add to them
    __syncthreads();
    for (int c = 0; c < n_cuts; ++c) {
        if (c == 0 || s_tau[c] != s_tau[c - 1]) {
            rs_group_reps(s_dk, s_root, K, s_tau[c]);
            rs_number_groups(s_used, s_root, K, s_rep, s_pref, s_group);
        }
        int32_t *g_out = group_out + ((size_t)c * B + b) * K;
        for (int q = tid; q < K; q += AG_THREADS) g_out[q] = (int32_t)s_group[q];
        // a group past the cut's rows (a list that is no tree of `alive` leaves leaves more than R groups) has no row
        const int base = s_off[c], rows = min(s_off[c + 1], Rsum) - base;
        for (int q = wave; q < K; q += AG_WAVES) {
            const int g = s_group[q];                                      // (uniform over the wave)
            if (g < 0 || g >= rows) continue;
            u64 *row = out + (size_t)(base + g) * C;
            for (int e = lane; e < C; e += 64) {
                const u64 v = leaf[(size_t)q * C + e];
                if (v) atomicAdd(row + e, v);
            }
            if (lane < 4) {
                const int v = leaf_box[(size_t)q * 4 + lane];
                int *t = out_box + (size_t)(base + g) * 4 + lane;
                if (lane < 2) atomicMin(t, v);
                else atomicMax(t, v);
            }
        }
        __syncthreads();                                                   // s_group is read before the next cut renumbers
    }
}

// the packed mean colour of a table row: floor((2 S + n) / (2 n)) per channel (SPEC.md §4's rule), R in the low byte; n = 0: black
__device__ __forceinline__ unsigned rp_mean_rgb(const u64 *row) {
    const u64 n = row[0];
    if (n == 0) return 0u;
    unsigned v = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const u64 m = (2 * row[3 + ch] + n) / (2 * n);
        v |= (unsigned)(m < 255 ? m : 255) << (8 * ch);
    }
    return v;
}

__global__ __launch_bounds__(256) void rp_paint_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ group,
                                                       const u64 *__restrict__ sums, int H, int W, int K, int G, int C, int stride,
                                                       int in_lds, int aligned, uint8_t *__restrict__ rgb) {
    __shared__ unsigned s_mean[RP_PAINT_LDS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const size_t hw = (size_t)H * W;
    const u64 *tab = sums + (size_t)b * stride * C;          // image b's rows: `stride` rows apart
    if (group) group += (size_t)b * K;
    // pixels are numbered through the batch: quad j = pixels 4 j .. 4 j + 3 = bytes 12 j .. 12 j + 11 of rgb; a quad that straddles two
    // images is painted by both, each its own pixels
    const size_t first = (size_t)b * hw, last = first + hw;                // this image's pixels
    const size_t q0 = first / 4 + (size_t)blockIdx.x * (RP_PP / 4);
    const size_t q1 = min(q0 + RP_PP / 4, (last + 3) / 4);
    if (q0 >= q1) return;                                                  // (uniform over the workgroup)
    if (in_lds) {
        for (int g = tid; g < G; g += 256) s_mean[g] = rp_mean_rgb(tab + (size_t)g * C);
        __syncthreads();
    }
    for (size_t j = q0 + tid; j < q1; j += 256) {
        const size_t p0 = 4 * j;
        const bool whole = p0 >= first && p0 + 4 <= last;
        int l[4];
        if (whole && aligned) {
            const int4 v = *reinterpret_cast<const int4 *>(labels + p0);   // (16 j bytes into the tensor)
            l[0] = v.x, l[1] = v.y, l[2] = v.z, l[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) l[k] = p0 + k >= first && p0 + k < last ? labels[p0 + k] : -1;
        }
        unsigned c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int g = -1;
            if ((unsigned)l[k] < (unsigned)K) g = group ? group[l[k]] : l[k];
            c[k] = 0u;
            if ((unsigned)g < (unsigned)G) c[k] = in_lds ? s_mean[g] : rp_mean_rgb(tab + (size_t)g * C);
        }
        if (whole && aligned) {
            uint3 v;
            v.x = c[0] | (c[1] << 24);
            v.y = (c[1] >> 8) | (c[2] << 16);
            v.z = (c[2] >> 16) | (c[3] << 8);
            *reinterpret_cast<uint3 *>(rgb + 3 * p0) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k >= first && p0 + k < last) {
                    uint8_t *o = rgb + 3 * (p0 + k);
                    o[0] = (uint8_t)c[k], o[1] = (uint8_t)(c[k] >> 8), o[2] = (uint8_t)(c[k] >> 16);
                }
        }
    }
}

bool rp_map_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= RP_HW_MAX && W <= RP_HW_MAX; }

}  // namespace

extern "C" int gcs_region_props(const int32_t *labels, const uint8_t *img, const uint16_t *feats, int B, int H, int W, int D, int K,
                                uint64_t *sums_out, int32_t *bbox_out, gcs_stream_t stream) {
    if (!labels || !sums_out || !bbox_out) return gcs_fail(GCS_EINVAL, "gcs_region_props: NULL pointer");
    if (!rp_map_ok(B, H, W) || D < 0 || D > RP_D_MAX || K < 1)
        return gcs_fail(GCS_EINVAL, "gcs_region_props: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 0 <= D <= 207, K >= 1)");
    if ((feats == nullptr) != (D == 0)) return gcs_fail(GCS_EINVAL, "gcs_region_props: feats must be NULL exactly when D = 0");
    const int C = RP_FIXED + D;
    if ((long long)B * K * C >= 0x80000000LL) return gcs_fail(GCS_EINVAL, "gcs_region_props: B * K * (6 + D) must be below 2^31");
    RpArgs A{};
    A.labels = labels, A.img = img, A.feats = feats;
    A.sums = reinterpret_cast<u64 *>(sums_out), A.bbox = bbox_out;
    A.H = H, A.W = W, A.D = D, A.K = K;
    const size_t n_rows = (size_t)B * K, n_sums = n_rows * C;
    const int fgrid = (int)std::min<size_t>((n_sums + 255) / 256, (size_t)gcs_cu_count() * 8);
    hipLaunchKernelGGL(rp_fill_kernel, dim3(fgrid), dim3(256), 0, stream, A.sums, n_sums, bbox_out, n_rows, H, W);
    GCS_CHECK_LAUNCH("gcs_region_props (fill)");
    const dim3 tiles((W + LT_TW - 1) / LT_TW, (H + LT_TH - 1) / LT_TH, B);
    hipLaunchKernelGGL(rp_stats_kernel, tiles, dim3(LT_THREADS), (size_t)LT_SLOTS * (C + 5) * 4 + 16, stream, A);
    GCS_CHECK_LAUNCH("gcs_region_props (statistics)");
    return GCS_OK;
}

extern "C" int gcs_region_props_cuts(const uint64_t *sums, const int32_t *bbox, const int32_t *merges, const int32_t *alive,
                                     const int32_t *regions, int B, int H, int W, int K, int C, int n_cuts, int Rsum,
                                     int32_t *group_out, uint64_t *sums_out, int32_t *bbox_out, gcs_stream_t stream) {
    if (!sums || !bbox || !alive || !regions || !group_out || !sums_out || !bbox_out || (K > 1 && !merges))
        return gcs_fail(GCS_EINVAL, "gcs_region_props_cuts: NULL pointer");
    if (!rp_map_ok(B, H, W) || K < 1 || K > RS_K_MAX || C < RP_FIXED || C > RP_FIXED + RP_D_MAX || n_cuts < 1 || n_cuts > RS_CUTS_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_region_props_cuts: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, 1 <= K <= 4096, "
                                    "6 <= C <= 213, 1 <= n_cuts <= 64)");
    if (Rsum < 1 || Rsum > n_cuts * K) return gcs_fail(GCS_EINVAL, "gcs_region_props_cuts: Rsum must be in 1 .. n_cuts * K");
    if ((long long)B * K * C >= 0x80000000LL || (long long)B * Rsum * C >= 0x80000000LL || (long long)n_cuts * B * K >= 0x80000000LL)
        return gcs_fail(GCS_EINVAL, "gcs_region_props_cuts: B * K * C, B * Rsum * C and n_cuts * B * K must be below 2^31");
    hipLaunchKernelGGL(rp_cuts_kernel, dim3(B), dim3(AG_THREADS), 0, stream, reinterpret_cast<const u64 *>(sums), bbox, merges, alive,
                       regions, B, H, W, K, C, n_cuts, Rsum, group_out, reinterpret_cast<u64 *>(sums_out), bbox_out);
    GCS_CHECK_LAUNCH("gcs_region_props_cuts");
    return GCS_OK;
}

extern "C" int gcs_region_paint(const int32_t *labels, const int32_t *group, const uint64_t *sums, int B, int H, int W, int K, int G,
                                int C, int row_stride, uint8_t *rgb_out, gcs_stream_t stream) {
    if (!labels || !sums || !rgb_out) return gcs_fail(GCS_EINVAL, "gcs_region_paint: NULL pointer");
    if (!rp_map_ok(B, H, W) || K < 1 || G < 1 || C < RP_FIXED || C > RP_FIXED + RP_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_region_paint: bad shape (1 <= B <= 65535, 1 <= H, W <= 4096, K >= 1, G >= 1, 6 <= C <= 213)");
    if (!group && G != K) return gcs_fail(GCS_EINVAL, "gcs_region_paint: without a group table the labels index the rows: G must be K");
    if (row_stride < G) return gcs_fail(GCS_EINVAL, "gcs_region_paint: row_stride (rows from one image's table to the next) must be at least G");
    if ((long long)B * row_stride * C >= 0x80000000LL || (long long)B * K >= 0x80000000LL)
        return gcs_fail(GCS_EINVAL, "gcs_region_paint: B * row_stride * C and B * K must be below 2^31");
    const size_t hw = (size_t)H * W;
    const unsigned chunks = (unsigned)(((hw + 6) / 4 + RP_PP / 4 - 1) / (RP_PP / 4));   // an image's first quad may start 3 pixels before it
    const int aligned = (reinterpret_cast<uintptr_t>(rgb_out) & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 15) == 0;
    hipLaunchKernelGGL(rp_paint_kernel, dim3(chunks, B), dim3(256), 0, stream, labels, group, reinterpret_cast<const u64 *>(sums), H, W,
                       K, G, C, row_stride, G <= RP_PAINT_LDS ? 1 : 0, aligned, rgb_out);
    GCS_CHECK_LAUNCH("gcs_region_paint");
    return GCS_OK;
}
