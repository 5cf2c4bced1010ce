// edge_match.hip — one-to-one matching counts of a level map against annotator contours at every level at once, SPEC.md §27.
// The levels are nested (P_tau = {q > tau} only grows as tau falls), so ONE incremental maximum matching serves all of them: the
// map's pixels are added in descending level, one alternating-path search per pixel, and the matching's size is read off at the
// end of each level.
//
//   tt_kernel        the thin contour Q_t of an annotator map (a pixel whose right or lower neighbour carries another label) as a
//                    byte plane, and |Q_t| (one atomic per wave).
//   em_hist_kernel   levels of an image -> hist[b][0 .. 256] (LDS histogram per workgroup, then one atomic per bin).
//   em_scan_kernel   above[b][tau] = #{q > tau}, and the first slot of every level in the sorted list.
//   em_scatter_kernel  counting sort: the pixels with q >= 1 into order[b], descending level. The order inside a level is free
//                    (the matching's cardinality does not depend on it), so a slot is drawn with an atomic.
//   em_state_kernel  state[t][p] of a map from its thin plane: free on a contour pixel, "far" elsewhere.
//   em_near_kernel   every contour pixel turns the "far" pixels that reach it (p - offset) into "no contour pixel": what stays far
//                    has no contour pixel in reach, and a search from it would fail at its first probe without marking anything -
//                    on a thick map that is most of the searches. The work is |Q_t| x n_off stores per map.
//   em_match_kernel  ONE 64-lane workgroup per annotator map. The wave takes 64 entries of the sorted list at a time, gathers their
//                    own state words and ballots: only the pixels that are not far are searched from. A search step at map pixel
//                    v: lane l of each 64-offset chunk forms v + offsets[l], tests it against the image and gathers the contour
//                    pixel's state; a ballot finds a free one (augment: the mates on the stack are flipped); else the lowest
//                    live, unvisited lane is marked visited and pushed, and the search goes on from its mate; else the stack is
//                    popped. An empty stack: the search failed, and every contour pixel it visited is dead for good (SPEC.md
//                    §27: the set is closed and saturated). D2 = 18, the BSD value, has 61 offsets: one gather per step.
//                    state: >= 0 the mate's pixel index (bit 30: visited by the running search), -1 free, -2 no contour pixel,
//                    -3 dead, -4 far (no contour pixel, and none in reach). The visit log of a search (every pixel it pushed)
//                    undoes the marks or turns them into dead ones.
//                    Every loop is bounded by construction: the walk by the sorted list's length, a search by cap pushes (a
//                    contour pixel is pushed at most once per search) and as many pops, a probe by ceil(n_off / 64) chunks.
//                    State stores are read by other lanes in the next step: a workgroup barrier stands between them.
// The device code knows no geometry: gcs_match_offsets (host) makes the disc's table, and any table is exact.
#include "common.h"
#include "gcs_match.h"

namespace {

typedef unsigned long long u64;
constexpr int EM_HW_MAX = 4096, EM_BT_MAX = 65535, EM_LEVELS_MAX = 256, EM_OFF_MAX = 512, EM_D2_MAX = 160;
constexpr int EM_CAP_MAX = EM_HW_MAX * EM_HW_MAX + 1;
constexpr int EM_BINS = EM_LEVELS_MAX + 1;                   // bins of a histogram row, whatever `levels` is
constexpr int EM_THREADS = 256, EM_PER_THREAD = 8;           // the per-pixel kernels
constexpr int EM_FREE = -1, EM_NOT = -2, EM_DEAD = -3, EM_FAR = -4, EM_VIS = 1 << 30, EM_MATE = EM_VIS - 1;
constexpr int EM_OFF_CLAMP = 2 * EM_HW_MAX;                  // an offset this large leaves every image

__device__ __forceinline__ int em_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int em_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------------------------------------------------------------------------------- the truth

__global__ void em_zero_kernel(int32_t *p, int n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) p[i] = 0;
}

template <typename L>
__global__ __launch_bounds__(EM_THREADS) void tt_kernel(const L *__restrict__ maps, int H, int W, uint8_t *__restrict__ thin,
                                                        int32_t *__restrict__ counts) {
    const int hw = H * W, p = (int)blockIdx.x * EM_THREADS + (int)threadIdx.x, t = (int)blockIdx.y;
    const size_t base = (size_t)t * (size_t)hw;              // 64-bit: T H W passes 2^31
    bool on = false;
    if (p < hw) {
        const int y = p / W, x = p - y * W;
        const L s = maps[base + p];
        on = (x + 1 < W && maps[base + p + 1] != s) || (y + 1 < H && maps[base + p + W] != s);
        thin[base + p] = on ? 1 : 0;
    }
    const u64 vote = __ballot(on);
    if ((threadIdx.x & 63) == 0 && vote) atomicAdd(counts + t, __popcll(vote));
}

// ---------------------------------------------------------------------------------------------------------- the sorted list

__global__ __launch_bounds__(EM_THREADS) void em_hist_kernel(const int32_t *__restrict__ q, int hw, int levels, int32_t *__restrict__ hist) {
    __shared__ int s_hist[EM_BINS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    for (int i = tid; i < EM_BINS; i += EM_THREADS) s_hist[i] = 0;
    __syncthreads();
    const int32_t *img = q + (size_t)b * (size_t)hw;
    const int p0 = (int)blockIdx.x * EM_THREADS * EM_PER_THREAD + tid;
#pragma unroll
    for (int j = 0; j < EM_PER_THREAD; ++j) {
        const int p = p0 + j * EM_THREADS;
        if (p < hw) atomicAdd(&s_hist[em_clamp(img[p], 0, levels)], 1);
    }
    __syncthreads();
    for (int i = tid; i < EM_BINS; i += EM_THREADS)
        if (s_hist[i]) atomicAdd(hist + b * EM_BINS + i, s_hist[i]);
}

// above[b][tau] = the bins above tau; cursor[b][v] = the first slot of level v in order[b] = above[b][v]
__global__ __launch_bounds__(64) void em_scan_kernel(const int32_t *__restrict__ hist, int levels, int32_t *__restrict__ cursor,
                                                     int32_t *__restrict__ above) {
    const int b = (int)blockIdx.x;
    if (threadIdx.x != 0) return;
    int run = 0;
    for (int v = levels; v >= 1; --v) {
        cursor[b * EM_BINS + v] = run;
        run += hist[b * EM_BINS + v];
        above[b * levels + v - 1] = run;
    }
}

__global__ __launch_bounds__(EM_THREADS) void em_scatter_kernel(const int32_t *__restrict__ q, int hw, int levels, int32_t *__restrict__ cursor,
                                                                int32_t *__restrict__ order) {
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const int32_t *img = q + (size_t)b * (size_t)hw;
    int32_t *list = order + (size_t)b * (size_t)hw;
    const int p0 = (int)blockIdx.x * EM_THREADS * EM_PER_THREAD + tid;
#pragma unroll
    for (int j = 0; j < EM_PER_THREAD; ++j) {
        const int p = p0 + j * EM_THREADS;
        if (p >= hw) continue;
        const int v = em_clamp(img[p], 0, levels);
        if (v < 1) continue;
        const int slot = atomicAdd(cursor + b * EM_BINS + v, 1);
        if ((unsigned)slot < (unsigned)hw) list[slot] = p;   // (always, while q holds what the histogram saw)
    }
}

__global__ __launch_bounds__(EM_THREADS) void em_state_kernel(const uint8_t *__restrict__ thin, int hw, int32_t *__restrict__ state) {
    const int p = (int)blockIdx.x * EM_THREADS + (int)threadIdx.x;
    const size_t at = (size_t)blockIdx.y * (size_t)hw + (size_t)p;
    if (p < hw) state[at] = thin[at] ? EM_FREE : EM_FAR;
}

// A contour pixel u is reached from v = u - offset: those of them that are no contour pixels themselves stop being far. Every
// store of a word stores the same value, and contour pixels' words are not touched: no order matters.
__global__ __launch_bounds__(EM_THREADS) void em_near_kernel(const uint8_t *__restrict__ thin, int H, int W, const int32_t *__restrict__ offsets,
                                                             int n_off, int32_t *__restrict__ state) {
    const int hw = H * W, p = (int)blockIdx.x * EM_THREADS + (int)threadIdx.x;
    const size_t base = (size_t)blockIdx.y * (size_t)hw;
    if (p >= hw || !thin[base + p]) return;
    const int y = p / W, x = p - y * W;
    for (int i = 0; i < n_off; ++i) {
        const int yy = y - em_clamp(offsets[2 * i], -EM_OFF_CLAMP, EM_OFF_CLAMP);
        const int xx = x - em_clamp(offsets[2 * i + 1], -EM_OFF_CLAMP, EM_OFF_CLAMP);
        if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
        const int v = yy * W + xx;
        if (!thin[base + v]) state[base + v] = EM_NOT;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the matcher

__global__ __launch_bounds__(64) void em_match_kernel(const int32_t *__restrict__ img_of, int B, int H, int W, int levels,
                                                      const int32_t *__restrict__ offsets, int n_off, int cap,
                                                      const int32_t *__restrict__ order_all, int32_t *state_all, int32_t *stack_all,
                                                      int32_t *log_all, uint32_t *stats, const int32_t *above_all, int32_t *matched) {
    __shared__ int s_dy[EM_OFF_MAX], s_dx[EM_OFF_MAX];
    const int lane = (int)threadIdx.x, t = (int)blockIdx.x, hw = H * W;
    int32_t *row = matched + (size_t)t * (size_t)levels;
    const int b = em_uniform(img_of[t]);
    if ((unsigned)b >= (unsigned)B) {                        // no such image: the row says so
        for (int i = lane; i < levels; i += 64) row[i] = -1;
        if (lane < 4) stats[4 * t + lane] = 0;
        return;
    }
    for (int i = lane; i < n_off; i += 64) {
        s_dy[i] = em_clamp(offsets[2 * i], -EM_OFF_CLAMP, EM_OFF_CLAMP);
        s_dx[i] = em_clamp(offsets[2 * i + 1], -EM_OFF_CLAMP, EM_OFF_CLAMP);
    }
    __syncthreads();
    const int32_t *order = order_all + (size_t)b * (size_t)hw;
    const int32_t *above = above_all + (size_t)b * (size_t)levels;
    int32_t *state = state_all + (size_t)t * (size_t)hw;     // 64-bit: T H W passes 2^31
    int32_t *stack = stack_all + (size_t)t * (size_t)cap * 2;      // [cap][2]: the contour pixel pushed, the map pixel it was pushed from
    int32_t *visit = log_all + (size_t)t * (size_t)cap;      // every contour pixel the running search pushed
    const int chunks = (n_off + 63) >> 6;
    int count = 0;
    unsigned steps = 0, probes = 0, deepest = 0, failed = 0;
    bool over = false;

    for (int lv = levels; lv >= 1 && !over; --lv) {
        const int begin = lv == levels ? 0 : em_clamp(em_uniform(above[lv]), 0, hw), end = em_clamp(em_uniform(above[lv - 1]), 0, hw);
        for (int base = begin; base < end && !over; base += 64) {
            const int mine = base + lane < end ? order[base + lane] : -1;
            // (a pixel's own word is far or not for good: searches change the words of contour pixels only)
            u64 todo = __ballot((unsigned)mine < (unsigned)hw && state[mine] != EM_FAR);
            while (todo && !over) {
                const int v0 = em_uniform(__shfl(mine, __ffsll(todo) - 1));
                todo &= todo - 1;
                int depth = 0, logn = 0, cur = v0;
                for (;;) {                                   // one step: a push, a pop or the search's end
                    ++steps;
                    const int y = cur / W, x = cur - y * W;
                    int fu = -1, next = -1, nextmate = 0;
                    for (int c = 0; c < chunks; ++c) {
                        ++probes;
                        const int i = c * 64 + lane;
                        int u = -1, st = EM_NOT;
                        if (i < n_off) {
                            const int yy = y + s_dy[i], xx = x + s_dx[i];
                            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                                u = yy * W + xx;
                                st = state[u];
                            }
                        }
                        const u64 fr = __ballot(st == EM_FREE);
                        if (fr) {
                            fu = em_uniform(__shfl(u, __ffsll(fr) - 1));
                            break;
                        }
                        if (next < 0) {
                            const u64 live = __ballot(st >= 0 && !(st & EM_VIS));
                            if (live) {
                                const int l = __ffsll(live) - 1;
                                next = em_uniform(__shfl(u, l));
                                nextmate = em_uniform(__shfl(st, l));
                            }
                        }
                    }
                    if (fu >= 0) {                           // augment: the marks go, then the path's mates move one down
                        for (int j = lane; j < logn; j += 64) state[visit[j]] &= EM_MATE;
                        __syncthreads();
                        for (int i = lane; i < depth; i += 64) state[stack[2 * i]] = stack[2 * i + 1];
                        if (lane == 0) state[fu] = cur;
                        __syncthreads();
                        ++count;
                        break;
                    }
                    if (next >= 0) {
                        if (logn >= cap) {
                            over = true;
                            break;
                        }
                        if (lane == 0) {
                            state[next] = nextmate | EM_VIS;
                            stack[2 * depth] = next;
                            stack[2 * depth + 1] = cur;
                            visit[logn] = next;
                        }
                        ++depth, ++logn;
                        cur = nextmate;
                        deepest = (unsigned)depth > deepest ? (unsigned)depth : deepest;
                        __syncthreads();
                        continue;
                    }
                    if (depth == 0) {                        // failed: what it visited is closed and saturated - dead for good
                        for (int j = lane; j < logn; j += 64) state[visit[j]] = EM_DEAD;
                        __syncthreads();
                        ++failed;
                        break;
                    }
                    --depth;
                    cur = em_uniform(stack[2 * depth + 1]);
                }
            }
        }
        if (!over && lane == 0) row[lv - 1] = count;
    }
    if (over) {
        __syncthreads();
        for (int i = lane; i < levels; i += 64) row[i] = -1;
    }
    if (lane == 0) {
        stats[4 * t] = steps, stats[4 * t + 1] = probes, stats[4 * t + 2] = deepest, stats[4 * t + 3] = failed;
    }
}

// ------------------------------------------------------------------------------------------------------------------- host

struct EmLayout {
    size_t stats, hist, cursor, order, state, stack, log, total;
};

size_t em_align(size_t v) { return (v + 255) / 256 * 256; }

EmLayout em_layout(int B, int T, int H, int W, int cap) {
    EmLayout lo;
    const size_t hw = (size_t)H * (size_t)W;
    size_t at = 0;
    lo.stats = at, at = em_align(at + (size_t)T * 16);
    lo.hist = at, at = em_align(at + (size_t)B * EM_BINS * 4);
    lo.cursor = at, at = em_align(at + (size_t)B * EM_BINS * 4);
    lo.order = at, at = em_align(at + (size_t)B * hw * 4);
    lo.state = at, at = em_align(at + (size_t)T * hw * 4);
    lo.stack = at, at = em_align(at + (size_t)T * (size_t)cap * 8);
    lo.log = at, at = em_align(at + (size_t)T * (size_t)cap * 4);
    lo.total = at;
    return lo;
}

bool em_shape_ok(int B, int T, int H, int W, int cap) {
    return B >= 1 && B <= EM_BT_MAX && T >= 1 && T <= EM_BT_MAX && H >= 1 && H <= EM_HW_MAX && W >= 1 && W <= EM_HW_MAX && cap >= 1 &&
           cap <= EM_CAP_MAX;
}

bool em_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int gcs_match_offsets(int d2, int32_t *offsets_out, int *n_out) {
    if (!offsets_out || !n_out) return gcs_fail(GCS_EINVAL, "gcs_match_offsets: NULL pointer");
    if (d2 < 0 || d2 > EM_D2_MAX) return gcs_fail(GCS_EINVAL, "gcs_match_offsets: bad argument (0 <= d2 <= 160)");
    int reach = 0;
    while ((reach + 1) * (reach + 1) <= d2) ++reach;
    int n = 0;
    for (int dy = -reach; dy <= reach; ++dy)
        for (int dx = -reach; dx <= reach; ++dx)
            if (dy * dy + dx * dx <= d2) offsets_out[2 * n] = dy, offsets_out[2 * n + 1] = dx, ++n;
    *n_out = n;
    return GCS_OK;
}

extern "C" int gcs_truth_thin(const void *maps, int T, int H, int W, int is_u8, uint8_t *thin_out, int32_t *counts_out, gcs_stream_t stream) {
    if (!maps || !thin_out || !counts_out) return gcs_fail(GCS_EINVAL, "gcs_truth_thin: NULL pointer");
    if (T < 1 || T > EM_BT_MAX || H < 1 || W < 1 || H > EM_HW_MAX || W > EM_HW_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_truth_thin: bad shape (1 <= T <= 65535, 1 <= H, W <= 4096)");
    const size_t px = (size_t)T * (size_t)H * (size_t)W, in_bytes = px * (is_u8 ? 1 : 2);
    if (em_overlap(thin_out, px, maps, in_bytes) || em_overlap(counts_out, (size_t)T * 4, maps, in_bytes) ||
        em_overlap(thin_out, px, counts_out, (size_t)T * 4))
        return gcs_fail(GCS_EINVAL, "gcs_truth_thin: an output overlaps the maps or the other output");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(em_zero_kernel, dim3((T + 255) / 256), dim3(256), 0, st, counts_out, T);
    GCS_CHECK_LAUNCH("gcs_truth_thin (zero)");
    const dim3 grid((H * W + EM_THREADS - 1) / EM_THREADS, T);
    if (is_u8)
        hipLaunchKernelGGL(tt_kernel<uint8_t>, grid, dim3(EM_THREADS), 0, st, (const uint8_t *)maps, H, W, thin_out, counts_out);
    else
        hipLaunchKernelGGL(tt_kernel<uint16_t>, grid, dim3(EM_THREADS), 0, st, (const uint16_t *)maps, H, W, thin_out, counts_out);
    GCS_CHECK_LAUNCH("gcs_truth_thin");
    return GCS_OK;
}

extern "C" size_t gcs_edge_match_bytes(int B, int T, int H, int W, int cap) {
    if (!em_shape_ok(B, T, H, W, cap)) return 0;
    return em_layout(B, T, H, W, cap).total;
}

extern "C" int gcs_edge_match(const int32_t *q, const uint8_t *thin, const int32_t *img_of, int B, int T, int H, int W, int levels,
                              const int32_t *offsets, int n_off, int cap, void *workspace, int32_t *matched, int32_t *above,
                              gcs_stream_t stream) {
    if (!q || !thin || !img_of || !offsets || !workspace || !matched || !above) return gcs_fail(GCS_EINVAL, "gcs_edge_match: NULL pointer");
    if (!em_shape_ok(B, T, H, W, cap))
        return gcs_fail(GCS_EINVAL, "gcs_edge_match: bad shape (1 <= B, T <= 65535, 1 <= H, W <= 4096, 1 <= cap <= 16777217)");
    if (levels < 1 || levels > EM_LEVELS_MAX || n_off < 1 || n_off > EM_OFF_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_edge_match: bad argument (1 <= levels <= 256, 1 <= n_off <= 512)");
    if ((uintptr_t)workspace % 256) return gcs_fail(GCS_EINVAL, "gcs_edge_match: the workspace is not 256-byte aligned");
    const EmLayout lo = em_layout(B, T, H, W, cap);
    const size_t hw = (size_t)H * (size_t)W;
    const void *in[4] = {q, thin, img_of, offsets};
    const size_t in_bytes[4] = {(size_t)B * hw * 4, (size_t)T * hw, (size_t)T * 4, (size_t)n_off * 8};
    const void *out[3] = {workspace, matched, above};
    const size_t out_bytes[3] = {lo.total, (size_t)T * levels * 4, (size_t)B * levels * 4};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 4; ++i)
            if (em_overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return gcs_fail(GCS_EINVAL, "gcs_edge_match: an output overlaps an input");
        for (int p = o + 1; p < 3; ++p)
            if (em_overlap(out[o], out_bytes[o], out[p], out_bytes[p])) return gcs_fail(GCS_EINVAL, "gcs_edge_match: two outputs overlap");
    }
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    uint32_t *stats = (uint32_t *)(ws + lo.stats);
    int32_t *hist = (int32_t *)(ws + lo.hist), *cursor = (int32_t *)(ws + lo.cursor), *order = (int32_t *)(ws + lo.order);
    int32_t *state = (int32_t *)(ws + lo.state), *stack = (int32_t *)(ws + lo.stack), *log = (int32_t *)(ws + lo.log);
    const int ihw = H * W;
    const dim3 per_px((ihw + EM_THREADS * EM_PER_THREAD - 1) / (EM_THREADS * EM_PER_THREAD), B);
    hipLaunchKernelGGL(em_zero_kernel, dim3((B * EM_BINS + 255) / 256), dim3(256), 0, st, hist, B * EM_BINS);
    GCS_CHECK_LAUNCH("gcs_edge_match (zero)");
    hipLaunchKernelGGL(em_hist_kernel, per_px, dim3(EM_THREADS), 0, st, q, ihw, levels, hist);
    GCS_CHECK_LAUNCH("gcs_edge_match (histogram)");
    hipLaunchKernelGGL(em_scan_kernel, dim3(B), dim3(64), 0, st, hist, levels, cursor, above);
    GCS_CHECK_LAUNCH("gcs_edge_match (scan)");
    hipLaunchKernelGGL(em_scatter_kernel, per_px, dim3(EM_THREADS), 0, st, q, ihw, levels, cursor, order);
    GCS_CHECK_LAUNCH("gcs_edge_match (sort)");
    hipLaunchKernelGGL(em_state_kernel, dim3((ihw + EM_THREADS - 1) / EM_THREADS, T), dim3(EM_THREADS), 0, st, thin, ihw, state);
    GCS_CHECK_LAUNCH("gcs_edge_match (state)");
    hipLaunchKernelGGL(em_near_kernel, dim3((ihw + EM_THREADS - 1) / EM_THREADS, T), dim3(EM_THREADS), 0, st, thin, H, W, offsets, n_off, state);
    GCS_CHECK_LAUNCH("gcs_edge_match (near)");
    hipLaunchKernelGGL(em_match_kernel, dim3(T), dim3(64), 0, st, img_of, B, H, W, levels, offsets, n_off, cap, order, state, stack, log, stats,
                       above, matched);
    GCS_CHECK_LAUNCH("gcs_edge_match");
    return GCS_OK;
}
