// scoring.hip — evaluation-side kernels of libgcs.so (gfx950): boundary recall / precision counts
// (/root/reference/BSD_metrics/metrics.py:58-96), region tables (metrics.py:102-201), region agreement (SPEC.md §8) and the two
// sweeps over a region tree's cuts (SPEC.md §15, §16) with the undersegmentation sums of every cut (SPEC.md §17; the shape counts
// of §17: cut_shapes.hip). Connected regions and the small-region merge: regions.hip.
// Nothing here allocates, frees or synchronises; every entry point enqueues on the caller's stream.
#include <limits.h>

#include "common.h"
#include "tree_cuts.h"

// ======================================================================= boundary scoring (§8f-1)
// Integer restatement of /root/reference/BSD_metrics/metrics.py:25-51,58-96 for ONE image:
//   bd(M)   = thick boundaries of an integer map M: max != min over the 3x3 cross (find_boundaries
//             defaults; reflect border == clamped indices for max/min filters)
//   dil5(b) = 5x5 binary dilation (dilation(., rectangle(5,5)); same border argument)
// counts[0] = sum bd(L);  per annotator a: counts[1+3a] = sum dil5(bd(L)) & bd(T_a)   (recall numerator)
//                                           counts[2+3a] = sum bd(T_a)                 (recall denominator)
//                                           counts[3+3a] = sum bd(L) & dil5(bd(T_a))   (precision numerator)
// The float divisions and the per-annotator mean stay on the host, in the reference's order.
template <typename T>
__device__ __forceinline__ bool thick_boundary(const T *m, int H, int W, int y, int x) {
    const T c = m[(size_t)y * W + x];
    const T u = m[(size_t)max(y - 1, 0) * W + x], d = m[(size_t)min(y + 1, H - 1) * W + x];
    const T l = m[(size_t)y * W + max(x - 1, 0)], r = m[(size_t)y * W + min(x + 1, W - 1)];
    return u != c || d != c || l != c || r != c;   // max != min over {c,u,d,l,r}
}

// Batched form: B label maps [B][H][W] and T annotator maps [T][H][W] (all annotators of all images, image after image);
// img_of[t] = image of annotator t (NULL: every annotator belongs to image 0, the single-image call).
// maps: planes 0..B-1 = boundaries of the label maps, planes B..B+T-1 = boundaries of the annotator maps
__global__ void boundary_maps_kernel(const int32_t *__restrict__ labels, const uint16_t *__restrict__ truth, int B, int T,
                                     int H, int W, uint8_t *__restrict__ maps) {
    const size_t n = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)(B + T) * n; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i / n), p = (int)(i % n), y = p / W, x = p % W;
        maps[i] = q < B ? thick_boundary(labels + (size_t)q * n, H, W, y, x)
                        : thick_boundary(truth + (size_t)(q - B) * n, H, W, y, x);
    }
}

// counts: [b] = sum bd(L_b) for b < B; then per annotator t: [B + 3t] = sum dil5(bd(L_b)) & bd(T_t)   (recall numerator),
// [B + 3t + 1] = sum bd(T_t) (recall denominator), [B + 3t + 2] = sum bd(L_b) & dil5(bd(T_t)) (precision numerator),
// b = img_of[t]. With B = 1 this is the single-image layout [1 + 3A].
// One workgroup per (16 x 64 pixel tile, plane q): both boundary planes of the tile go to LDS with their two-pixel halo
// (pixels outside the image count as "no boundary", as dilation(., rectangle(5,5)) treats its border), the 5 x 5 dilation
// is evaluated separably (5 horizontal ORs into LDS, 5 vertical ORs per pixel) and the three sums leave the workgroup as
// one atomic each. Round 3 walked the 25 taps in global memory with a division per pixel: 336 us for 16 BSD images and
// their 87 annotator maps, 77 % of a segment + score loop (profiles/r4_notes.md).
constexpr int BC_TH = 16, BC_TW = 64, BC_HALO = 2;
__global__ __launch_bounds__(256) void boundary_counts_kernel(const uint8_t *__restrict__ maps, const int32_t *__restrict__ img_of,
                                                              int B, int T, int H, int W, unsigned long long *__restrict__ counts) {
    __shared__ uint8_t s_raw[2][BC_TH + 2 * BC_HALO][BC_TW + 2 * BC_HALO + 4];   // [label | annotator] boundary bits with halo
    __shared__ uint8_t s_hor[2][BC_TH + 2 * BC_HALO][BC_TW];                     // OR over the 5 horizontal neighbours
    __shared__ unsigned s_sum[3];
    const size_t n = (size_t)H * W;
    const int q = blockIdx.z;                         // < B: label-only count of image q; else annotator q - B
    const int b = q < B ? q : (img_of ? img_of[q - B] : 0);
    const uint8_t *lb = maps + (size_t)b * n;
    const uint8_t *tb = maps + (size_t)q * n;         // annotator plane (q >= B)
    const int x0 = blockIdx.x * BC_TW, y0 = blockIdx.y * BC_TH, tid = threadIdx.x;
    unsigned c0 = 0, c1 = 0, c2 = 0;
    if (tid < 3) s_sum[tid] = 0;
    if (q < B) {                                      // sum bd(L_q): no stencil
        for (int i = tid; i < BC_TH * BC_TW; i += 256) {
            const int y = y0 + i / BC_TW, x = x0 + i % BC_TW;
            if (y < H && x < W) c0 += lb[(size_t)y * W + x];
        }
    } else {
        constexpr int RW = BC_TW + 2 * BC_HALO, RH = BC_TH + 2 * BC_HALO;
        for (int i = tid; i < RH * RW; i += 256) {
            const int r = i / RW, c = i % RW, y = y0 + r - BC_HALO, x = x0 + c - BC_HALO;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            s_raw[0][r][c] = in ? lb[(size_t)y * W + x] : (uint8_t)0;
            s_raw[1][r][c] = in ? tb[(size_t)y * W + x] : (uint8_t)0;
        }
        __syncthreads();
        for (int i = tid; i < RH * BC_TW; i += 256) {
            const int r = i / BC_TW, c = i % BC_TW;
#pragma unroll
            for (int m = 0; m < 2; ++m)
                s_hor[m][r][c] = s_raw[m][r][c] | s_raw[m][r][c + 1] | s_raw[m][r][c + 2] | s_raw[m][r][c + 3] | s_raw[m][r][c + 4];
        }
        __syncthreads();
        for (int i = tid; i < BC_TH * BC_TW; i += 256) {
            const int r = i / BC_TW, c = i % BC_TW;
            if (y0 + r < H && x0 + c < W) {
                const unsigned bl = s_raw[0][r + BC_HALO][c + BC_HALO], bt = s_raw[1][r + BC_HALO][c + BC_HALO];
                const unsigned dl = s_hor[0][r][c] | s_hor[0][r + 1][c] | s_hor[0][r + 2][c] | s_hor[0][r + 3][c] | s_hor[0][r + 4][c];
                const unsigned dt = s_hor[1][r][c] | s_hor[1][r + 1][c] | s_hor[1][r + 2][c] | s_hor[1][r + 3][c] | s_hor[1][r + 4][c];
                c0 += bt & dl;                        // recall numerator
                c1 += bt;                             // recall denominator
                c2 += bl & dt;                        // precision numerator
            }
        }
    }
    // wave reduction, then one atomic per sum and workgroup (integers: order-independent)
    for (int m = 32; m >= 1; m >>= 1) {
        c0 += __shfl_xor(c0, m);
        c1 += __shfl_xor(c1, m);
        c2 += __shfl_xor(c2, m);
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        atomicAdd(&s_sum[0], c0);
        atomicAdd(&s_sum[1], c1);
        atomicAdd(&s_sum[2], c2);
    }
    __syncthreads();
    if (tid == 0) {
        if (q < B) {
            if (s_sum[0]) atomicAdd(&counts[q], (unsigned long long)s_sum[0]);
        } else {
            if (s_sum[0]) atomicAdd(&counts[B + 3 * (q - B)], (unsigned long long)s_sum[0]);
            if (s_sum[1]) atomicAdd(&counts[B + 3 * (q - B) + 1], (unsigned long long)s_sum[1]);
            if (s_sum[2]) atomicAdd(&counts[B + 3 * (q - B) + 2], (unsigned long long)s_sum[2]);
        }
    }
}

extern "C" size_t gcs_boundary_scratch_bytes(int A, int H, int W) {
    if (A <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)(A + 1) * H * W;
}
extern "C" size_t gcs_boundary_batch_scratch_bytes(int B, int T, int H, int W) {
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)(B + T) * H * W;
}

static int boundary_counts_launch(const int32_t *labels, const uint16_t *truth, const int32_t *img_of, int B, int T, int H,
                                  int W, void *scratch, uint64_t *counts, hipStream_t stream, const char *who) {
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)(B + 3 * T) * sizeof(uint64_t), stream);
    if (e != hipSuccess) return gcs_hip_fail(e, who);
    uint8_t *maps = static_cast<uint8_t *>(scratch);
    const int n = H * W;
    const size_t total = (size_t)(B + T) * n;
    hipLaunchKernelGGL(boundary_maps_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)),
                       dim3(256), 0, stream, labels, truth, B, T, H, W, maps);
    GCS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(boundary_counts_kernel, dim3((W + BC_TW - 1) / BC_TW, (H + BC_TH - 1) / BC_TH, B + T), dim3(256), 0, stream,
                       maps, img_of, B, T, H, W, reinterpret_cast<unsigned long long *>(counts));
    GCS_CHECK_LAUNCH(who);
    return GCS_OK;
}

extern "C" int gcs_boundary_counts(const int32_t *labels, const uint16_t *truth, int A, int H, int W, void *scratch,
                                   uint64_t *counts, gcs_stream_t stream) {
    if (!labels || !truth || !scratch || !counts) return gcs_fail(GCS_EINVAL, "gcs_boundary_counts: NULL pointer");
    if (A <= 0 || A > 65534 || H <= 0 || W <= 0 || (long long)H * W * (A + 1) > 0x7fffffffLL)
        return gcs_fail(GCS_EINVAL, "gcs_boundary_counts: bad shape");
    return boundary_counts_launch(labels, truth, nullptr, 1, A, H, W, scratch, counts, stream, "gcs_boundary_counts");
}

extern "C" int gcs_boundary_counts_batch(const int32_t *labels, const uint16_t *truth, const int32_t *img_of, int B, int T,
                                         int H, int W, void *scratch, uint64_t *counts, gcs_stream_t stream) {
    if (!labels || !truth || !img_of || !scratch || !counts)
        return gcs_fail(GCS_EINVAL, "gcs_boundary_counts_batch: NULL pointer");
    if (B <= 0 || T <= 0 || B + T > 65535 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
        return gcs_fail(GCS_EINVAL, "gcs_boundary_counts_batch: bad shape");
    return boundary_counts_launch(labels, truth, img_of, B, T, H, W, scratch, counts, stream, "gcs_boundary_counts_batch");
}

// ============================================================ boundary scoring on resident ground truth (round 5)
// The annotator maps are constants of the data set (/root/reference/BSD_metrics/metrics.py:48-49 recomputes
// find_boundaries(truth) for every image it scores, groundtruth.py:44-48 rescans the directories per id): their thick boundaries
// bd(T_t), the 5x5 dilation dil5(bd(T_t)) and sum bd(T_t) are computed ONCE per annotator map (gcs_truth_prepare) and kept on the
// device as BIT planes, rows of 64-bit words (bit i of word w of a row = pixel 64 w + i), all bd planes first, then all dil5
// planes. A scoring call derives the two bit planes of each label map and the three sums are AND + popcount over 2 568 words per
// plane (321 x 481): kilobytes, where round 4 uploaded 40 MB of annotator maps per 24 images and re-derived 129 byte planes.
__host__ __device__ static inline int bits_wp(int W) { return (W + 63) / 64; }

// bd bit planes of M maps: one wave per 64 consecutive pixels of a row (coalesced), the plane word by ballot. `smax`: per-map
// maximum value (metrics.py:51 for the label maps; zeroed by the caller), or NULL.
template <typename T>
__global__ __launch_bounds__(256) void bits_boundary_kernel(const T *__restrict__ maps, int M, int H, int W,
                                                            unsigned long long *__restrict__ bd, int *__restrict__ smax) {
    const int wp = bits_wp(W);
    const long long nw = (long long)M * H * wp;
    const int lane = threadIdx.x & 63;
    for (long long wi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); wi < nw; wi += (long long)gridDim.x * 4) {
        const int wx = (int)(wi % wp), y = (int)((wi / wp) % H), m = (int)(wi / ((long long)wp * H));
        const int x = wx * 64 + lane;
        const T *mp = maps + (size_t)m * H * W;
        bool b = false;
        int v = 0;
        if (x < W) {
            b = thick_boundary(mp, H, W, y, x);
            v = (int)mp[(size_t)y * W + x];
        }
        const unsigned long long word = __ballot(b);
        if (lane == 0) bd[wi] = word;
        if (smax) {
            // one atomic per wave only while it can still raise the maximum: unconditional, 41 000 waves hammered 16 addresses and
            // this kernel took 305 us for 16 BSD label maps (6 us without)
            for (int s = 32; s >= 1; s >>= 1) v = max(v, __shfl_xor(v, s));
            if (lane == 0 && v > __hip_atomic_load(&smax[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&smax[m], v);
        }
    }
}

// dil5 bit planes: OR over the 5 x 5 neighbourhood; pixels outside the image count as 0 (dilation(., rectangle(5,5)) through
// scipy's max filter with its reflect border sees in-image values only)
__global__ __launch_bounds__(256) void bits_dilate_kernel(const unsigned long long *__restrict__ bd, int M, int H, int W,
                                                          unsigned long long *__restrict__ dil) {
    const int wp = bits_wp(W);
    const long long nw = (long long)M * H * wp;
    const unsigned long long last_mask = (W & 63) ? ((1ull << (W & 63)) - 1) : ~0ull;
    for (long long wi = (long long)blockIdx.x * blockDim.x + threadIdx.x; wi < nw; wi += (long long)gridDim.x * blockDim.x) {
        const int wx = (int)(wi % wp), y = (int)((wi / wp) % H);
        const unsigned long long *row0 = bd + (wi - wx) - (long long)y * wp;    // row 0 of this map
        unsigned long long acc = 0;
        for (int dy = -2; dy <= 2; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            const unsigned long long *r = row0 + (long long)yy * wp;
            const unsigned long long w = r[wx], pv = wx > 0 ? r[wx - 1] : 0ull, nx = wx + 1 < wp ? r[wx + 1] : 0ull;
            acc |= w | (w << 1) | (w << 2) | (w >> 1) | (w >> 2) | (pv >> 63) | (pv >> 62) | (nx << 63) | (nx << 62);
        }
        dil[wi] = wx == wp - 1 ? acc & last_mask : acc;
    }
}

__global__ __launch_bounds__(256) void bits_popcount_kernel(const unsigned long long *__restrict__ planes, int words,
                                                            unsigned long long *__restrict__ out) {
    __shared__ unsigned s_sum[4];
    const unsigned long long *p = planes + (size_t)blockIdx.x * words;
    unsigned c = 0;
    for (int i = threadIdx.x; i < words; i += 256) c += __popcll(p[i]);
    for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (unsigned long long)s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// One workgroup per output plane q (no atomics, no zeroing): q < B: counts[q] = sum bd(L_q); else annotator t = q - B of image
// b = img_of[t]: counts[B + 3t] = sum dil5(bd(L_b)) & bd(T_t), [B + 3t + 1] = sum bd(T_t) (prepared), [B + 3t + 2] = sum bd(L_b) &
// dil5(bd(T_t)). Annotator planes [2][T][words] (bd, then dil5); label planes [2][B][words].
// (Dilating the label planes word by word in here instead, one launch less, measured 28 us against 5 + 8: not done.)
__global__ __launch_bounds__(256) void bits_counts_kernel(const unsigned long long *__restrict__ lab,
                                                          const unsigned long long *__restrict__ tru,
                                                          const unsigned long long *__restrict__ tru_bd_counts,
                                                          const int32_t *__restrict__ img_of, int B, int T, int H, int W,
                                                          unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_sum[2][4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int words = H * bits_wp(W);
    unsigned c0 = 0, c1 = 0;
    if (q < B) {
        const unsigned long long *l = lab + (size_t)q * words;
        for (int i = tid; i < words; i += 256) c0 += __popcll(l[i]);
    } else {
        const int t = q - B, b = img_of[t];
        const unsigned long long *lbd = lab + (size_t)b * words, *ldil = lab + ((size_t)B + b) * words;
        const unsigned long long *tbd = tru + (size_t)t * words, *tdil = tru + ((size_t)T + t) * words;
        for (int i = tid; i < words; i += 256) {
            c0 += __popcll(ldil[i] & tbd[i]);
            c1 += __popcll(lbd[i] & tdil[i]);
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        c0 += __shfl_xor(c0, s);
        c1 += __shfl_xor(c1, s);
    }
    if ((tid & 63) == 0) {
        s_sum[0][tid >> 6] = c0;
        s_sum[1][tid >> 6] = c1;
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long r0 = (unsigned long long)s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
        const unsigned long long r1 = (unsigned long long)s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
        if (q < B) counts[q] = r0;
        else {
            counts[B + 3 * (q - B)] = r0;
            counts[B + 3 * (q - B) + 1] = tru_bd_counts[q - B];
            counts[B + 3 * (q - B) + 2] = r1;
        }
    }
}

// several small buffers zeroed in ONE launch (a hipMemsetAsync each is a launch each)
struct ZeroList { unsigned *p[4]; unsigned n[4]; };
__global__ void zero_kernel(ZeroList z) {
    for (int k = 0; k < 4; ++k)
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < z.n[k]; i += gridDim.x * blockDim.x) z.p[k][i] = 0u;
}

__global__ void narrow_u16_u8_kernel(const uint16_t *__restrict__ in, size_t n, uint8_t *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = (uint8_t)in[i];
}

static inline unsigned grid_for(long long items, int per_block, unsigned cap) {
    const long long g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

extern "C" size_t gcs_bit_planes_bytes(int M, int H, int W) {
    if (M <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)M * 2 * H * bits_wp(W) * sizeof(unsigned long long);
}

extern "C" int gcs_truth_prepare(const uint16_t *truth, int T, int H, int W, void *planes, uint64_t *bd_counts, uint8_t *truth8,
                                 gcs_stream_t stream) {
    if (!truth || !planes || !bd_counts) return gcs_fail(GCS_EINVAL, "gcs_truth_prepare: NULL pointer");
    if (T <= 0 || T > 1000000 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
        return gcs_fail(GCS_EINVAL, "gcs_truth_prepare: bad shape");
    const int words = H * bits_wp(W);
    const long long nw = (long long)T * words;
    unsigned long long *bd = static_cast<unsigned long long *>(planes), *dil = bd + nw;
    hipLaunchKernelGGL(bits_boundary_kernel<uint16_t>, dim3(grid_for(nw, 4, 16384)), dim3(256), 0, stream, truth, T, H, W, bd,
                       (int *)nullptr);
    GCS_CHECK_LAUNCH("gcs_truth_prepare(boundaries)");
    hipLaunchKernelGGL(bits_dilate_kernel, dim3(grid_for(nw, 256, 16384)), dim3(256), 0, stream, bd, T, H, W, dil);
    GCS_CHECK_LAUNCH("gcs_truth_prepare(dilation)");
    hipLaunchKernelGGL(bits_popcount_kernel, dim3(T), dim3(256), 0, stream, bd, words, reinterpret_cast<unsigned long long *>(bd_counts));
    GCS_CHECK_LAUNCH("gcs_truth_prepare(counts)");
    if (truth8) {
        const size_t n = (size_t)T * H * W;
        hipLaunchKernelGGL(narrow_u16_u8_kernel, dim3(grid_for((long long)n, 256, 8192)), dim3(256), 0, stream, truth, n, truth8);
        GCS_CHECK_LAUNCH("gcs_truth_prepare(narrow)");
    }
    return GCS_OK;
}

// The label side of the resident boundary scorer, three launches: bd(L) bit planes (+ the label maxima into seg_max, which the
// caller has zeroed, or NULL) | their dilation | the counts. scratch: the label planes [2][B][words].
static int bits_counts_launch(const int32_t *labels, const void *truth_planes, const uint64_t *truth_bd_counts, const int32_t *img_of,
                              int B, int T, int H, int W, void *scratch, uint64_t *counts, int32_t *seg_max, hipStream_t stream,
                              const char *who) {
    const long long nw = (long long)B * H * bits_wp(W);
    unsigned long long *bd = static_cast<unsigned long long *>(scratch), *dil = bd + nw;
    hipLaunchKernelGGL(bits_boundary_kernel<int32_t>, dim3(grid_for(nw, 4, 16384)), dim3(256), 0, stream, labels, B, H, W, bd, seg_max);
    GCS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(bits_dilate_kernel, dim3(grid_for(nw, 256, 16384)), dim3(256), 0, stream, bd, B, H, W, dil);
    GCS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(bits_counts_kernel, dim3(B + T), dim3(256), 0, stream, bd, static_cast<const unsigned long long *>(truth_planes),
                       reinterpret_cast<const unsigned long long *>(truth_bd_counts), img_of, B, T, H, W,
                       reinterpret_cast<unsigned long long *>(counts));
    GCS_CHECK_LAUNCH(who);
    return GCS_OK;
}

extern "C" int gcs_boundary_counts_resident(const int32_t *labels, const void *truth_planes, const uint64_t *truth_bd_counts,
                                            const int32_t *img_of, int B, int T, int H, int W, void *scratch, uint64_t *counts,
                                            int32_t *seg_max, gcs_stream_t stream) {
    if (!labels || !truth_planes || !truth_bd_counts || !img_of || !scratch || !counts)
        return gcs_fail(GCS_EINVAL, "gcs_boundary_counts_resident: NULL pointer");
    if (B <= 0 || T <= 0 || B + T > 1000000 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
        return gcs_fail(GCS_EINVAL, "gcs_boundary_counts_resident: bad shape");
    if (seg_max) {
        hipError_t e = hipMemsetAsync(seg_max, 0, (size_t)B * sizeof(int32_t), stream);
        if (e != hipSuccess) return gcs_hip_fail(e, "gcs_boundary_counts_resident(memset)");
    }
    return bits_counts_launch(labels, truth_planes, truth_bd_counts, img_of, B, T, H, W, scratch, counts, seg_max, stream,
                              "gcs_boundary_counts_resident");
}

// ================================================= boundary counts of every cut of a region tree at once (SPEC.md §15)
// A contour map U (gcs_region_tree_contours) holds, per pixel, the level at which its boundary disappears: the thick boundary of the
// cut at R is U > tau, tau = max(0, alive - R), and its 5 x 5 dilation is M5(U) > tau, M5 = the maximum of U over the window clipped
// to the image. So the three counts gcs_boundary_counts_resident returns for ONE cut are suffix sums of three histograms of U:
//   hist [b][s]          = #{ U = s }                       rows 0 .. B-1
//   hist [B + 2t][s]     = #{ bd(T_t)   : M5(U) = s }       (recall numerator)
//   hist [B + 2t + 1][s] = #{ dil5(T_t) : U = s }           (precision numerator)        s = 1 .. K; bin 0 stays 0
// One workgroup per 16 x 64 tile of one image: U with a two-pixel halo in LDS (outside the image: INT_MIN, it never wins a
// maximum), the 5 x 5 maximum separably, then only pixels with U or M5 in 1 .. K touch the annotator bit planes and a histogram.
// The annotators of image b are the run of t with img_of[t] = b (img_of is non-decreasing: PackedTruth.stack's order). The
// (1 + 2 A_b)(K + 1) counters of the image sit in LDS when they fit the launch's SW_LDS_COUNTERS and leave with one vector atomic
// per non-zero counter; otherwise every count is a global atomic (slow, exact). Integer counts: any order, the same bits.
constexpr int SW_TH = 16, SW_TW = 64, SW_HALO = 2;             // (SW_LDS_COUNTERS: tree_cuts.h)
__global__ __launch_bounds__(256) void boundary_sweep_kernel(const int32_t *__restrict__ contours,
                                                             const unsigned long long *__restrict__ tru,
                                                             const int32_t *__restrict__ img_of, int B, int T, int H, int W, int K,
                                                             int lds_counters, unsigned *__restrict__ hist) {
    extern __shared__ unsigned sw_hist[];
    __shared__ int s_u[SW_TH + 2 * SW_HALO][SW_TW + 2 * SW_HALO + 1];
    __shared__ int s_hor[SW_TH + 2 * SW_HALO][SW_TW];
    __shared__ int s_t[2];
    const int tid = threadIdx.x, b = blockIdx.z, y0 = blockIdx.y * SW_TH, x0 = blockIdx.x * SW_TW;
    const int32_t *u = contours + (size_t)b * H * W;
    if (tid < 2) s_t[tid] = 0;
    __syncthreads();
    int below = 0, upto = 0;
    for (int t = tid; t < T; t += 256) {
        const int i = img_of[t];
        below += i < b ? 1 : 0;
        upto += i <= b ? 1 : 0;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        below += __shfl_xor(below, s);
        upto += __shfl_xor(upto, s);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_t[0], below);
        atomicAdd(&s_t[1], upto);
    }
    for (int i = tid; i < (SW_TH + 2 * SW_HALO) * (SW_TW + 2 * SW_HALO); i += 256) {
        const int r = i / (SW_TW + 2 * SW_HALO), c = i % (SW_TW + 2 * SW_HALO);
        const int y = y0 + r - SW_HALO, x = x0 + c - SW_HALO;
        s_u[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? u[(size_t)y * W + x] : INT_MIN;
    }
    __syncthreads();
    const int t0 = s_t[0], A = s_t[1] - s_t[0], E = K + 1;
    const long long want = (long long)(1 + 2 * A) * E;
    const bool local = want <= (long long)lds_counters;                    // (uniform over the workgroup)
    if (local)
        for (int i = tid; i < (int)want; i += 256) sw_hist[i] = 0u;
    for (int i = tid; i < (SW_TH + 2 * SW_HALO) * SW_TW; i += 256) {
        const int r = i / SW_TW, c = i % SW_TW;
        int m = s_u[r][c];
#pragma unroll
        for (int d = 1; d <= 2 * SW_HALO; ++d) m = max(m, s_u[r][c + d]);
        s_hor[r][c] = m;
    }
    __syncthreads();
    const int wp = bits_wp(W);
    const size_t words = (size_t)H * wp;
    unsigned *g_map = hist + (size_t)b * E, *g_ann = hist + ((size_t)B + 2 * (size_t)t0) * E;
    for (int i = tid; i < SW_TH * SW_TW; i += 256) {
        const int ty = i / SW_TW, tx = i % SW_TW, y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const int v = s_u[ty + SW_HALO][tx + SW_HALO];
        int m5 = s_hor[ty][tx];
#pragma unroll
        for (int d = 1; d <= 2 * SW_HALO; ++d) m5 = max(m5, s_hor[ty + d][tx]);
        const bool v_ok = v >= 1 && v <= K, m_ok = m5 >= 1 && m5 <= K;   // a value outside 1 .. K is counted nowhere
        if (!v_ok && !m_ok) continue;
        if (v_ok) atomicAdd(local ? &sw_hist[v] : &g_map[v], 1u);
        const size_t wi = (size_t)y * wp + (x >> 6);
        const int bit = x & 63;
        for (int a = 0; a < A; ++a) {
            if (m_ok && ((tru[(size_t)(t0 + a) * words + wi] >> bit) & 1ull))
                atomicAdd(local ? &sw_hist[(size_t)(1 + 2 * a) * E + m5] : &g_ann[(size_t)(2 * a) * E + m5], 1u);
            if (v_ok && ((tru[((size_t)T + t0 + a) * words + wi] >> bit) & 1ull))
                atomicAdd(local ? &sw_hist[(size_t)(2 + 2 * a) * E + v] : &g_ann[(size_t)(2 * a + 1) * E + v], 1u);
        }
    }
    if (!local) return;
    __syncthreads();
    for (int i = tid; i < (int)want; i += 256) {
        const unsigned c = sw_hist[i];
        if (c) atomicAdd(i < E ? &g_map[i] : &g_ann[i - E], c);
    }
}

extern "C" int gcs_boundary_sweep_resident(const int32_t *contours, const void *truth_planes, const int32_t *img_of, int B, int T,
                                           int H, int W, int K, uint32_t *hist_out, gcs_stream_t stream) {
    if (!contours || !truth_planes || !img_of || !hist_out) return gcs_fail(GCS_EINVAL, "gcs_boundary_sweep_resident: NULL pointer");
    if (B < 1 || B > 65535 || T < 1 || T > 1000000 || H < 1 || W < 1 || H > 4096 || W > 4096 || K < 1 || K > 4096)
        return gcs_fail(GCS_EINVAL, "gcs_boundary_sweep_resident: bad shape (1 <= B <= 65535, 1 <= T <= 1000000, 1 <= H, W <= 4096, 1 <= K <= 4096)");
    const long long n = ((long long)B + 2LL * T) * (K + 1);
    if (n > 0x7fffffffLL) return gcs_fail(GCS_EINVAL, "gcs_boundary_sweep_resident: (B + 2 T)(K + 1) must be below 2^31");
    ZeroList z{};
    z.p[0] = hist_out;
    z.n[0] = (unsigned)n;
    hipLaunchKernelGGL(zero_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, z);
    GCS_CHECK_LAUNCH("gcs_boundary_sweep_resident(zero)");
    const long long most = (1LL + 2LL * T) * (K + 1);                      // (the kernel decides per image: A_b is data)
    const int lds_counters = (int)(most < SW_LDS_COUNTERS ? most : SW_LDS_COUNTERS);
    hipLaunchKernelGGL(boundary_sweep_kernel, dim3((W + SW_TW - 1) / SW_TW, (H + SW_TH - 1) / SW_TH, B), dim3(256),
                       (size_t)lds_counters * sizeof(unsigned), stream, contours, static_cast<const unsigned long long *>(truth_planes),
                       img_of, B, T, H, W, K, lds_counters, hist_out);
    GCS_CHECK_LAUNCH("gcs_boundary_sweep_resident");
    return GCS_OK;
}

// ======================================================================= region tables (§8f-2)
// Integer part of /root/reference/BSD_metrics/metrics.py:102-146 (label x annotator contingency table and region
// areas) and :160-181 (4-neighbour perimeter: image-border pixels, or pixels with a different 4-neighbour). One
// thread per pixel; workgroup-private tables in LDS when they fit (k-means label maps: a few clusters, every
// atomic on a handful of addresses), global atomics otherwise (connected regions: thousands of sparse rows).
// Batched: blockIdx.y = image b with annotators first[b] .. first[b+1]-1 of the concatenated truth stack (first == NULL:
// one image with annotators 0 .. A-1); hist [T][n_seg][stride], area / perim [B][n_seg].
template <typename TT>
__global__ __launch_bounds__(256) void region_counts_kernel(const int32_t *__restrict__ labels,
                                                            const TT *__restrict__ truth,
                                                            const int32_t *__restrict__ first, int A, int H, int W,
                                                            int n_seg, int stride, int use_lds,
                                                            unsigned *__restrict__ hist, unsigned *__restrict__ area,
                                                            unsigned *__restrict__ perim) {
    extern __shared__ unsigned s_tab[];                        // [A_b][n_seg][stride] hist | [n_seg] area | [n_seg] perim
    const int b = blockIdx.y;
    const int t0 = first ? first[b] : 0, a_n = first ? first[b + 1] - first[b] : A;
    const int P = H * W;
    labels += (size_t)b * P;
    truth += (size_t)t0 * P;
    hist += (size_t)t0 * n_seg * stride;
    area += (size_t)b * n_seg;
    perim += (size_t)b * n_seg;
    const int n_hist = a_n * n_seg * stride, n_tab = n_hist + 2 * n_seg;
    // the dynamic LDS was sized by the host for A annotators per image: an image that brings more (a caller that understated
    // max_annotators) takes the global-atomics path instead of writing past its allocation
    use_lds = use_lds && a_n <= A;
    if (use_lds) {
        for (int i = threadIdx.x; i < n_tab; i += blockDim.x) s_tab[i] = 0u;
        __syncthreads();
    }
    unsigned *t_hist = use_lds ? s_tab : hist, *t_area = use_lds ? s_tab + n_hist : area,
             *t_perim = use_lds ? s_tab + n_hist + n_seg : perim;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int l = labels[p];
        if ((unsigned)l >= (unsigned)n_seg) continue;          // caller passes n_seg = max + 1; never index outside
        const int y = p / W, x = p - y * W;
        bool edge = y == 0 || y == H - 1 || x == 0 || x == W - 1;
        if (!edge) edge = labels[p - W] != l || labels[p + W] != l || labels[p - 1] != l || labels[p + 1] != l;
        atomicAdd(&t_area[l], 1u);
        if (edge) atomicAdd(&t_perim[l], 1u);
        for (int a = 0; a < a_n; ++a) {
            const int t = truth[(size_t)a * P + p];
            if (t < stride) atomicAdd(&t_hist[((size_t)a * n_seg + l) * stride + t], 1u);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_tab; i += blockDim.x) {
            const unsigned v = s_tab[i];
            if (v) atomicAdd(i < n_hist ? &hist[i] : i < n_hist + n_seg ? &area[i - n_hist] : &perim[i - n_hist - n_seg], v);
        }
    }
}

template <typename TT>
static int region_counts_launch(const int32_t *labels, const TT *truth, const int32_t *first, int B, int T, int Amax,
                                int H, int W, int n_segments, int n_truth_labels, uint32_t *hist, uint32_t *area,
                                uint32_t *perim, hipStream_t stream, const char *who, bool zeroed = false) {
    const size_t n_hist = (size_t)T * n_segments * n_truth_labels;
    if (!zeroed) {
        hipError_t e = hipMemsetAsync(hist, 0, n_hist * sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(area, 0, (size_t)B * n_segments * sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(perim, 0, (size_t)B * n_segments * sizeof(uint32_t), stream);
        if (e != hipSuccess) return gcs_hip_fail(e, who);
    }
    const size_t lds = ((size_t)Amax * n_segments * n_truth_labels + 2 * (size_t)n_segments) * sizeof(unsigned);
    const int use_lds = lds <= 48 * 1024;
    const int P = H * W;
    int blocks = use_lds ? min(256, (P + 1023) / 1024) : min(2048, (P + 255) / 256);
    if (B > 16) blocks = min(blocks, 32);
    hipLaunchKernelGGL(region_counts_kernel<TT>, dim3(blocks, B), dim3(256), use_lds ? lds : 0, stream, labels, truth, first,
                       Amax, H, W, n_segments, n_truth_labels, use_lds, hist, area, perim);
    GCS_CHECK_LAUNCH(who);
    return GCS_OK;
}

// The shape rules the region-table entry points share (the single-image entry passes B = 1, T = max_annotators = A).
static bool region_shape_ok(int B, int T, int max_annotators, int H, int W, int n_segments, int n_truth_labels, bool u8) {
    return B > 0 && B <= 65535 && T > 0 && max_annotators > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL &&
           n_segments > 0 && n_truth_labels > 0 && !(u8 && n_truth_labels > 256) &&
           (long long)T * n_segments * n_truth_labels <= 0x40000000LL;      // 2^30 counters, 4 GiB: the last one ends at byte 2^32
}

extern "C" int gcs_region_counts(const int32_t *labels, const uint16_t *truth, int A, int H, int W, int n_segments,
                                 int n_truth_labels, uint32_t *hist, uint32_t *area, uint32_t *perim,
                                 gcs_stream_t stream) {
    if (!labels || !truth || !hist || !area || !perim) return gcs_fail(GCS_EINVAL, "gcs_region_counts: NULL pointer");
    if (!region_shape_ok(1, A, A, H, W, n_segments, n_truth_labels, false)) return gcs_fail(GCS_EINVAL, "gcs_region_counts: bad shape");
    return region_counts_launch(labels, truth, nullptr, 1, A, A, H, W, n_segments, n_truth_labels, hist, area, perim, stream,
                                "gcs_region_counts");
}

extern "C" int gcs_region_counts_batch(const int32_t *labels, const uint16_t *truth, const int32_t *first, int B, int T,
                                       int max_annotators, int H, int W, int n_segments, int n_truth_labels, uint32_t *hist,
                                       uint32_t *area, uint32_t *perim, gcs_stream_t stream) {
    if (!labels || !truth || !first || !hist || !area || !perim)
        return gcs_fail(GCS_EINVAL, "gcs_region_counts_batch: NULL pointer");
    if (!region_shape_ok(B, T, max_annotators, H, W, n_segments, n_truth_labels, false))
        return gcs_fail(GCS_EINVAL, "gcs_region_counts_batch: bad shape");
    return region_counts_launch(labels, truth, first, B, T, max_annotators, H, W, n_segments, n_truth_labels, hist, area,
                                perim, stream, "gcs_region_counts_batch");
}

// The two integer sums metrics.py:128-140 takes from an annotator's contingency table, one workgroup per annotator map t of image
// b = img_of[t]:  under[t] = sum_seg (area[b][seg] - max_col hist[t][seg][col])                       (metrics.py:129-130)
//                 under_np[t] = sum_seg sum_col min(hist[t][seg][col], rowsum[t][seg] - hist[t][seg][col])   (metrics.py:137-139)
// Integers: exact in any order. The host then needs 16 bytes per annotator instead of the table (109 x 8 x 114 counters for 16 BSD
// images) and its array passes over it.
__global__ __launch_bounds__(256) void region_reduce_kernel(const unsigned *__restrict__ hist, const unsigned *__restrict__ area,
                                                            const int32_t *__restrict__ img_of, int n_seg, int stride,
                                                            unsigned long long *__restrict__ under,
                                                            unsigned long long *__restrict__ under_np) {
    __shared__ unsigned long long s_u[4], s_n[4];
    const int t = blockIdx.x, b = img_of[t], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned *h = hist + (size_t)t * n_seg * stride;
    unsigned long long u = 0, n = 0;                        // (lane 0 of each wave carries the wave's share)
    for (int seg = wave; seg < n_seg; seg += 4) {           // one wave per table row, lanes across its columns
        const unsigned *row = h + (size_t)seg * stride;
        unsigned mx = 0;
        unsigned long long sum = 0;
        for (int c = lane; c < stride; c += 64) {
            const unsigned v = row[c];
            mx = v > mx ? v : mx;
            sum += v;
        }
        for (int s = 32; s >= 1; s >>= 1) {
            mx = max(mx, (unsigned)__shfl_xor((int)mx, s));
            sum += __shfl_xor(sum, s);
        }
        unsigned long long mn = 0;
        for (int c = lane; c < stride; c += 64) {
            const unsigned long long v = row[c], o = sum - v;
            mn += v < o ? v : o;
        }
        for (int s = 32; s >= 1; s >>= 1) mn += __shfl_xor(mn, s);
        u += (unsigned long long)area[(size_t)b * n_seg + seg] - mx;    // area >= row sum >= max: never negative
        n += mn;
    }
    if (lane == 0) {
        s_u[wave] = u;
        s_n[wave] = n;
    }
    __syncthreads();
    if (tid == 0) {
        under[t] = s_u[0] + s_u[1] + s_u[2] + s_u[3];
        under_np[t] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    }
}

extern "C" int gcs_region_reduce(const uint32_t *hist, const uint32_t *area, const int32_t *img_of, int T, int n_segments,
                                 int n_truth_labels, uint64_t *under, uint64_t *under_np, gcs_stream_t stream) {
    if (!hist || !area || !img_of || !under || !under_np) return gcs_fail(GCS_EINVAL, "gcs_region_reduce: NULL pointer");
    if (T <= 0 || T > 1000000 || n_segments <= 0 || n_truth_labels <= 0) return gcs_fail(GCS_EINVAL, "gcs_region_reduce: bad shape");
    hipLaunchKernelGGL(region_reduce_kernel, dim3(T), dim3(256), 0, stream, hist, area, img_of, n_segments, n_truth_labels,
                       reinterpret_cast<unsigned long long *>(under), reinterpret_cast<unsigned long long *>(under_np));
    GCS_CHECK_LAUNCH("gcs_region_reduce");
    return GCS_OK;
}

// the same tables from annotator maps narrowed to uint8 (gcs_truth_prepare: BSD500's largest annotator label is 208), half the bytes
extern "C" int gcs_region_counts_batch_u8(const int32_t *labels, const uint8_t *truth8, const int32_t *first, int B, int T,
                                          int max_annotators, int H, int W, int n_segments, int n_truth_labels, uint32_t *hist,
                                          uint32_t *area, uint32_t *perim, gcs_stream_t stream) {
    if (!labels || !truth8 || !first || !hist || !area || !perim)
        return gcs_fail(GCS_EINVAL, "gcs_region_counts_batch_u8: NULL pointer");
    if (!region_shape_ok(B, T, max_annotators, H, W, n_segments, n_truth_labels, true))
        return gcs_fail(GCS_EINVAL, "gcs_region_counts_batch_u8: bad shape");
    return region_counts_launch(labels, truth8, first, B, T, max_annotators, H, W, n_segments, n_truth_labels, hist, area,
                                perim, stream, "gcs_region_counts_batch_u8");
}

// Everything evaluate.metrics.get_metrics() needs of a batch, on resident ground truth, in SIX launches: zero | bd(L) bit planes +
// label maxima | their dilation | boundary counts | region tables | their reduction.
extern "C" int gcs_score_batch_resident(const int32_t *labels, const void *truth_planes, const uint64_t *truth_bd_counts,
                                        const void *truth_maps, int truth_is_u8, const int32_t *first, const int32_t *img_of, int B,
                                        int T, int max_annotators, int H, int W, int n_segments, int n_truth_labels, void *scratch,
                                        uint32_t *hist, uint64_t *counts, int32_t *seg_max, uint32_t *area, uint32_t *perim,
                                        uint64_t *under, uint64_t *under_np, gcs_stream_t stream) {
    if (!labels || !truth_planes || !truth_bd_counts || !truth_maps || !first || !img_of || !scratch || !hist || !counts || !seg_max ||
        !area || !perim || !under || !under_np)
        return gcs_fail(GCS_EINVAL, "gcs_score_batch_resident: NULL pointer");
    if (!region_shape_ok(B, T, max_annotators, H, W, n_segments, n_truth_labels, truth_is_u8 != 0) || B + T > 1000000 ||
        (long long)B * n_segments > 0x3fffffffLL)
        return gcs_fail(GCS_EINVAL, "gcs_score_batch_resident: bad shape");
    ZeroList z;
    z.p[0] = hist; z.n[0] = (unsigned)((size_t)T * n_segments * n_truth_labels);
    z.p[1] = area; z.n[1] = (unsigned)((size_t)B * n_segments);       // (B * n_segments < 2^30: checked above)
    z.p[2] = perim; z.n[2] = (unsigned)((size_t)B * n_segments);
    z.p[3] = reinterpret_cast<unsigned *>(seg_max); z.n[3] = (unsigned)B;
    hipLaunchKernelGGL(zero_kernel, dim3(grid_for((long long)z.n[0], 256, 1024)), dim3(256), 0, stream, z);
    GCS_CHECK_LAUNCH("gcs_score_batch_resident(zero)");
    int rc = bits_counts_launch(labels, truth_planes, truth_bd_counts, img_of, B, T, H, W, scratch, counts, seg_max, stream,
                                "gcs_score_batch_resident(boundary)");
    if (rc != GCS_OK) return rc;
    auto regions = [&](auto *maps) {                           // the tables are zeroed above
        return region_counts_launch(labels, maps, first, B, T, max_annotators, H, W, n_segments, n_truth_labels, hist, area, perim,
                                    stream, "gcs_score_batch_resident(regions)", true);
    };
    rc = truth_is_u8 ? regions(static_cast<const uint8_t *>(truth_maps)) : regions(static_cast<const uint16_t *>(truth_maps));
    if (rc != GCS_OK) return rc;
    hipLaunchKernelGGL(region_reduce_kernel, dim3(T), dim3(256), 0, stream, hist, area, img_of, n_segments, n_truth_labels,
                       reinterpret_cast<unsigned long long *>(under), reinterpret_cast<unsigned long long *>(under_np));
    GCS_CHECK_LAUNCH("gcs_score_batch_resident");
    return GCS_OK;
}

// ======================================================================= region agreement (SPEC.md §8)
// PRI / VoI / covering of the BSDS500 benchmark are functions of the same contingency tables: per annotator map t,
//   sums[t]  = { N = sum_j b_j, sum_i a_i^2, sum_j b_j^2, sum_ij n_ij^2 }                         (uint64, exact)
//   terms[t] = { sum a log2 a, sum b log2 b, sum n log2 n, sum_j b_j * n*_j / u*_j }              (double)
// with a_i / b_j the row / column sums of the table itself and n*_j / u*_j the largest n_ij / (a_i + b_j - n_ij) of column j.
// ONE workgroup per map, 16 waves; wave w owns rows w, w + 16, ... (lanes across the columns), AG_ROWS of them per step with
// their loads issued together (one row per step left a wave waiting on one load at a time). The columns go in chunks of
// AG_CHUNK: per-wave column state [16][AG_CHUNK] in LDS (128 KiB of the CU's 160 KiB: the column sums in sweep 1, the best
// (n, u) pair in sweep 2), combined in wave order at the end of each chunk. Sweep 1 also leaves the row sums a_i (one lane of the
// owning wave, added up chunk by chunk) and the column sums b_j in the caller's scratch for sweep 2: every table element is read
// twice at most, and rows above the image's largest label (seg_max) not at all.
// Every float sum runs in an order fixed by the row / column INDEX alone (row mod 16 and its step, column mod 64 or mod 1024,
// chunk), then a fixed shuffle tree and the waves in order: empty rows and columns (a table allocated at a capacity) add
// nothing, so tables of the same maps at different shapes give the same bits. No float atomics.
constexpr int AG_CHUNK = 1024, AG_ROWS = 8;                    // (AG_WAVES = 16, AG_THREADS = 1024: tree_cuts.h)

template <typename V>
__device__ __forceinline__ V ag_wave_sum(V v) {
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// The reduction of ONE table h [.][stride], rows 0 .. rows-1, by the whole workgroup (AG_THREADS threads, all of them call it): a_s
// [rows] and b_s [stride] are the table's scratch, out_sums [4] / out_terms [4] its outputs. Shared by region_agreement_kernel (one
// table per workgroup) and region_sweep_kernel (one table per workgroup and cut). Ends with the outputs written by threads 0 .. 7; a
// caller that calls it again puts a __syncthreads() in between.
__device__ __forceinline__ void ag_table_reduce(const unsigned *__restrict__ h, int rows, int stride, unsigned *__restrict__ a_s,
                                                unsigned *__restrict__ b_s, unsigned long long *__restrict__ out_sums,
                                                double *__restrict__ out_terms) {
    __shared__ unsigned s_w[2][AG_WAVES][AG_CHUNK];            // sweep 1: [0] column sums; sweep 2: [0] best n, [1] best u
    __shared__ unsigned s_b[AG_CHUNK];
    __shared__ unsigned long long s_u[AG_WAVES][4];
    __shared__ double s_d[AG_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    static_assert(AG_ROWS <= 64, "one lane per row of a step");
    unsigned long long n_tot = 0, sa2 = 0, sb2 = 0, sn2 = 0;
    double sal = 0.0, sbl = 0.0, snl = 0.0, cov = 0.0;

    // ---- sweep 1: a_i, b_j, sum n^2, sum n log2 n
    for (int c0 = 0; c0 < stride; c0 += AG_CHUNK) {
        const int cw = min(AG_CHUNK, stride - c0);
        const bool last = c0 + AG_CHUNK >= stride;
        unsigned *col = s_w[0][wave];
        for (int c = lane; c < cw; c += 64) col[c] = 0u;      // the same lane updates these columns below
        for (int i0 = wave; i0 < rows; i0 += AG_WAVES * AG_ROWS) {   // AG_ROWS rows of this wave with their loads in flight
            unsigned rs[AG_ROWS] = {};
            for (int c = lane; c < cw; c += 64) {
                unsigned v[AG_ROWS];
#pragma unroll
                for (int u = 0; u < AG_ROWS; ++u) {
                    const int i = i0 + u * AG_WAVES;
                    v[u] = i < rows ? h[(size_t)i * stride + c0 + c] : 0u;
                }
                unsigned pend = 0;
#pragma unroll
                for (int u = 0; u < AG_ROWS; ++u) {
                    if (v[u]) {
                        col[c] += v[u];
                        rs[u] += v[u];                           // a row sum is at most H * W < 2^31
                        sn2 += (unsigned long long)v[u] * v[u];
                        pend |= 1u << u;
                    }
                }
                // the FP64 log2 only for this lane's own non-zeros, in row order: a sparse table (a few non-zeros per row) does
                // not pay one log2 per row for the whole wave
                while (pend) {
                    const int sel = __builtin_ctz(pend);
                    pend &= pend - 1;
                    unsigned x = 0;
#pragma unroll
                    for (int u = 0; u < AG_ROWS; ++u) x = u == sel ? v[u] : x;
                    snl += (double)x * log2((double)x);
                }
            }
            // row i0 + 16u belongs to lane u: its row sum, a^2 and a log2 a (the same lane in every chunk and in sweep 2)
            unsigned r = 0;
#pragma unroll
            for (int u = 0; u < AG_ROWS; ++u) {
                const unsigned t = ag_wave_sum(rs[u]);
                r = lane == u ? t : r;
            }
            const int i = i0 + lane * AG_WAVES;
            if (lane < AG_ROWS && i < rows) {
                const unsigned a = r + (c0 ? a_s[i] : 0u);
                a_s[i] = a;                                      // read back by this same lane only
                if (last && a) {
                    sa2 += (unsigned long long)a * a;
                    sal += (double)a * log2((double)a);
                }
            }
        }
        __syncthreads();
        for (int c = tid; c < cw; c += AG_THREADS) {
            unsigned b = 0;
            for (int w = 0; w < AG_WAVES; ++w) b += s_w[0][w][c];
            b_s[c0 + c] = b;                                   // read back by this same thread in sweep 2
            if (b) {
                n_tot += b;
                sb2 += (unsigned long long)b * b;
                sbl += (double)b * log2((double)b);
            }
        }
        __syncthreads();
    }

    // ---- sweep 2: per column the largest n / (a + b - n), compared exactly (n < 2^31, u < 2^32: 64-bit products)
    for (int c0 = 0; c0 < stride; c0 += AG_CHUNK) {
        const int cw = min(AG_CHUNK, stride - c0);
        for (int c = tid; c < cw; c += AG_THREADS) s_b[c] = b_s[c0 + c];
        unsigned *bn = s_w[0][wave], *bu = s_w[1][wave];
        for (int c = lane; c < cw; c += 64) {
            bn[c] = 0u;
            bu[c] = 1u;
        }
        __syncthreads();
        for (int i0 = wave; i0 < rows; i0 += AG_WAVES * AG_ROWS) {
            const int ia = i0 + lane * AG_WAVES;                 // lane u wrote a_i of row i0 + 16u in sweep 1
            const unsigned mine = lane < AG_ROWS && ia < rows ? a_s[ia] : 0u;
            unsigned a[AG_ROWS];
#pragma unroll
            for (int u = 0; u < AG_ROWS; ++u) a[u] = __shfl(mine, u);
            for (int c = lane; c < cw; c += 64) {
                unsigned v[AG_ROWS];
#pragma unroll
                for (int u = 0; u < AG_ROWS; ++u) {
                    const int i = i0 + u * AG_WAVES;
                    v[u] = i < rows ? h[(size_t)i * stride + c0 + c] : 0u;
                }
                const unsigned b = s_b[c];
                unsigned n = bn[c], d = bu[c];
#pragma unroll
                for (int u = 0; u < AG_ROWS; ++u) {               // rows in index order: the first of equal ratios stays
                    if (v[u]) {
                        const unsigned uu = a[u] + b - v[u];       // >= n >= 1
                        if ((unsigned long long)v[u] * d > (unsigned long long)n * uu) {
                            n = v[u];
                            d = uu;
                        }
                    }
                }
                bn[c] = n;
                bu[c] = d;
            }
        }
        __syncthreads();
        for (int c = tid; c < cw; c += AG_THREADS) {
            unsigned n = s_w[0][0][c], u = s_w[1][0][c];
            for (int w = 1; w < AG_WAVES; ++w) {
                const unsigned n2 = s_w[0][w][c], u2 = s_w[1][w][c];
                if ((unsigned long long)n2 * u > (unsigned long long)n * u2) {
                    n = n2;
                    u = u2;
                }
            }
            if (n) cov += (double)s_b[c] * ((double)n / (double)u);
        }
        __syncthreads();
    }

    // ---- fixed-order reduction: shuffle tree per wave, then the waves in index order
    n_tot = ag_wave_sum(n_tot);
    sa2 = ag_wave_sum(sa2);
    sb2 = ag_wave_sum(sb2);
    sn2 = ag_wave_sum(sn2);
    sal = ag_wave_sum(sal);
    sbl = ag_wave_sum(sbl);
    snl = ag_wave_sum(snl);
    cov = ag_wave_sum(cov);
    if (lane == 0) {
        s_u[wave][0] = n_tot; s_u[wave][1] = sa2; s_u[wave][2] = sb2; s_u[wave][3] = sn2;
        s_d[wave][0] = sal;   s_d[wave][1] = sbl; s_d[wave][2] = snl; s_d[wave][3] = cov;
    }
    __syncthreads();
    if (tid < 8) {
        const int k = tid & 3;
        if (tid < 4) {
            unsigned long long v = 0;
            for (int w = 0; w < AG_WAVES; ++w) v += s_u[w][k];
            out_sums[k] = v;
        } else {
            double v = 0.0;
            for (int w = 0; w < AG_WAVES; ++w) v += s_d[w][k];
            out_terms[k] = v;
        }
    }
}

__global__ __launch_bounds__(AG_THREADS) void region_agreement_kernel(const unsigned *__restrict__ hist,
                                                                      const int32_t *__restrict__ img_of,
                                                                      const int32_t *__restrict__ seg_max, int n_seg,
                                                                      int stride, unsigned *__restrict__ scratch,
                                                                      unsigned long long *__restrict__ sums,
                                                                      double *__restrict__ terms) {
    const int t = blockIdx.x;
    int rows = n_seg;
    if (seg_max) rows = min(n_seg, max(0, seg_max[img_of ? img_of[t] : 0] + 1));
    unsigned *a_s = scratch + (size_t)t * (n_seg + stride);
    ag_table_reduce(hist + (size_t)t * n_seg * stride, rows, stride, a_s, a_s + n_seg, sums + (size_t)t * 4, terms + (size_t)t * 4);
}

extern "C" size_t gcs_region_agreement_scratch_bytes(int T, int n_segments, int n_truth_labels) {
    if (T <= 0 || n_segments <= 0 || n_truth_labels <= 0) return 0;
    return (size_t)T * ((size_t)n_segments + n_truth_labels) * sizeof(uint32_t);
}

extern "C" int gcs_region_agreement(const uint32_t *hist, const int32_t *img_of, const int32_t *seg_max, int T, int n_segments,
                                    int n_truth_labels, void *scratch, uint64_t *sums, double *terms, gcs_stream_t stream) {
    if (!hist || !scratch || !sums || !terms) return gcs_fail(GCS_EINVAL, "gcs_region_agreement: NULL pointer");
    if (seg_max && !img_of) return gcs_fail(GCS_EINVAL, "gcs_region_agreement: seg_max_dev needs img_of_dev");
    if (T <= 0 || T > 1000000 || n_segments <= 0 || n_truth_labels <= 0 ||
        (long long)T * n_segments * n_truth_labels > 0x40000000LL)
        return gcs_fail(GCS_EINVAL, "gcs_region_agreement: bad shape");
    hipLaunchKernelGGL(region_agreement_kernel, dim3(T), dim3(AG_THREADS), 0, stream, hist, img_of, seg_max, n_segments,
                       n_truth_labels, static_cast<unsigned *>(scratch), reinterpret_cast<unsigned long long *>(sums), terms);
    GCS_CHECK_LAUNCH("gcs_region_agreement");
    return GCS_OK;
}

// ================================================= region metrics of every cut of a region tree at once (SPEC.md §16)
// Every group of a cut is a union of superpixels, so its row of the contingency table is the sum of its superpixels' rows: the leaf
// tables (gcs_region_counts_batch[_u8] with n_segments = K) are made once from the pixels and every coarser table follows from the
// merge list by adding rows. ONE workgroup per annotator map t of image b = img_of[t], the requested cuts in their (decreasing) order
// of R, so the table only ever gets coarser and is coarsened IN PLACE:
//   1. death[q] = the row that absorbs label q, with its absorber (rs_absorbers, tree_cuts.h).
//   2. per cut, tau = max(0, alive - R): pointer jumping (rs_group_reps, tree_cuts.h) gives every label's group rep; the rows absorbed
//      since the previous cut (tau_prev <= death < tau) are added into their rep's row, element by element with integer atomics
//      (exact in any order; a rep is never absorbed in the same cut, so no row is read and written), and emptied.
//   3. the table is reduced: by rs_under_reduce to { N, under, under_np } of SPEC.md §17 (UNDER: gcs_region_sweep_under), by
//      ag_table_reduce, the function gcs_region_agreement runs (AGREE: gcs_region_sweep, and gcs_region_sweep_under when asked):
//      every float sum in an order fixed by the table indices alone, no running float sums carried from cut to cut. The
//      instantiation without AGREE does not carry ag_table_reduce's 132 KiB of LDS.
constexpr int RS_UNROLL = 4;
constexpr int RU_ROWS = 4, RU_COLS = 4;                        // rs_under_reduce: rows of a wave in flight, registers per lane and row

// The three integer sums SPEC.md §17 takes from ONE table h [K][stride], by the whole workgroup: out = { N = sum_i a_i,
// sum_i (a_i - max_j n_ij), sum_ij min(n_ij, a_i - n_ij) }, a_i the row sums of the table itself (metrics.py:129-131, :137-140).
// A wave per row, lanes across the columns, maximum and row sum by cross-lane shuffles as in region_reduce_kernel; RU_ROWS rows of
// a wave with their loads in flight together, and a row of at most 64 * RU_COLS columns (uint8 annotator maps) is read once and
// kept in registers. Rows absorbed below tau are empty and are not read. Integers: exact in any order. s_p: [AG_WAVES][3] of LDS;
// a caller that calls it again puts a __syncthreads() in between.
__device__ __forceinline__ void rs_under_reduce(const unsigned *h, int K, int stride, const unsigned *s_dk, int tau,
                                                unsigned long long (*s_p)[3], unsigned long long *out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long n = 0, u = 0, np = 0;                   // (every lane of a wave carries the wave's share)
    for (int q0 = wave; q0 < K; q0 += AG_WAVES * RU_ROWS) {
        bool live[RU_ROWS];
#pragma unroll
        for (int r = 0; r < RU_ROWS; ++r) {
            const int q = q0 + r * AG_WAVES;
            live[r] = q < K && (s_dk[q] >> 12) >= (unsigned)tau;          // (uniform over the wave)
        }
        if (stride <= 64 * RU_COLS) {
            unsigned v[RU_ROWS][RU_COLS];
#pragma unroll
            for (int r = 0; r < RU_ROWS; ++r)
#pragma unroll
                for (int j = 0; j < RU_COLS; ++j) {
                    const int c = lane + 64 * j;
                    v[r][j] = live[r] && c < stride ? h[(size_t)(q0 + r * AG_WAVES) * stride + c] : 0u;
                }
#pragma unroll
            for (int r = 0; r < RU_ROWS; ++r) {
                if (!live[r]) continue;
                unsigned mx = 0, sum = 0;                      // a row sum is at most H * W < 2^31
#pragma unroll
                for (int j = 0; j < RU_COLS; ++j) {
                    mx = max(mx, v[r][j]);
                    sum += v[r][j];
                }
                for (int s = 32; s >= 1; s >>= 1) {
                    mx = max(mx, (unsigned)__shfl_xor((int)mx, s));
                    sum += (unsigned)__shfl_xor((int)sum, s);
                }
                unsigned mn = 0;                               // at most the row sum
#pragma unroll
                for (int j = 0; j < RU_COLS; ++j) mn += min(v[r][j], sum - v[r][j]);
                for (int s = 32; s >= 1; s >>= 1) mn += (unsigned)__shfl_xor((int)mn, s);
                n += sum;
                u += sum - mx;
                np += mn;
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < RU_ROWS; ++r) {
                if (!live[r]) continue;
                const unsigned *row = h + (size_t)(q0 + r * AG_WAVES) * stride;
                unsigned mx = 0, sum = 0;
                for (int c = lane; c < stride; c += 64) {
                    const unsigned x = row[c];
                    mx = max(mx, x);
                    sum += x;
                }
                for (int s = 32; s >= 1; s >>= 1) {
                    mx = max(mx, (unsigned)__shfl_xor((int)mx, s));
                    sum += (unsigned)__shfl_xor((int)sum, s);
                }
                unsigned mn = 0;
                for (int c = lane; c < stride; c += 64) {
                    const unsigned x = row[c];
                    mn += min(x, sum - x);
                }
                for (int s = 32; s >= 1; s >>= 1) mn += (unsigned)__shfl_xor((int)mn, s);
                n += sum;
                u += sum - mx;
                np += mn;
            }
        }
    }
    if (lane == 0) {
        s_p[wave][0] = n;
        s_p[wave][1] = u;
        s_p[wave][2] = np;
    }
    __syncthreads();
    if (tid < 3) {
        unsigned long long v = 0;
        for (int w = 0; w < AG_WAVES; ++w) v += s_p[w][tid];
        out[tid] = v;
    }
}

template <bool UNDER, bool AGREE>
__global__ __launch_bounds__(AG_THREADS) void region_sweep_kernel(unsigned *hist, const int32_t *__restrict__ merges,
                                                                  const int32_t *__restrict__ alive_p,
                                                                  const int32_t *__restrict__ img_of,
                                                                  const int32_t *__restrict__ regions, int B, int T, int K, int stride,
                                                                  int n_cuts, unsigned *scratch, unsigned long long *under,
                                                                  unsigned long long *sums, double *terms) {
    __shared__ unsigned s_dk[RS_K_MAX];
    __shared__ unsigned short s_root[RS_K_MAX];
    __shared__ unsigned long long s_p[UNDER ? AG_WAVES : 1][3];
    __shared__ int s_changed;
    const int t = blockIdx.x, tid = threadIdx.x;
    const int b = img_of[t];
    const bool img_ok = (unsigned)b < (unsigned)B;             // an image index outside the batch: the leaf table at every cut
    unsigned *h = hist + (size_t)t * K * stride;
    unsigned *a_s = scratch + (size_t)t * (K + stride), *b_s = a_s + K;
    const int alive = img_ok ? alive_p[b] : 0;
    const int n_rows = img_ok ? K - 1 : 0;
    const int32_t *rows = merges + (img_ok ? (size_t)b * (K - 1) * 2 : 0);   // (not read with n_rows = 0: NULL with K = 1)

    // ---- 1. which rows count, and what absorbs every label
    rs_absorbers(rows, n_rows, K, s_dk, &s_changed);

    // ---- 2. and 3. per cut: coarsen the table in place, reduce it
    const long long cells = (long long)K * stride;
    int tau_prev = 0;
    for (int ci = 0; ci < n_cuts; ++ci) {
        const int tau = rs_tau(alive, regions[ci], n_rows);
        if (tau > tau_prev) {                                  // (a list that is not decreasing never un-merges: no launch can check it)
            rs_group_reps(s_dk, s_root, K, tau);
            // the cells of the rows absorbed in this cut, RS_UNROLL of them per thread with their loads in flight together
            for (long long i0 = tid; i0 < cells; i0 += (long long)AG_THREADS * RS_UNROLL) {
                unsigned v[RS_UNROLL];
                long long dst[RS_UNROLL];
#pragma unroll
                for (int u = 0; u < RS_UNROLL; ++u) {
                    const long long i = i0 + (long long)u * AG_THREADS;
                    v[u] = 0u;
                    dst[u] = 0;
                    if (i < cells) {
                        const int q = (int)(i / stride);
                        const unsigned d = s_dk[q] >> 12;
                        if (d >= (unsigned)tau_prev && d < (unsigned)tau) {
                            v[u] = h[i];
                            dst[u] = i + ((long long)s_root[q] - q) * stride;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < RS_UNROLL; ++u)
                    if (v[u]) {
                        atomicAdd(&h[dst[u]], v[u]);
                        h[i0 + (long long)u * AG_THREADS] = 0u;
                    }
            }
            tau_prev = tau;
        }
        __syncthreads();                                       // (with its workgroup-scope fences: this workgroup's atomics and stores
                                                               // are visible to its own loads below; nobody else reads the table)
        if constexpr (UNDER) {
            rs_under_reduce(h, K, stride, s_dk, tau_prev, s_p, under + ((size_t)ci * T + t) * 3);
            __syncthreads();
        }
        if constexpr (AGREE) {
            ag_table_reduce(h, K, stride, a_s, b_s, sums + ((size_t)ci * T + t) * 4, terms + ((size_t)ci * T + t) * 4);
            __syncthreads();
        }
    }
}

static bool region_sweep_shape_ok(int T, int K, int n_truth_labels, int n_cuts) {
    return T >= 1 && T <= 1000000 && K >= 1 && K <= RS_K_MAX && n_truth_labels >= 1 && n_cuts >= 1 && n_cuts <= RS_CUTS_MAX &&
           (long long)T * K * n_truth_labels < 0x80000000LL;
}

extern "C" size_t gcs_region_sweep_workspace_bytes(int T, int K, int n_truth_labels, int n_cuts) {
    if (!region_sweep_shape_ok(T, K, n_truth_labels, n_cuts)) return 0;
    return (size_t)T * ((size_t)K + n_truth_labels) * sizeof(uint32_t);    // per map: the row and column sums of the table in hand
}

extern "C" int gcs_region_sweep(uint32_t *leaf_hist, const int32_t *merges, const int32_t *alive, const int32_t *img_of,
                                const int32_t *regions, int B, int T, int K, int n_truth_labels, int n_cuts, void *workspace,
                                uint64_t *sums_out, double *terms_out, gcs_stream_t stream) {
    if (!leaf_hist || !alive || !img_of || !regions || !workspace || !sums_out || !terms_out || (K > 1 && !merges))
        return gcs_fail(GCS_EINVAL, "gcs_region_sweep: NULL pointer");
    if (B < 1 || B > 65535 || T < 1 || T > 1000000 || K < 1 || K > RS_K_MAX || n_truth_labels < 1 || n_cuts < 1 || n_cuts > RS_CUTS_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_region_sweep: bad shape (1 <= B <= 65535, 1 <= T <= 1000000, 1 <= K <= 4096, 1 <= n_cuts <= 64)");
    if (!region_sweep_shape_ok(T, K, n_truth_labels, n_cuts))
        return gcs_fail(GCS_EINVAL, "gcs_region_sweep: T * K * n_truth_labels must be below 2^31");
    hipLaunchKernelGGL((region_sweep_kernel<false, true>), dim3(T), dim3(AG_THREADS), 0, stream, leaf_hist, merges, alive, img_of,
                       regions, B, T, K, n_truth_labels, n_cuts, static_cast<unsigned *>(workspace), nullptr,
                       reinterpret_cast<unsigned long long *>(sums_out), terms_out);
    GCS_CHECK_LAUNCH("gcs_region_sweep");
    return GCS_OK;
}

// ---- the same walk with the undersegmentation sums of every cut (SPEC.md §17), and the agreement outputs too when asked
extern "C" size_t gcs_region_sweep_under_workspace_bytes(int T, int K, int n_truth_labels, int n_cuts) {
    return gcs_region_sweep_workspace_bytes(T, K, n_truth_labels, n_cuts);
}

extern "C" int gcs_region_sweep_under(uint32_t *leaf_hist, const int32_t *merges, const int32_t *alive, const int32_t *img_of,
                                      const int32_t *regions, int B, int T, int K, int n_truth_labels, int n_cuts, void *workspace,
                                      uint64_t *under_out, uint64_t *sums_out, double *terms_out, gcs_stream_t stream) {
    if (!leaf_hist || !alive || !img_of || !regions || !workspace || !under_out || (K > 1 && !merges))
        return gcs_fail(GCS_EINVAL, "gcs_region_sweep_under: NULL pointer");
    if (!sums_out != !terms_out)
        return gcs_fail(GCS_EINVAL, "gcs_region_sweep_under: sums_out_dev and terms_out_dev are given together or both NULL");
    if (B < 1 || B > 65535 || T < 1 || T > 1000000 || K < 1 || K > RS_K_MAX || n_truth_labels < 1 || n_cuts < 1 || n_cuts > RS_CUTS_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_region_sweep_under: bad shape (1 <= B <= 65535, 1 <= T <= 1000000, 1 <= K <= 4096, 1 <= n_cuts <= 64)");
    if (!region_sweep_shape_ok(T, K, n_truth_labels, n_cuts))    // (the outputs: n_cuts * T * 4 <= 2.56e8 elements)
        return gcs_fail(GCS_EINVAL, "gcs_region_sweep_under: T * K * n_truth_labels must be below 2^31");
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(T), dim3(AG_THREADS), 0, stream, leaf_hist, merges, alive, img_of, regions, B, T, K,
                           n_truth_labels, n_cuts, static_cast<unsigned *>(workspace), reinterpret_cast<unsigned long long *>(under_out),
                           reinterpret_cast<unsigned long long *>(sums_out), terms_out);
    };
    if (sums_out)
        launch(region_sweep_kernel<true, true>);
    else
        launch(region_sweep_kernel<true, false>);
    GCS_CHECK_LAUNCH("gcs_region_sweep_under");
    return GCS_OK;
}
