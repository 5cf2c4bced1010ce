// kmeans_seed.hip — k-means++ seeding of the Lloyd stage (SPEC.md §29): k seeds per codebook set, drawn by D^2 sampling with
// greedy trials among at most 4096 CANDIDATE pixels of the set (a regular grid over its images), read from the FEATURE SLAB (either
// format, every level at its own resolution), in exact integers.
//
//   ks_kernel   ONE workgroup of 1024 threads per set runs all k rounds (64 workgroups at batch 64 with per-image codebooks, one
//               with a global codebook; what a round costs: DESIGN.md §4.27). m(q), the squared distance of candidate q to its
//               nearest seed so far, lives in LDS (4096 x 8 bytes). A round:
//                 1. draws: thread i sums m over ITS four consecutive candidates, a block scan of the 1024 sums gives the prefix
//                    in front of it, and the thread whose range holds a trial's rho walks its four values: the smallest q whose
//                    inclusive prefix sum exceeds rho (so m(q) > 0). (Round 0 and T = 0: one uniform pick, no scan.)
//                 2. the trial centres go to LDS, permuted to physical plane order ([plane][TB] uint16), fetched plane-parallel.
//                 3. sweep: thread i takes candidates i, i + 1024, ...: it locates each once per level (slab_tap) and sums the TB
//                    distances in one walk over the candidate's planes (slab_next), as ke_level does (csrc/kmeans_model.hip), so
//                    a round reads every candidate's features once; min(m, d_t) stays in registers for every trial.
//                 4. pot_t = sum_q min(m(q), d_t(q)): wave shuffles, then LDS. Every thread takes the same winner (ties: lowest t),
//                    writes its min(m, d_win) back to m; the winner's centre leaves for cent_out in logical order.
//               T, the scan and the pot_t are 64-bit integer sums: any order gives the same bits.
//               TB = trials rounded up to 2, 4 or 8: the padding centres are zero and never compared.
// No workspace, no allocation, no host synchronisation: one launch (capturable).
#include "slab_slots.h"
#include "gcs_seed.h"

namespace {

typedef unsigned long long u64;

constexpr int KS_THREADS = 1024, KS_WAVES = KS_THREADS / 64;
constexpr int KS_N_MAX = 4096, KS_CPT = KS_N_MAX / KS_THREADS;     // candidates per set, and per thread
constexpr int KS_T_MAX = 8;
constexpr int KS_HW_MAX = 4096, KS_D_MAX = 1536;                   // 8 x 1536 centre values = 24 KB of LDS

__host__ __device__ __forceinline__ u64 ks_mix(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The candidate grid of one image and of a set.
struct KsGrid {
    int stride, ny, nx, per, n;       // per = ny * nx candidates per image, n per set
};

// candidate q of set `set` -> its image and full-resolution pixel
__device__ __forceinline__ void ks_candidate(const GcsLayout &lo, const KsGrid &g, int per_image, int set, int q, int &b, int &y, int &x) {
    const int bi = q / g.per, rem = q - bi * g.per, i = rem / g.nx, j = rem - i * g.nx;
    b = per_image ? set : bi;
    y = min(g.stride * i + (g.stride >> 1), lo.H - 1);
    x = min(g.stride * j + (g.stride >> 1), lo.W - 1);
}

// d[t] += sum over the planes of level L of (x - c_t)^2 at level pixel (yl, xl), which lies inside the level image.
template <bool SPLIT, int TB>
__device__ __forceinline__ void ks_level(const GcsLayout &lo, const unsigned char *img, const uint16_t *s_cent, int L, int yl, int xl,
                                         u64 (&d)[TB]) {
    SlabTap t = slab_tap(lo, img, L, yl, xl);
    const unsigned npl = (unsigned)KP_TP >> (2 * L);
    const unsigned *c = reinterpret_cast<const unsigned *>(s_cent + (size_t)lo.row0[L] * TB);
    for (int n = lo.DL[L]; n > 0; --n, c += TB / 2) {
        const unsigned v = (unsigned)slab_next<SPLIT>(lo, img, t, npl);
#pragma unroll
        for (int j = 0; j < TB; j += 2) {
            const unsigned cc = c[j >> 1];              // two centres' values of this plane
            const unsigned a0 = __usad(v, cc & 0xffffu, 0u), a1 = __usad(v, cc >> 16, 0u);
            d[j] += (u64)a0 * a0;                       // |x - c| <= 65535: a term is below 2^32, the sum is 64-bit
            d[j + 1] += (u64)a1 * a1;
        }
    }
}

template <bool SPLIT, int TB>
__global__ __launch_bounds__(KS_THREADS) void ks_kernel(const unsigned char *__restrict__ slab, GcsLayout lo, KsGrid g, int k,
                                                        int per_image, int trials, u64 seed_mixed, uint16_t *__restrict__ cent_out,
                                                        int32_t *__restrict__ picks_out, long long *__restrict__ potential_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *s_cent = reinterpret_cast<uint16_t *>(smem);                 // [D][TB], physical plane order
    __shared__ __attribute__((aligned(16))) u64 s_m[KS_N_MAX];             // m(q); 0 behind the set's last candidate
    __shared__ u64 s_part[KS_WAVES * KS_T_MAX];                            // per wave: scan totals, then partial potentials
    __shared__ u64 s_pot[KS_T_MAX];
    __shared__ int s_q[KS_T_MAX];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, set = (int)blockIdx.x;
#pragma unroll
    for (int c = 0; c < KS_CPT; ++c) {
        const int q = c * KS_THREADS + tid;
        s_m[q] = q < g.n ? ~0ull : 0ull;                                   // round 0: min(m, d) = d
    }
    u64 T = 0ull;
    for (int r = 0; r < k; ++r) {
        const bool uniform = r == 0 || T == 0ull;                          // (the same in every thread)
        const int ntr = uniform ? 1 : trials;
        // ---- 1. the draws
        if (uniform) {
            if (tid == 0) s_q[0] = (int)__umul64hi(ks_mix(seed_mixed ^ (u64)(16 * r)), (u64)g.n);
        } else {
            u64 mine[KS_CPT], sum = 0ull;
#pragma unroll
            for (int e = 0; e < KS_CPT; ++e) {
                mine[e] = s_m[KS_CPT * tid + e];
                sum += mine[e];
            }
            u64 v = sum;                                                   // inclusive scan inside the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const u64 up = __shfl_up(v, off, 64);
                if (lane >= off) v += up;
            }
            if (lane == 63) s_part[wave] = v;
            __syncthreads();
            u64 front = v - sum;                                           // the prefix in front of this thread's candidates
            for (int w = 0; w < wave; ++w) front += s_part[w];
            for (int t = 0; t < ntr; ++t) {
                const u64 rho = __umul64hi(ks_mix(seed_mixed ^ (u64)(16 * r + t)), T);     // rho < T
                if (rho >= front && rho < front + sum) {                   // exactly one thread: its range holds rho
                    u64 run = front;
                    int e = 0;
#pragma unroll
                    for (int i = 0; i < KS_CPT - 1; ++i) {
                        run += mine[i];
                        if (run <= rho && e == i) e = i + 1;
                    }
                    s_q[t] = KS_CPT * tid + e;
                }
            }
        }
        __syncthreads();
        // ---- 2. the trial centres, plane-parallel
        for (int i = tid; i < lo.D * TB; i += KS_THREADS) {
            const int pl = i / TB, t = i % TB;
            unsigned v = 0u;
            if (t < ntr) {
                int b, y, x;
                ks_candidate(lo, g, per_image, set, s_q[t], b, y, x);
                v = gcs_slab_value(slab, lo, b, pl, y, x);
            }
            s_cent[i] = (uint16_t)v;
        }
        __syncthreads();
        // ---- 3. one sweep over the candidates: min(m, d_t) for every trial
        u64 nm[KS_CPT][TB];
#pragma unroll
        for (int c = 0; c < KS_CPT; ++c) {
            const int q = c * KS_THREADS + tid;
            u64 d[TB];
#pragma unroll
            for (int t = 0; t < TB; ++t) d[t] = 0ull;
            u64 m = 0ull;
            if (q < g.n) {
                int b, y, x;
                ks_candidate(lo, g, per_image, set, q, b, y, x);
                const unsigned char *img = slab + (size_t)b * (size_t)lo.img_bytes;
                for (int L = 0; L < lo.n_levels; ++L) ks_level<SPLIT, TB>(lo, img, s_cent, L, y >> L, x >> L, d);
                m = s_m[q];
            }
#pragma unroll
            for (int t = 0; t < TB; ++t) nm[c][t] = d[t] < m ? d[t] : m;     // (q >= n: 0)
        }
        // ---- 4. the potentials, the winner, the new m
#pragma unroll
        for (int t = 0; t < TB; ++t) {
            u64 v = 0ull;
#pragma unroll
            for (int c = 0; c < KS_CPT; ++c) v += nm[c][t];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) s_part[wave * KS_T_MAX + t] = v;
        }
        __syncthreads();
        if (tid < TB) {
            u64 v = 0ull;
            for (int w = 0; w < KS_WAVES; ++w) v += s_part[w * KS_T_MAX + tid];
            s_pot[tid] = v;
        }
        __syncthreads();
        int win = 0;
        T = s_pot[0];
#pragma unroll
        for (int t = 1; t < TB; ++t) {
            const u64 p = s_pot[t];
            if (t < ntr && p < T) {                                        // strictly: ties stay with the lowest t
                T = p;
                win = t;
            }
        }
#pragma unroll
        for (int c = 0; c < KS_CPT; ++c) {
            const int q = c * KS_THREADS + tid;
            u64 v = nm[c][0];
#pragma unroll
            for (int t = 1; t < TB; ++t) v = t == win ? nm[c][t] : v;
            if (q < g.n) s_m[q] = v;
        }
        uint16_t *crow = cent_out + ((size_t)set * k + r) * lo.D;
        for (int pl = tid; pl < lo.D; pl += KS_THREADS) crow[gcs_logical_of_plane(lo, pl)] = s_cent[pl * TB + win];
        if (tid == 0 && picks_out) picks_out[(size_t)set * k + r] = s_q[win];
        __syncthreads();                                                   // m, the centres and the picks are free again
    }
    if (tid == 0 && potential_out) potential_out[set] = (long long)T;
}

template <bool SPLIT, int TB>
void ks_launch(const unsigned char *slab, const GcsLayout &lo, const KsGrid &g, int k, int n_sets, int B, int trials, u64 seed_mixed,
               uint16_t *cent, int32_t *picks, int64_t *potential, hipStream_t stream) {
    hipLaunchKernelGGL((ks_kernel<SPLIT, TB>), dim3(n_sets), dim3(KS_THREADS), (size_t)round_up(lo.D * TB * 2, 16), stream, slab, lo, g,
                       k, n_sets == B ? 1 : 0, trials, seed_mixed, cent, picks, reinterpret_cast<long long *>(potential));
}

}  // namespace

extern "C" int gcs_kmeans_seed(const uint16_t *feats_slab, int B, int H, int W, int n_scales, int n_orient, int k, int n_sets,
                               int stride, int trials, uint64_t seed, uint16_t *cent_out, int32_t *picks_out, int64_t *potential_out,
                               gcs_stream_t stream) {
    if (!feats_slab || !cent_out) return gcs_fail(GCS_EINVAL, "gcs_kmeans_seed: NULL pointer");
    if (k < 1 || k > GCS_K_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_seed: k must be in 1..16");
    if (trials < 1 || trials > KS_T_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_seed: trials must be in 1..8");
    if (stride < 1 || stride > 4096 || (stride & (stride - 1)))
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_seed: stride must be a power of two in 1..4096");
    if (B >= 1 && n_sets != 1 && n_sets != B) return gcs_fail(GCS_EINVAL, "gcs_kmeans_seed: n_sets must be 1 or B");
    GcsLayout lo;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > KS_HW_MAX || W > KS_HW_MAX || !gcs_make_layout(H, W, n_scales, n_orient, &lo) ||
        lo.D > KS_D_MAX)
        return gcs_fail(GCS_EINVAL, "gcs_kmeans_seed: bad shape or bank (1 <= B <= 65535, 1 <= H, W <= 4096, a bank of at most 1536 features)");
    KsGrid g;
    g.stride = stride;
    g.ny = (H + stride - 1) / stride;
    g.nx = (W + stride - 1) / stride;
    g.per = g.ny * g.nx;
    const long long n = (long long)g.per * (n_sets == 1 ? B : 1);
    if (n > KS_N_MAX) return gcs_fail(GCS_EINVAL, "gcs_kmeans_seed: a set has more than 4096 candidates at this stride");
    g.n = (int)n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned char *slab = reinterpret_cast<const unsigned char *>(feats_slab);
    const u64 sm = ks_mix((u64)seed);
#define GCS_KS_GO(TB)                                                                                                     \
    do {                                                                                                                  \
        if (lo.split) ks_launch<true, TB>(slab, lo, g, k, n_sets, B, trials, sm, cent_out, picks_out, potential_out, s);  \
        else ks_launch<false, TB>(slab, lo, g, k, n_sets, B, trials, sm, cent_out, picks_out, potential_out, s);          \
    } while (0)
    if (trials <= 2) GCS_KS_GO(2);
    else if (trials <= 4) GCS_KS_GO(4);
    else GCS_KS_GO(8);
#undef GCS_KS_GO
    GCS_CHECK_LAUNCH("gcs_kmeans_seed");
    return GCS_OK;
}
