// kmeans_level.h - what the kernels that measure a feature slab against codebooks share (SPEC.md §28, §30): the tile of a
// workgroup and one level's share of the k squared distances of a pixel. Moved here unchanged from kmeans_model.hip, so that
// gcs_kmeans_evaluate (kmeans_model.hip) and gcs_kmeans_costs (label_relax.hip) run the same device code.
#pragma once
#include "slab_slots.h"

namespace {

typedef unsigned long long u64;

constexpr int KE_TW = 32, KE_TH = 8, KE_THREADS = KE_TW * KE_TH;
constexpr int KE_HW_MAX = 4096, KE_D_MAX = 1536;        // 16 x 1536 centroid values = 48 KB of LDS
constexpr int KE_LP = 64 + 16 + 4;                      // level pixels under a workgroup: level 1: 4 x 16, level 2: 2 x 8, level 3: 1 x 4

// d[j] += sum over the planes of level L of (x - c_j)^2 at level pixel (yl, xl), which lies inside the level image.
template <bool SPLIT, int KB>
__device__ __forceinline__ void ke_level(const GcsLayout &lo, const unsigned char *img, const uint16_t *s_cent, int L, int yl, int xl,
                                         u64 (&d)[KB]) {
    SlabTap t = slab_tap(lo, img, L, yl, xl);
    const unsigned npl = (unsigned)KP_TP >> (2 * L);
    const unsigned *c = reinterpret_cast<const unsigned *>(s_cent + (size_t)lo.row0[L] * KB);
    for (int n = lo.DL[L]; n > 0; --n, c += KB / 2) {
        const unsigned v = (unsigned)slab_next<SPLIT>(lo, img, t, npl);
#pragma unroll
        for (int j = 0; j < KB; j += 2) {
            const unsigned cc = c[j >> 1];              // two centroids' values of this plane
            const unsigned a0 = __usad(v, cc & 0xffffu, 0u), a1 = __usad(v, cc >> 16, 0u);
            d[j] += (u64)a0 * a0;                       // |x - c| <= 65535: a term is below 2^32, the sum is 64-bit
            d[j + 1] += (u64)a1 * a1;
        }
    }
}

}  // namespace
