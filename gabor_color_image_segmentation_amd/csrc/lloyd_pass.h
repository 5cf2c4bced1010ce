// lloyd_pass.h — what the three Lloyd translation units share. Private to csrc/ (the ABI is include/gcs.h).
//   kmeans.hip        the entry points, lloyd_pass and the small kernels (init, gather, generic pass, reduce, finalize, widen)
//   lloyd_mfma.hip    kmeans_pass_mfma_kernel (D <= 207 on the matrix cores: split, compact-level-1 and self-updating modes)
//   lloyd_native.hip  kmeans_pass_native_kernel (deep banks: every level at its own resolution)
// Here: the helpers and constants both pass kernels use, WHICH pass kernel a (bank, k) takes - gcs_pass_kernel, the one place that
// decides it (the deep-bank pass's own limits: lloyd_native_kernel), for lloyd_pass, gcs_kmeans_pass_fused, gcs_kmeans_fused_workspace_bytes and the test hook gcs_selftest_pass_kernel
// alike -, and the two launchers. Every instantiation's template arguments are written once, in the two lists below.
#pragma once
#include "common.h"
#include <stdlib.h>
#include <type_traits>

// D = a * b + c with a 64-bit accumulator in ONE instruction. hipcc strength-reduces the C expression
// into sign extensions, 64-bit shifts and borrow chains (~10 instructions); the count is what costs here.
__device__ __forceinline__ long long mad_i64_i32(int a, int b, long long c) {
    long long d;
    asm("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(d) : "v"(a), "s"(b), "v"(c) : "vcc");
    return d;
}

// Tile loads of the passes and the Infinity Cache (256 MiB). Passes sweep the slab in alternating directions, so a pass STARTS on the
// bytes its predecessor read last: those are worth keeping in the cache; everything before them is evicted before anyone returns
// and allocating it only costs. The split-slab pass and the deep-bank pass therefore load the list positions below `nt_limit` with
// the nontemporal hint (buffer_load ... nt) and the last KP_MALL_KEEP_DEFAULT bytes of every sweep plain. Measured, round 6 (same box,
// two interleaved rounds each; tools/dbg/mall_keep_sweep.sh - then an environment hook, now variant builds -, profiles/r6_mall_keep_sweep.txt), whole steps of 64 images:
//   deep-bank pass (8x8 bank, 1 265 MB per pass, HBM-bound): every load plain 0.237 - 0.243 ms per pass, step 3 075 - 3 117 Mpix/s;
//     every load nt 0.220 - 0.223 ms, 3 172; the last 128 / 192 / 256 / 320 / 384 / 512 MB plain: 0.215 - 0.218 / 0.216 - 0.217 /
//     0.214 - 0.219 / 0.214 - 0.217 / 0.215 - 0.216 / 0.219 - 0.220 ms, step 3 193 - 3 202 / 3 216 - 3 228 / 3 213 - 3 252 /
//     3 216 - 3 236 / 3 209 - 3 213 / 3 199 - 3 215 Mpix/s: + 4 % with 192 - 320 MB (5.9 TB/s of algorithmic bytes);
//   split-slab pass (4x6 bank, 671 MB per pass, bound by its dependency chains): every load plain 5 277 - 5 296 Mpix/s, every load
//     nt 5 144 - 5 201 (the next pass no longer finds the end of the sweep in the cache), the last 128 / 192 / 256 / 320 / 384 /
//     512 MB plain: 5 279 - 5 289 / 5 272 - 5 316 / 5 308 - 5 325 / 5 316 - 5 320 / 5 304 - 5 335 / 5 202 - 5 316: + 0.7 % at 256 MB.
//     (Isolated passes of a sequence that interleaves other work, tools/ab.py: every load nt 0.141 - 0.144 against 0.151 - 0.161 ms.)
// History: round 4 introduced the hint as `nt ? __builtin_nontemporal_load(p) : *p` - hipcc merges the two arms into ONE plain
// load (and two branches around global loads likewise): from that commit until round 6 no pass kernel contained an `nt` load
// (ISA), whatever the flag said. The cache policy of a raw buffer load is an immediate operand: two instructions that stay two.
// The wide-slab kernels of kmeans_pass_mfma_kernel (banks outside the BASELINE configurations, -DGCS_NO_SPLIT) load plain.
#ifndef GCS_KP_MALL_KEEP_MB       // (variant builds for same-box sweeps: 0 = every load nt, a huge value = every load plain)
#define GCS_KP_MALL_KEEP_MB 256
#endif
constexpr long long KP_MALL_KEEP_DEFAULT = (long long)GCS_KP_MALL_KEEP_MB << 20;
// list positions (per sweep list: the whole batch, or one image with per-image codebooks) below the result are loaded `nt`
static int kp_nt_limit(const GcsLayout &lo, int B, int n_sets, long long tile_stream_bytes) {
    const long long lists = n_sets == B ? B : 1, nlist = (long long)lo.ntiles * (n_sets == B ? 1 : B);
    const long long keep_tiles = KP_MALL_KEEP_DEFAULT / tile_stream_bytes / lists;
    return (int)(nlist > keep_tiles ? nlist - keep_tiles : 0);
}
// Logical feature of plane `pl` of level LL, and its inverse, with the level a COMPILE-TIME constant: `lo` is a by-value kernel
// argument, and indexing one of its arrays with a per-lane level (gcs_logical_of_plane / gcs_plane_of_logical on a run-time plane)
// makes hipcc fetch the element from the kernarg segment with a VECTOR load and wait for it - four dependent loads and
// s_waitcnt vmcnt(0) in front of every centroid gather and every partial-row store of the round-4 kernels (ISA; stamps:
// profiles/r5_notes.md). The callers unroll over the levels and keep the result of the lane's own level.
template <int LL>
__device__ __forceinline__ int kp_logical_of(const GcsLayout &lo, int pl) {
    const int c = pl / lo.FL[LL];
    return c * lo.F + 2 * LL * lo.n_orient + (pl - c * lo.FL[LL]);
}
// physical plane of logical feature e, or -1 when e is not on level LL (also gives the level: the caller's LL)
template <int LL>
__device__ __forceinline__ int kp_plane_on_level(const GcsLayout &lo, int c, int f) {
    const int fl = f - 2 * LL * lo.n_orient;                  // filter index inside level LL
    return (LL < lo.n_levels && fl >= 0 && fl < lo.FL[LL]) ? lo.row0[LL] + c * lo.FL[LL] + fl : -1;
}
constexpr int KP_PITCH = KP_TP * 2 + 64;  // bytes per plane row: +64 B = 16 banks per row, so the 4 rows x 64 B of a
                                          // tr_b16 half-wave and the 8 rows of a ds_read_b128 lane group hit distinct banks
constexpr int KP_P1 = 128 + 48;           // bytes per COMPACT plane row (kmeans_pass_mfma_kernel, CL1: 64 parents + 48 B: the 4 rows x 2 lane groups
                                          // of a tr_b16 read and the 16 rows of an update read hit distinct 8-byte bank slots; 16-byte aligned)
constexpr int KP_DSTEPS_NARROW = 5;       // D <= 79  (every 4x6 bank): 80 plane rows, 46 KB LDS, 3 workgroups / CU
constexpr int KP_DSTEPS_WIDE = 13;        // D <= 207 (the 8x8 bank, D = 192): 208 plane rows, 120 KB LDS, 1 workgroup / CU

// ---------------------------------------------------------------------------------------
// The pass instantiations: id, display name, template arguments. The choice returns an id; the launchers switch over the same lists.
//   kmeans_pass_mfma_kernel<KT, NST, DSTEPS, WAVES, SPLIT, L0T>   (FUSED: gcs_pass_self_updating below)
// narrow<1,9>, narrow<1,10> and narrow<2,10> serve -DGCS_NO_SPLIT builds only: by default a bank with D < 80 that is not on the split
// slab has three or more levels and at most 1 230 staging chunks per tile (nst <= 5).
#ifdef GCS_NO_SPLIT
#define GCS_MFMA_PASSES_NO_SPLIT(X)                                  \
    X(NARROW_1_9, "narrow<1,9>", 1, 9, KP_DSTEPS_NARROW, 4, false, 0)   \
    X(NARROW_1_10, "narrow<1,10>", 1, 10, KP_DSTEPS_NARROW, 4, false, 0) \
    X(NARROW_2_10, "narrow<2,10>", 2, 10, KP_DSTEPS_NARROW, 4, false, 0)
#else
#define GCS_MFMA_PASSES_NO_SPLIT(X)
#endif
#define GCS_MFMA_PASSES(X)                                           \
    X(SPLIT_1_3_2, "split<1,3,2>", 1, 3, KP_DSTEPS_NARROW, 4, true, 2) \
    X(SPLIT_1_3, "split<1,3>", 1, 3, KP_DSTEPS_NARROW, 4, true, 0)     \
    X(SPLIT_1_5, "split<1,5>", 1, 5, KP_DSTEPS_NARROW, 4, true, 0)     \
    X(SPLIT_2_5, "split<2,5>", 2, 5, KP_DSTEPS_NARROW, 4, true, 0)     \
    X(NARROW_1_3, "narrow<1,3>", 1, 3, KP_DSTEPS_NARROW, 4, false, 0)  \
    X(NARROW_1_6, "narrow<1,6>", 1, 6, KP_DSTEPS_NARROW, 4, false, 0)  \
    X(NARROW_2_6, "narrow<2,6>", 2, 6, KP_DSTEPS_NARROW, 4, false, 0)  \
    GCS_MFMA_PASSES_NO_SPLIT(X)                                      \
    X(WIDE8W_1_5, "wide8w<1,5>", 1, 5, KP_DSTEPS_WIDE, 8, false, 0)    \
    X(WIDE_1_18, "wide<1,18>", 1, 18, KP_DSTEPS_WIDE, 4, false, 0)     \
    X(WIDE_1_26, "wide<1,26>", 1, 26, KP_DSTEPS_WIDE, 4, false, 0)     \
    X(WIDE_2_10, "wide<2,10>", 2, 10, KP_DSTEPS_WIDE, 4, false, 0)     \
    X(WIDE_2_18, "wide<2,18>", 2, 18, KP_DSTEPS_WIDE, 4, false, 0)     \
    X(WIDE_2_26, "wide<2,26>", 2, 26, KP_DSTEPS_WIDE, 4, false, 0)
//   kmeans_pass_native_kernel<NL, MINB, N0>. N0 = 6: level 0 has all 48 planes. Four levels whose level 0 has fewer keep all eight
//   staging addresses in a table: that variant does not fit 168 VGPRs and runs with two workgroups per CU.
#ifndef GCS_NV_MINB
#define GCS_NV_MINB 3
#endif
#define GCS_STR_(x) #x
#define GCS_STR(x) GCS_STR_(x)
#define GCS_NATIVE_PASSES(X)                                                          \
    X(NATIVE_2_FULL, "native<2," GCS_STR(GCS_NV_MINB) ",6>", 2, GCS_NV_MINB, 6)         \
    X(NATIVE_2, "native<2," GCS_STR(GCS_NV_MINB) ",0>", 2, GCS_NV_MINB, 0)              \
    X(NATIVE_3_FULL, "native<3," GCS_STR(GCS_NV_MINB) ",6>", 3, GCS_NV_MINB, 6)         \
    X(NATIVE_3, "native<3," GCS_STR(GCS_NV_MINB) ",0>", 3, GCS_NV_MINB, 0)              \
    X(NATIVE_4_FULL, "native<4," GCS_STR(GCS_NV_MINB) ",6>", 4, GCS_NV_MINB, 6)         \
    X(NATIVE_4, "native<4,2,0>", 4, 2, 0)

enum GcsPassKernel {
    GCS_PASS_GENERIC,                 // kmeans_assign_kernel<k> (D >= 208)
#define GCS_PASS_ID(id, ...) GCS_PASS_##id,
    GCS_MFMA_PASSES(GCS_PASS_ID) GCS_NATIVE_PASSES(GCS_PASS_ID)
#undef GCS_PASS_ID
    GCS_PASS_NONE                     // (lloyd_native_kernel: not a deep bank)
};
static inline const char *gcs_pass_name(GcsPassKernel pk) {
    switch (pk) {
#define GCS_PASS_NAME(id, name, ...) \
    case GCS_PASS_##id:              \
        return name;
        GCS_MFMA_PASSES(GCS_PASS_NAME) GCS_NATIVE_PASSES(GCS_PASS_NAME)
#undef GCS_PASS_NAME
    case GCS_PASS_GENERIC: return "generic";
    default: return nullptr;
    }
}
static inline bool gcs_pass_is_native(GcsPassKernel pk) {
    switch (pk) {
#define GCS_PASS_CASE(id, ...) case GCS_PASS_##id:
        GCS_NATIVE_PASSES(GCS_PASS_CASE)
#undef GCS_PASS_CASE
        return true;
    default: return false;
    }
}
// The self-updating pass (template flag FUSED of kmeans_pass_mfma_kernel, entry gcs_kmeans_pass_fused) exists for the banks that take
// the CL1 kernels with three staging rounds - the split slab (at most two pyramid levels, D <= 79), k <= 8, a tile of at most 12 288
// slots: every 4x6-style bank - and is that bank's classic instantiation with FUSED = true.
constexpr bool gcs_pass_self_updating(GcsPassKernel pk) { return pk == GCS_PASS_SPLIT_1_3 || pk == GCS_PASS_SPLIT_1_3_2; }

// the deep-bank pass's kernel for this bank, GCS_PASS_NONE when the bank is not one of its (lloyd_native.hip: the NV_* limits)
GcsPassKernel lloyd_native_kernel(const GcsLayout &lo) __attribute__((visibility("hidden")));

// Which kernel runs one Lloyd pass over a bank with k clusters (1 <= k <= GCS_K_MAX). Host arithmetic on the layout alone.
static inline GcsPassKernel gcs_pass_kernel(const GcsLayout &lo, int k) {
    if (lo.D >= 16 * KP_DSTEPS_WIDE) return GCS_PASS_GENERIC;          // generic VALU pass for wider feature vectors
    // matrix-core pass (every BASELINE bank: 4x6 -> D = 72, 8x8 -> D = 192)
    const int nchunk = lo.tile_bytes / 16;
    const int nst = (nchunk + 255) / 256;                              // staging chunks per thread (4-wave workgroups)
    if (lo.split) {                                                    // (D < 80, at most two levels: csrc/common.h)
        const int rounds = ((lo.S >> 4) + 255) / 256;                  // staging rounds: items of 16 slots per thread
        // (measured and dropped, profiles/r6_notes.md: eight waves per workgroup at two workgroups per CU - 0.28 against 0.15 ms
        //  per pass -, the assign A fragments in LDS, the second sub-tile's transposed reads under the first one's epilogue)
        if (k <= 8 && rounds <= 3) return lo.DL[0] >= 32 ? GCS_PASS_SPLIT_1_3_2 : GCS_PASS_SPLIT_1_3;
        return k <= 8 ? GCS_PASS_SPLIT_1_5 : GCS_PASS_SPLIT_2_5;
    }
    if (lo.D < 16 * KP_DSTEPS_NARROW) {
#ifdef GCS_NO_SPLIT
        if (nst > 6) return k > 8 ? GCS_PASS_NARROW_2_10 : nst <= 9 ? GCS_PASS_NARROW_1_9 : GCS_PASS_NARROW_1_10;
#endif
        if (k > 8) return GCS_PASS_NARROW_2_6;
        return nst <= 3 ? GCS_PASS_NARROW_1_3 : GCS_PASS_NARROW_1_6;
    }
    if (k <= 8) {
        const GcsPassKernel native = lloyd_native_kernel(lo);
        if (native != GCS_PASS_NONE) return native;
        // pyramid banks (config 4: 2 040 chunks per tile) fit 5 chunks per thread of an 8-wave workgroup without spills
        if ((nchunk + 511) / 512 <= 5) return GCS_PASS_WIDE8W_1_5;
        return nst <= 18 ? GCS_PASS_WIDE_1_18 : GCS_PASS_WIDE_1_26;
    }
    return nst <= 10 ? GCS_PASS_WIDE_2_10 : nst <= 18 ? GCS_PASS_WIDE_2_18 : GCS_PASS_WIDE_2_26;
}

// The `nt` limit of one launch of `pk` (kp_nt_limit): the one place that decides it, for both launchers and the test hook
// gcs_selftest_pass_nt_limit. What a tile streams per pass: the split slab 12 of its 16 bits per value (LO and MID runs; the TOP
// run only where flagged), the deep-bank pass the whole tile. The wide-slab kernels and the generic pass load plain: 0.
static inline int gcs_pass_nt_limit(GcsPassKernel pk, const GcsLayout &lo, int B, int n_sets) {
    if (gcs_pass_is_native(pk)) return kp_nt_limit(lo, B, n_sets, lo.tile_bytes);
    switch (pk) {
#define GCS_PASS_CASE(id, name, KT, NST, DSTEPS, WAVES, SPLIT, L0T) \
    case GCS_PASS_##id:                                             \
        return SPLIT ? kp_nt_limit(lo, B, n_sets, lo.tile_bytes / 4 * 3) : 0;
        GCS_MFMA_PASSES(GCS_PASS_CASE)
#undef GCS_PASS_CASE
    default: return 0;
    }
}

// What one launch of a matrix-core or deep-bank pass can address (lloyd_pass and gcs_kmeans_pass_fused refuse the rest)
static inline bool kp_batch_fits(const GcsLayout &lo, int B) {         // 4 * (tile index in the batch list) is kept in an int
    return (long long)B * lo.ntiles <= 0x1fffffffLL;
}
static inline bool kp_image_fits(const GcsLayout &lo) {                // MID / TOP runs are addressed by 32-bit offsets from the LO run
    return !lo.split || (unsigned long long)lo.img_bytes < (1ull << 32);
}

// One pass launch. The pass kernels have ONE label output, in raster order (`lab_out`, uint8 when `lab_u8`); either output may be NULL.
struct LloydPassArgs {
    const unsigned char *feats;
    const uint16_t *cent;
    GcsLayout lo;
    int B, k, n_sets, parts;          // parts = gcs_kmeans_parts_per_image
    int reverse, row_lo, row_hi;
    uint64_t *partials;
    void *lab_out;
    int lab_u8;
    hipStream_t stream;
};
// Enqueue `pk` (one of the family's ids); the caller checks the launch. fz != NULL: the self-updating form (gcs_pass_self_updating).
// Both launchers take the `nt` limit from gcs_pass_nt_limit(pk, a.lo, a.B, a.n_sets).
void lloyd_mfma_launch(GcsPassKernel pk, const LloydPassArgs &a, const GcsFold *fz) __attribute__((visibility("hidden")));
void lloyd_native_launch(GcsPassKernel pk, const LloydPassArgs &a) __attribute__((visibility("hidden")));
