// lloyd_native.hip — the Lloyd pass of SPEC.md §4 for deep banks (csrc/lloyd_pass.h: which banks take which instantiation).
//   kmeans_pass_native_kernel  the pass for deep banks (BASELINE config 4): every level at its own resolution.
// Label maps leave the pass in RASTER order ([B][H][W] uint8 or int32), as from kmeans_pass_mfma_kernel (csrc/lloyd_mfma.hip).
// Nothing here allocates, frees or synchronises; the launcher enqueues on the caller's stream.
#include "lloyd_pass.h"

// ---------------------------------------------------------------------------------------
// One Lloyd pass for DEEP banks (80 <= D <= 207 with at most 48 planes on every pyramid level, k <= 8: the 8x8 bank of
// BASELINE config 4), every level consumed at its OWN resolution. The tile goes to LDS as it sits in HBM (32.6 KB for
// the 8x8 bank) instead of being replicated to 208 full-resolution plane rows (106 KB):
//   assign:  per level L the partial scores S_L[(j,pat)][parent] = A_pat^L * X^L on v_mfma_i32_32x32x32_i8 (3 K-steps of
//            16 planes per level; N = the block's 64 pixels, 16 / 4 / 1 parents). The key of SPEC.md §4 is linear in the
//            planes: key_j(px) = base_j - 32 U - 2^21 R2 with U = R0 + 256 R1 and (U, R2) summed over the levels at the
//            pixel's parents; the coarse (U, R2) pairs travel through a wave-private LDS table.
//   update:  (round 5) rows of the MFMA = (cluster j, byte b) - k <= 8 fills the 16 rows -, K = (pixel or parent, byte),
//            columns = 16 PLANES: sums[(j, b)][plane] = sel[(j, b)][(px, t)] * X[(px, t)][plane] with sel = the one-hot digit
//            (level 0: -128) or the count of voting pixels of label j under the parent (coarse levels) where t == b, 0
//            elsewhere. The B operand is then the plane row AS IT LIES in LDS (16 bytes = 8 pixels x (lo, hi): no byte
//            de-interleave), and a level's 48 planes are 3 accumulator tiles instead of 6: 48 accumulator VGPRs for the four
//            levels instead of 96 - with the compact tables below what lets THREE workgroups share a CU (168 VGPRs,
//            52.5 KB of LDS) instead of two. Level 0 on v_mfma_i32_16x16x64_i8 (two 32-pixel halves), the coarse levels on
//            v_mfma_i32_16x16x32_i8 (8 / 4 / 2 of the 8 K-slots of a lane group); n_j by v_bcnt.
// Same tile list, sweep order, validity rules, outputs and partial layout as kmeans_pass_mfma_kernel.
constexpr int NV_DL = 48, NV_KS = 3, NV_UT = 3;              // planes (LDS rows), assign K-steps and update plane tiles per level
constexpr int NV_NST = 8;                                     // 16-byte staging chunks per thread (tile_bytes <= 32 768)
constexpr int NV_P0 = KP_TP * 2, NV_P1 = 128 + 16, NV_P2 = 32 + 8, NV_P3 = 8;   // LDS bytes per plane row of level L
// Every LDS image below is laid out against the lane groups the LDS really serves (MI355X_MICROARCH.md, LDS: ds_read_b128 in FOUR
// NON-CONTIGUOUS groups of 16 lanes - {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -, ds_read_b64 / _tr_b16 in two
// groups of 32, ds_read_b32 in two groups of 32 on 32 banks), checked access by access with tools/design/lds_bank_model.py. The first
// round-5 build assumed contiguous groups of 16 and measured SQ_LDS_BANK_CONFLICT 31.5 M cycles per launch = 810 per tile.
//  * Level 0 (512-byte rows, no padding): chunk c of plane row r sits at chunk c ^ nv_swz(r). Transposed reads (4 consecutive rows x
//    64 bytes per half wave) want the HIGH two bits of the swizzle to differ over 4 consecutive rows; the update's operand read (16
//    rows, one chunk each; a lane group holds rows {0-3, 12-15} of K-group g and rows {4-11} of K-group g ^ 1, whose chunk differs by
//    XOR 2) wants the low two bits of rows 4-11 closed under XOR 2: the Gray code of r >> 2.
//  * Level 1 (128-byte rows + 16): 16 consecutive rows start in 16 distinct 16-byte columns (9 r mod 16) for the update's read, 4
//    consecutive rows' 32-byte windows are disjoint for the transposed read.
//  * Level 2 (32-byte rows + 8): 16 consecutive rows start in 16 distinct banks of the 32 a ds_read_b32 sees (10 r mod 32).
__host__ __device__ constexpr int nv_swz(int r) { return ((r & 3) << 2) | (((r >> 2) & 3) ^ ((r >> 3) & 1)); }
constexpr int NV_OFF1 = NV_DL * NV_P0, NV_OFF2 = NV_OFF1 + NV_DL * NV_P1, NV_OFF3 = NV_OFF2 + NV_DL * NV_P2;
constexpr int NV_END = NV_OFF3 + NV_DL * NV_P3;
constexpr int NV_PART_W = 8 * (16 + 4 + 1);                  // (U, R2) pairs per wave: [cluster][16 | 4 | 1 parents of level 1 | 2 | 3]
// A fragments per (level, K-step): slot 32 h + 16 g + 4 q + pat for K-half h, pattern pat (3 = all zero) of cluster jj, g = parity of
// jj's bit count, q = jj >> 1: the 16 lanes of a ds_read_b128 lane group hold four clusters of ONE parity class ({0, 3, 5, 6} or
// {1, 2, 4, 7}), so their 16 slots are 16 consecutive 16-byte columns (the round-5 first build, 49 slots with one shared zero slot,
// put a group's lanes on 8 columns: 384 of the 810 conflict cycles per tile)
constexpr int NV_APAT_SLOTS = 64;

// B fragments by hardware transpose (see kmeans_pass_mfma_kernel): issue only; nv_wait() then waits once for everything
template <int PITCH, int OFS = 0>
__device__ __forceinline__ void nv_issue(unsigned addr, v2i (&fa)[NV_KS], v2i (&fb)[NV_KS]) {
    static_assert(OFS + (NV_KS - 1) * 16 * PITCH + 4 * PITCH < 65536, "K-step offsets must fit the 16-bit DS offset field");
#pragma unroll
    for (int kk = 0; kk < NV_KS; ++kk)                       // ONE address register per chain: the K-steps are immediates
        asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%c3\n\t"
                     "ds_read_b64_tr_b16 %1, %2 offset:%c4"
                     : "=&v"(fa[kk]), "=&v"(fb[kk])
                     : "v"(addr), "i"(OFS + kk * 16 * PITCH), "i"(OFS + kk * 16 * PITCH + 4 * PITCH)
                     : "memory");
}
// level 0: the two reads of a K-step have bases of their own (swizzled rows)
__device__ __forceinline__ void nv_issue0(unsigned addr_a, unsigned addr_b, v2i (&fa)[NV_KS], v2i (&fb)[NV_KS]) {
#pragma unroll
    for (int kk = 0; kk < NV_KS; ++kk)
        asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%c4\n\t"
                     "ds_read_b64_tr_b16 %1, %3 offset:%c4"
                     : "=&v"(fa[kk]), "=&v"(fb[kk])
                     : "v"(addr_a), "v"(addr_b), "i"(kk * 16 * NV_P0)
                     : "memory");
}
__device__ __forceinline__ void nv_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void nv_take(v2i (&fa)[NV_KS], v2i (&fb)[NV_KS], v4i (&bfr)[NV_KS]) {
#pragma unroll
    for (int kk = 0; kk < NV_KS; ++kk) {
        asm volatile("" : "+v"(fa[kk]), "+v"(fb[kk]));
        bfr[kk] = v4i{fa[kk][0], fa[kk][1], fb[kk][0], fb[kk][1]};
    }
}
__device__ __forceinline__ long long nv_pack64(unsigned lo, unsigned hi) { return (long long)(((unsigned long long)hi << 32) | lo); }

// MINB = workgroups per CU the register budget is set for (3: 168 VGPRs); N0 = staging rounds wholly inside level 0 (see staging)
template <int NL, int MINB, int N0>
__global__ __launch_bounds__(256, MINB) void kmeans_pass_native_kernel(
    const unsigned char *__restrict__ feats, const uint16_t *__restrict__ cent, GcsLayout lo, int K, int per_image,
    int parts, int parts_eff, int reverse, int row_lo, int row_hi, uint64_t *__restrict__ partials,
    void *__restrict__ raster, int raster_u8, int nt_flag) {
    // LDS, one carve-up: [tile as in HBM, rows padded | (U, R2) tables | assign A fragments | labels | key bases | n_j].
    // The transposed reads of level 3 run up to 64 bytes past the tile (unused columns): they land in the tables.
    constexpr int TILE_B = NL == 2 ? NV_OFF2 : NL == 3 ? NV_OFF3 : NV_END;
    constexpr int PART_O = TILE_B, APAT_O = PART_O + 4 * NV_PART_W * 8, LAB_O = APAT_O + NL * NV_KS * NV_APAT_SLOTS * 16;
    constexpr int CONST_O = LAB_O + KP_TP, NJ_O = CONST_O + 16 * 8, LDS_B = NJ_O + 16 * 8;
    static_assert(MINB * ((LDS_B + 1279) / 1280) <= 128, "LDS: gfx950 allocates 160 KB in 1280-byte granules");
    __shared__ __attribute__((aligned(64))) unsigned char s_mem[LDS_B];   // (stage_write XORs bits 4-5 of full level-0 addresses: the base must be a multiple of 64)
    unsigned char *const s_tile = s_mem;
    v4i *const s_apat = reinterpret_cast<v4i *>(s_mem + APAT_O);             // [level][K-step][slot]
    unsigned char *const s_lab = s_mem + LAB_O;
    long long *const s_const = reinterpret_cast<long long *>(s_mem + CONST_O);
    long long *const s_nj = reinterpret_cast<long long *>(s_mem + NJ_O);

    typedef __attribute__((address_space(3))) v4i *lds_v4i_ptr;
    typedef __attribute__((address_space(3))) unsigned char *lds_uchar_ptr;
    const bool do_acc = partials != nullptr;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid (B, parts): workgroups are dispatched part-major, so the parts_eff * B working ones are the first to start
    const int b = blockIdx.x, part = blockIdx.y, nb = (int)gridDim.x;
    const int D = lo.D, D1 = D + 1;
    const uint16_t *cset = cent + (size_t)(per_image ? b : 0) * K * D;
    const int ntiles = lo.ntiles;
    const bool working = part < parts_eff;                   // MINB workgroups per CU are resident: the others only emit zeros
    const int nimg = per_image ? 1 : nb;
    const int G = parts_eff * nimg, g = per_image ? part : part * nb + b;
    const int nlist = ntiles * nimg;
    const size_t img0 = per_image ? (size_t)b * ntiles : 0;
    const unsigned char *fb = feats + img0 * lo.tile_bytes;
    auto prow = [&](int i) -> size_t { return partial_index(per_image, b, part, parts, nb, i, K * D1); };
    if (!working) {                                              // a zero partial row, nothing else
        if (do_acc)
            for (int i = tid; i < K * D1; i += 256) partials[prow(i)] = 0;
        return;
    }

    // ---- staging: chunk ci (16 bytes at byte 16*ci of the tile) keeps its place inside its level (level 0 swizzled, level-1
    //      plane rows at NV_P1, level-2 rows at NV_P2). The FIRST tile's loads go out inside the centroid prologue, right behind its
    //      gathers (below): the tile's HBM latency (3 - 4 us under load) passes under the key bases and the A fragments. (In
    //      kmeans_pass_mfma_kernel, whose prologue is 3 us, the same move measured nothing: 0.1566 against 0.1566 ms; not done there.)
    const int nchunk = lo.tile_bytes >> 4;
    const int c1s = NL > 1 ? lo.off[1] >> 4 : nchunk, c2s = NL > 2 ? lo.off[2] >> 4 : nchunk,
              c3s = NL > 3 ? lo.off[3] >> 4 : nchunk;
    // Rounds i < N0 lie wholly inside level 0 (N0 = 6 for the 48-plane level 0 of every bank with 8 orientations, else 0): chunk
    // tid + 256 i is 16 bytes at offset 16 tid + 4096 i of the tile, plane row (tid >> 5) + 8 i, whose swizzle is that of row tid >> 5
    // ^ 2 for odd i - ONE address register for all of them, a scalar add on the tile base per round. The other rounds keep a table.
    v4i st[NV_NST];
    unsigned sadr[NV_NST - N0];                             // per chunk: LDS byte address << 16 | byte offset inside the tile (both < 65 536)
    const unsigned s0adr = (unsigned)(size_t)(lds_uchar_ptr)s_mem + (tid >> 5) * NV_P0 + (((tid & 31) ^ nv_swz(tid >> 5)) << 4);
    static_assert((nv_swz(0) ^ nv_swz(8)) == 3 && (nv_swz(7) ^ nv_swz(15)) == 3 && nv_swz(5) == nv_swz(21), "staging: rows r and r + 8");
    int split = 0;                                          // rounds that hold level-2 chunks (40-byte rows: two 8-byte stores)
#pragma unroll
    for (int i = N0; i < NV_NST; ++i) {
        const int ci = min(tid + 256 * i, nchunk - 1);
        int d;
        if (ci < c1s) d = (ci >> 5) * NV_P0 + ((ci & 31) ^ nv_swz(ci >> 5)) * 16;
        else if (ci < c2s) d = NV_OFF1 + ((ci - c1s) >> 3) * NV_P1 + ((ci - c1s) & 7) * 16;
        else if (ci < c3s) d = NV_OFF2 + ((ci - c2s) >> 1) * NV_P2 + ((ci - c2s) & 1) * 16;
        else d = NV_OFF3 + (ci - c3s) * 16;
        sadr[i - N0] = ((unsigned)(size_t)(lds_uchar_ptr)s_mem + (unsigned)d) << 16 | (unsigned)(ci * 16);
        if (NL > 2 && 256 * i < c3s && 256 * i + 255 >= c2s) split |= 1 << i;
    }
    // Raw buffer loads: a descriptor over the tile (uniform base) + 32-bit lane offset; the cache policy is an immediate of the
    // intrinsic, so the plain and the `nt` form both survive (see stage_load_split of kmeans_pass_mfma_kernel and lloyd_pass)
    auto stage_load = [&](int tile, bool nt) {
        const unsigned char *tb = fb + (size_t)tile * lo.tile_bytes;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(tb), 0, -1, 0x00020000);
        unsigned o0 = (unsigned)tid * 16u;
        asm volatile("" : "+v"(o0));                        // (opaque: see below)
        auto go = [&](auto aux_c) {
            constexpr int AUX = decltype(aux_c)::value;     // gfx940+: bit 1 = nt
#pragma unroll
            for (int i = 0; i < N0; ++i) st[i] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)o0, i * 4096, AUX));
#pragma unroll
            for (int i = N0; i < NV_NST; ++i) {
                unsigned o = sadr[i - N0] & 0xffffu;        // (opaque: hoisted out of the tile loop these spilled - and a reload
                asm volatile("" : "+v"(o));                 //  inside the loop waits for vmcnt(0))
                st[i] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)o, 0, AUX));
            }
        };
        if (nt) go(std::integral_constant<int, 2>{});
        else go(std::integral_constant<int, 0>{});
    };
    auto stage_write = [&]() {
#pragma unroll
        for (int i = 0; i < N0; ++i) *reinterpret_cast<lds_v4i_ptr>((s0adr ^ ((i & 1) * 48u)) + i * 8 * NV_P0) = st[i];
#pragma unroll
        for (int i = N0; i < NV_NST; ++i) {
            const unsigned a = sadr[i - N0] >> 16;
            if (NL > 2 && (split >> i & 1)) {                // (wave-uniform) level-2 rows are 8-byte aligned only
                typedef __attribute__((address_space(3))) v2i *lds_v2i_ptr;
                *reinterpret_cast<lds_v2i_ptr>(a) = v2i{st[i][0], st[i][1]};
                *reinterpret_cast<lds_v2i_ptr>(a + 8) = v2i{st[i][2], st[i][3]};
            } else {
                *reinterpret_cast<lds_v4i_ptr>(a) = st[i];
            }
        }
    };
    auto phys = [&](int lt) { return reverse ? nlist - 1 - lt : lt; };
    // ---- centroids -> scratch [8 clusters][4 levels][48 planes] u16, offset-binary, zero where nothing exists. The six gathers of a
    //      thread go out FIRST, the first tile's eight loads behind them, and only then are the gathers consumed: loads return in
    //      order, so a gather issued behind the tile (the first round-5 build) waited for the tile's 32 KB as well (stamps: the
    //      gather loop took 5.6 - 6.7 us of a 10 - 11.6 us prologue).
    uint16_t *cs = reinterpret_cast<uint16_t *>(s_tile);
    static_assert(8 * 4 * NV_DL * 2 <= TILE_B && (8 * 4 * NV_DL) % 256 == 0, "centroid scratch: tile buffer, whole rounds");
    constexpr int NCS = 8 * 4 * NV_DL / 256;
    unsigned cv[NCS];
#pragma unroll
    for (int r = 0; r < NCS; ++r) {
        const int i = tid + 256 * r;
        const int j = i / (4 * NV_DL), L = (i / NV_DL) & 3, pl = i % NV_DL;
        bool ok = false;                                     // (levels unrolled: kp_logical_of)
        int e = 0;
        if (L == 0 && pl < lo.DL[0]) { ok = true; e = kp_logical_of<0>(lo, pl); }
        if (NL > 1 && L == 1 && pl < lo.DL[1]) { ok = true; e = kp_logical_of<1>(lo, pl); }
        if (NL > 2 && L == 2 && pl < lo.DL[2]) { ok = true; e = kp_logical_of<2>(lo, pl); }
        if (NL > 3 && L == 3 && pl < lo.DL[3]) { ok = true; e = kp_logical_of<3>(lo, pl); }
        ok = ok && j < K;
        const int src = ok ? j * D + e : 0;
        cv[r] = (unsigned)cset[src] | (ok ? 0u : 0x10000u);   // (bit 16: nothing exists there)
    }
    int ltile = g;
    const int nt_limit = __builtin_amdgcn_readfirstlane(nt_flag);   // list positions below it are loaded `nt` (lloyd_pass)
    if (ltile < nlist) stage_load(phys(ltile), ltile < nt_limit);
#pragma unroll
    for (int r = 0; r < NCS; ++r) cs[tid + 256 * r] = (cv[r] & 0x10000u) ? (uint16_t)0 : (uint16_t)(cv[r] ^ 0x8080u);
    __syncthreads();
    for (int j = tid >> 4; j < 16; j += 16) {                // key base, as in kmeans_pass_mfma_kernel
        const int sub = tid & 15;
        long long nrm = 0, scl = 0, sch = 0;
        if (j < K && j < 8) {
#pragma unroll
            for (int L = 0; L < NL; ++L)                       // (levels unrolled: every lo.DL[L] a plain kernel argument)
                for (int pl = sub; pl < lo.DL[L]; pl += 16) {
                    const unsigned c = cs[(j * 4 + L) * NV_DL + pl] ^ 0x8080u;
                    nrm += (long long)((unsigned long long)c * c);
                    scl += c & 255;
                    sch += c >> 8;
                }
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            nrm += __shfl_xor(nrm, m);
            scl += __shfl_xor(scl, m);
            sch += __shfl_xor(sch, m);
        }
        if (sub == 0) {
            const long long q = 16384LL * D;
            const long long gg = (128 * scl - q) + 256 * (128 * (sch + scl) - 2 * q) + 65536 * (128 * sch - q);
            s_const[j] = j < K ? 16 * (nrm - 2 * gg) + j : (1LL << 62) + j;
        }
    }
    // ---- assign A fragments per level: row r = 4*jj + pat (cluster jj), k-slot (h, t) of K-step kk = (plane 16*kk + 8*h + t/2,
    //      byte t&1) of the level; patterns LL / M / HH as in kmeans_pass_mfma_kernel. Row pattern 3 is all zero: the 16 lanes
    //      that hold it read a zero slot of their own (NV_APAT_SLOTS).
    const int a_jj = (lane & 31) >> 2;
    const int a_slot = 32 * (lane >> 5) + 16 * (__builtin_popcount(a_jj) & 1) + 4 * (a_jj >> 1) + (lane & 3);
    if (wave < NL) {                                         // one level per wave
        const int r = lane & 31, h = lane >> 5;
        const int jj = r >> 2, pat = r & 3;
        const unsigned msk = pat == 0 ? 0x00ff00ffu : pat == 1 ? 0xffffffffu : pat == 2 ? 0xff00ff00u : 0u;
        const unsigned sel = pat == 1 ? 0x02030001u : 0x03020100u;
        {
            const int L = wave;
#pragma unroll
            for (int kk = 0; kk < NV_KS; ++kk) {
                const v4i w = *reinterpret_cast<const v4i *>(&cs[(jj * 4 + L) * NV_DL + 16 * kk + 8 * h]);
                v4i f;
#pragma unroll
                for (int e = 0; e < 4; ++e) f[e] = (int)(__builtin_amdgcn_perm(0u, (unsigned)w[e], sel) & msk);
                s_apat[(L * NV_KS + kk) * NV_APAT_SLOTS + a_slot] = f;   // (pattern 3: msk == 0, f == 0)
            }
        }
    }
    __syncthreads();                                   // scratch reads done: the tile buffer is free
    v4i accu[NL][NV_UT];
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
        for (int nt = 0; nt < NV_UT; ++nt) accu[L][nt] = v4i{0, 0, 0, 0};
    int cntacc = 0;

    // update operand coordinates: row um = 2 * cluster + byte, K-group ukg = pixel rows 2 ukg, 2 ukg + 1 of the block
    const int um = lane & 15, ukg = lane >> 4;
    // one-hot bytes (b0 b1 b2 b3) of four pixels -> K-slots (px, t): (b0 0 b1 0 | b2 0 b3 0) for the low-byte rows, shifted up one
    // byte for the high-byte rows (v_perm: selectors 4 .. 7 = bytes of the zero operand). ONE register holds the row's personality:
    // the selector for (b0, b1); the one for (b2, b3) is it ^ 0x02020202, the byte shift of the count operands (it & 4) << 1,
    // and the cluster's compare pattern comes from the lane number (three invariants fewer than the tile loop can keep).
    const unsigned uselA0 = (um & 1) ? 0x01040004u : 0x04010400u;

    const int s1 = __builtin_amdgcn_readfirstlane(G % ntiles);
    const int q1 = __builtin_amdgcn_readfirstlane(4 * s1 / lo.bx_n), r1 = 4 * s1 - q1 * lo.bx_n;
    const int q2 = __builtin_amdgcn_readfirstlane(4 * (ntiles - s1) / lo.bx_n), r2 = 4 * (ntiles - s1) - q2 * lo.bx_n;
    int tin = __builtin_amdgcn_readfirstlane(phys(g < nlist ? g : 0) % ntiles);
    int by, bx;
    {
        const int blk0 = 4 * tin + wave;
        by = blk0 / lo.bx_n;
        bx = blk0 - by * lo.bx_n;
    }
    // ---- LDS addresses as plain integers: every lane keeps ONE base per access pattern and everything else is an
    //      immediate of the DS instruction (left to itself hipcc hoists one register per (level, cluster pair, K-step) out of the
    //      tile loop: 30 more invariants than three workgroups per CU leave room for)
    typedef __attribute__((address_space(3))) const v4i *lds_cv4i;
    typedef __attribute__((address_space(3))) const v2i *lds_cv2i;
    typedef __attribute__((address_space(3))) v2i *lds_v2i;
    typedef __attribute__((address_space(3))) const long long *lds_ci64;
    typedef __attribute__((address_space(3))) const unsigned *lds_cu32;
    typedef __attribute__((address_space(3))) const uint16_t *lds_cu16;
    typedef __attribute__((address_space(3))) unsigned char *lds_u8;
    const unsigned L0 = (unsigned)(size_t)(lds_uchar_ptr)s_mem;            // LDS address of the carve-up
    unsigned a_tr[4], a_tr0b, a_apat, a_pw[3], a_pr[2], a_labw, a_labr, a_ub[4];
    {
        const int n = lane & 31, h = lane >> 5, i16 = lane & 15, pxblk = (lane >> 4) & 1;
        const int rowq = 8 * h + (i16 >> 2), colq = 4 * (i16 & 3);
        // transposed reads. level 0 (swizzled rows, see nv_swz): the first read of a K-step takes rows rowq + 16 kk, the second rows
        // + 4 - their chunk columns differ (nv_swz(r + 4) != nv_swz(r)), hence two bases; sub-tile 1 = both ^ 64.
        // level 1: the block's 16 parents are columns 16*wave .. +15; level 2: its 4 parents are columns
        // 4*wave .. +3 of the plane's 16; level 3: its parent is column `wave` of the plane's 4 (the transpose read wants
        // 8-byte-aligned column starts, so these two read the whole plane row). The second 16-lane block of a half wave
        // (output columns 16 .. 31: kept by no coarse level) reads the addresses of the first: a broadcast, no bank of its own.
        const int c0 = wave * 8 + 2 * pxblk + ((i16 & 3) >> 1);
        a_tr[0] = rowq * NV_P0 + ((c0 ^ nv_swz(rowq)) << 4) + (i16 & 1) * 8;
        a_tr0b = (rowq + 4) * NV_P0 + ((c0 ^ nv_swz(rowq + 4)) << 4) + (i16 & 1) * 8;
        a_tr[1] = L0 + NV_OFF1 + rowq * NV_P1 + (16 * wave + colq) * 2;
        a_tr[2] = L0 + NV_OFF2 + rowq * NV_P2 + colq * 2;
        a_tr[3] = L0 + NV_OFF3 + rowq * NV_P3 + (16 * pxblk + colq) * 2;
        a_apat = L0 + APAT_O + a_slot * 16;
        // the wave's (U, R2) table: [cluster][16] level 1 | 128 + [cluster][4] level 2 | 160 + [cluster] level 3; cluster 2 gq + h
        const unsigned pw = L0 + PART_O + wave * NV_PART_W * 8;
        a_pw[0] = pw + (h * 16 + (n & 15)) * 8;
        a_pw[1] = pw + (128 + h * 4 + (n & 3)) * 8;
        a_pw[2] = pw + (160 + h) * 8;
        a_pr[0] = pw + (h * 16 + (n >> 4) * 4 + ((n & 7) >> 1)) * 8;       // sub-tile 0; sub-tile 1: 8 parents on
        a_pr[1] = pw + (128 + h * 4 + ((n & 7) >> 2)) * 8;                 // sub-tile 1: 2 parents on
        a_labw = L0 + LAB_O + wave * 64 + n;
        a_labr = L0 + LAB_O + wave * 64 + 16 * ukg;
        a_ub[0] = um * NV_P0 + (((wave * 8 + 2 * ukg) ^ nv_swz(um)) << 4);          // pixel row 2 ukg of the block; row 2 ukg + 1: ^ 16
        a_ub[1] = L0 + NV_OFF1 + um * NV_P1 + (wave * 16 + 4 * ukg) * 2;
        a_ub[2] = L0 + NV_OFF2 + um * NV_P2 + (wave * 4 + (ukg >> 1) * 2) * 2;
        a_ub[3] = L0 + NV_OFF3 + um * NV_P3 + wave * 2;
    }
    for (; ltile < nlist; ltile += G) {
        const int tile = phys(ltile);
        stage_write();
        __syncthreads();
        __builtin_amdgcn_s_setprio(3);
        if (ltile + G < nlist) stage_load(phys(ltile + G), ltile + G < nt_limit);   // in flight during the MFMAs
        __builtin_amdgcn_s_setprio(0);

        const int blk = 4 * tin + wave;
        const int n = lane & 31, h = lane >> 5;
        // -------- assign
        // Software pipeline over the five MFMA chains of a tile (levels 1 .. NL-1, then the two 32-pixel sub-tiles of level 0):
        // the transposed reads of chain c + 1 go out before the MFMAs of chain c, one chain's fragments in flight at a time
        // (all of them at once: 36 more VGPRs than three workgroups per CU leave).
        v2i fa[2][NV_KS], fbv[2][NV_KS];
        auto issue_chain = [&](int c, v2i (&xa)[NV_KS], v2i (&xb)[NV_KS]) {     // c = 0 .. NL-2: level c + 1; NL-1, NL: sub-tiles
            if (c == 0 && NL > 1) nv_issue<NV_P1>(a_tr[1], xa, xb);
            else if (c == 1 && NL > 2) nv_issue<NV_P2>(a_tr[2], xa, xb);
            else if (c == 2 && NL > 3) nv_issue<NV_P3>(a_tr[3], xa, xb);
            else nv_issue0(L0 + (a_tr[0] ^ (c == NL - 1 ? 0u : 64u)), L0 + (a_tr0b ^ (c == NL - 1 ? 0u : 64u)), xa, xb);
        };
        auto apat = [&](int L, int kk) { return *reinterpret_cast<lds_cv4i>(a_apat + (L * NV_KS + kk) * NV_APAT_SLOTS * 16); };
        issue_chain(0, fa[0], fbv[0]);
        // coarse levels: (U, R2) per cluster and parent of this wave's block -> the wave's table
#pragma unroll
        for (int L = 1; L < NL; ++L) {
            v4i bfr[NV_KS];
            nv_wait();
            nv_take(fa[(L - 1) & 1], fbv[(L - 1) & 1], bfr);
            issue_chain(L, fa[L & 1], fbv[L & 1]);
            v16i acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0;
#pragma unroll
            for (int kk = 0; kk < NV_KS; ++kk) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(apat(L, kk), bfr[kk], acc, 0, 0, 0);
            const bool keep = L == 1 ? n < 16 : L == 2 ? (n >> 2) == wave : n == wave;
            const int cstride = L == 1 ? 32 : L == 2 ? 8 : 2;          // two clusters on
            if (keep)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
                    *reinterpret_cast<lds_v2i>(a_pw[L - 1] + gq * cstride * 8) =
                        v2i{__mul24(acc[4 * gq + 1], 256) + acc[4 * gq], acc[4 * gq + 2]};
        }
        // level 0: two 32-pixel sub-tiles (rows 4*sub .. 4*sub+3 of the block), one after the other
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            v16i acc0;
            {
                const int c = NL - 1 + sub;
                v4i bfr[NV_KS];
                nv_wait();
                nv_take(fa[c & 1], fbv[c & 1], bfr);                          // chain c travels in buffer c & 1
                if (sub == 0) issue_chain(c + 1, fa[(c + 1) & 1], fbv[(c + 1) & 1]);
#pragma unroll
                for (int e = 0; e < 16; ++e) acc0[e] = 0;
#pragma unroll
                for (int kk = 0; kk < NV_KS; ++kk) acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(apat(0, kk), bfr[kk], acc0, 0, 0, 0);
            }
            long long best = 0x7fffffffffffffffLL;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                int u = __mul24(acc0[4 * gq + 1], 256) + acc0[4 * gq], r2v = acc0[4 * gq + 2];
                if (NL > 1) { const v2i c = *reinterpret_cast<lds_cv2i>(a_pr[0] + gq * 256 + sub * 64); u += c[0]; r2v += c[1]; }
                if (NL > 2) { const v2i c = *reinterpret_cast<lds_cv2i>(a_pr[1] + gq * 64 + sub * 16); u += c[0]; r2v += c[1]; }
                if (NL > 3) { const v2i c = *reinterpret_cast<lds_cv2i>(a_pw[2] + gq * 16); u += c[0]; r2v += c[1]; }
                // key base of cluster 2 gq + h: a broadcast read (uniform address per half wave)
                const long long kb = *reinterpret_cast<lds_ci64>(L0 + CONST_O + gq * 16 + h * 8);
                long long key = mad_i64_i32(u, -32, kb);
                key = mad_i64_i32(r2v, -2097152, key);
                best = key < best ? key : best;
            }
            const unsigned blo = (unsigned)best, bhi = (unsigned)((unsigned long long)best >> 32);
            const auto s0 = __builtin_amdgcn_permlane32_swap(blo, blo, false, false);
            const auto s1v = __builtin_amdgcn_permlane32_swap(bhi, bhi, false, false);
            // (element 0 = the lower half's best in both halves, element 1 = the upper half's: see kmeans_pass_mfma_kernel)
            const long long ka = (long long)(((unsigned long long)s1v[0] << 32) | s0[0]);
            const long long kb2 = (long long)(((unsigned long long)s1v[1] << 32) | s0[1]);
            const int bj = (int)((kb2 < ka ? s0[1] : s0[0]) & 15);
            if (h == 0) {
                const int yi = 4 * sub + (n >> 3), xi = n & 7;               // pixel inside the block
                int y = 8 * by + yi, x = 8 * bx + xi, xlim = lo.W;          // see kmeans_pass_mfma_kernel
                if (NL <= 2 && blk >= lo.nmain) {               // (deeper banks have main blocks only)
                    int no = n;
                    asm volatile("" : "+v"(no));
                    gcs_strip_pixel(lo, blk, 4 * sub + (no >> 3), no & 7, y, x, xlim);
                }
                const bool inimg = blk < lo.nblk && y < lo.H && x < xlim;
                const bool valid = inimg && y >= row_lo && y < row_hi;
                *reinterpret_cast<lds_u8>(a_labw + sub * 32) = valid ? (unsigned char)bj : (unsigned char)0xFF;
                if (raster && inimg) {                        // raster label map (see kmeans_pass_mfma_kernel)
                    const size_t o = ((size_t)(per_image ? b : tile / ntiles) * lo.H + y) * lo.W + x;
                    if (raster_u8) static_cast<uint8_t *>(raster)[o] = (uint8_t)bj;
                    else static_cast<int32_t *>(raster)[o] = bj;
                }
            }
        }
        // -------- update (the block's labels were written by this wave: no barrier)
        if (do_acc) {
            const v4i lw = *reinterpret_cast<lds_cv4i>(a_labr);   // labels of pixel rows 2 ukg (bytes 0-7), 2 ukg + 1
            unsigned uselA = uselA0, lno = (unsigned)lane;
            asm volatile("" : "+v"(uselA), "+v"(lno));            // (opaque: what follows is recomputed per tile, not hoisted)
            const unsigned uselB = uselA ^ 0x02020202u, ush = (uselA & 4u) << 1;
            const unsigned eqr = ((lno >> 1) & 7u) * 0x01010101u;
            v4i oh;                                              // byte 0x80 where label == this row's cluster
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned x = (unsigned)lw[i] ^ eqr;
                const unsigned y = (x | 0x80808080u) - 0x01010101u;
                oh[i] = (int)(~y & 0x80808080u);
            }
            cntacc += __builtin_popcount((unsigned)oh[0]) + __builtin_popcount((unsigned)oh[1]) +
                      __builtin_popcount((unsigned)oh[2]) + __builtin_popcount((unsigned)oh[3]);
            // level 0: half hf = pixel row 2 ukg + hf of the block for this K-group; K-slot 2 q + t = (pixel q of the row, byte t)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                v4i a0;
                a0[0] = (int)__builtin_amdgcn_perm(0u, (unsigned)oh[2 * hf], uselA);
                a0[1] = (int)__builtin_amdgcn_perm(0u, (unsigned)oh[2 * hf], uselB);
                a0[2] = (int)__builtin_amdgcn_perm(0u, (unsigned)oh[2 * hf + 1], uselA);
                a0[3] = (int)__builtin_amdgcn_perm(0u, (unsigned)oh[2 * hf + 1], uselB);
#pragma unroll
                for (int nt = 0; nt < NV_UT; ++nt) {
                    const v4i bq = *reinterpret_cast<lds_cv4i>(L0 + (a_ub[0] ^ (hf * 16u)) + nt * 16 * NV_P0);
                    accu[0][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bq, accu[0][nt], 0, 0, 0);
                }
            }
            if constexpr (NL > 1) {
                // counts of this row's label under the 4 level-1 parents of pixel rows 2 ukg, 2 ukg + 1 (parent row ukg, columns 0..3)
                const unsigned e0 = (unsigned)oh[0] >> 7, e1 = (unsigned)oh[1] >> 7, e2 = (unsigned)oh[2] >> 7, e3 = (unsigned)oh[3] >> 7;
                const unsigned sa = e0 + e2, sb = e1 + e3;       // bytes: columns 0..3 / 4..7, both rows
                const unsigned ta = (sa & 0x00ff00ffu) + ((sa >> 8) & 0x00ff00ffu);   // bytes (c0 0 c1 0): K-slots (parent 0, lo) (0, hi) (1, lo) (1, hi)
                const unsigned tb = (sb & 0x00ff00ffu) + ((sb >> 8) & 0x00ff00ffu);   // parents 2, 3
                const long long a1 = nv_pack64(ta << ush, tb << ush);
#pragma unroll
                for (int nt = 0; nt < NV_UT; ++nt) {
                    const v2i w = *reinterpret_cast<lds_cv2i>(a_ub[1] + nt * 16 * NV_P1);
                    accu[1][nt] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, nv_pack64((unsigned)w[0], (unsigned)w[1]), accu[1][nt], 0, 0, 0);
                }
                if constexpr (NL > 2) {
                    // level 2: this K-group's partial counts of the parents (ukg >> 1, 0 / 1): K-slots (parent column, byte)
                    const unsigned cl = (ta & 0xffu) + (ta >> 16), cr = (tb & 0xffu) + (tb >> 16);
                    const long long a2 = nv_pack64((cl | (cr << 16)) << ush, 0u);
#pragma unroll
                    for (int nt = 0; nt < NV_UT; ++nt) {
                        const unsigned w = *reinterpret_cast<lds_cu32>(a_ub[2] + nt * 16 * NV_P2);
                        accu[2][nt] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a2, nv_pack64(w, 0u), accu[2][nt], 0, 0, 0);
                    }
                    if constexpr (NL > 3) {
                        const long long a3 = nv_pack64((cl + cr) << ush, 0u);   // level 3: the block's one parent
#pragma unroll
                        for (int nt = 0; nt < NV_UT; ++nt) {
                            const unsigned w = *reinterpret_cast<lds_cu16>(a_ub[3] + nt * 16 * NV_P3);
                            accu[3][nt] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a3, nv_pack64(w, 0u), accu[3][nt], 0, 0, 0);
                        }
                    }
                }
            }
        }
        {                                                        // next tile of this workgroup (see kmeans_pass_mfma_kernel)
            const int tn = reverse ? tin - s1 : tin + s1;
            const bool wrap = reverse ? tn < 0 : tn >= ntiles;
            const bool up = reverse == wrap;
            const int dq = wrap ? q2 : q1, dr = wrap ? r2 : r1;
            tin = wrap ? (reverse ? tn + ntiles : tn - ntiles) : tn;
            if (up) {
                bx += dr;
                by += dq;
                if (bx >= lo.bx_n) { bx -= lo.bx_n; ++by; }
            } else {
                bx -= dr;
                by -= dq;
                if (bx < 0) { bx += lo.bx_n; --by; }
            }
        }
        __syncthreads();
    }
    if (!do_acc) return;

    // ---- fold, every level at once: the whole LDS image is free now, so each wave parks all its accumulators ([wave][level][16 rows]
    //      [48 planes] ints; row 2 j + t = byte t of cluster j) and its voting pixel counts, two barriers, and the row is written in
    //      LOGICAL feature order (consecutive threads = consecutive 8-byte elements of the partial row). The first round-5 build folded
    //      level by level through the tile buffer: eight barriers and stores in physical plane order.
    constexpr int RW = NV_UT * 16;
    int *red = reinterpret_cast<int *>(s_mem);
    int *s_cnt = red + 4 * NL * 16 * RW;                          // [wave][K-group][row]
    static_assert((4 * NL * 16 * RW + 4 * 4 * 16) * 4 <= NJ_O, "fold scratch exceeds the LDS image in front of s_nj");
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
        for (int nt = 0; nt < NV_UT; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[((wave * NL + L) * 16 + 4 * ukg + e) * RW + 16 * nt + um] = accu[L][nt][e];
    s_cnt[(wave * 4 + ukg) * 16 + um] = cntacc;
    __syncthreads();
    if (tid < 8) {
        long long c = 0;
        for (int w = 0; w < 16; ++w) c += s_cnt[w * 16 + 2 * tid];
        s_nj[tid] = c;
    }
    __syncthreads();
    for (int i = tid; i < K * D1; i += 256) {
        const int j = i / D1, e = i - j * D1;                     // e = LOGICAL feature (or D = the count)
        const long long nj = s_nj[j];
        long long out = nj;
        if (e < D) {
            const int c = e / lo.F, f = e - c * lo.F;           // level and plane in its level of logical feature e (levels unrolled)
            int L = 0, pl = 0;
            { const int q = kp_plane_on_level<0>(lo, c, f); if (q >= 0) { L = 0; pl = q - lo.row0[0]; } }
            if (NL > 1) { const int q = kp_plane_on_level<1>(lo, c, f); if (q >= 0) { L = 1; pl = q - lo.row0[1]; } }
            if (NL > 2) { const int q = kp_plane_on_level<2>(lo, c, f); if (q >= 0) { L = 2; pl = q - lo.row0[2]; } }
            if (NL > 3) { const int q = kp_plane_on_level<3>(lo, c, f); if (q >= 0) { L = 3; pl = q - lo.row0[3]; } }
            long long flo = 0, fhi = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                flo += red[((w * NL + L) * 16 + 2 * j) * RW + pl];
                fhi += red[((w * NL + L) * 16 + 2 * j + 1) * RW + pl];
            }
            if (L == 0) {                                         // the one-hot digit is -128
                flo = -flo / 128;
                fhi = -fhi / 128;
            }
            out = (flo + 128 * nj) + 256 * (fhi + 128 * nj);
        }
        partials[prow(i)] = (uint64_t)out;
    }
}

// Working workgroups per image of the native pass: GCS_NV_MINB (three) 4-wave workgroups per CU are resident, so at most
// 256 * GCS_NV_MINB / B of the `parts` workgroups of an image work (the others only write zero rows) - but never so few that a
// wave's int32 MFMA accumulators can overflow: they are flushed only at the end of the pass, a voting pixel adds up to 128 * 128
// to one of them and a wave sees a quarter of its workgroup's pixels, so a workgroup may own at most 2^31 / 2^14 * 4 = 524 288
// pixels; the bound used is half of that. (`parts` itself keeps a workgroup below 65 536 pixels: gcs_kmeans_parts_per_image.)
constexpr long long NV_MAX_PX_PER_WORKGROUP = 262144;
static int native_parts_eff(int B, int parts, long long px_image, int minb = GCS_NV_MINB) {
    const int slots = 256 * minb;
    int eff = slots / B > 0 ? slots / B : 1;
    const long long need = (px_image + NV_MAX_PX_PER_WORKGROUP - 1) / NV_MAX_PX_PER_WORKGROUP;
    if (eff < need) eff = (int)need;
    return eff < parts ? eff : parts;
}
// Test hook (host only): the working workgroups per image the native pass would use, 0 for a bad shape.
extern "C" int gcs_selftest_native_parts(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || gcs_tiles_upper(H, W) > 0x3fffffffLL) return 0;
    return native_parts_eff(B, (int)gcs_kmeans_parts_per_image(B, H, W), gcs_tiles_upper(H, W) * KP_TP);
}

GcsPassKernel lloyd_native_kernel(const GcsLayout &lo) {
    bool native = lo.tile_bytes / 16 <= 256 * NV_NST && lo.n_levels >= 2;      // every level at most 48 planes: levels at own resolution
    for (int L = 0; L < lo.n_levels; ++L) native = native && lo.DL[L] <= NV_DL;
#ifdef GCS_KP_NO_NATIVE
    native = false;
#endif
    if (!native) return GCS_PASS_NONE;
    const bool full0 = lo.DL[0] == NV_DL;
    return lo.n_levels == 2   ? (full0 ? GCS_PASS_NATIVE_2_FULL : GCS_PASS_NATIVE_2)
           : lo.n_levels == 3 ? (full0 ? GCS_PASS_NATIVE_3_FULL : GCS_PASS_NATIVE_3)
                              : (full0 ? GCS_PASS_NATIVE_4_FULL : GCS_PASS_NATIVE_4);
}

template <int NL, int MINB, int N0>
static void launch_native(const LloydPassArgs &a, int nt_limit) {
    // MINB 4-wave workgroups per CU are resident: that many work, the others write zero partial rows
    const int parts_eff = native_parts_eff(a.B, a.parts, (long long)a.lo.ntiles * KP_TP, MINB);
    hipLaunchKernelGGL((kmeans_pass_native_kernel<NL, MINB, N0>), dim3(a.B, a.parts), dim3(256), 0, a.stream, a.feats, a.cent, a.lo,
                       a.k, a.n_sets == a.B ? 1 : 0, a.parts, parts_eff, a.reverse ? 1 : 0, a.row_lo, a.row_hi, a.partials, a.lab_out,
                       a.lab_u8, nt_limit);
}

void lloyd_native_launch(GcsPassKernel pk, const LloydPassArgs &a) {
    const int nt_limit = gcs_pass_nt_limit(pk, a.lo, a.B, a.n_sets);   // which tile loads carry the nontemporal hint (csrc/lloyd_pass.h)
    switch (pk) {
#define GCS_PASS_LAUNCH(id, name, ...) \
    case GCS_PASS_##id:                \
        return launch_native<__VA_ARGS__>(a, nt_limit);
        GCS_NATIVE_PASSES(GCS_PASS_LAUNCH)
#undef GCS_PASS_LAUNCH
    default: return;
    }
}
