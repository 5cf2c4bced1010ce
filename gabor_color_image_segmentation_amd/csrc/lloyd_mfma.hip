// lloyd_mfma.hip — the matrix-core Lloyd pass of SPEC.md §4 (csrc/lloyd_pass.h: which banks take which instantiation).
//   kmeans_pass_mfma_kernel  one Lloyd pass (assign + update) on the matrix cores for D <= 207; a stream of the
//                            slab, which keeps pyramid level L at 1/4^L of the pixels: a tile's coarse planes are
//                            replicated over their 2^L x 2^L blocks while they are staged into LDS. 4x6-style banks
//                            (at most two levels, D <= 79) read the SPLIT slab: 12 of the 16 bits of every value, the
//                            last 4 for flagged tiles only (template flag SPLIT); with k <= 8 their level 1 stays COMPACT
//                            in LDS (CL1: block rows held as even | odd pixels, no replication). The CL1 kernels also exist as
//                            SELF-UPDATING passes (template flag FUSED, entry gcs_kmeans_pass_fused): the single-rank loop is then
//                            n_iter launches of this kernel and nothing else - no init, no reduce.
// Label maps leave the pass in RASTER order ([B][H][W] uint8 or int32): which slot of which block holds a pixel
// (csrc/common.h: main blocks and packed edge strips) is the pass's own business.
// Nothing here allocates, frees or synchronises; the launcher enqueues on the caller's stream.
#include "lloyd_pass.h"

// ---------------------------------------------------------------------------------------
// One Lloyd pass on the matrix cores (D <= 207: 80-row LDS tile for D <= 79, 208-row tile above).
// Per 256-pixel tile (four 8x8 blocks, one per wave), staged ONCE in LDS as D rows of 256 u16 (each byte offset by
// -128 so it is a signed MFMA digit; rows in PHYSICAL plane order, coarse levels replicated to full resolution):
//   assign:  scores[(j,pat)][px] = A_pat[(j,pat)][k] * X[k][px] on v_mfma_i32_32x32x32_i8, k =
//            (plane, byte). Patterns per cluster j: LL = cl*xl, M = ch*xl + cl*xh, HH = ch*xh, so
//            sum_d x_d c_jd = LL + 256 M + 65536 HH exactly (int32 partials, int64 combine);
//            argmin_j |c_j|^2 - 2 sum_d x_d c_jd, ties -> lowest j (SPEC.md §4).
//   update:  sums[j][byte-plane] = onehot[j][px] * X[px][byte-plane] on v_mfma_i32_16x16x64_i8;
//            one spare byte-plane is all ones and yields the counts. Accumulators live in
//            registers for the whole workgroup; nothing but the tile load touches HBM.
// The one-hot digit is 0x80 (= -128) to save a shift; it is divided out exactly at the end.

#ifndef GCS_KP_WAVES
#define GCS_KP_WAVES 3
#endif
// Ablation builds of kmeans_pass_mfma_kernel for same-box A/B runs (tools/build_variant.sh x -DGCS_ABL=n, tools/ab.py; results are
// WRONG by construction): bit 0 = no assign phase, bit 1 = no update phase, bit 2 = the split slab's items go to LDS as loaded (no unpack).
#ifndef GCS_ABL
#define GCS_ABL 0
#endif
// DSTEPS = assign K-steps (16 planes = 32 byte-features each); LDS holds ROWS = 16*DSTEPS plane rows (>= D + 1:
// the spare row D is the count row); the update has NT = 2*DSTEPS N-tiles (8 planes = 16 byte-planes each).
// NST = 16-byte staging chunks per thread >= ceil(tile_bytes / 4096); surplus chunks re-copy the tile's last chunk.
// WAVES = 4 (narrow pass: wave w owns block w of the tile) or 8 (wide pass: 131 KB of LDS allow one workgroup per CU, so
// it brings 8 waves: wave w works on block w & 3; in the assign phase it takes the block's 32-pixel half w >> 2, in the
// update phase all 64 pixels for half of the plane tiles -> half the accumulators, twice the waves to hide latency).
// -DGCS_KP_PHASES (debugging aid, tools/dbg/pass_phases.py): every wave of kmeans_pass_mfma_kernel adds up, over its tile loop,
// the shader-clock cycles it spends in each phase of a tile (s_memtime around: staging writes | first barrier | next tile's loads
// | assign | update | second barrier) and stores the six sums behind the loop. Costs ~10 % of the wave's cycles; never in the product.
#ifdef GCS_KP_PHASES
__device__ unsigned long long g_kp_phases[1024 * 4 * 8];
extern "C" int gcs_debug_kp_phases(unsigned long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kp_phases), sizeof(unsigned long long) * 1024 * 4 * 8);
}
#define KP_PHASE_DECL unsigned long long kp_ph[6] = {0, 0, 0, 0, 0, 0}, kp_t0 = __builtin_amdgcn_s_memtime(), kp_tiles = 0
#define KP_PHASE(k)                                                   \
    do {                                                              \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();   \
        kp_ph[k] += t_ - kp_t0;                                       \
        kp_t0 = t_;                                                   \
    } while (0)
#define KP_PHASE_STORE                                                                                           \
    do {                                                                                                         \
        const int wg_ = (int)(blockIdx.y * gridDim.x + blockIdx.x);                                              \
        if (lane == 0 && wg_ < 1024) {                                                                           \
            for (int k_ = 0; k_ < 6; ++k_) g_kp_phases[(wg_ * 4 + (wid & 3)) * 8 + k_] = kp_ph[k_];             \
            g_kp_phases[(wg_ * 4 + (wid & 3)) * 8 + 6] = kp_tiles;                                               \
        }                                                                                                        \
    } while (0)
#else
#define KP_PHASE_DECL
#define KP_PHASE(k)
#define KP_PHASE_STORE
#endif

// L0T (CL1 kernel only): plane tiles (16 rows) known to lie wholly inside level 0 - the launcher passes 2 for banks whose level 0 has 32
// planes or more (the 4x6 bank: 36), else 0: see the update's operand reads.
// SPLIT (round 6): the split slab of csrc/common.h (narrow pass only). NST then counts staging ROUNDS: an ITEM = 16 consecutive slots of a
// tile = 16 low bytes + 8 bytes of MID nibbles (+ 8 bytes of TOP nibbles when the tile's flag word says that one of them is set),
// unpacked into the same LDS image as the wide slab's: 16 pixels of a level-0 plane row, or the 4 x 4 parents of one block of a
// level-1 plane, replicated over the block's 64 pixels.
// FUSED (round 7, the CL1 kernels only): the self-updating pass of gcs_kmeans_pass_fused (GcsFold, csrc/common.h). The prologue makes
// the centroids itself - the SPEC.md §4 init pixels on pass 0, else the fold of the previous pass's shared rows and the §4 update -,
// the epilogue adds the workgroup's sums into a shared row with vector atomics instead of storing a private row, and every
// workgroup clears its slice of the buffer the NEXT pass adds into. `cent` = the previous pass's centroids (an empty cluster keeps
// its own), `partials` = row 0 of the buffer this pass adds into (NULL on the last pass). A compile-time mode: the other
// instantiations never look at `fz`.
template <int KT, int NST, int DSTEPS, int WAVES, bool SPLIT = false, int L0T = 0, bool FUSED = false>
__global__ __launch_bounds__(64 * WAVES, (WAVES == 8 ? 2
                                          : DSTEPS == KP_DSTEPS_NARROW && KT == 1 && NST <= (SPLIT ? 3 : 6) ? GCS_KP_WAVES
                                          : DSTEPS == KP_DSTEPS_NARROW ? 2 : 1)) void kmeans_pass_mfma_kernel(
    const unsigned char *__restrict__ feats, const uint16_t *__restrict__ cent, GcsLayout lo, int K, int per_image,
    int parts, int reverse, int row_lo, int row_hi, uint64_t *__restrict__ partials, void *__restrict__ raster,
    int raster_u8, int nt_flag, GcsFold fz) {          // (nt_flag: the split slab's nt_limit, see lloyd_pass; unused by the wide kernels)
    constexpr int KP_ROWS = 16 * DSTEPS, KP_DSTEPS = DSTEPS, KP_NT = 2 * DSTEPS;
    constexpr int NTHR = 64 * WAVES;                         // threads per workgroup
    constexpr int NT_OWN = WAVES == 8 ? (KP_NT + 1) / 2 : KP_NT;   // update plane tiles a wave accumulates
    // compact copy of pyramid levels >= 2 of one tile (level 1 is replicated straight from the staging registers):
    // at most (D / 2) * 32 bytes plus 16-byte padding per level; sized for the worst case of the bucket
    constexpr int KP_COARSE = DSTEPS == KP_DSTEPS_NARROW ? 40 * 32 + 64 : 104 * 32 + 64;
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[KP_ROWS * KP_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char s_coarse[KP_COARSE];
    __shared__ __attribute__((aligned(16))) unsigned char s_lab[KP_TP];
    __shared__ long long s_const[16];
    constexpr int KP_FLAGS = 320;                            // tiles of one workgroup whose flag is kept (more: read as set, always exact)
    __shared__ unsigned char s_flag[SPLIT ? KP_FLAGS : 4];
    static_assert(!SPLIT || (DSTEPS == KP_DSTEPS_NARROW && WAVES == 4), "the split slab is the narrow pass's");
    static_assert(!FUSED || (SPLIT && KT == 1), "the self-updating pass exists for the CL1 kernels");

    // either output may be absent (host contract): raster == NULL on the passes whose assignment nobody reads (every
    // pass but the last), partials == NULL on the last pass, whose sums nobody reads (no update phase, no fold)
    const bool do_acc = partials != nullptr;                 // (raster: see the assign phase)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = tid >> 6;                                // 0 .. WAVES-1
    const int wave = wid & 3;                                // the block of the tile this wave works on
    const int half = wid >> 2;                               // WAVES == 8: which half of the assign / update work
    const int b = blockIdx.y, part = blockIdx.x;
    const int D = lo.D;
    const uint16_t *cset = cent + (size_t)(per_image ? b : 0) * K * D;
    const int ntiles = lo.ntiles;
    // The tile list this workgroup strides through. Per-image codebooks: the tiles of image b, stride `parts`. One
    // global codebook: the tiles of the WHOLE batch as one list, stride B * parts: at any moment the resident workgroups
    // then read one contiguous window of the slab (B * parts tiles, 17 MB) instead of B separate ones, which is what
    // HBM's channel / bank interleave is built for (same box: pass 0.190 -> 0.175 ms; profiles/r2_notes.md).
    const int nimg = per_image ? 1 : (int)gridDim.y;
    const int G = parts * nimg, g = per_image ? part : b * parts + part;
    const int nlist = ntiles * nimg;
    const unsigned char *fb = feats + (size_t)(per_image ? b : 0) * lo.img_bytes;   // first image of the list (wide: each tile one contiguous run)

    // ---- centroids -> LDS scratch (borrowed from the tile buffer): [8*KT clusters][KP_ROWS planes] u16 in PHYSICAL
    //      plane order, stored offset-binary (c ^ 0x8080: low byte = digit cl, high byte = digit ch), zero outside K x D.
    uint16_t *cs = reinterpret_cast<uint16_t *>(s_tile);
    if constexpr (FUSED) {
        const int D1 = D + 1, row_len = K * D1;
        const int set = per_image ? b : 0;
        const int wg = b * (int)gridDim.x + part, nwg = (int)(gridDim.x * gridDim.y);
        {   // this workgroup's slice of the buffer the next pass adds into
            const long long total = (long long)(per_image ? (int)gridDim.y : 1) * fz.rows * row_len;
            for (long long i = (long long)wg * NTHR + tid; i < total; i += (long long)nwg * NTHR) fz.clear[i] = 0ull;
        }
        // the set's sums of the previous pass: its shared rows folded, in the tile buffer behind the centroid scratch
        unsigned long long *fsum = reinterpret_cast<unsigned long long *>(s_tile + 8 * KT * KP_ROWS * 2);
        static_assert(8 * KT * KP_ROWS * 2 % 16 == 0 && 8 * KT * KP_ROWS * 2 + 8 * (8 * KT * KP_ROWS) <= KP_ROWS * KP_PITCH,
                      "the folded sums do not fit behind the centroid scratch");
        const bool later = fz.prev != nullptr;
        if (later) {
            const unsigned long long *pv = fz.prev + (size_t)set * fz.rows * row_len;
            for (int i = tid; i < row_len; i += NTHR) {
                unsigned long long s = 0;
                for (int r = 0; r < fz.rows; ++r) s += pv[(size_t)r * row_len + i];
                fsum[i] = s;
            }
            __syncthreads();
        }
        const bool writer = part == 0 && (per_image || b == 0);          // one workgroup per set publishes the centroids
        const long long P = (long long)lo.H * lo.W;
        for (int i = tid; i < 8 * KT * KP_ROWS; i += NTHR) {
            const int j = i / KP_ROWS, r = i % KP_ROWS;
            int e = 0;                                               // logical feature of physical plane r (kp_logical_of: levels unrolled)
            if (r >= lo.row0[0] && r < lo.row0[0] + lo.DL[0]) e = kp_logical_of<0>(lo, r - lo.row0[0]);
            if (lo.n_levels > 1 && r >= lo.row0[1] && r < lo.row0[1] + lo.DL[1]) e = kp_logical_of<1>(lo, r - lo.row0[1]);
            unsigned v = 0;
            if (j < K && r < D) {
                if (later) {
                    const unsigned long long c = fsum[j * D1 + D], s = fsum[j * D1 + e];
                    v = c > 0 ? (unsigned)((2 * s + c) / (2 * c)) : (unsigned)cset[j * D + e];
                } else {
                    const long long p = ((2LL * j + 1) * P) / (2LL * K);
                    v = gcs_slab_value(feats, lo, set, r, (int)(p / lo.W), (int)(p % lo.W));
                }
                if (writer) {
                    fz.cent_new[((size_t)set * K + j) * D + e] = (uint16_t)v;
                    fz.cent_out[((size_t)set * K + j) * D + e] = (uint16_t)v;
                }
                v ^= 0x8080u;
            }
            cs[i] = (uint16_t)v;
        }
    } else
    for (int i = tid; i < 8 * KT * KP_ROWS; i += NTHR) {
        const int j = i / KP_ROWS, r = i % KP_ROWS;
        int e = 0;                                               // logical feature of physical plane r (kp_logical_of: levels unrolled)
        if (r >= lo.row0[0] && r < lo.row0[0] + lo.DL[0]) e = kp_logical_of<0>(lo, r - lo.row0[0]);
        if (lo.n_levels > 1 && r >= lo.row0[1] && r < lo.row0[1] + lo.DL[1]) e = kp_logical_of<1>(lo, r - lo.row0[1]);
        if (lo.n_levels > 2 && r >= lo.row0[2] && r < lo.row0[2] + lo.DL[2]) e = kp_logical_of<2>(lo, r - lo.row0[2]);
        if (lo.n_levels > 3 && r >= lo.row0[3] && r < lo.row0[3] + lo.DL[3]) e = kp_logical_of<3>(lo, r - lo.row0[3]);
        cs[i] = (j < K && r < D) ? (uint16_t)(cset[j * D + e] ^ 0x8080u) : (uint16_t)0;
    }
    if constexpr (SPLIT) {
        // the flag words of this workgroup's tiles (csrc/common.h): is any TOP nibble of the tile non-zero?
        for (int it = tid; it < KP_FLAGS; it += NTHR) {
            const long long lt = (long long)g + (long long)it * G;
            unsigned char f = 0;
            if (lt < nlist) {
                const int T = reverse ? nlist - 1 - (int)lt : (int)lt;
                const int bi = T / ntiles, tn = T - bi * ntiles;
                f = *reinterpret_cast<const unsigned *>(fb + (size_t)bi * lo.img_bytes + lo.flag_off + 4 * (size_t)tn) != 0u;
            }
            s_flag[it] = f;
        }
    }
    __syncthreads();
    // ---- per-cluster key base (exact int64): 16 * (|c|^2 - 2*(offset terms of the -128 digits)) + j.
    //      key_j = base_j - 32 R0 - 8192 R1 - 2^21 R2 = 16 * score_j + j, so ONE 64-bit minimum yields the
    //      best score and the lowest index on ties. 16 lanes per cluster, folded with lane shuffles.
    {
      for (int j = tid >> 4; j < 16; j += NTHR / 16) {
        const int sub = tid & 15;
        long long nrm = 0, scl = 0, sch = 0;
        if (j < K)
            for (int d = sub; d < D; d += 16) {
                const long long c = cs[j * KP_ROWS + d] ^ 0x8080u;
                nrm += c * c;
                scl += c & 255;
                sch += c >> 8;
            }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            nrm += __shfl_xor(nrm, m);
            scl += __shfl_xor(scl, m);
            sch += __shfl_xor(sch, m);
        }
        if (sub == 0) {
            const long long q = 16384LL * D;
            const long long g = (128 * scl - q) + 256 * (128 * (sch + scl) - 2 * q) + 65536 * (128 * sch - q);
            s_const[j] = j < K ? 16 * (nrm - 2 * g) + j : (1LL << 62) + j;
        }
      }
    }
    // ---- assign A fragments: row r = 4*jj + pat of tile mt (cluster j = 8*mt + jj);
    //      k-slot (h, t) of K-step kk = (plane 16*kk + 8*h + t/2, byte t&1): the 8 planes of a fragment are one
    //      16-byte scratch read. Per plane (u16 w = digits cl | ch << 8) the pattern bytes (byte 0, byte 1) are
    //      LL = (cl, 0) = w & 0x00ff, M = (ch, cl) = bytes swapped, HH = (0, ch) = w & 0xff00, row 3 = 0.
    v4i apat[KT][KP_DSTEPS];
    {
        const int r = lane & 31, h = lane >> 5;
        const int jj = r >> 2, pat = r & 3;
        const unsigned msk = pat == 0 ? 0x00ff00ffu : pat == 1 ? 0xffffffffu : pat == 2 ? 0xff00ff00u : 0u;
        const unsigned sel = pat == 1 ? 0x02030001u : 0x03020100u;
#pragma unroll
        for (int mt = 0; mt < KT; ++mt)
#pragma unroll
            for (int kk = 0; kk < KP_DSTEPS; ++kk) {
                const v4i w = *reinterpret_cast<const v4i *>(&cs[(8 * mt + jj) * KP_ROWS + 16 * kk + 8 * h]);
                v4i f;
#pragma unroll
                for (int e = 0; e < 4; ++e) f[e] = (int)(__builtin_amdgcn_perm(0u, (unsigned)w[e], sel) & msk);
                apat[mt][kk] = f;
            }
    }
    __syncthreads();                                   // scratch reads done: the tile buffer is free again
    // the count row (plane D): byte-planes 2D, 2D+1 read as +1 for every pixel of every tile
    // CL1 (round 6, the split narrow pass with k <= 8): level 1 stays COMPACT in LDS - a plane row of level 1 (and every row behind it:
    // the count row, the padding) is 64 parents in (parent row, block, parent column) order at pitch KP_P1, NOT the 2 x 2 replication
    // to 256 pixels: a level-1 item then costs what a level-0 item costs (14 instead of 30 VALU instructions, 2 instead of 8
    // ds_write_b128: the replication was half of a tile's LDS write traffic and made three of the four waves' staging 45 % longer than
    // the fourth's). What makes it possible: the pixels of a block row lie in LDS as (x0 x2 x4 x6 | x1 x3 x5 x7), which is also the
    // column order of the assign MFMA and the K order of the update MFMA. The four consecutive elements a lane's address hands to
    // ds_read_b64_tr_b16 are then four pixels with four DIFFERENT consecutive parents - the parent row itself, read by the lanes of the
    // even pixels, of the odd pixels and of both fine rows alike -, and the 16 bytes = 8 pixels of an update operand are the parent
    // row twice (the same 8 bytes read into both halves of the operand).
    constexpr bool CL1 = SPLIT && KT == 1;
    const int DL0 = lo.DL[0];
    auto row_addr = [&](int r) -> int {                     // byte offset of plane row r in s_tile (CL1: rows >= DL0 are compact)
        return CL1 && r >= DL0 ? DL0 * KP_PITCH + (r - DL0) * KP_P1 : r * KP_PITCH;
    };
    // CL1: the 16-byte chunks of a full row r are swizzled by (r >> 3 & 1) * 32 bytes (chunk bit 1): the update's operand reads take
    // 8 bytes per lane from 16 consecutive rows, and rows r, r + 4, r + 8, r + 12 start on the same banks (the pitch is 16 dwords
    // modulo 64: what the transposed reads want) - four addresses per bank without the swizzle, two with it (tools/design/
    // lds_bank_model.py rules; SQ_LDS_BANK_CONFLICT). The transposed reads (4 consecutive rows of one aligned group of 8) and the staging
    // writes (8 lanes = one row) see a uniform shift.
    auto row_swz = [&](int r) -> int { return CL1 && r < DL0 ? ((r >> 3) & 1) * 32 : 0; };
    if (tid < (CL1 ? 32 : KP_TP / 2)) reinterpret_cast<unsigned *>(&s_tile[row_addr(D)])[tid] = 0x01010101u;   // (a compact row: 64 parents)
    // UPD2 (round 6, the split narrow pass with k <= 8): the update's MFMA rows are (cluster j, byte b), its K slots (pixel, byte) and
    // its columns 16 PLANES - sums[(j, b)][plane] = sel[(j, b)][(px, t)] * X[(px, t)][plane] with sel = the one-hot digit where t == b -,
    // so that the B operand is a plane row AS IT LIES in LDS (8 pixels x (lo, hi) = one 16-byte read, no byte de-interleave: 40 v_perm
    // per tile and wave less) and 80 plane rows are 5 accumulator tiles instead of 10 (the deep-bank pass's form, kmeans_pass_native_kernel).
    constexpr bool UPD2 = SPLIT && KT == 1;
    constexpr int NACC = UPD2 ? DSTEPS : NT_OWN;
    v4i accu[NACC];
#pragma unroll
    for (int nt = 0; nt < NACC; ++nt) accu[nt] = v4i{0, 0, 0, 0};

    // ---- staging (wide slab; the split slab's items: stage_load_split and the SPLIT branch of stage_write below): the tile is ONE
    //      contiguous run of tile_bytes (csrc/common.h), already offset-binary. Chunk
    //      ci = tid + 256*i is 16 bytes at byte 16*ci:
    //        level-0 chunks (the first 32*D_0) are 8 pixels of plane row ci>>5: copied as they are;
    //        level-1 chunks (the next 8*D_1) are 2 rows x 4 pixels of one block's 4x4 parents: each row is replicated
    //          into two fine rows of 8 pixels, i.e. 64 contiguous bytes of the plane row, straight from the registers
    //          (SPEC.md §3: feat[y][x] = g_L[y >> L][x >> L]);
    //        the rest (levels >= 2: deep banks only) goes to s_coarse untouched and is replicated by expand_deep().
    //      Loads and LDS writes are UNCONDITIONAL per wave: a per-chunk guard makes hipcc branch around every
    //      load / write with exec masking and drain vmcnt(0) before each write. Chunks beyond the tile
    //      are clamped to its last chunk: they re-read and re-write it with its own data.
    const int n0 = SPLIT ? 16 * lo.DL[0] : 32 * lo.DL[0];   // level-0 chunks (split slab: level-0 items)
    const int n1 = lo.n_levels > 1 ? 8 * lo.DL[1] : 0; // level-1 chunks
    const int nchunk = SPLIT ? lo.S >> 4 : lo.tile_bytes >> 4;   // (split slab: items per tile)
    v4i st[NST];
    v2i sm[NST], stt[NST];                             // split slab: MID and TOP nibbles of the item
#pragma unroll
    for (int i = 0; i < NST; ++i) stt[i] = v2i{0, 0};
    int sdst[NST], ssrc[NST];
    int scls[NST];                                     // wave-uniform: 0 = every lane copies, 1 = every lane replicates, 2 = mixed
    bool sl1[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const int ci = min(tid + NTHR * i, nchunk - 1);
        ssrc[i] = ci;
        const int c1 = ci - n0;
        const bool l1 = SPLIT ? c1 >= 0 : c1 >= 0 && c1 < n1;
        sl1[i] = l1;
        if constexpr (SPLIT)
            // slots of a plane come in (row, block, column) order (csrc/common.h). Level-0 item: row (ci & 15) >> 1 of blocks
            // 2 (ci & 1), 2 (ci & 1) + 1 of plane ci >> 4: two 16-byte pieces 128 bytes apart. Level-1 item: parent row c1 & 3 of
            // the four blocks of plane c1 >> 2: per block 4 parents = fine rows 2 p, 2 p + 1 = 32 bytes at q * 128 + 32 p.
            // (CL1: the item is parent row c1 & 3 of the plane's compact row - 16 parents = 32 bytes, blocks 0, 1 | blocks 2, 3)
            sdst[i] = l1 ? (CL1 ? (int)(size_t)&s_tile[row_addr(lo.row0[1] + (c1 >> 2)) + (c1 & 3) * 32]
                                : (int)(size_t)&s_tile[(lo.row0[1] + (c1 >> 2)) * KP_PITCH + (c1 & 3) * 32])
                         : (int)(size_t)&s_tile[(ci >> 4) * KP_PITCH + (((ci & 1) * 256 + ((ci & 15) >> 1) * 16) ^ row_swz(ci >> 4))];
        else
            sdst[i] = ci < n0 ? (int)(size_t)&s_tile[(ci >> 5) * KP_PITCH + (ci & 31) * 16]
                      : l1    ? (int)(size_t)&s_tile[(lo.row0[1] + (c1 >> 3)) * KP_PITCH + (c1 & 7) * 64]
                              : (int)(size_t)&s_coarse[(c1 - n1) * 16];
        const unsigned long long m = __builtin_amdgcn_ballot_w64(l1);
        scls[i] = m == 0ull ? 0 : m == ~0ull ? 1 : 2;
    }
    auto stage_load = [&](int tile) {
        const v4i *src = reinterpret_cast<const v4i *>(fb + (size_t)tile * lo.tile_bytes);
#pragma unroll
        for (int i = 0; i < NST; ++i) st[i] = src[ssrc[i]];
    };
    // split slab: the tile whose LO run starts at p_lo and whose MID run at p_mid (uniform pointers; 32-bit lane offsets: the loads
    // take an SGPR base and need no vector address arithmetic); the TOP run only when the tile's flag word is set
    // Raw buffer loads (one descriptor over the tile's LO run; the MID and TOP runs at scalar offsets from it): the cache policy is an
    // IMMEDIATE of the intrinsic, so the two forms - plain, and `nt` for the part of the sweep that no later pass finds in the Infinity
    // Cache (see lloyd_pass) - are different instructions. Written as `nt ? __builtin_nontemporal_load(p) : *p`, or as two branches
    // around global loads, hipcc merges them into ONE plain load: until round 6 not a single `nt` load was left in the pass kernels
    // (ISA). The address is SGPR descriptor + 32-bit lane offset + SGPR offset: no vector address arithmetic (hipcc built 64-bit lane
    // addresses for the global loads: a v_lshl_add_u64 per load and 18 VGPRs of offsets).
    auto stage_load_split = [&](const unsigned char *p_lo, unsigned mid_rel, bool top, bool nt) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(p_lo), 0, -1, 0x00020000);
        const unsigned top_rel = mid_rel + (unsigned)(lo.top_off - lo.mid_off);
        auto go = [&](auto aux_c) {
            constexpr int AUX = decltype(aux_c)::value;          // gfx940+: bit 1 = nt
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const unsigned o = (unsigned)ssrc[i] * 16u;
                st[i] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)o, 0, AUX));
                sm[i] = __builtin_bit_cast(v2i, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(o >> 1), (int)mid_rel, AUX));
            }
            if (top) {
#pragma unroll
                for (int i = 0; i < NST; ++i)
                    stt[i] = __builtin_bit_cast(v2i, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)((unsigned)ssrc[i] * 8u), (int)top_rel, AUX));
            } else {
                // no TOP run: stage_write's unpack does not read stt then. The registers are given a fresh (undefined) value so that
                // no old value lives through this path: with one, hipcc merged the paths through copies of the registers just
                // loaded - behind s_waitcnt vmcnt(0), i.e. every tile waited for its successor's loads at once (ISA, round 6)
#pragma unroll
                for (int i = 0; i < NST; ++i) {
                    v2i u;
                    asm("" : "=v"(u));
                    stt[i] = u;
                }
            }
        };
        if (nt) go(std::integral_constant<int, 2>{});
        else go(std::integral_constant<int, 0>{});
    };
    typedef __attribute__((address_space(3))) v4i *lds_v4i_ptr;
    // (wide slab) a level-1 chunk of the LDS image: coarse row 0 = pixels (v0.lo, v0.hi, v1.lo, v1.hi), row 1 = (v2.., v3..): each
    // pixel twice, each row into two fine rows = four 16-byte pieces of a 64-byte region. Lanes are 64 bytes apart, so piece k
    // of lanes l and l+2 would share banks (4-way conflicts: SQ_LDS_BANK_CONFLICT 0.4 M -> 17.7 M cycles per launch when every
    // lane wrote its pieces in the same order). Lanes therefore start on different pieces: bit 2 of the lane picks which coarse
    // row goes first, bit 1 which of its two pieces; the eight lanes of a ds_write_b128 group then cover 32 distinct banks.
    // split slab: the high bytes (XOR 0x80) of the first and the second half of a nibble group from its MID and TOP dwords
    // (`top_regs`: the tile in the staging registers brought its TOP nibbles - uniform; without them three instructions do)
    bool top_regs = false;
    // (TOPP: a compile-time copy of top_regs - ONE branch per tile around two forms of stage_write; tested inside split_hi it
    //  became four scalar branches per nibble group)
    auto stage_write_as = [&](auto topp) {
    constexpr bool TOPP = decltype(topp)::value;
    auto split_hi = [&](unsigned mid, unsigned top, unsigned &e, unsigned &o) {
        if constexpr (TOPP) {
            e = ((mid & 0x0f0f0f0fu) | ((top << 4) & 0xf0f0f0f0u)) ^ 0x80808080u;
            o = (((mid >> 4) & 0x0f0f0f0fu) | (top & 0xf0f0f0f0u)) ^ 0x80808080u;
        } else {
            e = (mid & 0x0f0f0f0fu) | 0x80808080u;
            o = ((mid >> 4) & 0x0f0f0f0fu) | 0x80808080u;
        }
    };
    {
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const v4i v = st[i];
            if constexpr (SPLIT) {
                const v2i m = sm[i], t = stt[i];
                auto level0 = [&]() {
                    // two groups of 8 pixels (the row of two neighbouring blocks): low bytes (a, b), high bytes e (pixels 0..3)
                    // and o (pixels 4..7) -> u16 pairs
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        unsigned e, o;
                        split_hi((unsigned)m[g], (unsigned)t[g], e, o);
                        const unsigned a = (unsigned)v[2 * g], bb = (unsigned)v[2 * g + 1];
                        v4i w;
                        if constexpr (CL1) {                                    // (x0 x2 | x4 x6 | x1 x3 | x5 x7)
                            w[0] = (int)__builtin_amdgcn_perm(e, a, 0x06020400u);
                            w[1] = (int)__builtin_amdgcn_perm(o, bb, 0x06020400u);
                            w[2] = (int)__builtin_amdgcn_perm(e, a, 0x07030501u);
                            w[3] = (int)__builtin_amdgcn_perm(o, bb, 0x07030501u);
                        } else {
                            w[0] = (int)__builtin_amdgcn_perm(e, a, 0x05010400u);
                            w[1] = (int)__builtin_amdgcn_perm(e, a, 0x07030602u);
                            w[2] = (int)__builtin_amdgcn_perm(o, bb, 0x05010400u);
                            w[3] = (int)__builtin_amdgcn_perm(o, bb, 0x07030602u);
                        }
                        *reinterpret_cast<lds_v4i_ptr>(sdst[i] + 128 * g) = w;
                    }
                };
                auto level1 = [&]() {
                    // one parent row of the tile's four blocks: block q's four parents are v[q] (low bytes) and two bytes of m / t
                    // (a nibble group = one parent row of one block); every parent twice, into the fine rows 2 p and 2 p + 1.
                    // Eight consecutive lanes are the four parent rows of two planes (576 bytes apart = 64 modulo 128): the
                    // odd plane's lanes write their two identical pieces in the other order, so that a ds_write_b128 group
                    // covers eight distinct 16-byte columns.
                    const int e16 = ((lane >> 2) & 1) * 16;
                    if constexpr (CL1) {
                        // compact: the four parents of a block as they come - two blocks = one 16-byte store, no replication
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            unsigned e, o;                               // e = (A p0, A p1, B p0, B p1), o = (A p2, A p3, B p2, B p3)
                            split_hi((unsigned)m[j], (unsigned)t[j], e, o);
                            const unsigned a0 = (unsigned)v[2 * j], a1 = (unsigned)v[2 * j + 1];
                            v4i w;
                            w[0] = (int)__builtin_amdgcn_perm(e, a0, 0x05010400u);   // A: parents 0, 1
                            w[1] = (int)__builtin_amdgcn_perm(o, a0, 0x05030402u);   //    parents 2, 3
                            w[2] = (int)__builtin_amdgcn_perm(e, a1, 0x07010600u);   // B
                            w[3] = (int)__builtin_amdgcn_perm(o, a1, 0x07030602u);
                            *reinterpret_cast<lds_v4i_ptr>(sdst[i] + 16 * j) = w;
                        }
                        return;
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        unsigned e, o;                                   // e = (A p0, A p1, B p0, B p1), o = (A p2, A p3, B p2, B p3)
                        split_hi((unsigned)m[j], (unsigned)t[j], e, o);
#pragma unroll
                        for (int qq = 0; qq < 2; ++qq) {
                            const unsigned a = (unsigned)v[2 * j + qq];
                            const unsigned w0 = __builtin_amdgcn_perm(e, a, qq ? 0x07010600u : 0x05010400u);   // parents 0, 1
                            const unsigned w1 = __builtin_amdgcn_perm(o, a, qq ? 0x07030602u : 0x05030402u);   // parents 2, 3
                            v4i w;
                            w[0] = (int)__builtin_amdgcn_perm(0u, w0, 0x01000100u);
                            w[1] = (int)__builtin_amdgcn_perm(0u, w0, 0x03020302u);
                            w[2] = (int)__builtin_amdgcn_perm(0u, w1, 0x01000100u);
                            w[3] = (int)__builtin_amdgcn_perm(0u, w1, 0x03020302u);
                            const int d = sdst[i] + 128 * (2 * j + qq);
                            *reinterpret_cast<lds_v4i_ptr>(d + e16) = w;
                            *reinterpret_cast<lds_v4i_ptr>(d + 16 - e16) = w;
                        }
                    }
                };
                if (GCS_ABL & 4) {
                    *reinterpret_cast<lds_v4i_ptr>(sdst[i]) = v;
                    *reinterpret_cast<lds_v4i_ptr>(sdst[i] + 128) = v4i{m[0], m[1], t[0], t[1]};
                } else
                if (scls[i] == 0) level0();
                else if (scls[i] == 1) level1();
                else if (sl1[i]) level1();
                else level0();
            } else if (scls[i] == 0) {
                *reinterpret_cast<lds_v4i_ptr>(sdst[i]) = v;
            } else {
                // (the wide slab's level-1 chunk, in the code shape the wide kernels' register allocation was tuned with)
                const bool f = (lane >> 2) & 1;
                const unsigned x0 = f ? (unsigned)v[2] : (unsigned)v[0], x1 = f ? (unsigned)v[3] : (unsigned)v[1];
                const unsigned y0 = f ? (unsigned)v[0] : (unsigned)v[2], y1 = f ? (unsigned)v[1] : (unsigned)v[3];
                v4i ra, rb;
                ra[0] = (int)__builtin_amdgcn_perm(0u, x0, 0x01000100u);
                ra[1] = (int)__builtin_amdgcn_perm(0u, x0, 0x03020302u);
                ra[2] = (int)__builtin_amdgcn_perm(0u, x1, 0x01000100u);
                ra[3] = (int)__builtin_amdgcn_perm(0u, x1, 0x03020302u);
                rb[0] = (int)__builtin_amdgcn_perm(0u, y0, 0x01000100u);
                rb[1] = (int)__builtin_amdgcn_perm(0u, y0, 0x03020302u);
                rb[2] = (int)__builtin_amdgcn_perm(0u, y1, 0x01000100u);
                rb[3] = (int)__builtin_amdgcn_perm(0u, y1, 0x03020302u);
                if (scls[i] == 1 || sl1[i]) {
                    const int e16 = ((lane >> 1) & 1) * 16, f32 = f ? 32 : 0;
                    *reinterpret_cast<lds_v4i_ptr>(sdst[i] + f32 + e16) = ra;
                    *reinterpret_cast<lds_v4i_ptr>(sdst[i] + f32 + 16 - e16) = ra;
                    *reinterpret_cast<lds_v4i_ptr>(sdst[i] + 32 - f32 + e16) = rb;
                    *reinterpret_cast<lds_v4i_ptr>(sdst[i] + 32 - f32 + 16 - e16) = rb;
                } else {                                  // a lane of a mixed wave whose chunk is not level 1
                    *reinterpret_cast<lds_v4i_ptr>(sdst[i]) = v;
                }
            }
        }
    }
    };
    auto stage_write = [&]() {
        if (SPLIT && top_regs) stage_write_as(std::true_type{});
        else stage_write_as(std::false_type{});
    };
    // Levels >= 2 (deep banks): every group of 8 consecutive pixels of a plane row (one row of one 8x8 block) is the
    // replication of 8 >> L level-L pixels of the compact copy in s_coarse.
    auto expand_deep = [&]() {
        for (int L = 2; L < lo.n_levels; ++L) {
            const int side = 8 >> L;                              // level-L pixels per block side
            const unsigned char *srcL = s_coarse + (lo.off[L] - lo.off[2]);
            const int items = lo.DL[L] * 32;                      // (plane, block in tile, fine row)
            for (int it = tid; it < items; it += NTHR) {
                const int rr = it >> 5, grp = it & 31;
                const int blkq = grp >> 3, iy = grp & 7;
                const unsigned char *s = srcL + (((rr * 4 + blkq) * side + (iy >> L)) * side) * 2;
                v4i o;
                if (L == 2) {
                    const unsigned v = *reinterpret_cast<const unsigned *>(s);  // 2 pixels
                    o[0] = o[1] = (int)__builtin_amdgcn_perm(0u, v, 0x01000100u);
                    o[2] = o[3] = (int)__builtin_amdgcn_perm(0u, v, 0x03020302u);
                } else {
                    const unsigned v = *reinterpret_cast<const uint16_t *>(s);  // 1 pixel
                    o[0] = o[1] = o[2] = o[3] = (int)(v | (v << 16));
                }
                *reinterpret_cast<v4i *>(&s_tile[(lo.row0[L] + rr) * KP_PITCH + (blkq * 64 + iy * 8) * 2]) = o;
            }
        }
    };

    const int un = lane & 15, ug = lane >> 4;             // update operand coordinates
    // CL1: LDS addresses of the assign's transposed reads (K-step kk, read rd: plane row 16 kk + 8 h + (i16 >> 2) + 4 rd, first
    // sub-tile) and of the update's operand reads (plane tile pt: row 16 pt + un; first half): a full row holds the lane's pixels at
    // their place in the tile, a compact row the parent row of the lane's two fine rows (of its fine row: update)
    unsigned a_tr[KP_DSTEPS][2], a_up[KP_DSTEPS][2];
    if constexpr (CL1) {
        const int i16 = lane & 15, pxblk = (lane >> 4) & 1, hh = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < KP_DSTEPS; ++kk)
#pragma unroll
            for (int rd = 0; rd < 2; ++rd) {
                const int r = 16 * kk + 8 * hh + (i16 >> 2) + 4 * rd;
                const int off = r < DL0 ? ((wave * 64 + 16 * pxblk + 4 * (i16 & 3)) * 2) ^ row_swz(r) : pxblk * 32 + wave * 8;
                a_tr[kk][rd] = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)&s_tile[row_addr(r) + off];
            }
#pragma unroll
        for (int pt = 0; pt < KP_DSTEPS; ++pt) {
            const int r = 16 * pt + un;
            const bool full = r < DL0;
            const int off = full ? ((wave * 64 + 8 * ug) * 2) ^ row_swz(r) : (ug >> 1) * 32 + wave * 8;
            a_up[pt][0] = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)&s_tile[row_addr(r) + off];
            a_up[pt][1] = a_up[pt][0] + (full ? 8u : 0u);     // second half of the operand: the next 4 pixels, or the parent row again
        }
    }
    const unsigned usel = (un & 1) ? 0x07050301u : 0x06040200u;
    const unsigned eqr = (unsigned)un * 0x01010101u;
    const int cnt_bp = 2 * D;

    // Sweep order: workgroup g takes list positions g, g+G, ...; on odd passes the physical order is reversed
    // (boustrophedon), so a pass starts on the tiles the previous pass read last, i.e. on what is still in the 256 MiB
    // Infinity Cache.
    auto phys = [&](int lt) { return reverse ? nlist - 1 - lt : lt; };
    int ltile = g;
    if constexpr (!SPLIT) {
        if (ltile < nlist) stage_load(phys(ltile));
    }
    // this wave's block (one 8x8 block per wave) as (block row, block column) inside ITS image, advanced without a
    // division: which pixels exist and vote is decided from it. A step moves the tile index inside the image by
    // s1 = G mod ntiles, or by s1 - ntiles when that runs past the image's last tile (global list only).
    const int s1 = __builtin_amdgcn_readfirstlane(G % ntiles);
    const int q1 = __builtin_amdgcn_readfirstlane(4 * s1 / lo.bx_n), r1 = 4 * s1 - q1 * lo.bx_n;
    const int q2 = __builtin_amdgcn_readfirstlane(4 * (ntiles - s1) / lo.bx_n), r2 = 4 * (ntiles - s1) - q2 * lo.bx_n;
    int tin = __builtin_amdgcn_readfirstlane(phys(g < nlist ? g : 0) % ntiles);   // tile index inside its image
    int by, bx;
    {
        const int blk0 = 4 * tin + wave;
        by = blk0 / lo.bx_n;
        bx = blk0 - by * lo.bx_n;
    }
    if constexpr (SPLIT) {                 // wave-uniform: in SGPRs, advanced on the scalar unit (the wide kernels' register
        by = __builtin_amdgcn_readfirstlane(by);   // allocation was tuned with them in VGPRs: left alone)
        bx = __builtin_amdgcn_readfirstlane(bx);
    }
    // split slab: the tile that is LOADED next - one step ahead of `tin` - as two running pointers (its LO and MID runs) and its
    // tile index inside its image, advanced like `tin`: s1 tiles on / back modulo the image, qG (+ 1 on a wrap) images on / back -
    // one of two precomputed 64-bit strides per pointer -, and the iteration whose flag that load needs
    const int qG = __builtin_amdgcn_readfirstlane(G / ntiles);
    int tin_l = tin, it_l = 0;
    const unsigned char *p_lo_l = nullptr;
    unsigned mid_rel_l = 0;                                  // the tile's MID run, in bytes from its LO run (< 2^32: host check)
    long long d_lo[2] = {0, 0};                              // [wrap]
    int d_rel[2] = {0, 0};
    if constexpr (SPLIT) {
        const int bi0 = __builtin_amdgcn_readfirstlane(phys(g < nlist ? g : 0) / ntiles);
        const unsigned char *img = fb + (size_t)bi0 * lo.img_bytes;
        p_lo_l = img + (size_t)tin * lo.S;
        mid_rel_l = (unsigned)(lo.mid_off - (size_t)tin * (lo.S >> 1));      // mid_off + tin S / 2 - tin S
        const long long sg = reverse ? -1 : 1;
        d_lo[0] = sg * ((long long)qG * lo.img_bytes + (long long)s1 * lo.S);
        d_lo[1] = sg * ((long long)(qG + 1) * lo.img_bytes + (long long)(s1 - ntiles) * lo.S);
        d_rel[0] = (int)(sg * -(long long)s1 * (lo.S >> 1));
        d_rel[1] = (int)(sg * -(long long)(s1 - ntiles) * (lo.S >> 1));
    }
    auto tile_has_top = [&](int it) -> bool {
        return __builtin_amdgcn_readfirstlane(it < KP_FLAGS ? (int)s_flag[it < KP_FLAGS ? it : 0] : 1) != 0;
    };
    const int nt_limit = __builtin_amdgcn_readfirstlane(nt_flag);   // split slab: list positions below it are loaded `nt`
    auto load_next_split = [&](bool top, int pos) {
        top_regs = top;
        stage_load_split(p_lo_l, mid_rel_l, top_regs, pos < nt_limit);
        const int tn = reverse ? tin_l - s1 : tin_l + s1;
        const bool wrap = reverse ? tn < 0 : tn >= ntiles;
        tin_l = wrap ? (reverse ? tn + ntiles : tn - ntiles) : tn;
        p_lo_l += wrap ? d_lo[1] : d_lo[0];
        mid_rel_l += (unsigned)(wrap ? d_rel[1] : d_rel[0]);
        ++it_l;
    };
    if constexpr (SPLIT) {
        if (ltile < nlist) load_next_split(tile_has_top(0), ltile);
    }
    // CL1: the lane's four key bases live in registers (the kernel has them to spare since the compact level 1; the wide kernels, at
    // their 168, read them from LDS in every sub-tile)
    long long kbase[KT][4];
    if constexpr (CL1) {
#pragma unroll
        for (int mt = 0; mt < KT; ++mt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) kbase[mt][g4] = s_const[8 * mt + 2 * g4 + (lane >> 5)];
    }
    KP_PHASE_DECL;
    for (; ltile < nlist; ltile += G) {
        const int tile = phys(ltile);
        // (split slab) the flag of the tile loaded in this iteration: read from LDS here, used behind the barrier
        int flag_next = 1;
        if constexpr (SPLIT) flag_next = it_l < KP_FLAGS ? (int)s_flag[it_l < KP_FLAGS ? it_l : 0] : 1;
        stage_write();
        KP_PHASE(0);
        __syncthreads();
        KP_PHASE(1);
        // the next tile's loads go out first: a wave issuing them outranks the waves of the other workgroups that
        // are in their compute phase (18 interleaved A/B runs: 0.252 -> 0.244 ms per pass)
        __builtin_amdgcn_s_setprio(3);
        if (ltile + G < nlist) {                              // in flight during the MFMAs
            if constexpr (SPLIT) load_next_split(__builtin_amdgcn_readfirstlane(flag_next) != 0, ltile + G);
            else stage_load(phys(ltile + G));
        }
        __builtin_amdgcn_s_setprio(0);
        KP_PHASE(2);
        if (!SPLIT && lo.n_levels > 2) {
            expand_deep();
            __syncthreads();
        }

        const int blk = 4 * tin + wave;                          // block index inside the image
        // (CL1; by, bx are scalars) a main block that lies wholly inside the image and the voting rows, on a pass that writes no
        // label map: the assign epilogue then skips the per-pixel existence tests (12 of its 44 vector instructions per sub-tile)
        const bool full_blk = CL1 && !raster && blk < lo.nmain && 8 * bx + 8 <= lo.W && 8 * by >= row_lo &&
                              8 * by + 8 <= (row_hi < lo.H ? row_hi : lo.H);
        // -------- assign: two 32-pixel sub-tiles per wave (rows 4*sub .. 4*sub+3 of the block)
#pragma unroll
        for (int sub_i = 0; sub_i < ((GCS_ABL & 1) ? 0 : WAVES == 8 ? 1 : 2); ++sub_i) {
            const int sub = WAVES == 8 ? half : sub_i;
            const int n = lane & 31, h = lane >> 5;
            const int pl = wave * 64 + sub * 32 + n;
            v16i acc[KT];
#pragma unroll
            for (int mt = 0; mt < KT; ++mt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mt][e] = 0;
            // B fragments by hardware transpose: per 16-lane group ds_read_b64_tr_b16 reads a block of
            // 4 rows (planes) x 16 columns (pixels) of 16-bit elements and gives lane i column i, i.e.
            // the four planes of ITS pixel (cdna guide T10). Lane 4q+p of the group supplies the address
            // of row q, columns 4p..4p+3. Two reads = 8 planes = the 16-byte fragment of one K-step.
            // (Replaces 8 ds_read_u16 + 4 pack ops per K-step.) One asm statement: loads + their wait.
            v4i bfr[KP_DSTEPS];
            {
                const int i16 = lane & 15, pxblk = (lane >> 4) & 1;
                const unsigned addr = (unsigned)(size_t)&s_tile[(8 * h + (i16 >> 2)) * KP_PITCH +
                                                                (wave * 64 + sub * 32 + 16 * pxblk + 4 * (i16 & 3)) * 2];
                v2i fa[KP_DSTEPS], fbv[KP_DSTEPS];
                if constexpr (CL1) {
                    // rows of either kind (a_tr: one address per K-step and read, set up before the tile loop); the second 32-pixel
                    // sub-tile is 64 bytes further in BOTH: 32 pixels of a full row, two parent rows of a compact one
#pragma unroll
                    for (int kk = 0; kk < KP_DSTEPS; ++kk)
                        asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%c4\n\t"
                                     "ds_read_b64_tr_b16 %1, %3 offset:%c4"
                                     : "=&v"(fa[kk]), "=&v"(fbv[kk])
                                     : "v"(a_tr[kk][0]), "v"(a_tr[kk][1]), "i"(sub * 64)
                                     : "memory");
                } else
#pragma unroll
                for (int kk = 0; kk < KP_DSTEPS; ++kk)       // the DS offset field holds 16 bits: K-step base in the VGPR
                    asm volatile("ds_read_b64_tr_b16 %0, %2\n\t"
                                 "ds_read_b64_tr_b16 %1, %2 offset:%c3"
                                 : "=&v"(fa[kk]), "=&v"(fbv[kk])
                                 : "v"(addr + kk * 16 * KP_PITCH), "i"(4 * KP_PITCH)
                                 : "memory");
                // hipcc does not count asm loads: one explicit wait, then tie every destination register to it
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int kk = 0; kk < KP_DSTEPS; ++kk) {
                    asm volatile("" : "+v"(fa[kk]), "+v"(fbv[kk]));
                    bfr[kk] = v4i{fa[kk][0], fa[kk][1], fbv[kk][0], fbv[kk][1]};
                }
            }
#pragma unroll
            for (int kk = 0; kk < KP_DSTEPS; ++kk)
#pragma unroll
                for (int mt = 0; mt < KT; ++mt)
                    acc[mt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(apat[mt][kk], bfr[kk], acc[mt], 0, 0, 0);
            // key = 16*score + j via v_mad_i64_i32 (3 instructions per cluster instead of ~25 of sign
            // extension / 64-bit shift / borrow arithmetic): U = R0 + 256 R1 fits int32 (|U| < 2^30).
            long long best = 0x7fffffffffffffffLL;
#pragma unroll
            for (int mt = 0; mt < KT; ++mt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int u = __mul24(acc[mt][4 * g + 1], 256) + acc[mt][4 * g];
                    long long key = mad_i64_i32(u, -32, CL1 ? kbase[mt][g] : s_const[8 * mt + 2 * g + h]);   // base: registers, or an LDS broadcast read
                    key = mad_i64_i32(acc[mt][4 * g + 2], -2097152, key);
                    best = key < best ? key : best;
                }
            // partner half's key by v_permlane32_swap (VALU; no LDS round trip like ds_bpermute)
            const unsigned blo = (unsigned)best, bhi = (unsigned)((unsigned long long)best >> 32);
            const auto s0 = __builtin_amdgcn_permlane32_swap(blo, blo, false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(bhi, bhi, false, false);
            // after swap(x, x): element 0 holds the LOWER half's x in both halves, element 1 the UPPER half's: the minimum of the two
            // pairs is the pixel's best key in every lane, with no select by half (and only its low word is needed: the label)
            const long long ka = (long long)(((unsigned long long)s1[0] << 32) | s0[0]);
            const long long kb = (long long)(((unsigned long long)s1[1] << 32) | s0[1]);
            const int bj = (int)((kb < ka ? s0[1] : s0[0]) & 15);
            if (h == 0 && CL1 && full_blk) {
                // (wave-uniform) every pixel of the block exists and votes, and no label map is asked for: nothing to decide
                s_lab[pl] = (unsigned char)bj;
            } else
            if (h == 0) {
                // which pixel this slot holds (csrc/common.h): a main block's, or - rarely - an edge strip's
                // (CL1: MFMA column n is the pixel at place n of the block row order (x0 x2 x4 x6 | x1 x3 x5 x7))
                const auto col_of = [&](int nn) { return CL1 ? 2 * (nn & 3) + ((nn >> 2) & 1) : nn & 7; };
                int y = 8 * by + 4 * sub + (n >> 3), x = 8 * bx + col_of(n), xlim = lo.W;
                if (blk >= lo.nmain) {           // 26 of the 2 426 blocks of a BSD image
                    // the slot coordinates are re-derived from an opaque copy of the lane number: derived from `n` they are
                    // loop invariants, hipcc keeps them in VGPRs across the tile loop and the pass (168 VGPRs for three
                    // workgroups per CU) spills
                    int no = n;
                    asm volatile("" : "+v"(no));
                    gcs_strip_pixel(lo, blk, 4 * sub + (no >> 3), col_of(no), y, x, xlim);
                }
                const bool inimg = blk < lo.nblk && y < lo.H && x < xlim;
                const bool valid = inimg && y >= row_lo && y < row_hi;      // votes in the sums (halo rows do not)
                s_lab[pl] = valid ? (unsigned char)bj : (unsigned char)0xFF;
                // the label map itself, raster order [B][H][W] (the last pass): in a main block eight lanes cover one row
                // of the block, 32 (int32) or 8 (uint8) contiguous bytes
                if (raster && inimg) {
                    const size_t o = ((size_t)(per_image ? b : tile / ntiles) * lo.H + y) * lo.W + x;
                    if (raster_u8) static_cast<uint8_t *>(raster)[o] = (uint8_t)bj;
                    else static_cast<int32_t *>(raster)[o] = bj;
                }
            }
        }
        KP_PHASE(3);
        if (WAVES == 8 && do_acc) __syncthreads();             // the block's labels come from two waves
        // -------- update: one-hot MFMA over the block's 64 pixels
        if constexpr (UPD2) {
          if (do_acc && !(GCS_ABL & 2)) {
            // lane (row r = un = (j, b), K group ug): pixels 8 ug .. 8 ug + 7 of the block's 32-pixel half hf
            const unsigned eqj = (unsigned)(un >> 1) * 0x01010101u;
            const unsigned sel01 = (un & 1) ? 0x010c000cu : 0x0c010c00u, sel23 = (un & 1) ? 0x030c020cu : 0x0c030c02u;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const v2i lw = *reinterpret_cast<const v2i *>(&s_lab[wave * 64 + hf * 32 + 8 * ug]);
                v4i oh;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const unsigned x = (unsigned)lw[i] ^ eqj;                    // byte == 0 <=> label == j
                    const unsigned y = (x | 0x80808080u) - 0x01010101u;        // top bit clear <=> byte == 0
                    const unsigned d = ~y & 0x80808080u;                        // digit -128 where label == j
                    oh[2 * i] = (int)__builtin_amdgcn_perm(0u, d, sel01);       // (px, t): the digit where t == b, 0 elsewhere
                    oh[2 * i + 1] = (int)__builtin_amdgcn_perm(0u, d, sel23);
                }
                // The five plane tiles' operand reads go out TOGETHER, each MFMA waits for its own (counted lgkmcnt: LDS returns in
                // order; whatever else is in flight only makes a wait longer). Left to itself hipcc reads, waits and multiplies
                // tile by tile - five exposed LDS latencies per half - whatever the source order and however many registers are
                // free (profiles/r6_notes.md); asm loads are invisible to its wait counting, hence the explicit waits.
                static_assert(DSTEPS == 5, "the update's read batch is written out for five plane tiles");
                // (CL1: two 8-byte reads per plane tile - the halves of a full row's 16 bytes, or a compact row's parent row twice. The
                //  first L0T plane tiles are known to hold full rows only: ONE 16-byte read each, conflict-free with the rows' swizzle
                //  where the 8-byte reads of 16 consecutive rows cannot do better than two addresses per bank)
                v4i bq[DSTEPS];
                v2i bl[DSTEPS], bh[DSTEPS];
#pragma unroll
                for (int pt = 0; pt < DSTEPS; ++pt) {
                    if (pt < L0T)
                        asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=&v"(bq[pt]) : "v"(a_up[pt][0]), "i"(hf * 64) : "memory");
                    else
                        asm volatile("ds_read_b64 %0, %2 offset:%c4\n\t"
                                     "ds_read_b64 %1, %3 offset:%c4"
                                     : "=&v"(bl[pt]), "=&v"(bh[pt])
                                     : "v"(a_up[pt][0]), "v"(a_up[pt][1]), "i"(hf * 64)
                                     : "memory");
                }
                // reads issued behind plane tile pt's: one per later tile below L0T, two per later tile from L0T on
#define KP_UPD_YOUNGER(pt_) (((pt_) + 1 < L0T ? L0T - 1 - (pt_) : 0) + 2 * (DSTEPS - ((pt_) + 1 < L0T ? L0T : (pt_) + 1)))
#define KP_UPD_STEP(pt_)                                                                                  \
    do {                                                                                                  \
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(KP_UPD_YOUNGER(pt_)) : "memory");                       \
        if ((pt_) < L0T) {                                                                                \
            asm volatile("" : "+v"(bq[pt_]));                                                             \
        } else {                                                                                          \
            asm volatile("" : "+v"(bl[pt_]), "+v"(bh[pt_]));                                              \
            bq[pt_] = v4i{bl[pt_][0], bl[pt_][1], bh[pt_][0], bh[pt_][1]};                                \
        }                                                                                                 \
        accu[pt_] = __builtin_amdgcn_mfma_i32_16x16x64_i8(oh, bq[pt_], accu[pt_], 0, 0, 0);               \
    } while (0)
                KP_UPD_STEP(0);
                KP_UPD_STEP(1);
                KP_UPD_STEP(2);
                KP_UPD_STEP(3);
                KP_UPD_STEP(4);
#undef KP_UPD_STEP
#undef KP_UPD_YOUNGER
            }
          }
        } else
        if (do_acc && !(GCS_ABL & 2)) {
            const v4i lw = *reinterpret_cast<const v4i *>(&s_lab[wave * 64 + 16 * ug]);
            v4i oh;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned x = (unsigned)lw[i] ^ eqr;                    // byte == 0 <=> label == un
                const unsigned y = (x | 0x80808080u) - 0x01010101u;        // top bit clear <=> byte == 0
                oh[i] = (int)(~y & 0x80808080u);                            // digit -128 where label == un
            }
#pragma unroll
            for (int nti = 0; nti < NT_OWN; ++nti) {
                const int nt = WAVES == 8 ? min(half * NT_OWN + nti, KP_NT - 1) : nti;    // (a clamped duplicate is dropped below)
                const int d = 8 * nt + (un >> 1);
                const v4i *src = reinterpret_cast<const v4i *>(&s_tile[d * KP_PITCH + (wave * 64 + 16 * ug) * 2]);
                const v4i w0 = src[0], w1 = src[1];
                v4i bx_;
                bx_[0] = (int)__builtin_amdgcn_perm((unsigned)w0[1], (unsigned)w0[0], usel);
                bx_[1] = (int)__builtin_amdgcn_perm((unsigned)w0[3], (unsigned)w0[2], usel);
                bx_[2] = (int)__builtin_amdgcn_perm((unsigned)w1[1], (unsigned)w1[0], usel);
                bx_[3] = (int)__builtin_amdgcn_perm((unsigned)w1[3], (unsigned)w1[2], usel);
                accu[nti] = __builtin_amdgcn_mfma_i32_16x16x64_i8(oh, bx_, accu[nti], 0, 0, 0);
            }
        }
        {                                                        // next tile of this workgroup: s1 tiles on / back, modulo the image
            const int tn = reverse ? tin - s1 : tin + s1;
            const bool wrap = reverse ? tn < 0 : tn >= ntiles;
            const bool up = reverse == wrap;                     // block index grows
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
        KP_PHASE(4);
        __syncthreads();
        KP_PHASE(5);
#ifdef GCS_KP_PHASES
        ++kp_tiles;
#endif
    }
    KP_PHASE_STORE;

    if constexpr (FUSED) {
        // the last pass leaves the buffers as a call finds them: the one it read is cleared by the workgroup that finishes last
        // (a ticket taken at the very end, never waited for: every workgroup has read `prev` long before any takes one)
        if (!do_acc && fz.prev != nullptr) {
            __shared__ int s_last;
            const int nwg = (int)(gridDim.x * gridDim.y);
            if (tid == 0) s_last = atomicAdd(fz.ticket, 1u) == (unsigned)(nwg - 1);
            __syncthreads();
            if (s_last) {
                const long long total = (long long)(per_image ? (int)gridDim.y : 1) * fz.rows * K * (D + 1);
                for (long long i = tid; i < total; i += NTHR) fz.prev[i] = 0ull;
                if (tid == 0) *fz.ticket = 0u;
            }
        }
    }
    if (!do_acc) return;
    if constexpr (UPD2) {
        // ---- fold (UPD2): rows = (cluster, byte), columns = planes
        constexpr int RW2 = 16 * DSTEPS;                      // planes per row
        int *red = reinterpret_cast<int *>(s_tile);           // [4 blocks of the tile][16 rows][RW2]
        static_assert(4 * 16 * RW2 * 4 <= KP_ROWS * KP_PITCH, "fold buffer exceeds the tile buffer");
#pragma unroll
        for (int pt = 0; pt < DSTEPS; ++pt)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[(wave * 16 + 4 * ug + e) * RW2 + 16 * pt + un] = accu[pt][e];
        __syncthreads();
        const int D1 = D + 1;
        auto folded = [&](int j, int bb, int plane) {
            int sm_ = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) sm_ += red[(w * 16 + 2 * j + bb) * RW2 + plane];
            return -(long long)sm_ / 128;                     // the one-hot digit is -128
        };
        for (int i = tid; i < K * D1; i += NTHR) {
            const int j = i / D1, e = i % D1;                 // e = LOGICAL feature (or D = the count)
            const long long nj = folded(j, 0, D);             // the count row reads +1 in both bytes
            long long out = nj;
            if (e < D) {
                const int c = e / lo.F, f = e - c * lo.F;       // physical plane of logical feature e (levels unrolled)
                int pe = kp_plane_on_level<0>(lo, c, f);
                { const int q = kp_plane_on_level<1>(lo, c, f); pe = q >= 0 ? q : pe; }
                { const int q = kp_plane_on_level<2>(lo, c, f); pe = q >= 0 ? q : pe; }
                { const int q = kp_plane_on_level<3>(lo, c, f); pe = q >= 0 ? q : pe; }
                out = (folded(j, 0, pe) + 128 * nj) + 256 * (folded(j, 1, pe) + 128 * nj);
            }
            if constexpr (FUSED) {
                // (vector atomic, result unused; a zero - an empty cluster's row - adds nothing)
                const int wg = b * (int)gridDim.x + part;
                unsigned long long *row = reinterpret_cast<unsigned long long *>(partials) +
                                          ((size_t)(per_image ? b : 0) * fz.rows + (size_t)(wg % fz.rows)) * (K * D1);
                if (out != 0) atomicAdd(&row[i], (unsigned long long)out);
            } else
            partials[partial_index(per_image, b, part, parts, (int)gridDim.y, i, K * D1)] = (uint64_t)out;
        }
    }
    if constexpr (!UPD2) {
    // ---- fold the four waves' accumulators (rows = clusters, cols = byte-planes) and emit the row: every wave
    //      parks its registers in its own slice of the tile buffer (no zero-fill, no atomics), one barrier.
    constexpr int RW = KP_NT * 16;                            // byte-planes per cluster row
    int *red = reinterpret_cast<int *>(s_tile);               // [4 blocks of the tile][16][RW]
    static_assert(4 * 16 * RW * 4 <= KP_ROWS * KP_PITCH, "fold buffer exceeds the tile buffer");
#pragma unroll
    for (int nti = 0; nti < NT_OWN; ++nti) {
        const int nt = WAVES == 8 ? half * NT_OWN + nti : nti;
        if (nt < KP_NT)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[(wave * 16 + 4 * ug + e) * RW + 16 * nt + un] = accu[nti][e];
    }
    __syncthreads();
    const int D1 = D + 1;
    auto folded = [&](int j, int bp) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += red[(w * 16 + j) * RW + bp];
        return -(long long)s / 128;                           // the one-hot digit is -128
    };
    for (int i = tid; i < K * D1; i += NTHR) {
        const int j = i / D1, e = i % D1;                     // e = LOGICAL feature (or D = the count)
        const long long nj = folded(j, cnt_bp);
        long long out = nj;
        if (e < D) {
            const int c = e / lo.F, f = e - c * lo.F;           // physical plane of logical feature e (levels unrolled)
            int pe = kp_plane_on_level<0>(lo, c, f);
            { const int q = kp_plane_on_level<1>(lo, c, f); pe = q >= 0 ? q : pe; }
            { const int q = kp_plane_on_level<2>(lo, c, f); pe = q >= 0 ? q : pe; }
            { const int q = kp_plane_on_level<3>(lo, c, f); pe = q >= 0 ? q : pe; }
            out = (folded(j, 2 * pe) + 128 * nj) + 256 * (folded(j, 2 * pe + 1) + 128 * nj);
        }
        partials[partial_index(per_image, b, part, parts, (int)gridDim.y, i, K * D1)] = (uint64_t)out;
    }
    }
}

template <int KT, int NST, int DSTEPS, int WAVES, bool SPLIT, int L0T, bool FUSED>
static void launch_mfma_as(const LloydPassArgs &a, const GcsFold &fz, int nt_flag) {
    hipLaunchKernelGGL((kmeans_pass_mfma_kernel<KT, NST, DSTEPS, WAVES, SPLIT, L0T, FUSED>), dim3(a.parts, a.B), dim3(64 * WAVES), 0,
                       a.stream, a.feats, a.cent, a.lo, a.k, a.n_sets == a.B ? 1 : 0, a.parts, a.reverse ? 1 : 0, a.row_lo, a.row_hi,
                       a.partials, a.lab_out, a.lab_u8, nt_flag, fz);
}
template <bool SELF, int KT, int NST, int DSTEPS, int WAVES, bool SPLIT, int L0T>
static void launch_mfma(const LloydPassArgs &a, const GcsFold *fz, int nt_flag) {
    if constexpr (SELF)
        if (fz) return launch_mfma_as<KT, NST, DSTEPS, WAVES, SPLIT, L0T, true>(a, *fz, nt_flag);
    launch_mfma_as<KT, NST, DSTEPS, WAVES, SPLIT, L0T, false>(a, GcsFold{}, nt_flag);
}

void lloyd_mfma_launch(GcsPassKernel pk, const LloydPassArgs &a, const GcsFold *fz) {
    // which tile loads carry the nontemporal hint (csrc/lloyd_pass.h: gcs_pass_nt_limit; 0 for the wide-slab kernels, which load plain)
    const int nt_flag = gcs_pass_nt_limit(pk, a.lo, a.B, a.n_sets);
    switch (pk) {
#define GCS_PASS_LAUNCH(id, name, ...)                                                      \
    case GCS_PASS_##id:                                                                     \
        return launch_mfma<gcs_pass_self_updating(GCS_PASS_##id), __VA_ARGS__>(a, fz, nt_flag);
        GCS_MFMA_PASSES(GCS_PASS_LAUNCH)
#undef GCS_PASS_LAUNCH
    default: return;
    }
}
