// gabor_plan.h — the launch plan of gcs_gabor_features: WHICH kernels one call launches, in which order, over which levels and
// filters, with which grid and on which stream. Host arithmetic on the layout, the batch and the device's compute-unit count alone;
// the one place that decides it, for gcs_gabor_features (csrc/gabor.hip executes the plan launch by launch) and the test hook
// gcs_selftest_gabor_plan alike. Private to csrc/ (the ABI is include/gcs.h). Every gabor_mfma_kernel instantiation the library
// compiles is written once, in GCS_GABOR_ARMS below.
#pragma once
#include "common.h"
#include <vector>

constexpr int GP_TW = 64, GP_TH = 32;                       // the bank kernel's output tile (csrc/gabor.hip: G_TW, G_TH)
#ifndef GCS_GABOR_MTMAX_
#define GCS_GABOR_MTMAX_ 3
#endif
constexpr int GCS_GABOR_MTMAX = GCS_GABOR_MTMAX_;           // row tiles (of four filters) per launch; two for the 15-row frame
constexpr long long GCS_GABOR_FORK_MIN_PIXELS = 1 << 21;    // smaller two-level calls stay on one stream

// gabor_mfma_kernel<MT, GQ, KS, LVL, FAST, SPLIT>: the arms (MT, GQ, KS, LVL, FAST), each compiled for both slab formats.
// MT x KS: the A operand is MT x KS x 4 VGPRs (84 for 3 x 7, 64 for 2 x 8). (GQ, FAST): (1, false) a last tile with one filter
// pair, (2, true) the short epilogue (shift == 8), (2, false) the general one. LVL: 0 / 1 a single launch of that level, -1 a fused
// list with the level a run-time value, -2 the fused list of exactly levels 0 and 1 (the only fused list that keeps a third tile).
#define GCS_GABOR_EPILOGUES(X, MT, KS, LVL) X(MT, 1, KS, LVL, false) X(MT, 2, KS, LVL, true) X(MT, 2, KS, LVL, false)
#define GCS_GABOR_LEVELS(X, MT, KS) GCS_GABOR_EPILOGUES(X, MT, KS, 0) GCS_GABOR_EPILOGUES(X, MT, KS, 1) GCS_GABOR_EPILOGUES(X, MT, KS, -1)
#define GCS_GABOR_ARMS(X)                                                                                              \
    GCS_GABOR_EPILOGUES(X, 3, 7, -2) GCS_GABOR_EPILOGUES(X, 3, 7, 0) GCS_GABOR_EPILOGUES(X, 3, 7, 1)                   \
    GCS_GABOR_LEVELS(X, 2, 7) GCS_GABOR_LEVELS(X, 1, 7) GCS_GABOR_LEVELS(X, 2, 8) GCS_GABOR_LEVELS(X, 1, 8)

enum GaborPlanKernel { GP_PLANE0, GP_DOWN_RGB, GP_DOWN, GP_PRE01, GP_STRIP, GP_MFMA };

struct GaborPlanLaunch {
    GaborPlanKernel kernel;
    int MT, GQ, KS, LVL;              // GP_MFMA: the template arguments (GP_STRIP: KS)
    bool FAST, SPLIT;
    int L0, L1;                       // levels [L0, L1) the launch writes (pre-passes: their planes; strips and bank: their features)
    int mt0;                          // GP_MFMA: first row tile of the launch inside its level (first filter 4 * mt0)
    unsigned grid_x, grid_y;
    int total_tiles;                  // GP_MFMA: tiles of the launch's list; GP_STRIP: its tasks
    bool side;                        // on the side stream (forked calls: everything of level 1)
    bool join;                        // the caller's stream waits for the side stream in front of this launch
};

// The launches are kept in place: a call allocates nothing on the host for any bank of up to 100 filters per level (4 pre-passes and
// 4 lists of a strip launch and at most 13 bank launches would be 60; the widest bank of the default workload takes 4 in all).
// Wider banks - gcs_make_layout sets no bound on n_orient - spill into `more`.
constexpr int GP_PLAN_INLINE = 32;
struct GaborPlan {
    bool forked;                      // level 1 runs on the side stream (the caller joins it after the last launch at the latest)
    bool fuse_small;
    int n;                            // launches, in order: at(0) .. at(n - 1)
    GaborPlanLaunch first[GP_PLAN_INLINE];
    std::vector<GaborPlanLaunch> more;
    const char *error;                // != NULL: the call is refused with this message (nothing is launched)
    const GaborPlanLaunch &at(int i) const { return i < GP_PLAN_INLINE ? first[i] : more[(size_t)(i - GP_PLAN_INLINE)]; }
    void push(const GaborPlanLaunch &l) {
        if (n < GP_PLAN_INLINE) first[n] = l;
        else more.push_back(l);
        ++n;
    }
};

// rows (columns) of pyramid level L of an image of n rows (columns): every level halves, rounding up
static inline int gabor_level_extent(int n, int L) {
    for (; L > 0; --L) n = (n + 1) / 2;
    return n;
}
static inline int gabor_hp(int H) { return (H + GP_TH - 1) / GP_TH * GP_TH + 15; }
static inline int gabor_wp(int W) { return (W + GP_TW - 1) / GP_TW * GP_TW + 32; }

// Main region of level L (what the bank kernel's tile list covers: the level without its packed edge strips) in 32 x 32 half tiles
struct GaborRegions {
    bool pack_r, pack_b;
    int HL[GCS_LEVELS_MAX], WL[GCS_LEVELS_MAX];
    explicit GaborRegions(const GcsLayout &lo) : pack_r(lo.Wm != GCS_NO_STRIP), pack_b(lo.Hm != GCS_NO_STRIP), lo_(lo) {
        for (int L = 0; L < GCS_LEVELS_MAX; ++L) {
            HL[L] = gabor_level_extent(lo.H, L);
            WL[L] = gabor_level_extent(lo.W, L);
        }
    }
    int region_h(int L) const { return pack_b ? lo_.Hm >> L : HL[L]; }
    int region_w(int L) const { return pack_r ? lo_.Wm >> L : WL[L]; }
    int htx(int L) const { return (region_w(L) + GP_TW / 2 - 1) / (GP_TW / 2); }
    long long half_tiles(int L) const { return (long long)htx(L) * ((region_h(L) + GP_TH - 1) / GP_TH); }
    long long tiles_per_image(int L) const { return (half_tiles(L) + 1) / 2; }
    // tasks per image of gabor_strip_kernel for level L (three channels x (segments of the right strip + of the bottom strip's rows))
    int strip_tasks(int L) const {
        const int nseg_col = pack_r ? (HL[L] + 31) / 32 : 0;
        const int row_n = pack_b ? HL[L] - (lo_.Hm >> L) : 0;
        const int row_w = pack_r ? lo_.Wm >> L : WL[L];
        return 3 * (nseg_col + row_n * ((row_w + 63) / 64));
    }
private:
    const GcsLayout &lo_;
};

// A two-level bank (the default) on a batch of GCS_GABOR_FORK_MIN_PIXELS or more runs level 1 on a side stream when the caller has one
// to give (not while its stream is being captured): csrc/gabor.hip.
static inline bool gabor_fork_wanted(const GcsLayout &lo, int B) {
    return lo.n_levels == 2 && (long long)B * lo.H * lo.W >= GCS_GABOR_FORK_MIN_PIXELS;
}

// The plan of gcs_gabor_features(B images of lo.H x lo.W, bank of lo, ksize, shift) on a device of `cu_count` compute units.
// `side_stream`: the caller has a side stream (the plan forks only where gabor_fork_wanted). The arguments are those
// gcs_gabor_features has accepted (B, shape, ksize, shift in range).
static inline GaborPlan gabor_plan(const GcsLayout &lo, int B, int ksize, int shift, int cu_count, bool side_stream) {
    GaborPlan P{};
    const GaborRegions R(lo);
    const bool strips = R.pack_r || R.pack_b;
    P.forked = side_stream && gabor_fork_wanted(lo, B);
    const bool forked = P.forked;
    bool joined = !forked, join_next = false;                  // the side stream has (nothing / something) the caller must wait for
    auto join = [&]() {
        if (!joined) join_next = true;
        joined = true;
    };
    auto push = [&](GaborPlanLaunch l) {
        l.side = !joined && l.L0 >= 1;            // (nothing goes to the side stream once the caller has joined it)
        l.join = join_next;
        join_next = false;
        P.push(l);
    };
    // A call so small that the tiles of ALL its levels fit the resident slots at once (one to four BSD images) also takes
    // the fused list: level 1's tiles then run beside level 0's instead of in a launch of their own behind them (one image:
    // the two launches take 19 us each, one after the other; the slot is called once per image, script.py:22-30).
    long long tiles_all = 0;
    for (int L = 0; L < lo.n_levels; ++L) tiles_all += (long long)B * R.tiles_per_image(L);
    // (not for a split-slab bank whose level is three row tiles that cannot run as groups - 9 to 11 filters per level -: the fused
    //  three-tile kernel with both split store paths live spills 50 VGPRs; such a call takes the two single-level launches)
    const bool fuse_small = lo.n_levels == 2 && tiles_all <= 2LL * cu_count &&
                            !(lo.split && mtiles(lo.FL[0]) == 3 && lo.FL[0] % 4 != 0);
    P.fuse_small = fuse_small;
    // ---- pre-passes: the padded planes of every level (level L >= 2 reads level L-1's compact image)
    for (int L = 0; L < lo.n_levels; ++L) {
        const int Hp = gabor_hp(R.HL[L]), Wp = gabor_wp(R.WL[L]);
        GaborPlanLaunch l{};
        l.L0 = L;
        l.L1 = L + 1;
        l.grid_y = (unsigned)B;
        if (fuse_small && !forked) {                           // a small call: both pre-passes of the two-level bank in one launch
            if (L == 1) continue;
            l.kernel = GP_PRE01;
            l.L1 = 2;
            l.grid_x = (unsigned)((Hp * (Wp / 16) + 511) / 512 + gabor_hp(R.HL[1]));
        } else if (L == 0) {
            // level-0 pre-pass: about two interior items (16 bytes x 3 channels) per thread and loop round
            l.kernel = GP_PLANE0;
            l.grid_x = (unsigned)((Hp * (Wp / 16) + 511) / 512);
        } else {
            l.kernel = L == 1 ? GP_DOWN_RGB : GP_DOWN;
            l.grid_x = (unsigned)Hp;
        }
        push(l);
    }
    // ---- the bank: one launch per run of levels with the same filter count (every level of an even-scale bank)
    const int mtmax = ksize <= 13 ? GCS_GABOR_MTMAX : 2;   // A operand: MT x KS x 4 VGPRs (84 for 3 x 7, 64 for 2 x 8)
    const int KS = ksize <= 13 ? 7 : 8;                       // 7 K-steps need the kernel inside rows 1..13 of the 15-row frame
    for (int L0 = 0, L1 = 0; L0 < lo.n_levels; L0 = L1) {
        L1 = L0 + 1;
        // fused lists pay ~2 % for level fields that are no longer launch constants and win the small levels' ramp and
        // tail back: a gain from three levels on (8x8 bank: 0.90 -> 0.80 ms), a small loss for two (0.552 -> 0.557 ms)
        if (lo.n_levels > 2 || fuse_small)
            while (L1 < lo.n_levels && lo.FL[L1] == lo.FL[L0]) ++L1;
        // The packed edge strips (57 + 30 tasks of a few microseconds per BSD image), one small launch per level on the level's
        // stream IN FRONT of its MFMA launch: level 0's right behind the plane pre-pass, while the chip is still empty (a launch
        // behind the MFMA kernels cost 27 us at the end of the stage; reserving four CUs for it beside level 0 held level 1 back:
        // profiles/r4_notes.md), level 1's on the side stream in the tail of level 0 like level 1 itself.
        // (a fused list - L1 > L0 + 1 - joins the side stream first: every level's planes are then ready on the caller's stream)
        if (L0 == 0 && L1 > 1) join();
        if (strips) {
            const int Ls = L1 < 2 ? L1 : 2;
            long long tasks = 0;
            for (int L = L0; L < Ls; ++L) tasks += R.strip_tasks(L);
            const long long total = tasks * B;
            if (total > 0x3fffffffLL) { P.error = "gcs_gabor_features: too many strip tasks"; return P; }
            GaborPlanLaunch l{};
            l.kernel = GP_STRIP;
            l.KS = KS;
            l.L0 = L0;
            l.L1 = Ls;
            l.grid_x = (unsigned)((total + 3) / 4);
            l.grid_y = 1;
            l.total_tiles = (int)total;
            push(l);
        }
        const int FLg = lo.FL[L0], MT = mtiles(FLg);
        // three row tiles only for single launches of level 0 / 1 (compile-time level): with the level a run-time value the
        // store path of every level is live and a third tile's 28 A registers spill
        // (a fused list of exactly levels 0 and 1 - LVL = -2: two store paths - keeps the third tile too)
        const bool single = L1 - L0 == 1, two_fused = lo.n_levels == 2 && L0 == 0 && L1 == 2;
        const int mtmax_here = ((single && L0 <= 1) || two_fused) ? mtmax : 2;
        // a small call (fuse_small) whose filters fill whole row tiles: ONE launch of MT groups of one-tile workgroups (blockIdx.y)
        const bool grouped = fuse_small && FLg % 4 == 0 && MT > 1;
        const int passes = grouped ? 1 : (MT + mtmax_here - 1) / mtmax_here;
        const int per_pass = grouped ? MT : (MT + passes - 1) / passes;   // 4 tiles -> 2 + 2, not 3 + 1
        long long total_ll = 0;
        for (int L = L0; L < L1; ++L) total_ll += R.tiles_per_image(L) * B;
        if (total_ll > 0x3fffffffLL) { P.error = "gcs_gabor_features: too many tiles"; return P; }
        for (int mt0 = 0; mt0 < MT; mt0 += per_pass) {
            const int n = grouped ? 1 : MT - mt0 >= per_pass ? per_pass : MT - mt0;
            // filters of this launch: [4*mt0, min(FL, 4*(mt0+n))) of each level (planes c*FL + f)
            const int fl_here = FLg - 4 * mt0 < 4 * n ? FLg - 4 * mt0 : 4 * n;
            GaborPlanLaunch l{};
            l.kernel = GP_MFMA;
            l.MT = n;
            l.GQ = (fl_here - 4 * (n - 1) + 1) / 2;
            l.KS = KS;
            // single launches of level 0 / level 1 (every bank of at most two levels) compile that level's store path alone
            l.LVL = single && L0 <= 1 ? L0 : (n == 3 && two_fused) ? -2 : -1;
            // the short epilogue needs shift == 8 (bytes 1-2 of the low accumulator) and no unused accumulator quad
            l.FAST = l.GQ == 2 && shift == 8;
            l.SPLIT = lo.split != 0;
            l.L0 = L0;
            l.L1 = L1;
            l.mt0 = mt0;
            // persistent grid: one workgroup per resident slot (two 54 KB workgroups per CU)
            const int total_tiles = (int)total_ll, slots = cu_count * 2;
            l.grid_x = (unsigned)(total_tiles < slots ? total_tiles : slots);
            l.grid_y = (unsigned)(grouped ? MT : 1);
            l.total_tiles = total_tiles;
            push(l);
        }
    }
    return P;
}

// One text line per launch (gcs_selftest_gabor_plan, include/gcs.h)
static inline int gabor_plan_line(const GaborPlanLaunch &l, char *buf, size_t n) {
    char name[64];
    switch (l.kernel) {
    case GP_PLANE0: snprintf(name, sizeof name, "gabor_plane_kernel<0>"); break;
    case GP_DOWN_RGB: snprintf(name, sizeof name, "gabor_down_kernel<true>"); break;
    case GP_DOWN: snprintf(name, sizeof name, "gabor_down_kernel<false>"); break;
    case GP_PRE01: snprintf(name, sizeof name, "gabor_pre01_kernel"); break;
    case GP_STRIP: snprintf(name, sizeof name, "gabor_strip_kernel<%d>", l.KS); break;
    default:
        snprintf(name, sizeof name, "gabor_mfma_kernel<%d,%d,%d,%d,%s,%s>", l.MT, l.GQ, l.KS, l.LVL, l.FAST ? "true" : "false",
                 l.SPLIT ? "true" : "false");
    }
    return snprintf(buf, n, "%s levels=%d:%d f0=%d grid=%ux%u tiles=%d stream=%s join=%d\n", name, l.L0, l.L1, 4 * l.mt0, l.grid_x,
                    l.grid_y, l.total_tiles, l.side ? "side" : "main", l.join ? 1 : 0);
}
