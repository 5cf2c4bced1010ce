/* gcs.h — C ABI of libgcs.so: the MI355X (gfx950) Gabor-bank + k-means segmenter path.
 *
 * Drop-in boundary: the reference has NO plugin/operator/FFI registry for this path; its
 * whole interface is one positional Python call,
 *     labels = <callable>(img)            /root/reference/BSD_metrics/script.py:30
 * with img (H,W,3) uint8 (script.py:25) and labels (H,W) integer consumed by
 * metrics.__init__ (/root/reference/BSD_metrics/metrics.py:43-51). The functions below are
 * what a binding for that slot calls underneath; INTEGRATION.md shows the
 * ctypes stub. Arithmetic is defined by SPEC.md (exact integers).
 *
 * Conventions: every pointer named *_dev is device memory owned by the caller; no device memory is
 * allocated or freed and the host is never blocked here; work is ordered on `stream` (a hipStream_t; NULL = default
 * stream): when a call returns, everything it enqueued precedes whatever the caller enqueues on `stream` next.
 * gcs_gabor_features may run part of a large batch on a library-owned side stream (one per device, created on first
 * use) between an event fork from and an event join back into `stream` — the pattern stream capture records as a
 * graph. Return 0 on success, GCS_E* otherwise, with a thread-local message in gcs_last_error(). Not thread-safe per
 * buffer.
 *
 * Streams: a caller may rely on three things, for every entry point that takes a `stream` (tests/test_gpu_stream_contract.py holds
 * them on each one). Order on `stream` alone: every kernel, memset and copy of a call is enqueued on `stream` - none on the null
 * stream, none on a stream the call did not tie to `stream` -, so inputs may still be in the making by earlier work on `stream`
 * when the call is made, and outputs are complete for whatever follows on `stream`; no other stream or event need be waited for.
 * The Gabor side stream is joined before return: where gcs_gabor_features uses it (eager calls on a two-level bank whose batch holds 2^21
 * pixels or more: GCS_GABOR_FORK_MIN_PIXELS, csrc/gabor_plan.h), it waits for an event recorded on `stream` before its first launch and `stream` waits for it behind
 * its last, both enqueued inside the call; under stream capture the same work runs on `stream` alone and writes the same bytes.
 * No host wait: no call synchronises a stream, an event or the device, so a call returns while earlier work on `stream` is still
 * running. There is no exception: gcs_download included (its copies are asynchronous for pinned host memory, which it requires).
 * The entry points marked "(capturable)" can be recorded into a graph on any stream and replayed on other buffer contents.
 *
 * Buffers: a buffer of exactly the stated size - an array's element count, or what its *_bytes() function returns - is enough: no
 * call writes a byte outside it. Unless a function's comment says otherwise, every output and every workspace / scratch buffer may
 * hold anything on entry (what a call accumulates into is zeroed by the call), every output element is written, workspace and
 * scratch contents are undefined afterwards, and inputs are read only. The exceptions are named where they occur: buffers updated in
 * place (the slab under gcs_smooth_features and gcs_position_features, centroids_dev of gcs_kmeans_finalize and
 * gcs_kmeans_reduce_finalize, leaf_hist_dev of the sweeps), the workspace of gcs_kmeans_pass_fused (the caller zeroes it once), and
 * the slots of a feature slab that hold no pixel (no call writes them: they keep their bytes). Arrays larger than 2^31 elements or
 * 2^32 bytes are inside this contract wherever a function's own bounds admit them: tests/test_gpu_large_maps.py runs the label-map,
 * image, annotator-stack and canonical-tensor entry points on both sides of those lines (its table names what it does not run).
 */
#ifndef GCS_H
#define GCS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t *gcs_stream_t; /* == hipStream_t */

enum {
    GCS_OK = 0,
    GCS_EINVAL = 1, /* bad argument (shape, range, NULL) */
    GCS_EHIP = 2    /* HIP runtime error at launch */
};

#define GCS_ABI_VERSION 18
#define GCS_KSIZE_MAX 15  /* tap frame: 15 rows x 16 columns (SPEC.md §2) */
#define GCS_K_MAX 16      /* clusters */
#define GCS_TAP_ABS_SUM_MAX 32896 /* per filter and part: 255 * sum|tapq| < 2^23 (gcs_bank_pack rejects larger banks) */
#define GCS_SCALES_MAX 8  /* octave pyramid of at most 4 levels: scales 2L, 2L+1 run on level L (SPEC.md §2) */

int gcs_abi_version(void);
/* Compute units of the current HIP device (hipDeviceProp_t::multiProcessorCount): the persistent Gabor grid is sized from it;
 * the Lloyd pass geometry (gcs_kmeans_parts_per_image: a pure host function, so that buffers can be sized without a device)
 * is tuned for the 256 CUs of an MI355X in SPX mode and merely less efficient elsewhere. */
int gcs_device_cu_count(void);
const char *gcs_last_error(void);

/* The bank is described by (n_scales, n_orient): F = n_scales * n_orient filters, f = s * n_orient + o,
 * D = 3F features per pixel, d = c * F + f (SPEC.md §2-§3). */

/* ---- host-only helpers (no GPU needed) ------------------------------------------------ */

/* Filters are packed level by level, each level padded to a multiple of 4 filters (one 32-row MFMA tile =
 * 4 filters x {re,im} x {lo,hi} digits x 2 pixel shifts). Bytes of the packed A-operand image / number of int32 bias words. */
size_t gcs_bank_packed_bytes(int n_scales, int n_orient);
size_t gcs_bank_bias_count(int n_scales, int n_orient);

/* Pack quantised taps tapq[F][2][ks][ks] (int16, SPEC.md §2) into the lane-linear int8 A-fragments of
 * v_mfma_i32_32x32x32_i8 and the per-filter bias 128*sum(tapq_re) (pixels are fed as img-128).
 * Replaces nothing in the reference (bank absent). */
int gcs_bank_pack(const int16_t *tapq, int n_scales, int n_orient, int ksize, int8_t *packed, int32_t *bias);

/* Feature slab: every pyramid level at its own resolution, tile-major (a tile = four 8x8-pixel blocks with
 * their level-1..3 parents, one contiguous run; edge strips of one or two pixel columns / rows - both sides of a BSD500
 * image are 8k + 1 pixels - are packed into virtual blocks for banks of at most two levels; see csrc/common.h), uint16
 * stored offset-binary (x ^ 0x8080: both bytes are signed MFMA digits). Opaque to callers; gcs_features_unpack gives the
 * canonical [B][D][H][W] uint16 tensor of SPEC.md §3. "Label slab": a uint8 label map in RASTER order, [B][H][W]
 * (gcs_label_slab_bytes = B*H*W rounded up to 16). */
size_t gcs_feature_slab_bytes(int B, int H, int W, int n_scales, int n_orient);
/* ABI 18: banks of at most two pyramid levels with D <= 79 (every 4x6-style bank) keep the slab SPLIT: per image three planar
 * arrays in the same tile / plane / slot order - the low bytes, bits 8..11 and bits 12..15 of every value - and one flag word
 * per tile that says whether any of the tile's bits 12..15 is set (values of 4096 and more are 6e-5 of what BSD500 produces:
 * profiles/r6_notes.md). A Lloyd pass streams the first two arrays and, for flagged tiles only, the third: exact for any data.
 * gcs_feature_slab_bytes(B, ...) == B * gcs_feature_slab_bytes(1, ...) for every bank: image b's slab starts at b times that
 * (callers may hand a sub-batch's part of a slab to any entry point). gcs_feature_pass_bytes: the feature bytes ONE Lloyd
 * pass reads when no tile is flagged (3/4 of the feature bytes of a split slab, all of them otherwise; padding included).
 * Size bounds (img_bytes = gcs_feature_slab_bytes(1, ...); tests/test_gpu_large_offsets.py runs both sides of byte offsets 2^31 and
 * 2^32, tests/test_large_offset_geometry.py both sides of every bound):
 *   - one image of a SPLIT slab: img_bytes < 2^32 (held as: value bytes + 4 flag bytes per tile + 256 <= 2^32 - 1), else both size
 *     functions return 0 and every slab entry point refuses the shape (the MID / TOP / FLAG arrays are addressed by 32-bit offsets
 *     from the image's base);
 *   - one image of a wide slab: the size functions take any img_bytes; gcs_gabor_features refuses img_bytes > 2^32 - 1 (32-bit lane
 *     offsets inside one image);
 *   - a batch: B * img_bytes is a 64-bit product everywhere, so a slab may be far larger than 4 GiB; gcs_gabor_features refuses B >
 *     65535 and B * img_bytes >= 2^47; the Lloyd-pass entry points refuse B > 65535 and B * (tiles per image) > 2^29 - 1 (four times
 *     a tile's position in the batch list is kept in an int);
 *   - the entry points that take H, W <= 4096 only (gcs_feature_gradient, gcs_region_tree_slab) are inside all of these per image. */
size_t gcs_feature_pass_bytes(int B, int H, int W, int n_scales, int n_orient);
size_t gcs_label_slab_bytes(int B, int H, int W);
/* uint64 partial sums written by one assign pass: one row of k * (D+1) values per k-means workgroup, stored in chunks
 * of 16 elements, padded (opaque: only gcs_kmeans_reduce / gcs_kmeans_reduce_finalize read them). */
size_t gcs_kmeans_parts_per_image(int B, int H, int W);
size_t gcs_kmeans_partial_bytes(int B, int H, int W, int D, int k);

/* Device memory -> pinned host memory on `stream` through the copy engines (SDMA). The pipelined host path
 * (Segmenter.segment_stream) uses it instead of hipMemcpyAsync, which in this direction is served by a chip-filling blit
 * kernel that stalls the kernels of every other stream for as long as PCIe takes. */
int gcs_download(const void *src_dev, void *dst_host, size_t bytes, gcs_stream_t stream);

/* ---- device entry points ---------------------------------------------------------------- */

/* Scratch for gcs_gabor_features: reflect-padded planar (pixel-128) pyramid levels. */
size_t gcs_gabor_workspace_bytes(int B, int H, int W, int n_scales);

/* SPEC.md §3: img_dev [B][H][W][3] uint8 -> feats_dev slab (pyramid + filter bank + magnitude).
 * Fills the slot's first stage (script.py:30). Requires H, W >= 8; ksize and shift are those of the packed bank
 * (ksize <= 13 and shift == 8, i.e. every default-style Q15 bank, take the shorter kernels). shift is in 0..23; at shift == 8 the
 * bounds of gcs_bank_pack keep every response a 16-bit value and re^2 + im^2 < 2^31 (features <= 36 635); with any smaller shift
 * the caller guarantees that domain for its bank and images (SPEC.md §3 "Value range": features <= 46 340). workspace_dev:
 * gcs_gabor_workspace_bytes() bytes of device scratch, contents undefined before and after. feats_dev: gcs_feature_slab_bytes()
 * bytes that may hold anything on entry: every slot that holds a pixel and every flag word of a split slab is written. */
int gcs_gabor_features(const uint8_t *img_dev, int B, int H, int W, const int8_t *packed_dev,
                       const int32_t *bias_dev, int n_scales, int n_orient, int ksize, int shift, void *workspace_dev,
                       uint16_t *feats_dev, gcs_stream_t stream);

/* Slab -> canonical [B][D][H][W] uint16 (level-L responses replicated over 2^L blocks; tests / debugging). out_dev may hold
 * anything on entry; every element is written. */
int gcs_features_unpack(const uint16_t *feats_dev, int B, int H, int W, int n_scales, int n_orient,
                        uint16_t *out_dev, gcs_stream_t stream);

/* SPEC.md §4 init. n_sets == B: per-image codebooks (set s from image s); n_sets == 1:
 * global codebook from image 0. centroids_dev: uint16 [n_sets][k][D], may hold anything on entry, written whole. */
int gcs_kmeans_init(const uint16_t *feats_dev, int B, int H, int W, int n_scales, int n_orient, int k,
                    int n_sets, uint16_t *centroids_dev, gcs_stream_t stream);

/* out_dev uint16 [n][D] = feature vectors of the n pixels byx_dev[i] = (image, row, col) (int32 triples in
 * device memory); b < 0 yields a zero row. out_dev may hold anything on entry; every row is written. Used to publish
 * init centroids when one image is sharded by rows over several ranks (BASELINE config 5). */
int gcs_features_gather(const uint16_t *feats_dev, int B, int H, int W, int n_scales, int n_orient, int n,
                        const int32_t *byx_dev, uint16_t *out_dev, gcs_stream_t stream);

/* SPEC.md §4 assign + per-workgroup partial sums (one streaming pass over the slab).
 * Only rows [row_lo, row_hi) of each image vote in the sums (whole image: 0, H); halo rows of
 * a row-sharded image are labelled but do not vote. `reverse` != 0 sweeps the slab back to front:
 * alternate it from pass to pass so that each pass starts on what the previous one left in the
 * Infinity Cache (results do not depend on it). Long sweeps load the part of the slab that no later pass finds in that cache
 * with the nontemporal hint (gcs_selftest_pass_nt_limit): the hint only affects performance, results are identical bit for bit
 * with either load form. labels_dev: uint8 [B][H][W] label map (every pixel of every image is
 * labelled, rows outside the voting window included: B * H * W bytes, no byte behind them is written); partials_dev:
 * gcs_kmeans_partial_bytes() bytes, fully overwritten (no zeroing needed). D <= 207 (every BASELINE bank) runs on
 * the matrix cores, wider feature vectors on a generic VALU pass; k <= GCS_K_MAX. The same n_sets must be passed
 * to the reduce call that follows (it selects the partial layout).
 * Either output may be NULL (not both): labels_dev == NULL skips the label store (the passes whose assignment nobody
 * reads: all but the last), partials_dev == NULL skips the sums (the last pass: assignment only). */
int gcs_kmeans_assign_accumulate(const uint16_t *feats_dev, const uint16_t *centroids_dev, int B,
                                 int H, int W, int n_scales, int n_orient, int k, int n_sets, int row_lo,
                                 int row_hi, int reverse, uint8_t *labels_dev, uint64_t *partials_dev,
                                 gcs_stream_t stream);

/* The LAST Lloyd pass in one launch: assignment only (SPEC.md §4; the schedule's last pass has no update) with the label map
 * written straight in raster order, out_dev [B][H][W] int32 (out_u8 == 0: what metrics.py:43-51 consumes) or uint8
 * (out_u8 != 0). Same result as gcs_kmeans_assign_accumulate(labels, NULL) (followed by gcs_labels_widen for int32).
 * scratch_labels_dev: a uint8 label map (gcs_label_slab_bytes) that is needed, and then also filled, only for int32 output of
 * feature vectors of 208 or more planes (the generic pass); may be NULL otherwise - for D <= 207 it is never written, even when
 * passed. out_dev may hold anything on entry; every element is written. Whole images only (no row window). */
int gcs_kmeans_assign_raster(const uint16_t *feats_dev, const uint16_t *centroids_dev, int B, int H, int W, int n_scales,
                             int n_orient, int k, int n_sets, int reverse, void *out_dev, int out_u8,
                             uint8_t *scratch_labels_dev, gcs_stream_t stream);

/* partials -> sums_dev int64 [n_sets][k][D+1] ([..][D] = count). Deterministic slab
 * reduction (no float, no atomics). sums_dev may hold anything on entry: every element is written (nothing is added to what it
 * held). In global mode the caller all-reduces sums_dev across
 * ranks (RCCL, int64 sum) between this call and gcs_kmeans_finalize. */
int gcs_kmeans_reduce(const uint64_t *partials_dev, int B, int H, int W, int D, int k, int n_sets,
                      int64_t *sums_dev, gcs_stream_t stream);

/* SPEC.md §4 update: c = floor((2S + n) / (2n)), empty cluster keeps its centroid. centroids_dev uint16 [n_sets][k][D] is
 * updated in place: on entry it holds the previous centroids; the rows of the clusters that own a pixel are written, the others
 * are kept. */
int gcs_kmeans_finalize(const int64_t *sums_dev, int n_sets, int k, int D,
                        uint16_t *centroids_dev, gcs_stream_t stream);

/* Single-rank update: gcs_kmeans_reduce + gcs_kmeans_finalize in ONE launch (no all-reduce needed
 * in between). sums_dev may be NULL (then only the centroids are written); given, it may hold anything on entry and is written
 * whole. centroids_dev: in place, as in gcs_kmeans_finalize. */
int gcs_kmeans_reduce_finalize(const uint64_t *partials_dev, int B, int H, int W, int D, int k,
                               int n_sets, int64_t *sums_dev, uint16_t *centroids_dev,
                               gcs_stream_t stream);

/* Self-updating Lloyd passes (single rank, whole images): the loop is n_iter calls of gcs_kmeans_pass_fused and nothing else -
 * no gcs_kmeans_init, no reduce. Pass t makes its own centroids (t == 0: the SPEC.md §4 init pixels; else the §4 update from the
 * sums pass t - 1 left in the workspace), assigns, and - unless `last` - adds its sums into the workspace with 64-bit integer
 * atomics (any order gives the same bits). Same labels and centroids as init / assign_accumulate / reduce_finalize.
 *   gcs_kmeans_fused_workspace_bytes  bytes of the workspace, or 0 when this bank / k / n_sets has no such pass (then use the
 *                                     entry points above): today the split-slab banks (at most two pyramid levels, D <= 79, a
 *                                     tile of at most 12 288 slots) with k <= 8. A pure host function.
 *   workspace_dev                     ZEROED once by the caller when it is allocated; every complete loop (passes 0 .. n - 1, the
 *                                     last with last != 0) leaves everything a pass reads before writing it - the sum buffers, the
 *                                     counter of finished workgroups and all padding: every byte but the two centroid arrays - zero
 *                                     as it found it, whatever n, so loops may follow one another (also as replays of one captured
 *                                     graph). The two centroid arrays inside ([n_sets][k][D] uint16 each) keep the centroids of the
 *                                     loop's last two passes; pass 0 reads neither. This holds for loops of the SAME shape (B, H, W,
 *                                     bank, k, n_sets): another shape lays the workspace out differently and would find the old
 *                                     centroids inside its sum buffers, so the caller zeroes the workspace again before it is used
 *                                     for another shape. One loop at a time per workspace.
 *   pass                              t, counted from 0; `reverse` as in gcs_kmeans_assign_accumulate.
 *   centroids_dev                     uint16 [n_sets][k][D], WRITTEN whole: the centroids pass t used (nothing is read from it).
 *   out_dev, out_u8                   the raster label map of the last pass, as in gcs_kmeans_assign_raster (may hold anything
 *                                     on entry, written whole); ignored otherwise. */
size_t gcs_kmeans_fused_workspace_bytes(int B, int H, int W, int n_scales, int n_orient, int k, int n_sets);
int gcs_kmeans_pass_fused(const uint16_t *feats_dev, int B, int H, int W, int n_scales, int n_orient, int k, int n_sets,
                          int reverse, int pass, int last, void *workspace_dev, uint16_t *centroids_dev, void *out_dev,
                          int out_u8, gcs_stream_t stream);

/* uint8 label map [B][H][W] -> int32 [B][H][W] (the dtype handed to metrics.py:43). Both pointers 4-byte aligned. out_dev may
 * hold anything on entry; every element is written, and no byte behind the B * H * W bytes of labels_dev is needed. */
int gcs_labels_widen(const uint8_t *labels_dev, int B, int H, int W, int32_t *out_dev,
                     gcs_stream_t stream);

/* Test hook: counts in *bad_dev (uint32, device) the 4096-value chunks of [0, n_max] on which the kernels' 7-instruction
 * exact integer square root and its biased form in the epilogue (SPEC.md §3: n <= 2 * 32767^2 < 2^31, guaranteed by the
 * tap-sum bound of gcs_bank_pack) is wrong. Expected 0. *bad_dev may hold anything on entry: it is zeroed by the call. */
int gcs_selftest_isqrt(unsigned n_max, unsigned *bad_dev, gcs_stream_t stream);
/* Test hook (host only): working workgroups per image of the deep-bank Lloyd pass for a batch shape, computed from the
 * shape's tile count WITHOUT packed edge strips (an upper bound of every bank's tile count; the launcher uses the bank's own
 * count, which can only lower the pixels per workgroup); B * H * W / that many pixels per workgroup must stay below the
 * int32 accumulator bound (262 144 pixels). 0 for a bad shape. */
int gcs_selftest_native_parts(int B, int H, int W);
/* Test hook (host only, added within ABI 18): which kernel gcs_kmeans_assign_accumulate / gcs_kmeans_assign_raster run for this
 * bank and k, as a display name - split<KT,NR[,L0T]>, narrow<KT,NST>, wide<KT,NST>, wide8w<1,5>, native<NL,MINB,N0>, generic (a
 * static string) -, or NULL for a shape, bank or k they refuse. gcs_kmeans_fused_workspace_bytes != 0 exactly for split<1,3> and
 * split<1,3,2>. Launches nothing and touches no device. */
const char *gcs_selftest_pass_kernel(int H, int W, int n_scales, int n_orient, int k);
/* Test hook (host only, added within ABI 18: a new entry point changes no existing call, so GCS_ABI_VERSION did not move): the
 * `nt` limit one Lloyd pass over this batch would be launched with. The split-slab and the deep-bank kernels load the positions
 * below it of every sweep list (the whole batch, or one image when n_sets == B) with the nontemporal hint and the last 256 MiB of
 * the list plain; 0 for a kernel that loads every tile plain (wide slab, generic) and for a list of 256 MiB or less; -1 for a call
 * gcs_kmeans_assign_accumulate refuses (shape, bank, B, k, n_sets). Launches nothing and touches no device. */
int gcs_selftest_pass_nt_limit(int B, int H, int W, int n_scales, int n_orient, int k, int n_sets);
/* Test hook (host only, added within ABI 18: a new entry point changes no existing call, so GCS_ABI_VERSION did not move): the
 * launch plan of gcs_gabor_features for this call - the very list it executes (csrc/gabor_plan.h) - as text in buf (NUL-terminated;
 * lines that do not fit buf_bytes are left out, buf may be NULL), one line per launch in launch order:
 *     <kernel> levels=<L0>:<L1> f0=<first filter> grid=<x>x<y> tiles=<n> stream=<main|side> join=<0|1>
 * <kernel>: gabor_plane_kernel<0>, gabor_down_kernel<true|false>, gabor_pre01_kernel (the padded planes of levels [L0, L1)),
 * gabor_strip_kernel<7|8> (the packed edge strips of those levels; tiles = its tasks) or gabor_mfma_kernel<MT,GQ,KS,LVL,FAST,SPLIT>
 * (filters f0 .. of those levels; tiles = the launch's tile list, grid.y = its row-tile groups). join=1: the caller's stream waits
 * for the side stream in front of the launch (it always does behind the last one). cu_count: the compute units the persistent grids
 * and the small-call rule are sized for, 0 = those of the current device (gcs_device_cu_count; the only case that touches a
 * device). forked != 0: the caller has a side stream to give (no graph capture): the plan uses it where the bank and the batch
 * size ask for one. Returns the number of launches, -1 for a call gcs_gabor_features refuses. Launches nothing. */
int gcs_selftest_gabor_plan(int B, int H, int W, int n_scales, int n_orient, int ksize, int shift, int cu_count, int forked,
                            char *buf, size_t buf_bytes);

/* ---- boundary scoring of one image -------------------------------------- */

/* Integer part of /root/reference/BSD_metrics/metrics.py:25-51 (thick find_boundaries of the label
 * map and of each annotator map), :58-74 (recall) and :77-96 (precision): labels_dev int32 [H][W],
 * truth_dev uint16 [A][H][W] (the `Segmentation` arrays groundtruth.py:22-26 returns). Writes
 * counts_dev uint64 [1 + 3A]: [0] = #boundary pixels of the label map (metrics.py:90); for
 * annotator a: [1+3a] = sum(dilate5(bd(labels)) & bd(T_a)) and [2+3a] = sum(bd(T_a)) (metrics.py:69-72),
 * [3+3a] = sum(bd(labels) & dilate5(bd(T_a))) (metrics.py:93-94). The caller divides and averages in
 * the reference's order. scratch_dev: gcs_boundary_scratch_bytes() bytes. scratch_dev and counts_dev may hold anything on entry:
 * counts_dev is zeroed by the call and every element of it is a result. */
size_t gcs_boundary_scratch_bytes(int A, int H, int W);
int gcs_boundary_counts(const int32_t *labels_dev, const uint16_t *truth_dev, int A, int H, int W,
                        void *scratch_dev, uint64_t *counts_dev, gcs_stream_t stream);

/* Batched form: labels_dev int32 [B][H][W], truth_dev uint16 [T][H][W] = the annotator maps of image 0, then of image 1, ...
 * (T = total annotators; ragged: BSD500 has 4-9 per image, groundtruth.py:33-50), img_of_dev int32 [T] = image of each
 * annotator map. ONE pair of launches for the whole batch. counts_dev uint64 [B + 3T]: [b] = #boundary pixels of label map
 * b; for annotator t: [B+3t], [B+3t+1], [B+3t+2] = the three sums above. scratch_dev: gcs_boundary_batch_scratch_bytes().
 * scratch_dev and counts_dev may hold anything on entry: counts_dev is zeroed by the call. */
size_t gcs_boundary_batch_scratch_bytes(int B, int T, int H, int W);
int gcs_boundary_counts_batch(const int32_t *labels_dev, const uint16_t *truth_dev, const int32_t *img_of_dev, int B, int T,
                              int H, int W, void *scratch_dev, uint64_t *counts_dev, gcs_stream_t stream);

/* ---- boundary scoring on RESIDENT ground truth (ABI 17) -------------------------------------- */

/* The annotator maps are constants of the data set: /root/reference/BSD_metrics/metrics.py:48-49 re-derives
 * find_boundaries(truth) for every image it scores and groundtruth.py:44-48 rescans the directories per id. gcs_truth_prepare
 * does that work ONCE per annotator map: truth_dev uint16 [T][H][W] -> planes_dev, gcs_bit_planes_bytes(T, H, W) bytes of BIT
 * planes (rows of 64-bit words, bit i of word w = pixel 64 w + i; all thick-boundary planes bd(T_t), then all 5x5-dilated planes),
 * bd_counts_dev uint64 [T] = sum bd(T_t) (the recall denominators, metrics.py:72), and - when truth8_dev is not NULL - the maps
 * narrowed to uint8 [T][H][W] for gcs_region_counts_batch_u8. The CALLER guarantees that every annotator label is below 256 when
 * it passes truth8_dev (BSD500: at most 208; the narrowing keeps the low byte and does not check: evaluate_gpu.DeviceTruth does).
 * The caller keeps all of it on the device for as long as it scores images of these ids. planes_dev, bd_counts_dev and truth8_dev
 * may hold anything on entry; every word of the planes (the bits at and beyond column W are 0), every count and every byte of
 * truth8_dev ([T][H][W] bytes exactly) is written. */
size_t gcs_bit_planes_bytes(int M, int H, int W);
int gcs_truth_prepare(const uint16_t *truth_dev, int T, int H, int W, void *planes_dev, uint64_t *bd_counts_dev,
                      uint8_t *truth8_dev, gcs_stream_t stream);

/* gcs_boundary_counts_batch on prepared annotator planes: the same counts_dev uint64 [B + 3T] (every element written, no
 * atomics), from the bit planes of the B label maps (scratch_dev: gcs_bit_planes_bytes(B, H, W)) ANDed with the resident planes.
 * seg_max_dev int32 [B] (may be NULL): the largest label of each map (metrics.py:51 wants max + 1). scratch_dev, counts_dev and
 * seg_max_dev may hold anything on entry (seg_max_dev is zeroed by the call). */
int gcs_boundary_counts_resident(const int32_t *labels_dev, const void *truth_planes_dev, const uint64_t *truth_bd_counts_dev,
                                 const int32_t *img_of_dev, int B, int T, int H, int W, void *scratch_dev, uint64_t *counts_dev,
                                 int32_t *seg_max_dev, gcs_stream_t stream);

/* ---- region tables of one image ------------------------------------------ */

/* Integer part of /root/reference/BSD_metrics/metrics.py:102-146 (undersegmentation: the label x annotator
 * contingency table `hist` and the region areas) and :160-201 (compactness: the 4-neighbour `perimeters`).
 * labels_dev int32 [H][W] with values in [0, n_segments) (metrics.py:51: n_segments = max + 1); truth_dev
 * uint16 [A][H][W] with values < n_truth_labels (the largest `max(truth) + 1` over the annotators,
 * metrics.py:116). Writes hist_dev uint32 [A][n_segments][n_truth_labels], area_dev and perim_dev uint32
 * [n_segments]. hist_dev, area_dev and perim_dev may hold anything on entry: all three are zeroed by the call. The caller does the
 * reference's float arithmetic in the reference's order. */
int gcs_region_counts(const int32_t *labels_dev, const uint16_t *truth_dev, int A, int H, int W,
                      int n_segments, int n_truth_labels, uint32_t *hist_dev, uint32_t *area_dev,
                      uint32_t *perim_dev, gcs_stream_t stream);

/* Batched form (same ragged truth stack as gcs_boundary_counts_batch): first_dev int32 [B+1] = index of each image's first
 * annotator map (first[B] = T), max_annotators = the largest per-image count (it sizes the
 * workgroup-private tables; an image that brings more annotators than stated falls back to global atomics, still exact). hist_dev uint32 [T][n_segments][n_truth_labels],
 * area_dev / perim_dev uint32 [B][n_segments]; the three may hold anything on entry and are zeroed by the call. One launch for the
 * whole batch behind the zeroing. Every entry point that takes such a table stack (gcs_region_counts*, gcs_score_batch_resident,
 * gcs_region_agreement) refuses T * n_segments * n_truth_labels > 2^30 with GCS_EINVAL: a stack is at most 4 GiB. */
int gcs_region_counts_batch(const int32_t *labels_dev, const uint16_t *truth_dev, const int32_t *first_dev, int B, int T,
                            int max_annotators, int H, int W, int n_segments, int n_truth_labels, uint32_t *hist_dev,
                            uint32_t *area_dev, uint32_t *perim_dev, gcs_stream_t stream);

/* What metrics.py:128-140 takes from the tables of gcs_region_counts_batch, per annotator map t of image img_of[t]:
 * under_dev[t] = sum_seg (area[seg] - max_col hist[t][seg][col]) (metrics.py:129-130) and under_np_dev[t] = sum_seg sum_col
 * min(hist, rowsum - hist) (metrics.py:137-139), uint64 [T] each, integers. The host divides by H * W and averages over the
 * annotators in the reference's order without ever fetching the tables. under_dev and under_np_dev may hold anything on entry;
 * every element is written; the tables are read only. */
int gcs_region_reduce(const uint32_t *hist_dev, const uint32_t *area_dev, const int32_t *img_of_dev, int T, int n_segments,
                      int n_truth_labels, uint64_t *under_dev, uint64_t *under_np_dev, gcs_stream_t stream);

/* gcs_region_counts_batch on annotator maps narrowed to uint8 by gcs_truth_prepare (n_truth_labels <= 256): half the bytes. */
int gcs_region_counts_batch_u8(const int32_t *labels_dev, const uint8_t *truth8_dev, const int32_t *first_dev, int B, int T,
                               int max_annotators, int H, int W, int n_segments, int n_truth_labels, uint32_t *hist_dev,
                               uint32_t *area_dev, uint32_t *perim_dev, gcs_stream_t stream);

/* Everything metrics.get_metrics() (metrics.py:246-255) needs of a batch, on resident ground truth, in one call (six launches:
 * gcs_boundary_counts_resident + gcs_region_counts_batch[_u8] + gcs_region_reduce with their zeroing folded into one launch). truth_maps_dev: the uint8 (truth_is_u8 != 0) or uint16 annotator maps; scratch_dev:
 * gcs_bit_planes_bytes(B, H, W); hist_dev [T][n_segments][n_truth_labels] is scratch the caller may keep on the device; the other
 * outputs as documented at the three calls. Every output, hist_dev and scratch_dev may hold anything on entry (the call zeroes
 * what it accumulates into); the resident planes, counts and maps are read only. */
int gcs_score_batch_resident(const int32_t *labels_dev, const void *truth_planes_dev, const uint64_t *truth_bd_counts_dev,
                             const void *truth_maps_dev, int truth_is_u8, const int32_t *first_dev, const int32_t *img_of_dev, int B,
                             int T, int max_annotators, int H, int W, int n_segments, int n_truth_labels, void *scratch_dev,
                             uint32_t *hist_dev, uint64_t *counts_dev, int32_t *seg_max_dev, uint32_t *area_dev, uint32_t *perim_dev,
                             uint64_t *under_dev, uint64_t *under_np_dev, gcs_stream_t stream);

/* ---- region agreement: PRI, VoI, segmentation covering (SPEC.md §8) ----------------------------- */

/* The three region metrics of the BSDS500 benchmark out of the contingency tables the calls above leave on the device
 * (gcs_region_counts[_batch[_u8]], gcs_score_batch_resident): hist_dev uint32 [T][n_segments][n_truth_labels], one table per
 * annotator map t, n_ij = pixels with label i and annotator label j. With a_i = sum_j n_ij and b_j = sum_i n_ij taken from
 * the table itself, writes per map t
 *   sums_dev  uint64 [T][4] = { N_t = sum_j b_j, sum_i a_i^2, sum_j b_j^2, sum_ij n_ij^2 }                  (exact)
 *   terms_dev double [T][4] = { sum a_i log2 a_i, sum b_j log2 b_j, sum n_ij log2 n_ij,
 *                               sum_j b_j * n*_j / u*_j }  (over non-zero entries; n*_j / u*_j = the largest
 *                               n_ij / (a_i + b_j - n_ij) of column j, compared exactly)
 * The host checks N_t == H * W (a label outside the table was not counted) and finishes PRI / VoI / covering (SPEC.md §8).
 * seg_max_dev int32 [B] (may be NULL; needs img_of_dev int32 [T] = image of map t): rows above seg_max[img_of[t]] are not
 * read (tables allocated at a capacity of segments). scratch_dev: gcs_region_agreement_scratch_bytes(T, n_segments,
 * n_truth_labels) bytes. Float sums run in an order fixed by the table indices alone: the same maps give the same bits at any
 * table shape, from run to run. scratch_dev, sums_dev and terms_dev may hold anything on entry; every element of the two outputs
 * is written; hist_dev is read only. */
size_t gcs_region_agreement_scratch_bytes(int T, int n_segments, int n_truth_labels);
int gcs_region_agreement(const uint32_t *hist_dev, const int32_t *img_of_dev, const int32_t *seg_max_dev, int T, int n_segments,
                         int n_truth_labels, void *scratch_dev, uint64_t *sums_dev, double *terms_dev, gcs_stream_t stream);

/* ---- connected regions (SPEC.md §7) -------------------------------------- */

/* labels_dev int32 [B][H][W] -> out_dev int32 [B][H][W]: 4-connected components of equal labels,
 * renumbered 0,1,2,... in raster order of each component's first pixel, per image. Makes
 * `Regions = max + 1` (/root/reference/BSD_metrics/metrics.py:51) count connected regions.
 * scratch_dev: gcs_connected_scratch_bytes() bytes. out_dev may not alias labels_dev. scratch_dev and out_dev may hold anything
 * on entry; every element of out_dev is written. */
size_t gcs_connected_scratch_bytes(int B, int H, int W);
int gcs_connected_regions(const int32_t *labels_dev, int B, int H, int W, void *scratch_dev,
                          int32_t *out_dev, gcs_stream_t stream);

/* ---- small-region merging (SPEC.md §9) ------------------------------------------------------ */

/* labels_dev int32 [B][H][W] -> out_dev int32 [B][H][W]: the connected regions of §7, then rounds in which every region
 * of fewer than min_size pixels that has a neighbour joins its largest neighbour (ties: the earlier first pixel), until
 * none is left; numbered 0,1,2,... in raster order of first pixel, per image. min_size <= 1 gives gcs_connected_regions
 * bit for bit. Stream-ordered, no host synchronisation. scratch_dev: gcs_merge_scratch_bytes() bytes (about 20 per pixel;
 * 0 for a bad shape or min_size < 0). out_dev may not alias labels_dev. scratch_dev and out_dev may hold anything on entry; every
 * element of out_dev is written. */
size_t gcs_merge_scratch_bytes(int B, int H, int W, int min_size);
int gcs_merge_small_regions(const int32_t *labels_dev, int B, int H, int W, int min_size, void *scratch_dev,
                            int32_t *out_dev, gcs_stream_t stream);

/* ---- node map of the region tree on connected regions (SPEC.md §18) --------------------------- */

/* labels_dev int32 [B][H][W] -> nodes_out_dev int32 [B][H][W]: per image, with C = the number of connected regions of §7 and
 * m_guard = ceil(H W / k_cap), the map of gcs_merge_small_regions at m_b = max(min_size, m_guard) if C > k_cap, else at min_size
 * (m_b <= 1: gcs_connected_regions bit for bit). Every node is 4-connected, an image has at most k_cap of them (§9 leaves no
 * region below m_b pixels beside another, so at most H W / m_guard <= k_cap), numbered 0,1,2,... in raster order of first pixel.
 * n_nodes_out_dev int32 [B]: the node count; min_size_used_dev int32 [B] (may be NULL): m_b. The decision is taken per image on
 * the device: one launch sequence for the batch, in which an image with m_b <= 1 runs no round (its blocks return at once), and
 * with min_size <= 1 and H W <= k_cap no round is enqueued. Stream-ordered, no allocation, no host synchronisation (capturable).
 * scratch_dev: gcs_region_nodes_scratch_bytes() bytes (about 20 per pixel; 0 for a bad shape), contents undefined before and after.
 * GCS_EINVAL, with nothing launched: a NULL labels / scratch / nodes_out / n_nodes_out pointer, a nodes_out_dev range that overlaps
 * the labels_dev range, B outside 1..65535, H or W outside 1..4096, min_size < 0, k_cap outside 1..4096.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
size_t gcs_region_nodes_scratch_bytes(int B, int H, int W);
int gcs_region_nodes(const int32_t *labels_dev, int B, int H, int W, int min_size, int k_cap, void *scratch_dev,
                     int32_t *nodes_out_dev, int32_t *n_nodes_out_dev, int32_t *min_size_used_dev, gcs_stream_t stream);

/* ---- smoothing of the feature levels (SPEC.md §10) --------------------------------------------- */

/* In place on a feature slab that gcs_gabor_features has filled (either format: split or wide): every plane of every level
 * becomes h = (sum_{dy,dx} w_dy w_dx g[r(y+dy), r(x+dx)] + 2^23) >> 24 at the level's own resolution (reflect border), with the
 * taps of the plane's filter scale; the flag words of a split slab are rewritten to match. taps_dev int32 [n_scales][49], tap i of
 * scale s at [s][24 + i], i = -R_s .. R_s (the rest is not read); radius_dev int32 [n_scales]. Both are read on the device: a
 * scale whose radius is outside 1..24 or whose taps are negative or do not sum to 4096 is left unsmoothed (the host validates
 * before it uploads; bank.smoothing_taps). Stream-ordered, two launches, no host synchronisation, no allocation (capturable).
 * workspace_dev: gcs_smooth_workspace_bytes() bytes (the level planes, 2 bytes per value; 0 for a bad shape), contents undefined
 * before and after. Slab slots that hold no pixel keep their bytes. Requires H, W >= 8. */
size_t gcs_smooth_workspace_bytes(int B, int H, int W, int n_scales, int n_orient);
int gcs_smooth_features(uint16_t *feats_dev, int B, int H, int W, int n_scales, int n_orient, const int32_t *taps_dev,
                        const int32_t *radius_dev, void *workspace_dev, gcs_stream_t stream);

/* ---- opponent colours (SPEC.md §11) ------------------------------------------------------------- */

/* img_dev uint8 [n_pixels][3] interleaved RGB -> out_dev uint8 [n_pixels][3] interleaved (Y, Co, Cg) of T_gain (SPEC.md §11:
 * Y = (R + 2G + B + 2) >> 2, Co = clamp(128 + ((gain (R - B)) >> 1), 0, 255), Cg = clamp(128 + ((gain (2G - R - B)) >> 2), 0, 255),
 * arithmetic shifts). Both pointers may have ANY byte alignment (a sub-batch of 481 x 321 images starts at any byte) and n_pixels
 * may be any count >= 1: exactly the bytes [0, 3 n_pixels) of img_dev are read and of out_dev written. Stream-ordered, one
 * launch, no allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched, for a NULL pointer, a gain
 * outside 1..16, n_pixels == 0 and for an out_dev range that overlaps the img_dev range (not in place).
 * Added within ABI 18: a new entry point changes no existing call, so GCS_ABI_VERSION did not move. */
int gcs_colour_opponent(const uint8_t *img_dev, size_t n_pixels, int gain, uint8_t *out_dev, gcs_stream_t stream);

/* ---- position features (SPEC.md §12) ------------------------------------------------------------ */

/* In place on a feature slab (either format) of a bank whose LAST slot of every scale is the coordinate slot (zero taps; n_orient
 * here counts it, as everywhere in this header): channel 0 of slot n_orient - 1 of scale s (level L = s / 2) becomes
 * weight * (y0 + (yl << L)), channel 1 weight * (xl << L) at level pixel (yl, xl); channel 2 and every other plane keep what the
 * Gabor stage (and gcs_smooth_features, which must run first when it is used) left. y0 = global row of row 0 (row strips of a
 * taller image; 0 otherwise). A split slab's flag byte of level L is SET for a tile that receives a value of 4096 or more and is
 * never cleared; slots that hold no pixel keep their bytes. One launch for all levels, stream-ordered, no workspace, no atomics,
 * no allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched, for a NULL pointer, a bad shape
 * (B >= 1, H, W >= 8, a representable bank), a weight outside 1..255, weight * (max(y0 + H, W) - 1) > 46 340 (SPEC.md §3's value
 * range) and a y0 that is negative or not a multiple of 2^(levels - 1).
 * Added within ABI 18: a new entry point changes no existing call, so GCS_ABI_VERSION did not move. */
int gcs_position_features(uint16_t *feats_dev, int B, int H, int W, int n_scales, int n_orient, int weight, int y0,
                          gcs_stream_t stream);

/* ---- superpixels: grid-local k-means (SPEC.md §13) ------------------------------------------------ */

/* The Lloyd stage of §4 replaced by K = ny * nx centres per image on a grid, each pixel compared with the centres of the 3 x 3 grid
 * cells around its own only: dist = sum_d (x_d - c_d)^2 + lambda ((y - cy)^2 + (x - cx)^2) in 64-bit integers, ties to the lowest
 * centre index; update = §4's rounding rule on every feature and on cy, cx (an empty centre keeps its values); n_iter assigns, n_iter - 1
 * updates. The kernels read the CANONICAL tensor of gcs_features_unpack, [B][D][H][W] uint16 (2 D bytes per pixel per pass), not the slab.
 *   gcs_superpixel_grid             host only: S = max(1, rint(sqrt(H W / n))), ny = max(1, rint(H / S)), nx = max(1, rint(W / S)), rint =
 *                                   round-half-even on the double value (any out pointer may be NULL). GCS_EINVAL outside 1 <= H, W <= 4096,
 *                                   2 <= n <= 4096. ny * nx may exceed 4096 (small S): the two calls below refuse such a grid.
 *   gcs_superpixel_workspace_bytes  host only: bytes of workspace_dev for the grid of (H, W, n): per image the centres, their positions
 *                                   and one [K][D + 3] row set of uint64 sums (features, y, x, count). 0 for a bad argument. Contents are
 *                                   undefined before and after a call (nothing to zero). For a caller-chosen ny x nx grid: the call lays
 *                                   the workspace out by its own K = ny * nx, so the size for any n whose grid has at least that many
 *                                   centres suffices.
 *   gcs_superpixel_segment          enqueues the whole schedule on `stream`: init (centre (i, j) := the pixel at cy = floor((2i+1) H /
 *                                   (2 ny)), cx = floor((2j+1) W / (2 nx))), then n_iter assign passes with an update launch behind all
 *                                   but the last: 2 n_iter launches (+1 with centres_out_dev). No allocation, no host synchronisation
 *                                   (capturable). labels_out_dev int32 [B][H][W] in 0 .. K-1 (the last assign). centres_out_dev: NULL, or
 *                                   int32 [B][K][D + 2] = the D features, cy, cx of every centre as the last assign used them.
 * GCS_EINVAL, with nothing launched: a NULL feats / workspace / labels pointer, B outside 1..65535, H or W outside 1..4096, D outside
 * 1..207, ny outside 1..H, nx outside 1..W, ny * nx > 4096, lambda outside 1..65535, n_iter < 1. In that domain a distance is at most
 * 207 * 46340^2 + 65535 * 2 * 4095^2 < 2^63.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
int gcs_superpixel_grid(int H, int W, int n, int *S_out, int *ny_out, int *nx_out);
size_t gcs_superpixel_workspace_bytes(int B, int H, int W, int D, int n);
int gcs_superpixel_segment(const uint16_t *feats_canonical_dev, int B, int H, int W, int D, int ny, int nx, int lambda, int n_iter,
                           void *workspace_dev, int32_t *labels_out_dev, int32_t *centres_out_dev, gcs_stream_t stream);

/* ---- region tree: merging a label map's regions on their adjacency graph (SPEC.md §14) ------------ */

/* Nodes = the labels 0 .. K-1 of labels_dev that own a pixel (`alive` of them); per node the pixel count n, the exact feature sums and
 * the mean m_d = floor((2 S_d + n) / (2 n)); two nodes are adjacent when a pixel of one is a 4-neighbour of a pixel of the other;
 * cost(A, B) = sum_d (m_A,d - m_B,d)^2 * min(n_A, n_B) in unsigned 64 bits (< 2^62). Per round every node picks the adjacent node of
 * least (cost, rep), rep = the smallest label of a group; mutual picks merge; a round's merges are listed in (cost, smaller rep) order.
 *   gcs_region_tree_workspace_bytes  host only: bytes of workspace_dev: per image the [K][D + 1] uint64 sums, the K x K adjacency bit
 *                                    matrix and the [K][D] uint16 means. 0 for a bad argument. Contents are undefined before and after a
 *                                    call (the call zeroes what it accumulates into).
 *   gcs_region_tree                  enqueues three launches on `stream` (zero, statistics + adjacency in one read of feats and labels,
 *                                    every merge round inside one kernel, a workgroup per image). No allocation, no host synchronisation
 *                                    (capturable). merges_out_dev int32 [B][K - 1][2]: row t = the reps (a < b) of the two groups merged at
 *                                    step t; costs_out_dev: NULL, or uint64 [B][K - 1]; alive_out_dev int32 [B]. Rows that no merge filled
 *                                    (rows >= alive - 1) are (-1, -1) with cost 0. The tree does not depend on any R.
 *   gcs_region_tree_cut              one launch: the first max(0, alive - R) rows applied, the groups numbered 0, 1, ... in increasing order
 *                                    of their rep: labels_out_dev int32 [B][H][W] has min(alive, R) labels per image. labels_out_dev may
 *                                    BE labels_dev (in place); it must not overlap it otherwise. Any list is taken: a row that is not
 *                                    0 <= a < b < K with both still reps at that step is skipped, as in gcs_region_sweep.
 * A pixel whose label is outside 0 .. K-1 is counted nowhere, is adjacent to nothing and leaves the cut as -1. feats_canonical_dev is
 * the [B][D][H][W] uint16 tensor of gcs_features_unpack. With K = 1 there are no rows: merges / costs pointers are not read.
 * Every output (merges, costs, alive, labels_out) may hold anything on entry and is written whole; inputs are read only. The one
 * exception is the in-place cut: labels_out_dev == labels_dev then holds the input on entry, and every element is replaced.
 * GCS_EINVAL, with nothing launched: a NULL feats / labels / workspace / alive / labels_out pointer, a NULL merges pointer with K > 1,
 * B outside 1..65535, H or W outside 1..4096, D outside 1..207, K outside 1..4096, R < 1.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
size_t gcs_region_tree_workspace_bytes(int B, int H, int W, int D, int K);
int gcs_region_tree(const uint16_t *feats_canonical_dev, const int32_t *labels_dev, int B, int H, int W, int D, int K,
                    void *workspace_dev, int32_t *merges_out_dev, uint64_t *costs_out_dev, int32_t *alive_out_dev, gcs_stream_t stream);
int gcs_region_tree_cut(const int32_t *labels_dev, const int32_t *merges_dev, const int32_t *alive_dev, int B, int H, int W, int K,
                        int R, int32_t *labels_out_dev, gcs_stream_t stream);

/* gcs_region_tree with the statistics taken from the feature slab itself (SPEC.md §21): feats_slab_dev is the slab gcs_gabor_features
 * (and gcs_smooth_features / gcs_position_features) filled for B images of H x W and the bank (n_scales, n_orient = slots per scale),
 * either slab format; D = 3 n_scales n_orient. One launch replaces the statistics launch: every level's values are read at the level's
 * own resolution and added to the labels of the full-resolution pixels they cover. Sums, adjacency, merges, costs and alive are, bit
 * for bit, those of gcs_region_tree on gcs_features_unpack of the same slab; workspace_dev: gcs_region_tree_workspace_bytes(B, H, W,
 * D, K), whose head holds the [B][K][D + 1] uint64 sums after the call's second launch (the merge kernel adds merged rows in place).
 * Three launches, no allocation, no host synchronisation (capturable).
 * GCS_EINVAL, with nothing launched: as gcs_region_tree, and a bank gcs_feature_slab_bytes refuses or of more than 207 features.
 * Added within ABI 18: a new entry point changes no existing call, so GCS_ABI_VERSION did not move. */
int gcs_region_tree_slab(const uint16_t *feats_slab_dev, const int32_t *labels_dev, int B, int H, int W, int n_scales, int n_orient,
                         int K, void *workspace_dev, int32_t *merges_out_dev, uint64_t *costs_out_dev, int32_t *alive_out_dev,
                         gcs_stream_t stream);

/* ---- contour map of the region tree, and the boundary counts of every cut at once (SPEC.md §15) ---- */

/* U(y, x) = the largest s(L(y, x), L(y', x')) over the 4-neighbours inside the image, s(p, q) = t + 1 for the row t of merges_dev whose
 * merge first puts the labels p and q into one group, `alive` where no row does or one of them is outside 0 .. K-1, 0 for p = q. For
 * every R >= 1, U > max(0, alive - R) is the thick boundary map of gcs_region_tree_cut at R.
 *   gcs_region_tree_contours_workspace_bytes  host only: per image K uint16 positions and a range-maximum table of ceil(log2 K) levels
 *                                    of K uint16 entries. 0 for a bad argument. Contents are undefined before and after a call.
 *   gcs_region_tree_contours         two launches on `stream` (prepare: a workgroup per image; pixels). No allocation, no host
 *                                    synchronisation (capturable). merges_dev / alive_dev as gcs_region_tree wrote them, or any list
 *                                    whose written rows come first and have a < b, both reps at that step (a row that is not is
 *                                    skipped). contours_out_dev int32 [B][H][W], values 0 .. alive; it must NOT overlap labels_dev
 *                                    (neighbours are read). With K = 1 merges_dev is not read.
 *   gcs_boundary_sweep_resident      two launches (zero, one pass over the map). hist_out_dev uint32 [B + 2T][K + 1], zeroed by the call:
 *                                    row b: #{U_b = s}; row B + 2t: #{bd(T_t) : M5(U) = s}; row B + 2t + 1: #{dil5(bd(T_t)) : U = s},
 *                                    for s = 1 .. K (bin 0 stays 0, a value of U outside 1 .. K is counted nowhere), M5 = the maximum over
 *                                    the 5 x 5 window clipped to the image. With tau = max(0, alive_b - R) the sums over s > tau are the
 *                                    counts [b], [B + 3t] and [B + 3t + 2] of gcs_boundary_counts_resident for the cut at R.
 *                                    truth_planes_dev: what gcs_truth_prepare wrote; img_of_dev int32 [T], non-decreasing (the
 *                                    annotators of an image are consecutive). No allocation, no host synchronisation (capturable).
 * contours_out_dev and hist_out_dev may hold anything on entry and are written whole; inputs are read only.
 * GCS_EINVAL, with nothing launched: a NULL pointer (merges_dev may be NULL with K = 1), contours_out_dev == labels_dev, B outside
 * 1..65535, H or W outside 1..4096, K outside 1..4096, T outside 1..1000000, (B + 2T)(K + 1) >= 2^31.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
size_t gcs_region_tree_contours_workspace_bytes(int B, int K);
int gcs_region_tree_contours(const int32_t *labels_dev, const int32_t *merges_dev, const int32_t *alive_dev, int B, int H, int W, int K,
                             void *workspace_dev, int32_t *contours_out_dev, gcs_stream_t stream);
int gcs_boundary_sweep_resident(const int32_t *contours_dev, const void *truth_planes_dev, const int32_t *img_of_dev, int B, int T,
                                int H, int W, int K, uint32_t *hist_out_dev, gcs_stream_t stream);

/* ---- region metrics of every cut of the region tree at once (SPEC.md §16) --------------------------- */

/* Every group of a cut is a union of superpixels, so its row of the contingency table is the sum of its superpixels' rows. The leaf
 * tables leaf_hist_dev uint32 [T][K][n_truth_labels] (gcs_region_counts_batch[_u8] with n_segments = K on the label map of
 * gcs_region_tree) are made once from the pixels; for annotator map t of image b = img_of_dev[t] and every R = regions_dev[c] the
 * table of the cut is the leaf table with the first tau = max(0, alive_b - R) rows of image b's merge list applied (a row with
 * a < b, both reps at that step, adds row b into row a and empties row b; (-1, -1) rows and rows not of that form are skipped, as in
 * gcs_region_tree_contours), and the call writes what gcs_region_agreement writes for that table:
 *   sums_out_dev  uint64 [n_cuts][T][4] = { N, sum a_i^2, sum b_j^2, sum n_ij^2 }
 *   terms_out_dev double [n_cuts][T][4] = { sum a log2 a, sum b log2 b, sum n log2 n, sum_j b_j n*_j / u*_j }
 * through the same per-table reduction (float sums in an order fixed by the table indices alone, no float atomics: the same inputs
 * give the same bits from run to run; every cut is evaluated from its own table, no float is carried from cut to cut).
 *   gcs_region_sweep_workspace_bytes  host only: per map the row and column sums of the table in hand. 0 for a bad argument.
 *   gcs_region_sweep                  one launch on `stream`, a workgroup per annotator map. No allocation, no host synchronisation
 *                                     (capturable). leaf_hist_dev is CONSUMED: coarsened in place, it holds the table of the last cut
 *                                     afterwards. regions_dev int32 [n_cuts] must be strictly decreasing (the cuts are nested, the
 *                                     table only ever gets coarser); it is read on the device, so the call cannot check it: an entry
 *                                     that is not below its predecessor gets the sums of a coarser table, nothing is read or written
 *                                     out of range. R >= alive gives the leaf table itself. img_of_dev int32 [T]: an entry outside
 *                                     0 .. B-1 gets the leaf table at every cut. Workspace and outputs may hold anything on entry;
 *                                     every output element is written. With K = 1 merges_dev is not read and may be NULL.
 * GCS_EINVAL, with nothing launched: a NULL pointer (merges_dev may be NULL with K = 1), B outside 1..65535, T outside 1..1000000,
 * K outside 1..4096, n_truth_labels < 1, n_cuts outside 1..64, T * K * n_truth_labels >= 2^31.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
size_t gcs_region_sweep_workspace_bytes(int T, int K, int n_truth_labels, int n_cuts);
int gcs_region_sweep(uint32_t *leaf_hist_dev, const int32_t *merges_dev, const int32_t *alive_dev, const int32_t *img_of_dev,
                     const int32_t *regions_dev, int B, int T, int K, int n_truth_labels, int n_cuts, void *workspace_dev,
                     uint64_t *sums_out_dev, double *terms_out_dev, gcs_stream_t stream);

/* ---- the reference's region and shape metrics of every cut of the region tree at once (SPEC.md §17) --- */

/* The integer part of underseg, undersegNP, compactness and density of /root/reference/BSD_metrics/metrics.py:128-201 for the cut at
 * every R = regions_dev[c], from the inputs of gcs_region_sweep and the contour map of gcs_region_tree_contours; no pixel is
 * relabelled. The host finishes the floats (evaluate_gpu.sweep_reference_scores).
 *   gcs_region_sweep_under_workspace_bytes  host only: what gcs_region_sweep_workspace_bytes returns. 0 for a bad argument.
 *   gcs_region_sweep_under           gcs_region_sweep's walk over the same inputs under the same rules (one launch, a workgroup per
 *                                    annotator map, leaf_hist_dev CONSUMED, regions_dev strictly decreasing and read on the device: an
 *                                    entry that is not below its predecessor gets the sums of a coarser table, nothing is read or
 *                                    written out of range; an img_of_dev entry outside 0 .. B-1 gets the leaf table at every cut). Per
 *                                    cut and annotator map, from the table of the cut with a_i its row sums:
 *                                      under_out_dev uint64 [n_cuts][T][3] = { N = sum_i a_i, sum_i (a_i - max_j n_ij),
 *                                                                              sum_ij min(n_ij, a_i - n_ij) }
 *                                    sums_out_dev / terms_out_dev: both NULL, or both given: they then receive exactly what
 *                                    gcs_region_sweep writes for the same inputs, bit for bit, from the same walk; under_out_dev does not
 *                                    depend on them. No allocation, no host synchronisation (capturable). Workspace and outputs may hold
 *                                    anything on entry; every output element is written.
 *   gcs_cut_shapes_workspace_bytes   host only: per image uint32 bins [K][n_cuts + 1], area [K], bd [n_cuts + 1]. 0 for a bad argument.
 *   gcs_cut_shapes                   three launches on `stream` (zero; one pass over labels_dev and contours_dev; a workgroup per image).
 *                                    contours_dev int32 [B][H][W]: what gcs_region_tree_contours wrote for the same labels_dev,
 *                                    merges_dev and alive_dev. With tau_c = max(0, alive_b - regions_dev[c]) and rep(q) the smallest
 *                                    label of q's group in the cut c (the merge rows that count: as in gcs_region_sweep):
 *                                      area_out_dev     uint32 [n_cuts][B][K]  [c][b][r] = #{pixels whose label's rep is r}
 *                                      perim_out_dev    uint32 [n_cuts][B][K]  [c][b][r] = #{those on the image border or with U > tau_c}
 *                                      boundary_out_dev uint32 [n_cuts][B]     [c][b]    = #{pixels with U > tau_c}
 *                                    Labels that are absorbed or own no pixel have area 0 and perimeter 0. A pixel whose label is
 *                                    outside 0 .. K-1 is counted in no area and no perimeter; it counts in boundary_out_dev by its U.
 *                                    regions_dev int32 [n_cuts], strictly decreasing, read on the device: an entry that is not below its
 *                                    predecessor gets its predecessor's (coarser) cut, nothing is read or written out of range. No
 *                                    allocation, no host synchronisation (capturable). Workspace and outputs may hold anything on entry;
 *                                    every output element is written. With K = 1 merges_dev is not read and may be NULL.
 * GCS_EINVAL, with nothing launched: a NULL pointer (merges_dev may be NULL with K = 1; sums_out_dev and terms_out_dev may both be
 * NULL, not one of them), B outside 1..65535, T outside 1..1000000, H or W outside 1..4096, K outside 1..4096, n_truth_labels < 1,
 * n_cuts outside 1..64, T * K * n_truth_labels >= 2^31, B * H * W >= 2^31, B * (K * (n_cuts + 2) + n_cuts + 1) >= 2^31 (the
 * workspace counters; the outputs are fewer).
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
size_t gcs_region_sweep_under_workspace_bytes(int T, int K, int n_truth_labels, int n_cuts);
int gcs_region_sweep_under(uint32_t *leaf_hist_dev, const int32_t *merges_dev, const int32_t *alive_dev, const int32_t *img_of_dev,
                           const int32_t *regions_dev, int B, int T, int K, int n_truth_labels, int n_cuts, void *workspace_dev,
                           uint64_t *under_out_dev, uint64_t *sums_out_dev, double *terms_out_dev, gcs_stream_t stream);
size_t gcs_cut_shapes_workspace_bytes(int B, int K, int n_cuts);
int gcs_cut_shapes(const int32_t *labels_dev, const int32_t *contours_dev, const int32_t *merges_dev, const int32_t *alive_dev,
                   const int32_t *regions_dev, int B, int H, int W, int K, int n_cuts, void *workspace_dev, uint32_t *area_out_dev,
                   uint32_t *perim_out_dev, uint32_t *boundary_out_dev, gcs_stream_t stream);

/* ---- region descriptors and mean-colour maps of label maps and tree cuts (SPEC.md §19) --------------- */

/* A table row describes one region: C = 6 + D uint64 columns { n, sum y, sum x, sum R, sum G, sum B, sum x_0 .. sum x_{D-1} } and a box
 * int32 (y0, x0, y1, x1), inclusive, (H, W, -1, -1) for a row that owns no pixel. Sums add and boxes take min / max, so the rows of
 * every group of every cut follow from the rows of the leaves; exact integers, the same bits in any execution order.
 *   gcs_region_props        two launches on `stream` (fill; one pass over the pixels). labels_dev int32 [B][H][W]; img_dev uint8
 *                           [B][H][W][3] or NULL (the colour columns are then 0); feats_canonical_dev uint16 [B][D][H][W], NULL exactly
 *                           when D = 0. sums_out_dev uint64 [B][K][C], bbox_out_dev int32 [B][K][4]: written whole, they may hold
 *                           anything on entry. A pixel whose label is outside 0 .. K-1 is counted nowhere. K is bounded only by
 *                           B * K * C < 2^31 (the map of gcs_connected_regions has more than 4096 labels).
 *   gcs_region_props_cuts   one launch, a workgroup per image. sums_dev / bbox_dev: the leaf table of gcs_region_props at the K of the
 *                           tree; merges_dev / alive_dev as gcs_region_tree wrote them, or any list gcs_region_tree_contours accepts
 *                           (a row that is not (a < b, both reps at that step) is skipped); regions_dev int32 [n_cuts], decreasing,
 *                           read on the device: an entry that is not below its predecessor repeats its predecessor's cut.
 *                             group_out_dev int32 [n_cuts][B][K]  [c][b][q] = the label gcs_region_tree_cut at R_c gives the leaf label
 *                                                                 q (groups numbered by increasing rep), -1 for a leaf with n = 0
 *                             sums_out_dev  uint64 [B][Rsum][C], bbox_out_dev int32 [B][Rsum][4]: cut c owns the min(K, R_c) rows from
 *                                                                 row sum_{c' < c} min(K, R_c') on; row g = the sum and the box of the
 *                                                                 leaves with group g; the rows behind the cut's groups hold zeros
 *                                                                 and the empty box. Rsum = sum_c min(K, R_c) is the caller's: no
 *                                                                 row at or past Rsum is written, whatever regions_dev holds, and a
 *                                                                 group whose number is not below min(K, R_c) (a list that leaves
 *                                                                 more than R_c groups: no tree of `alive` leaves) has no row.
 *                           Every output element is written. With K = 1 merges_dev is not read and may be NULL.
 *   gcs_region_paint        one launch. rgb_out_dev uint8 [B][H][W][3]: the pixel of label l gets the mean colour of row g =
 *                           group_dev[b][l] (group_dev int32 [B][K], one cut's slice of group_out_dev) or, with group_dev NULL, of row
 *                           g = l (G must be K) of image b's G rows, which start at row b * row_stride of sums_dev (uint64 [..][C];
 *                           row_stride = G for a table [B][G][C]; one cut's rows inside sums_out_dev: sums_dev = the cut's first
 *                           row, row_stride = Rsum, no copy): floor((2 S + n) / (2 n)) per channel, at most 255. (0, 0, 0) where l
 *                           is outside 0 .. K-1, g outside 0 .. G-1 or n = 0.
 * No allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched: a NULL pointer (img_dev and group_dev may
 * be NULL; feats_canonical_dev with D = 0 and merges_dev with K = 1 must / may be), B outside 1..65535, H or W outside 1..4096, D
 * outside 0..207 (C outside 6..213), K < 1, K > 4096 in gcs_region_props_cuts, n_cuts outside 1..64, Rsum outside 1 .. n_cuts * K,
 * G < 1, G != K without group_dev, row_stride < G, B * K * C, B * Rsum * C, n_cuts * B * K, B * row_stride * C or B * K not below 2^31.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
int gcs_region_props(const int32_t *labels_dev, const uint8_t *img_dev, const uint16_t *feats_canonical_dev, int B, int H, int W, int D,
                     int K, uint64_t *sums_out_dev, int32_t *bbox_out_dev, gcs_stream_t stream);
int gcs_region_props_cuts(const uint64_t *sums_dev, const int32_t *bbox_dev, const int32_t *merges_dev, const int32_t *alive_dev,
                          const int32_t *regions_dev, int B, int H, int W, int K, int C, int n_cuts, int Rsum, int32_t *group_out_dev,
                          uint64_t *sums_out_dev, int32_t *bbox_out_dev, gcs_stream_t stream);
int gcs_region_paint(const int32_t *labels_dev, const int32_t *group_dev, const uint64_t *sums_dev, int B, int H, int W, int K, int G,
                     int C, int row_stride, uint8_t *rgb_out_dev, gcs_stream_t stream);

/* ---- region adjacency graph of label maps and tree cuts (SPEC.md §20) -------------------------------- */

/* The edges of a label map are the label pairs (a, b), a < b, both in 0 .. K-1, that meet across at least one horizontal or vertical
 * pixel pair (a crossing). An edge carries three uint64 columns { length, contrast, strength }: the number of crossings, the sum over
 * crossings of the squared colour difference (all three channels), and the sum over crossings of max(E(p), 0) + max(E(q), 0) for a
 * plane E. A table of an image is E_cap rows: count rows (a, b) / columns sorted by (a, b) ascending, then rows (-1, -1) / zeros;
 * an image with more than E_cap edges gets count = -1 and sentinel rows only (the other images are unaffected).
 *   gcs_region_adjacency       three launches on `stream` (fill; one pass over the pixels; sort and write). labels_dev int32 [B][H][W];
 *                              img_dev uint8 [B][H][W][3] or NULL (contrast = 0); strength_dev int32 [B][H][W] or NULL (strength = 0),
 *                              any int32, negatives count as 0. A pair with a label outside 0 .. K-1 is a crossing of nothing.
 *                              workspace_dev: gcs_region_adjacency_workspace_bytes(B, E_cap) bytes, 8-byte aligned.
 *                                edges_out_dev int32 [B][E_cap][2], vals_out_dev uint64 [B][E_cap][3], count_out_dev int32 [B]
 *   gcs_region_adjacency_cuts  three launches. edges_dev / vals_dev / count_dev: a leaf table at E_cap; group_dev int32 [n_cuts][B][K],
 *                              any values (a slice per cut of gcs_region_props_cuts' group_out_dev). Under cut c a leaf edge (a, b)
 *                              of image b' with g_a = group[c][b'][a], g_b = group[c][b'][b], both in 0 .. G-1 and different, adds
 *                              its columns into edge (min(g_a, g_b), max(g_a, g_b)); every other leaf edge (and a row whose labels
 *                              are outside 0 .. K-1) is dropped. count = -1 in gives count = -1 out, in every cut.
 *                              workspace_dev: gcs_region_adjacency_workspace_bytes(n_cuts * B, E_out_cap) bytes.
 *                                edges_out_dev int32 [n_cuts][B][E_out_cap][2], vals_out_dev uint64 [n_cuts][B][E_out_cap][3],
 *                                count_out_dev int32 [n_cuts][B], each table in the format above at E_out_cap
 * Every output element is written; outputs and workspace may hold anything on entry; inputs are read only. Exact integers and a final
 * sort: the same bits in any execution order. No allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched:
 * a NULL pointer (img_dev and strength_dev may be NULL), B outside 1..65535, H or W outside 1..4096, K < 1, G < 1, E_cap or E_out_cap
 * outside 1..16384, n_cuts outside 1..64, B * H * W, n_cuts * B * K, B * E_cap * 3 or the 8-byte words of the workspace not below
 * 2^31. gcs_region_adjacency_workspace_bytes returns 0 for B < 1 or E_cap outside 1..16384.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
size_t gcs_region_adjacency_workspace_bytes(int B, int E_cap);
int gcs_region_adjacency(const int32_t *labels_dev, const uint8_t *img_dev, const int32_t *strength_dev, int B, int H, int W, int K,
                         int E_cap, void *workspace_dev, int32_t *edges_out_dev, uint64_t *vals_out_dev, int32_t *count_out_dev,
                         gcs_stream_t stream);
int gcs_region_adjacency_cuts(const int32_t *edges_dev, const uint64_t *vals_dev, const int32_t *count_dev, const int32_t *group_dev,
                              int B, int K, int G, int E_cap, int n_cuts, int E_out_cap, void *workspace_dev, int32_t *edges_out_dev,
                              uint64_t *vals_out_dev, int32_t *count_out_dev, gcs_stream_t stream);

/* ---- texture-gradient edge map of the feature slab (SPEC.md §22) ---- */

/* grad_out_dev int32 [B][H][W]: G = floor(sqrt(E)), E = the sum over the bank's pyramid levels L of (DX_L >> 2L) + (DY_L >> 2L),
 * DX_L / DY_L = the squared central differences (clamped at the level's edge) of the level's planes at the level pixel
 * (y >> L, x >> L), summed over the planes. feats_slab_dev: the slab gcs_gabor_features (and gcs_smooth_features /
 * gcs_position_features) filled for B images of H x W and the bank (n_scales, n_orient = slots per scale), either slab format; every
 * level is read at its own resolution, the canonical tensor is never made. E < 2^41 for any 16-bit values and the root is exact.
 * One launch, no workspace, no allocation, no host synchronisation (capturable). grad_out_dev must not overlap the slab; it may
 * hold anything on entry and every element is written.
 * GCS_EINVAL, with nothing launched: a NULL pointer, B outside 1..65535, H or W outside 1..4096, a bank gcs_feature_slab_bytes refuses
 * or of more than 207 features.
 * Added within ABI 18: a new entry point changes no existing call, so GCS_ABI_VERSION did not move. */
int gcs_feature_gradient(const uint16_t *feats_slab_dev, int B, int H, int W, int n_scales, int n_orient, int32_t *grad_out_dev,
                         gcs_stream_t stream);

/* ---- region tree merged by boundary strength, from an edge table (SPEC.md §23) ---- */

/* The tree of SPEC.md §14 with the cost of an adjacent pair of groups cost(A, B) = floor(128 s / l), l and s = the length and the
 * strength of SPEC.md §20 summed over the leaf edges between A and B (256 times the mean of the strength plane over the pixels on
 * both sides of the common boundary; computed as 128 q + floor(128 r / l), s = q l + r; below 2^40 for s <= 2^32 l). Rounds, ties,
 * merge list and outputs are §14's, so gcs_region_tree_cut, gcs_region_tree_contours, the sweeps, gcs_region_props_cuts and
 * gcs_region_adjacency_cuts consume the result unchanged. On a merge the edges of the dead node move to the rep, edges that become
 * parallel add their l and s, the pair's own edge disappears. No features, no node statistics, no float.
 * Precondition: 1 <= l < 2^57 and s <= 2^32 l in every row and every sum of rows (every table of gcs_region_adjacency meets it).
 * Beyond it a cost no longer fits the 40 bits the picks give it and the merge order is undefined (every access stays in bounds,
 * every output element is still written); l = 0 counts as 1.
 *   gcs_region_tree_edges  one launch: a workgroup per image runs every round. edges_dev int32 [B][E_cap][2], vals_dev uint64
 *                          [B][E_cap][3] and count_dev int32 [B] are what gcs_region_adjacency wrote (the contrast column is not
 *                          read; a row with a label outside 0 .. K-1, with a = b or with a label that is not in use is ignored; rows
 *                          of the same pair add up). used_dev int32 [B][K]: not 0 = the label owns a pixel (a per-label pixel count
 *                          or the flags of gcs_label_used); alive = the number of such labels. A label in use without an edge never
 *                          merges. An image with count outside 0 .. E_cap (-1: more edges than E_cap) gets alive as defined, every row
 *                          (-1, -1) with cost 0; the other images are unaffected.
 *                          workspace_dev: gcs_region_tree_edges_workspace_bytes(B, K, E_cap) bytes, 8-byte aligned.
 *                            merges_out_dev int32 [B][K-1][2], costs_out_dev uint64 [B][K-1] (may be NULL), alive_out_dev int32 [B]
 *   gcs_label_used         one launch: used_out_dev int32 [B][K] = 1 where a pixel of labels_dev int32 [B][H][W] carries the label, else 0.
 * Every output element is written; outputs and workspace may hold anything on entry; inputs are read only. Integer adds and minima
 * only: the same bits in any execution order. No allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing
 * launched: a NULL pointer (costs_out_dev may be; merges_out_dev with K = 1 may be), B outside 1..65535, K outside 1..4096, E_cap
 * outside 1..16384, H or W outside 1..4096. gcs_region_tree_edges_workspace_bytes returns 0 for such a shape.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
size_t gcs_region_tree_edges_workspace_bytes(int B, int K, int E_cap);
int gcs_region_tree_edges(const int32_t *edges_dev, const uint64_t *vals_dev, const int32_t *count_dev, const int32_t *used_dev, int B,
                          int K, int E_cap, void *workspace_dev, int32_t *merges_out_dev, uint64_t *costs_out_dev,
                          int32_t *alive_out_dev, gcs_stream_t stream);
int gcs_label_used(const int32_t *labels_dev, int B, int H, int W, int K, int32_t *used_out_dev, gcs_stream_t stream);

/* ---- texton gradient of a label map, joined with an edge map (SPEC.md §24) ---- */

/* The chi-square distance between the label histograms of the two halves of a disc of radius r around every pixel, at n directions:
 * chi_i = the sum over the labels j of floor(64 (g_j - h_j)^2 / (g_j + h_j)) (bins with g_j + h_j = 0 add nothing), g_j / h_j = the
 * number of offsets of half A / half B of direction i whose pixel, mirrored at the image's border without repeating the edge pixel,
 * carries label j; TG = the maximum over i, dir = the lowest i that attains it (0 where TG = 0).
 *   gcs_texton_masks      host only: masks_out uint32 [n][2][2r+1], the half discs of SPEC.md §24 (side 0 = A, 1 = B; row dy + r,
 *                         bit dx + r). GCS_EINVAL: a NULL pointer, r outside 1..15, n outside 1..16.
 *   gcs_texton_gradient   one launch. labels_dev int32 [B][H][W]; a value outside 0 .. K-1 counts in no bin. masks_dev: a table laid
 *                         out as above, on the device; the kernel is exact for ANY table (bits above 2r of a row are ignored), also
 *                         one whose B is not the mirror image of A. grad_dev int32 [B][H][W] or NULL: given, out = floor(sqrt(TG *
 *                         G)) with the exact root of SPEC.md §22 (a negative G counts as 0); NULL, out = TG. out_dev int32
 *                         [B][H][W]; dir_out_dev uint8 [B][H][W] or NULL. TG <= 64 * 2 * 961 < 2^17.
 * Every output element is written (out_dev and dir_out_dev may hold anything on entry; dir_out_dev is B * H * W bytes exactly);
 * inputs are read only and must not overlap the outputs. No workspace, no allocation, no host
 * synchronisation (capturable). GCS_EINVAL, with nothing launched: a NULL pointer (grad_dev and dir_out_dev may be), B outside
 * 1..65535, H or W outside 1..4096, K outside 1..64, r outside 1..15, n outside 1..16.
 * Added within ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. */
int gcs_texton_masks(int r, int n, uint32_t *masks_out);
int gcs_texton_gradient(const int32_t *labels_dev, int B, int H, int W, int K, int r, int n, const uint32_t *masks_dev,
                        const int32_t *grad_dev, int32_t *out_dev, uint8_t *dir_out_dev, gcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GCS_H */
