/* gcs_match.h - entry points of libgcs.so added beside include/gcs.h, include/gcs_cues.h and include/gcs_thin.h: the same
 * conventions (extern "C", raw device pointers plus a stream, no framework types, int return codes of gcs.h, gcs_last_error for
 * the message). Everything here belongs to ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. A
 * library built before this header existed does not export these symbols; the binding
 * (gabor_color_image_segmentation_amd/_lib.py, MATCH_EXTENSIONS) sets up the ones it finds. */
#ifndef GCS_MATCH_H
#define GCS_MATCH_H

#include "gcs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one-to-one matching counts of a level map against annotator contours, every level at once (SPEC.md §27) ----
 *
 * With q' = clamp(q, 0, levels), P_tau = {q' > tau} and Q_t the thin contour of annotator map t (SPEC.md §26: a pixel whose right
 * or lower neighbour carries another label), M[t][tau] is the cardinality of a maximum matching between P_tau of image
 * img_of[t] and Q_t, a pair (p, p + (dy, dx)) being allowed iff (dy, dx) is a row of the offset table.
 *
 * gcs_match_offsets (host only) writes the offsets with dy^2 + dx^2 <= d2 in row-major order (dy ascending, then dx) as int32
 * [n][2] and their number to *n_out: 1 at d2 = 0, 5 at 1, 61 at 18, 69 at 20, 505 at 160. offsets_out needs room for 512 rows
 * at most. GCS_EINVAL: a NULL pointer, d2 outside 0..160. */
int gcs_match_offsets(int d2, int32_t *offsets_out, int *n_out);

/*   maps_dev       the annotator maps [T][H][W], uint8 (is_u8 != 0) or 16-bit (is_u8 == 0): DeviceTruth's layout
 *   thin_out_dev   uint8 [T][H][W]: 1 on Q_t, else 0
 *   counts_out_dev int32 [T]: |Q_t|
 * Two launches; every element of both outputs is written (they may hold anything on entry); the maps are read only. No
 * workspace, no allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched: a NULL pointer; T outside
 * 1..65535, H or W outside 1..4096; an output range that overlaps the maps or the other output. */
int gcs_truth_thin(const void *maps_dev, int T, int H, int W, int is_u8, uint8_t *thin_out_dev, int32_t *counts_out_dev,
                   gcs_stream_t stream);

/* Bytes of gcs_edge_match's workspace; 0 for arguments that call would refuse. */
size_t gcs_edge_match_bytes(int B, int T, int H, int W, int cap);

/*   q_dev          int32 [B][H][W], read as clamp(q, 0, levels)
 *   thin_dev       uint8 [T][H][W] (thin_out_dev of gcs_truth_thin; any non-zero byte is a contour pixel)
 *   img_of_dev     int32 [T]: the image of map t. A map whose entry is outside 0..B-1 gets -1 in its whole row of matched.
 *   offsets_dev    int32 [n_off][2] on the device: gcs_match_offsets' table, or any table of 1..512 rows (dy, dx), for which the
 *                  kernel is exact; a neighbour outside the image is no neighbour, whatever the offset.
 *   cap            capacity of the search stack of a map, in contour pixels. A search pushes each contour pixel at most once, so
 *                  cap >= max_t |Q_t| + 1 is never exceeded. A map whose search would push more than cap pixels gets -1 in its
 *                  whole row of matched and stops there; nothing is ever written out of bounds.
 *   workspace_dev  gcs_edge_match_bytes(B, T, H, W, cap) bytes, 256-byte aligned; it may hold anything on entry. On return its
 *                  first 16 T bytes hold, per map, uint32 {search steps, 64-lane probes, deepest stack, failed searches}, of the
 *                  pixels that were searched from.
 *   matched_dev    int32 [T][levels]: M[t][tau]
 *   above_dev      int32 [B][levels]: #{q'_b > tau}
 * Seven launches on `stream`: the histogram's zeroing, a histogram of the levels per image, its scan (above), a counting sort of
 * the pixels with q' >= 1 by descending level, the state of every map from thin_dev, the marks of the pixels that have a contour
 * pixel in reach (the others are never searched from), and the matcher: one 64-lane workgroup per map adds the pixels
 * level by level, one alternating-path search per pixel, the contour pixels a failed search visited being dead from then on
 * (SPEC.md §27 says why that is exact). Every element of matched_dev and above_dev is written; inputs are read only. No
 * allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched: a NULL pointer; B or T outside 1..65535,
 * H or W outside 1..4096, levels outside 1..256, n_off outside 1..512, cap outside 1..16777217; a workspace that is not 256-byte
 * aligned; an output or workspace range that overlaps an input or another of them. */
int gcs_edge_match(const int32_t *q_dev, const uint8_t *thin_dev, const int32_t *img_of_dev, int B, int T, int H, int W, int levels,
                   const int32_t *offsets_dev, int n_off, int cap, void *workspace_dev, int32_t *matched_dev, int32_t *above_dev,
                   gcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GCS_MATCH_H */
