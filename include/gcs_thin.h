/* gcs_thin.h - entry points of libgcs.so added beside include/gcs.h and include/gcs_cues.h: the same conventions (extern "C",
 * raw device pointers plus a stream, no framework types, int return codes of gcs.h, gcs_last_error for the message). Everything
 * here belongs to ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. A library built before this
 * header existed does not export these symbols; the binding (gabor_color_image_segmentation_amd/_lib.py, THIN_EXTENSIONS) sets up
 * the ones it finds. */
#ifndef GCS_THIN_H
#define GCS_THIN_H

#include "gcs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- thin boundary maps: non-maximum suppression of an edge map along its direction map (SPEC.md §26) ----
 *
 * With V = max(E, 0), c(y, x) = V at coordinates clamped to the image, i = dir(p) and row i of the step table
 * (dy1, dx1, dy2, dx2, w1, w2, 0, 0), q1 = (dy1, dx1), q2 = (dy2, dx2), m = w1 + w2:
 *     plus  = w1 * c(p + q1) + w2 * c(p + q2)          minus = w1 * c(p - q1) + w2 * c(p - q2)
 *     T(p)  = V(p)  if  V(p) > 0  and  m * V(p) > minus  and  m * V(p) >= plus,   else 0;      T(p) = 0 where dir(p) >= n
 * in 64-bit products: the linear interpolation of V between the two ring neighbours the direction's normal passes between.
 *
 * gcs_thin_steps (host only) writes the table of n directions, int32 [n][8], from the normals of SPEC.md §24. */
int gcs_thin_steps(int n, int32_t *steps_out);

/*   edges_dev      int32 [B][H][W] (E: a map of gcs_texton_gradient or gcs_cue_gradient, or any other; negatives count as 0)
 *   dir_dev        uint8 [B][H][W] (the dir_out of those entry points)
 *   steps_dev      int32 [n][8] on the device: gcs_thin_steps' table, or any table with offsets in -1 .. 1, w >= 0 and
 *                  1 <= w1 + w2 <= 2048, for which the kernel is exact. An offset outside -1 .. 1 is the caller's error: it is
 *                  clamped to that range, and nothing is read out of bounds for any table.
 *   out_dev        int32 [B][H][W]: T
 * One launch; every element of out_dev is written (it may hold anything on entry); inputs are read only. No workspace, no
 * allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched: a NULL pointer; B outside 1..65535, H or W
 * outside 1..4096, n outside 1..16; an out_dev range that overlaps an input. */
int gcs_edge_thin(const int32_t *edges_dev, const uint8_t *dir_dev, int B, int H, int W, int n, const int32_t *steps_dev,
                  int32_t *out_dev, gcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GCS_THIN_H */
