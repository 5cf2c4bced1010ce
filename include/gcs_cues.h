/* gcs_cues.h - entry points of libgcs.so added beside include/gcs.h: the same conventions (extern "C", raw device pointers
 * plus a stream, no framework types, int return codes of gcs.h, gcs_last_error for the message). Everything here belongs to
 * ABI 18: new entry points change no existing call, so GCS_ABI_VERSION did not move. A library built before this header existed
 * does not export these symbols; the binding (gabor_color_image_segmentation_amd/_lib.py, EXTENSIONS) sets up the ones it finds. */
#ifndef GCS_CUES_H
#define GCS_CUES_H

#include "gcs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- boundary map from a label map and three quantised image channels, joined per direction (SPEC.md §25) ----
 *
 * Four cue slots. Slot 0: labels_dev int32 [B][H][W], K bins, a value outside 0 .. K-1 counts in no bin (SPEC.md §24). Slots 1 - 3:
 * the three channels of img_dev uint8 [B][H][W][3] (interleaved), bin = value >> shift, 256 >> shift bins (shift 2 .. 7: 64 .. 2 bins).
 * With chi_{c,i} the chi-square distance of §24 of cue c at direction i (the same offsets, halves, mask table, mirror border and
 * per-bin floor) and integer weights 0 <= w_c <= 16, not all zero:
 *     P_i = sum over c of w_c * chi_{c,i}     PB = max over i of P_i     dir = the lowest i that attains it (0 where PB = 0)
 * PB <= 4 * 16 * 2^17 = 2^23. A cue of weight 0 is not read and its pointer may be NULL; w = (1, 0, 0, 0) is the texton gradient
 * of §24 bit for bit, dir included.
 *   masks_dev      the table of gcs_texton_masks, uint32 [n][2][2r+1], on the device; any table is exact (bits above 2r ignored).
 *   grad_dev       int32 [B][H][W] or NULL: given, out = floor(sqrt(PB * max(G, 0))) with the exact root of SPEC.md §22 (for
 *                  G < 2^20, §22's range, the product is below 2^43); NULL, out = PB.
 *   out_dev        int32 [B][H][W]; dir_out_dev uint8 [B][H][W] (B * H * W bytes exactly) or NULL.
 * One launch; every element of every given output is written (they may hold anything on entry); inputs are read only. No
 * workspace, no allocation, no host synchronisation (capturable). GCS_EINVAL, with nothing launched: masks_dev or out_dev NULL;
 * a cue of non-zero weight without its plane (labels_dev for w0, img_dev for w1 .. w3); every weight 0; a weight outside 0 .. 16;
 * shift outside 2 .. 7; B outside 1..65535, H or W outside 1..4096, K outside 1..64, r outside 1..15, n outside 1..16; an output
 * range that overlaps an input that is read, or the other output. */
int gcs_cue_gradient(const int32_t *labels_dev, const uint8_t *img_dev, int B, int H, int W, int K, int shift, int w0, int w1, int w2,
                     int w3, int r, int n, const uint32_t *masks_dev, const int32_t *grad_dev, int32_t *out_dev, uint8_t *dir_out_dev,
                     gcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GCS_CUES_H */
