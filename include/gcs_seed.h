/* gcs_seed.h - entry points of libgcs.so added beside include/gcs.h, include/gcs_cues.h, include/gcs_thin.h, include/gcs_match.h
 * and include/gcs_model.h: the same conventions (extern "C", raw device pointers plus a stream, no framework types, int return
 * codes of gcs.h, gcs_last_error for the message). Everything here belongs to ABI 18: new entry points change no existing call,
 * so GCS_ABI_VERSION did not move. A library built before this header existed does not export these symbols; the binding
 * (gabor_color_image_segmentation_amd/_lib.py, SEED_EXTENSIONS) sets up the ones it finds. */
#ifndef GCS_SEED_H
#define GCS_SEED_H

#include "gcs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- k-means++ seeding of the Lloyd stage from a feature slab (SPEC.md §29) ----
 *
 * The candidates of an image are the pixels (y_i, x_j), y_i = min(stride * i + stride / 2, H - 1) for i < ceil(H / stride), x_j
 * the same on W, in raster order of (i, j); the candidates of a set are those of its images in batch order (set s = image s when
 * n_sets == B, every image when n_sets == 1), n of them. With x_q the D features of candidate q (level L read at (y >> L, x >> L))
 * and d the 64-bit squared distance of SPEC.md §28, all draws in arithmetic mod 2^64:
 *     mix(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31
 *     u(r, t)    = mix(mix(seed) ^ (16 r + t))
 *     pick(u, T) = floor(u * T / 2^64)
 *   round 0:          q_0 = pick(u(0, 0), n), c_0 = x_{q_0}, m(q) = d(x_q, c_0)
 *   round r = 1..k-1: T = sum_q m(q).  T == 0: q_r = pick(u(r, 0), n).  Otherwise every trial t < trials draws
 *                     rho_t = pick(u(r, t), T), takes q_t = the smallest q whose inclusive prefix sum of m exceeds rho_t and
 *                     weighs it by pot_t = sum_q min(m(q), d(x_q, x_{q_t})); q_r = the q_t of the smallest pot_t (ties: the
 *                     lowest t).  Then c_r = x_{q_r} and m <- min(m, d(., c_r)).
 *
 *   feats_slab_dev      the slab gcs_gabor_features filled (either format)
 *   cent_out_dev        uint16 [n_sets][k][D], logical feature order (what gcs_kmeans_init writes): the seeds c_0 .. c_{k-1}
 *   picks_out_dev       int32 [n_sets][k]: the candidate indices q_0 .. q_{k-1}, or NULL
 *   potential_out_dev   int64 [n_sets]: sum_q m(q) after the last round, or NULL
 * A NULL optional output is never touched; every element of a given output is written (it may hold anything on entry). Inputs
 * are read only. One launch, one workgroup per set; no workspace, no allocation, no host synchronisation (capturable).
 * GCS_EINVAL, with nothing launched: a NULL slab or cent_out_dev; k outside 1..16; trials outside 1..8; a stride that is not a
 * power of two in 1..4096; n_sets neither 1 nor B; B outside 1..65535, H or W outside 1..4096, a bank gcs.h refuses or one of more
 * than 1536 features; n > 4096 (then sum_q m(q) <= 4096 * 1536 * 2^32 < 2^55). */
int gcs_kmeans_seed(const uint16_t *feats_slab_dev, int B, int H, int W, int n_scales, int n_orient, int k, int n_sets, int stride,
                    int trials, uint64_t seed, uint16_t *cent_out_dev, int32_t *picks_out_dev, int64_t *potential_out_dev,
                    gcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GCS_SEED_H */
