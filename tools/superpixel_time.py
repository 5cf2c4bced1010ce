#!/usr/bin/env python3
"""Time of the superpixel path (SPEC.md §13) at batch 64 x 481x321, n = 300, lambda = 576, colour bank (5, 1/8, 4; D = 72).

Every figure is the median of ``reps`` calls after ``warm`` warm-up calls, each call bracketed by two events on the stream, on
device-resident inputs:
  unpack_ms          gcs_features_unpack: slab -> the canonical (B, D, H, W) tensor the stage reads
  stage_ms           gcs_superpixel_segment: init + 10 assign passes + 9 updates (one call)
  step_ms            Segmenter(n_superpixels=300).segment_device: Gabor stage, unpack, stage
  kmeans_step_ms     the same batch and bank through the k = 8 Lloyd path (the plan without the argument), the yardstick
``pass_bytes`` = B * D * H * W * 2, the feature bytes one assign pass reads; ``pass_TBps`` divides them by stage_ms / n_iter (an upper
bound of the per-pass time: the accumulating passes read the planes twice, the second time from cache, and the update launches are
inside the span).
Usage: superpixel_time.py [out.json]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_TBPS = 8.0


def _median_ms(torch, fn, reps, warm):
    times = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main(batch=64, h=481, w=321, n=300, lam=576, reps=25, warm=4):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, superpixel_grid
    from gabor_color_image_segmentation_amd.segmenter import _step_features
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    bank = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
    imgs = torch.from_numpy(synthetic_batch(batch, h, w, seed=0)).cuda()
    seg = Segmenter(n_superpixels=n, spatial_weight=lam, **bank)
    ops, d = seg.ops, seg.bank.n_features
    s, ny, nx = superpixel_grid(h, w, n)
    ws = seg._workspace(batch, h, w, "per_image")
    _step_features(ops, seg._opt, ws, imgs, batch, h, w)
    canon, spws = ops.superpixel_buffers(batch, h, w, n)
    out = torch.empty((batch, h, w), dtype=torch.int32, device="cuda")
    res = dict(batch=batch, shape=[h, w], n_superpixels=n, spatial_weight=lam, S=s, grid=[ny, nx], D=d, n_iter=seg.n_iter, reps=reps,
               warm=warm, pass_bytes=batch * d * h * w * 2, slab_bytes=ws["feats"].numel())
    for name, fn in (("unpack", lambda: ops.features_unpack(ws["feats"], batch, h, w, out=canon)),
                     ("stage", lambda: ops.superpixels(canon, batch, h, w, ny, nx, lam, seg.n_iter, out, spws)),
                     ("step", lambda: seg.segment_device(imgs, out=out))):
        m = _median_ms(torch, fn, reps, warm)
        res.update({name + "_ms": m[0], name + "_ms_min": m[1], name + "_ms_max": m[2]})
    km = Segmenter(**bank)
    m = _median_ms(torch, lambda: km.segment_device(imgs, out=out), reps, warm)
    res.update(kmeans_step_ms=m[0], kmeans_step_ms_min=m[1], kmeans_step_ms_max=m[2])
    mpix = batch * h * w / 1e6
    res.update(unpack_share_of_unpack_plus_stage=res["unpack_ms"] / (res["unpack_ms"] + res["stage_ms"]),
               pass_TBps=res["pass_bytes"] / (res["stage_ms"] / seg.n_iter) / 1e9, hbm_peak_TBps=HBM_PEAK_TBPS,
               step_Mpix_per_s=mpix / res["step_ms"] * 1e3, kmeans_step_Mpix_per_s=mpix / res["kmeans_step_ms"] * 1e3,
               cpu_oracle_kmeans_Mpix_per_s=[0.64, 1.3])
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    r = main()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(r, f, indent=1)
