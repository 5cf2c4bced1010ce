#!/usr/bin/env python3
"""Cost of the feature smoothing (gcs_smooth_features, SPEC.md §10) at batch 64 x 481x321 with the default 4x6 bank.

Per K: the Gabor stage fills a slab once; every timed call starts from a copy of it (the copy is outside the timed span) and is
bracketed by two events on the stream; the median over the calls is reported, with the bytes the two launches must move at
least (slab read without TOP runs + level planes written + level planes read + slab written) and that floor's time at
6.3 TB/s. Then the whole segment_device step with and without the smoothing. Run it under
`rocprofv3 --kernel-trace --stats -f csv -d <dir> -o run --` for the per-kernel times.
Usage: smooth_time.py [out.json] [K ...]   (default K: 1 3)
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBPS = 6.3


def main(ks=(1.0, 3.0), batch=64, h=321, w=481, reps=20, warm=3):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = torch.from_numpy(synthetic_batch(batch, h, w, seed=0)).cuda()
    rows = []
    for K in ks:
        seg = Segmenter(smoothing=K)
        ops, lib = seg.ops, seg.ops.lib
        bk = (seg.bank.n_scales, seg.bank.n_orient)
        slab = ops.feature_slab(batch, h, w)
        ops.gabor_features(imgs, slab)
        pristine = slab.clone()
        scratch = ops.smooth_scratch(batch, h, w)
        times = []
        for i in range(warm + reps):
            slab.copy_(pristine)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.smooth_features(slab, batch, h, w, scratch=scratch)
            e1.record()
            e1.synchronize()
            if i >= warm:
                times.append(e0.elapsed_time(e1))
        slab_b = lib.gcs_feature_slab_bytes(batch, h, w, *bk)
        floor_b = lib.gcs_feature_pass_bytes(batch, h, w, *bk) + 2 * scratch.numel() + slab_b
        ms = statistics.median(times)
        step = {}
        for name, s in (("step_K0", Segmenter()), ("step_K", seg)):
            out = torch.empty((batch, h, w), dtype=torch.int32, device="cuda")
            for _ in range(warm):
                s.segment_device(imgs, out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                s.segment_device(imgs, out=out)
            e1.record()
            e1.synchronize()
            step[name + "_ms"] = e0.elapsed_time(e1) / reps
        row = {"K": K, "batch": batch, "shape": [h, w], "radius": ops.smooth_radius.cpu().tolist(), "ms_per_call": ms,
               "ms_min": min(times), "ms_max": max(times), "slab_bytes": slab_b, "planes_bytes": scratch.numel(),
               "floor_bytes": floor_b, "floor_ms_at_6.3TBps": floor_b / COPY_TBPS / 1e9,
               "fraction_of_floor": floor_b / COPY_TBPS / 1e9 / ms, **step}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del slab, pristine, scratch
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    out = args.pop(0) if args and args[0].endswith(".json") else None
    rows = main(tuple(float(a) for a in args) or (1.0, 3.0))
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
