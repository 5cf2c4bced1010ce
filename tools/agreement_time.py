#!/usr/bin/env python3
"""Cost of the region agreement launch (gcs_region_agreement, SPEC.md §8) on the 24 packed BSD val maps, resident ground truth,
label maps as stored (k-means, k = 8) and as 4-connected regions (connectivity=True: 1 417 - 5 831 regions, tables at a capacity
of 8 192 segments). Warm-up, then timed calls of all_scores_batch_resident with agreement False / True per shape group.

Run it under `rocprofv3 --kernel-trace --stats -d <dir> -o run --` for the kernel times; it prints, per case, the host time per
call and the bytes the agreement kernel reads (the rows up to each image's largest label, two sweeps, 4 B per counter).
Usage: agreement_time.py [rows.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(reps=20, warm=3):
    import torch
    from gabor_color_image_segmentation_amd import _lib
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    val = np.load(os.path.join(gold, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    lib = _lib.load()
    ids = [str(i) for i in val["ids"]]
    rows = []
    for shape in sorted({val["labels_" + i].shape for i in ids}):
        group = [i for i in ids if val["labels_" + i].shape == shape]
        dt = pt.to_device(group)
        stored = torch.from_numpy(np.stack([val["labels_" + i].astype(np.int32) for i in group])).cuda()
        b, h, w = stored.shape
        scratch = torch.empty(lib.gcs_connected_scratch_bytes(b, h, w), dtype=torch.uint8, device=stored.device)
        conn = torch.empty_like(stored)
        _lib.check(lib.gcs_connected_regions(stored.data_ptr(), b, h, w, scratch.data_ptr(), conn.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "gcs_connected_regions")
        for kind, labs in (("stored", stored), ("connected", conn)):
            seg_max = labs.reshape(b, -1).max(dim=1).values.cpu().numpy().astype(np.int64)
            for agreement in (False, True):
                for _ in range(warm):
                    all_scores_batch_resident(labs, dt, agreement=agreement)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    all_scores_batch_resident(labs, dt, agreement=agreement)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / reps * 1e3
                cap = dt._out[0]
                read = int(2 * 4 * dt.stride * np.sum(seg_max[dt.img_of] + 1))
                row = {"shape": list(shape), "images": b, "maps": dt.t, "kind": kind, "agreement": agreement,
                       "capacity": cap, "stride": dt.stride, "max_regions": int(seg_max.max()) + 1,
                       "table_bytes": 4 * dt.t * cap * dt.stride, "agreement_read_bytes": read, "ms_per_call": ms}
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


if __name__ == "__main__":
    result = main()
    if len(sys.argv) > 1:                                   # optional: write the rows as JSON
        json.dump(result, open(sys.argv[1], "w"), indent=1)
