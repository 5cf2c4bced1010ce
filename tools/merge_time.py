#!/usr/bin/env python3
"""Cost of the small-region merge post-pass (gcs_merge_small_regions, SPEC.md §9) beside gcs_connected_regions (§7), at batch
64 x 481x321: the 20 landscape val label maps of tests/golden/bsd_val_images.npz (k-means, k = 8, as stored), repeated to 64.

Per case: warm-up, then timed calls between two events on the stream (device time per call, scratch allocated once outside).
Run it under `rocprofv3 --kernel-trace --stats -f csv -d <dir> -o run --` for the per-kernel times. The cc_* kernels run in
both entries, so their rows in the stats file mix the cases; `merge_time.py --split <kernel_trace.csv>` cuts the trace into
calls (each starts with its init kernel) and prints, per case, the median time of each kernel per call, round by round.
Usage: merge_time.py [rows.json] [m ...]   (default m: 1 16 64 256 1024)
       merge_time.py --split run_kernel_trace.csv [split.json]
"""
import collections
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(sizes=(1, 16, 64, 256, 1024), batch=64, reps=20, warm=3):
    import torch
    from gabor_color_image_segmentation_amd import _lib
    val = np.load(os.path.join(ROOT, "tests", "golden", "bsd_val_images.npz"))
    maps = [val["labels_" + str(i)] for i in val["ids"] if val["labels_" + str(i)].shape == (321, 481)]
    labs = torch.from_numpy(np.stack([maps[j % len(maps)] for j in range(batch)]).astype(np.int32)).cuda()
    b, h, w = labs.shape
    lib = _lib.load()
    stream = torch.cuda.current_stream()
    out = torch.empty_like(labs)
    cases = [("connected", None)] + [("merge", int(m)) for m in sizes]
    rows = []
    for kind, m in cases:
        if kind == "connected":
            scratch = torch.empty(lib.gcs_connected_scratch_bytes(b, h, w), dtype=torch.uint8, device="cuda")
            call = lambda: lib.gcs_connected_regions(labs.data_ptr(), b, h, w, scratch.data_ptr(), out.data_ptr(),
                                                     stream.cuda_stream)
        else:
            scratch = torch.empty(lib.gcs_merge_scratch_bytes(b, h, w, m), dtype=torch.uint8, device="cuda")
            call = lambda: lib.gcs_merge_small_regions(labs.data_ptr(), b, h, w, m, scratch.data_ptr(), out.data_ptr(),
                                                       stream.cuda_stream)
        for _ in range(warm):
            _lib.check(call(), kind)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            _lib.check(call(), kind)
        e1.record()
        e1.synchronize()
        regions = (out.reshape(b, -1).max(dim=1).values + 1).cpu().numpy()
        row = {"case": kind, "min_size": m, "batch": b, "shape": [h, w], "scratch_bytes": scratch.numel(),
               "ms_per_call": e0.elapsed_time(e1) / reps, "regions_min": int(regions.min()), "regions_max": int(regions.max())}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del scratch
    return rows


def split(trace_csv, sizes=(1, 16, 64, 256, 1024), warm=3, reps=20):
    """Per case of main(): median per call of every kernel (round kernels per round; rounds >= 3 summed) from a kernel trace."""
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").strip()
        if name in ("cc_local_init_kernel", "mr_init_kernel"):
            cur = []
            calls.append(cur)
        if cur is not None and name.startswith(("cc_", "mr_")):
            cur.append((name, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = []
    for ci, case in enumerate(["connected"] + list(sizes)):
        grp = calls[ci * (warm + reps) + warm:(ci + 1) * (warm + reps)]
        per = collections.defaultdict(list)
        for g in grp:
            agg, rnd = collections.defaultdict(float), -1
            for name, t0, t1 in g:
                rnd += name == "mr_size_kernel"
                key = name if name in ("mr_init_kernel",) or not name.startswith("mr_") else \
                    "%s[r%s]" % (name, rnd if rnd < 3 else ">=3")
                agg[key] += (t1 - t0) / 1e3
            for k, v in agg.items():
                per[k].append(v)
        row = {"case": case, "launches": len(grp[0]),
               "median_span_us": round(float(np.median([(g[-1][2] - g[0][1]) / 1e3 for g in grp])), 1),
               "kernels_us": {k: round(float(np.median(v)), 1) for k, v in per.items()}}
        print(json.dumps(row))
        out.append(row)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--split":
        res = split(args[1])
        if len(args) > 2:
            json.dump(res, open(args[2], "w"), indent=1)
        sys.exit(0)
    path = args.pop(0) if args and args[0].endswith(".json") else None
    result = main(tuple(int(a) for a in args) or (1, 16, 64, 256, 1024))
    if path:
        json.dump(result, open(path, "w"), indent=1)
