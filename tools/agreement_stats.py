#!/usr/bin/env python3
"""Per-case kernel times of a `rocprofv3 --kernel-trace -f csv` run of tools/agreement_time.py.

    agreement_stats.py <run_kernel_trace.csv> <agreement_time rows.json>

Splits the trace into scoring calls (each starts with the resident scorer's zero_kernel), assigns them to the cases of the rows
file in order (warm-up calls first, then the timed ones), and prints per case the median time of the six kernels of
gcs_score_batch_resident and, with agreement, of region_agreement_kernel: the bytes it reads over that time, as a share of the
8 TB/s HBM peak, and as a share of the scorer's kernels. One JSON line per case.
"""
import csv
import json
import sys

import numpy as np

SCORER = ("zero_kernel", "bits_boundary_kernel<int>", "bits_dilate_kernel", "bits_counts_kernel", "region_counts_kernel",
          "region_reduce_kernel")
HBM_PEAK = 8.0e12


def main(trace, rows_json, warm=3, reps=20):
    with open(trace) as f:
        ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    calls, cur = [], None
    for t0, t1, name in ks:
        short = name[5:] if name.startswith("void ") else name
        short = short.split("(")[0]
        if short.startswith("zero_kernel"):
            cur = {"scorer": 0, "agreement": None}
            calls.append(cur)
        if cur is None:
            continue
        if short.startswith("region_agreement_kernel"):
            cur["agreement"] = t1 - t0
        elif short.startswith(SCORER):
            cur["scorer"] += t1 - t0
    rows = json.load(open(rows_json))
    per = warm + reps
    assert len(calls) == per * len(rows), (len(calls), len(rows))
    for k, row in enumerate(rows):
        timed = calls[k * per + warm:(k + 1) * per]
        out = {key: row[key] for key in ("shape", "maps", "kind", "agreement", "capacity", "stride", "max_regions")}
        out["scorer_us"] = float(np.median([c["scorer"] for c in timed])) / 1e3
        if row["agreement"]:
            ag = np.array([c["agreement"] for c in timed], np.float64)
            us = float(np.median(ag)) / 1e3
            out.update(agreement_us=us, agreement_min_us=float(ag.min()) / 1e3, agreement_max_us=float(ag.max()) / 1e3,
                       read_mb=row["agreement_read_bytes"] / 1e6,
                       read_tb_s=row["agreement_read_bytes"] / (us * 1e-6) / 1e12,
                       hbm_share=row["agreement_read_bytes"] / (us * 1e-6) / HBM_PEAK,
                       share_of_scorer=us / out["scorer_us"])
        print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
