#!/usr/bin/env python3
"""Quality table of SPEC.md §12 on the CPU: the 24 val fixture images through the restatement
(tests/position_ref.py, C oracle), k = 8, 10 passes, raw cluster labels unless a row says ``merge``; means of recall, precision,
boundary F, PRI, VoI and covering, on how many images F rose against the default 4x6 bank, and the range of connected regions of
the merged row. No GPU is used.
Usage: position_quality.py [out.json] [n_images]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

# (n_orient, color_weight, chroma_gain, position_weight, merge)
ROWS = [(6, 0.0, 0, 0, 0), (5, 0.0, 0, 4, 0), (5, 0.0, 0, 6, 0), (5, 1 / 8, 4, 0, 0), (4, 1 / 8, 4, 0, 0), (4, 1 / 8, 4, 4, 0),
        (4, 1 / 8, 4, 6, 0), (4, 1 / 8, 4, 8, 0), (4, 1 / 8, 4, 12, 0), (5, 1 / 8, 4, 6, 0), (4, 1 / 8, 4, 6, 64)]


def main(out_path=None, n_images=24):
    import position_ref as pr
    from merge_ref import merge_small_regions
    from gabor_color_image_segmentation_amd.evaluate import boundary_scores, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"][:n_images]]
    rows, base = [], None
    for no, w, g, mu, merge in ROWS:
        per, regions = [], []
        for i in ids:
            lab = pr.segment(val["img_" + i], w, g, mu, n_orient=no)
            if merge:
                lab = merge_small_regions(lab, merge)
                regions.append(int(lab.max()) + 1)
            bs, ra = boundary_scores(lab, pt[i]), region_agreement(lab, pt[i])
            per.append([bs["recall"], bs["precision"], bs["fmeasure"], ra["PRI"], ra["VoI"], ra["covering"]])
        per = np.array(per)
        base = per if base is None else base
        m = per.mean(axis=0)
        row = dict(n_orient=no, color_weight=w, chroma_gain=g, position_weight=mu, merge=merge,
                   D=3 * 4 * pr.n_slots(no, w, mu), recall=m[0], precision=m[1], fmeasure=m[2], PRI=m[3], VoI=m[4], covering=m[5],
                   f_up=int((per[:, 2] > base[:, 2]).sum()))
        if merge:
            row["regions_min"], row["regions_max"] = min(regions), max(regions)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(images=len(ids), k=8, n_iter=10, rows=rows), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 24)
