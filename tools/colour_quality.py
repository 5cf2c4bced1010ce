#!/usr/bin/env python3
"""Quality table of SPEC.md §11 on the CPU: the 24 val fixture images through the restatement
(tests/colour_ref.py, C oracle), k = 8, 10 passes, raw cluster labels, means of recall, precision, boundary F, PRI, VoI and
covering, and on how many images F rose against the default 4x6 bank. No GPU is used.
Usage: colour_quality.py [out.json] [n_images]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")


def main(out_path=None, n_images=24):
    import colour_ref as cr
    from merge_ref import merge_small_regions
    from gabor_color_image_segmentation_amd.evaluate import boundary_scores, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in val["ids"][:n_images]]

    def run(no, w, g, smoothing=0.0, merge=0):
        per = []
        for i in ids:
            lab = cr.segment(val["img_" + i], w, g, n_orient=no, smoothing=smoothing)
            if merge:
                lab = merge_small_regions(lab, merge)
            bs, ra = boundary_scores(lab, pt[i]), region_agreement(lab, pt[i])
            per.append([bs["recall"], bs["precision"], bs["fmeasure"], ra["PRI"], ra["VoI"], ra["covering"]])
        return np.array(per)

    base = run(6, 0.0, 0)
    rows = []

    def add(no, w, g, **kw):
        per = base if (no, w, g, kw) == (6, 0.0, 0, {}) else run(no, w, g, **kw)
        m = per.mean(axis=0)
        row = dict(n_orient=no, color_weight=w, chroma_gain=g, D=3 * 4 * (no + (1 if w else 0)), **kw,
                   recall=m[0], precision=m[1], fmeasure=m[2], PRI=m[3], VoI=m[4], covering=m[5],
                   f_up=int((per[:, 2] > base[:, 2]).sum()))
        rows.append(row)
        print(json.dumps(row), flush=True)

    add(6, 0.0, 0)
    for no in (5, 6):
        for w in (1 / 16, 1 / 8, 1 / 4):
            for g in (0, 1, 2, 4, 8):
                add(no, w, g)
    best = max(rows[1:], key=lambda r: r["fmeasure"])
    # the best F of the grid and the recommended setting of default cost, each with smoothing = 1 and with min_region_size = 64
    for no, w, g in dict.fromkeys([(best["n_orient"], best["color_weight"], best["chroma_gain"]), (5, 1 / 8, 4)]):
        add(no, w, g, smoothing=1.0)
        add(no, w, g, merge=64)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(images=len(ids), k=8, n_iter=10, rows=rows), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 24)
