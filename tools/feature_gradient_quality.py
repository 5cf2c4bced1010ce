#!/usr/bin/env python3
"""Quality table of SPEC.md §22 on the CPU: the texture-gradient edge map of the 24 val fixture images through the
restatements (the features of tests/position_ref.py: C oracle Gabor stage, tests/smooth_ref.py; tests/feature_gradient_ref.py)
scored by ``evaluate.edge_scores`` at ABSOLUTE thresholds:

  default   n_orient 6, no colour slot                       smoothing 0 and 1.0
  colour    n_orient 5, color_weight 1/8, chroma_gain 4      smoothing 0 and 1.0

Per setting: step = ceil((largest G of the 24 maps + 1) / 256), thresholds step (tau + 1) - 1 for tau = 0 .. 255 (the levels of
``evaluate_gpu.edge_sweep_resident`` on the whole set as one batch), ODS (the best mean F of one threshold) with its threshold, OIS
(the mean of every image's best F), and per image its best F with that threshold, its scores at the ODS threshold and the largest
value of its map (tests/test_feature_gradient.py reproduces the first six). The yardsticks are the contour-map rows of
profiles/contour_map_quality.json and the "components" rows of profiles/component_tree_quality.json. No GPU is used.
Usage: feature_gradient_quality.py [out.json] [n_images] [jobs]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

BANKS = dict(default=dict(n_orient=6, color_weight=0.0, chroma_gain=0),
             colour=dict(n_orient=5, color_weight=1 / 8, chroma_gain=4))
SMOOTHINGS = (0.0, 1.0)
LEVELS = 256


def setting_name(bank, smoothing):
    return f"{bank}_s{smoothing:g}"


def edge_map(img, bank, smoothing):
    """G of SPEC.md §22 of one image under a bank of BANKS: (H, W) int32."""
    import feature_gradient_ref as fg
    import position_ref as pr
    b = BANKS[bank]
    x = pr.features(img, b["color_weight"], b["chroma_gain"], 0, 4, b["n_orient"], smoothing=smoothing)
    return fg.gradient(x, 4, pr.n_slots(b["n_orient"], b["color_weight"], 0))


def thresholds(step):
    return [step * (tau + 1) - 1 for tau in range(LEVELS)]


def map_job(job):
    i, bank, smoothing = job
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    return job, edge_map(img, bank, smoothing)


def score_job(job):
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    i, name, g, step = job
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]
    sc = edge_scores(g, truth, thresholds(step))
    return i, name, {k: v.tolist() for k, v in sc.items()}


def main(out_path=None, n_images=24, jobs=4):
    from multiprocessing import Pool
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    ids = [str(i) for i in np.load(os.path.join(GOLD, "bsd_val_images.npz"))["ids"][:n_images]]
    runs = [(bank, s) for bank in BANKS for s in SMOOTHINGS]
    maps = {}
    with Pool(jobs) as pool:
        for (i, bank, s), g in pool.imap_unordered(map_job, [(i, bank, s) for bank, s in runs for i in ids]):
            maps.setdefault(setting_name(bank, s), {})[i] = g
            print("map", setting_name(bank, s), i, int(g.max()), flush=True)
        steps = {name: -(-(max(int(g.max()) for g in per.values()) + 1) // LEVELS) for name, per in maps.items()}
        table = {}
        for i, name, sc in pool.imap_unordered(score_job, [(i, name, maps[name][i], steps[name]) for name in maps for i in ids]):
            table.setdefault(name, {})[i] = sc
    rows, per_image, curves = [], {}, {}
    for bank, s in runs:
        name = setting_name(bank, s)
        th = thresholds(steps[name])
        f = [table[name][i]["fmeasure"] for i in ids]
        res = ods_ois(f, th)                                # (its "regions" axis is the threshold: ties go to the lowest)
        j = th.index(res["ODS_regions"])
        rows.append(dict(setting=name, bank=bank, smoothing=s, step=steps[name], ODS=res["ODS"], ODS_threshold=res["ODS_regions"],
                         OIS=res["OIS"],
                         recall_at_ODS=float(np.mean([table[name][i]["recall"][j] for i in ids])),
                         precision_at_ODS=float(np.mean([table[name][i]["precision"][j] for i in ids]))))
        print(json.dumps(rows[-1]), flush=True)
        curves[name] = np.mean(np.array(f), axis=0).tolist()
        per_image[name] = {i: dict(best_f=table[name][i]["fmeasure"][th.index(t)], best_threshold=t,
                                   f_at_ods=table[name][i]["fmeasure"][j], recall_at_ods=table[name][i]["recall"][j],
                                   precision_at_ods=table[name][i]["precision"][j], g_max=int(maps[name][i].max()))
                           for i, t in zip(ids, res["OIS_regions"])}
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(dict(images=len(ids), ids=ids, levels=LEVELS, banks=BANKS, smoothings=list(SMOOTHINGS), rows=rows,
                           per_image=per_image, mean_f_per_level=curves), fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 24,
         int(sys.argv[3]) if len(sys.argv) > 3 else 4)
