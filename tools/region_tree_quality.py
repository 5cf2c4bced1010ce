#!/usr/bin/env python3
"""Quality table of SPEC.md §14 on the CPU: the 24 val fixture images through the restatements
(tests/region_tree_ref.py on the superpixels of tests/superpixel_ref.py and the features of tests/position_ref.py, C oracle) at the
recommended superpixel setting (colour bank: n_orient 5, color_weight 1/8, chroma_gain 4; n = 300, lambda = 576, 10 passes), cut at
R in {4, 6, 8, 12, 16, 32}, each scored as the raw cut and after ``min_region_size = S * S // 4`` (tests/merge_ref.py). The first
row is the k-means setting README recommends (n_orient 4, colour, position_weight 6, k = 8), the baseline. Means of boundary
recall, precision, F, PRI, VoI, covering and regions (``evaluate.metrics``: regions = max label + 1); the per-image scores at
R = 8 are kept beside the means (tests/test_region_tree.py and tests/test_gpu_region_tree.py compare against them), and the
rounds the tree took per image. No GPU is used.
Usage: region_tree_quality.py [out.json] [n_images] [jobs]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

BANK = dict(n_orient=5, color_weight=1 / 8, chroma_gain=4)
N, LAMBDA, N_ITER = 300, 576, 10
RS = (4, 6, 8, 12, 16, 32)
PER_IMAGE_R = 8
KMEANS = dict(n_orient=4, color_weight=1 / 8, chroma_gain=4, position_weight=6, k=8)
KEYS = ("recall", "precision", "fmeasure", "underseg", "undersegNP", "compactness", "density", "PRI", "VoI", "covering", "regions",
        "used")


def scores(lab, truth):
    from gabor_color_image_segmentation_amd.evaluate import metrics, region_agreement
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    m = metrics(None, lab, truth)
    m.set_metrics()
    got, ra = m.get_metrics(), region_agreement(lab, truth)
    got.update(PRI=ra["PRI"], VoI=ra["VoI"], covering=ra["covering"], used=len(np.unique(lab)))
    return [float(got[k]) for k in KEYS]


def one_image(i):
    import position_ref as pr
    import region_tree_ref as rt
    import superpixel_ref as sr
    from merge_ref import merge_small_regions
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]
    out = {"kmeans": scores(pr.segment(img, KMEANS["color_weight"], KMEANS["chroma_gain"], KMEANS["position_weight"], k=KMEANS["k"],
                                       n_orient=KMEANS["n_orient"]), truth)}
    x = pr.features(img, BANK["color_weight"], BANK["chroma_gain"], 0, 4, BANK["n_orient"])
    s, ny, nx = sr.grid(img.shape[0], img.shape[1], N)
    lab = sr.superpixels(x, N, LAMBDA, N_ITER)
    info = {}
    merges, _, alive = rt.build_tree(x, lab, ny * nx, info)
    for r in RS:
        cut = rt.cut(lab, merges, alive, r)
        out[(r, 0)] = scores(cut, truth)
        out[(r, 1)] = scores(merge_small_regions(cut, s * s // 4), truth)
    return i, out, dict(alive=int(alive), rounds=info["rounds"])


def main(out_path=None, n_images=24, jobs=4):
    from multiprocessing import Pool
    ids = [str(i) for i in np.load(os.path.join(GOLD, "bsd_val_images.npz"))["ids"][:n_images]]
    per, tree = {}, {}
    with Pool(jobs) as pool:
        for i, out, info in pool.imap_unordered(one_image, ids):
            tree[i] = info
            for key, val in out.items():
                per.setdefault(key, {})[i] = val
            print("done", i, info, flush=True)

    def mean_row(key, **head):
        vals = np.array([per[key][i] for i in ids])
        head.update({k: float(v) for k, v in zip(KEYS, vals.mean(axis=0))})
        print(json.dumps(head), flush=True)
        return head

    rows = [mean_row("kmeans", setting="kmeans", **KMEANS)]
    per_image = {}
    for r in RS:
        for merge in (0, 1):
            rows.append(mean_row((r, merge), setting="region_tree", n_regions=r, merge=merge))
            if r == PER_IMAGE_R:
                per_image["merged" if merge else "raw"] = {i: dict(zip(KEYS, per[(r, merge)][i])) for i in ids}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(images=len(ids), ids=ids, n_iter=N_ITER, merge_rule="min_region_size = S * S // 4",
                           superpixels=dict(bank="colour", n_superpixels=N, spatial_weight=LAMBDA, **BANK), kmeans_baseline=KMEANS,
                           per_image_n_regions=PER_IMAGE_R, rows=rows, per_image=per_image,
                           tree={i: tree[i] for i in ids}), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 24,
         int(sys.argv[3]) if len(sys.argv) > 3 else 4)
