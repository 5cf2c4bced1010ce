#!/usr/bin/env python3
"""Quality table of SPEC.md §18 on the CPU: the 24 val fixture images through the restatements (the features of
tests/position_ref.py, the superpixels of tests/superpixel_ref.py, tests/region_tree_ref.py, tests/merge_ref.py,
tests/component_tree_ref.py) at the recommended superpixel setting (colour bank: n_orient 5, color_weight 1/8, chroma_gain 4; n = 300,
lambda = 576, 10 passes), cut at R in {4, 6, 8, 12, 16, 32} in both modes of ``tree_nodes``:

  superpixels        the tree on the raw §13 map, the raw cut              ("today")
  superpixels+post   that cut followed by ``min_region_size = S * S // 4``  ("today + post")
  components         the tree on the connected regions of the §13 map (m = 0), cut at R: the delivered map

Means of boundary recall, precision, F, PRI, VoI, covering and regions (``evaluate.metrics``: regions = max label + 1), the best R
of the new mode by mean F, per image the node count and the rounds of both trees, whether every cut of the new mode has exactly
min(nodes, R) labels, and the new mode's per-image scores at R = 8 (tests/test_component_tree.py compares against them). No GPU is used.
Usage: component_tree_quality.py [out.json] [n_images] [jobs]
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
MODES = ("superpixels", "superpixels+post", "components")
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
    import component_tree_ref as ct
    import position_ref as pr
    import region_tree_ref as rt
    import superpixel_ref as sr
    from merge_ref import merge_small_regions
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]
    x = pr.features(img, BANK["color_weight"], BANK["chroma_gain"], 0, 4, BANK["n_orient"])
    s, ny, nx = sr.grid(img.shape[0], img.shape[1], N)
    lab = sr.superpixels(x, N, LAMBDA, N_ITER)
    old, new, out = {}, {}, {}
    merges, _, alive = rt.build_tree(x, lab, ny * nx, old)
    n_map, n_merges, _, n_alive = ct.tree(x, lab, info=new)
    exact = True
    for r in RS:
        cut = rt.cut(lab, merges, alive, r)
        out[(r, MODES[0])] = scores(cut, truth)
        out[(r, MODES[1])] = scores(merge_small_regions(cut, s * s // 4), truth)
        cut = rt.cut(n_map, n_merges, n_alive, r)
        exact = exact and len(np.unique(cut)) == min(n_alive, r) == int(cut.max()) + 1
        out[(r, MODES[2])] = scores(cut, truth)
    return i, out, dict(alive=int(alive), rounds=old["rounds"], components=new["components"], nodes=new["nodes"],
                        min_size=new["min_size"], component_rounds=new["rounds"], exact_counts=bool(exact))


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
    rows = []
    for r in RS:
        for mode in MODES:
            vals = np.array([per[(r, mode)][i] for i in ids])
            rows.append(dict(n_regions=r, tree_nodes=mode, **{k: float(v) for k, v in zip(KEYS, vals.mean(axis=0))}))
            print(json.dumps(rows[-1]), flush=True)
    best = max((row for row in rows if row["tree_nodes"] == "components"), key=lambda row: row["fmeasure"])["n_regions"]
    print("best R of tree_nodes = components by mean F:", best, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(images=len(ids), ids=ids, n_iter=N_ITER, post_rule="min_region_size = S * S // 4",
                           superpixels=dict(bank="colour", n_superpixels=N, spatial_weight=LAMBDA, **BANK),
                           per_image_n_regions=PER_IMAGE_R, best_n_regions=best, rows=rows,
                           per_image={i: dict(zip(KEYS, per[(PER_IMAGE_R, "components")][i])) for i in ids},
                           tree={i: tree[i] for i in ids}), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 24,
         int(sys.argv[3]) if len(sys.argv) > 3 else 4)
