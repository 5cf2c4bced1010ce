#!/usr/bin/env python3
"""Quality table of SPEC.md §21 on the CPU: the 24 val fixture images through the restatements (the features of
tests/position_ref.py, the k-means of the C oracle, tests/component_tree_ref.py, tests/region_tree_ref.py, composed by
tests/cluster_tree_ref.py) with ``tree_nodes="clusters"``, m = 0, 10 passes:

  colour    n_orient 5, color_weight 1/8, chroma_gain 4           k in {8, 12, 16}
  position  n_orient 4, the same colour slot, position_weight 6    k = 8   (the tree on those features too)

each cut at R in {4, 6, 8, 12, 16, 32} from one tree per image and setting. Means of boundary recall, precision, F, PRI, VoI,
covering and regions (``evaluate.metrics``: regions = max label + 1), per image and setting the components, nodes and rounds of the
tree and whether the K_cap guard triggered, whether every cut has exactly min(nodes, R) labels, and the per-image scores at R = 8
(tests/test_cluster_tree.py compares against them). The yardstick is the "components" rows of profiles/component_tree_quality.json.
No GPU is used. Usage: cluster_tree_quality.py [out.json] [n_images] [jobs]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

SETTINGS = dict(colour=dict(n_orient=5, color_weight=1 / 8, chroma_gain=4, position_weight=0),
                position=dict(n_orient=4, color_weight=1 / 8, chroma_gain=4, position_weight=6))
RUNS = (("colour", 8), ("colour", 12), ("colour", 16), ("position", 8))
N_ITER = 10
RS = (4, 6, 8, 12, 16, 32)
PER_IMAGE_R = 8
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


def one_job(job):
    import cluster_tree_ref as cl
    import position_ref as pr
    import region_tree_ref as rt
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    i, setting, k = job
    bank = SETTINGS[setting]
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]
    x = pr.features(img, bank["color_weight"], bank["chroma_gain"], bank["position_weight"], 4, bank["n_orient"])
    lab = cl.kmeans_maps(x[None], k, N_ITER)[0]
    info = {}
    n_map, merges, _, alive = cl.tree(x, lab, info=info)
    out, exact = {}, True
    for r in RS:
        cut = rt.cut(n_map, merges, alive, r)
        exact = exact and len(np.unique(cut)) == min(alive, r) == int(cut.max()) + 1
        out[r] = scores(cut, truth)
    return job, out, dict(components=info["components"], nodes=info["nodes"], min_size=info["min_size"], rounds=info["rounds"],
                          guard=bool(info["components"] > cl.K_CAP), exact_counts=bool(exact))


def main(out_path=None, n_images=24, jobs=4):
    from multiprocessing import Pool
    ids = [str(i) for i in np.load(os.path.join(GOLD, "bsd_val_images.npz"))["ids"][:n_images]]
    per, tree = {}, {}
    with Pool(jobs) as pool:
        for (i, setting, k), out, info in pool.imap_unordered(one_job, [(i, s, k) for s, k in RUNS for i in ids]):
            name = f"{setting}_k{k}"
            tree.setdefault(name, {})[i] = info
            per.setdefault(name, {})[i] = out
            print("done", name, i, info, flush=True)
    rows = []
    for setting, k in RUNS:
        name = f"{setting}_k{k}"
        for r in RS:
            vals = np.array([per[name][i][r] for i in ids])
            rows.append(dict(setting=setting, k=k, n_regions=r, **{key: float(v) for key, v in zip(KEYS, vals.mean(axis=0))},
                             nodes=float(np.mean([tree[name][i]["nodes"] for i in ids])),
                             rounds=float(np.mean([tree[name][i]["rounds"] for i in ids])),
                             exact_counts=all(tree[name][i]["exact_counts"] for i in ids),
                             guard_images=sum(tree[name][i]["guard"] for i in ids)))
            print(json.dumps(rows[-1]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(images=len(ids), ids=ids, n_iter=N_ITER, regions=list(RS), settings=SETTINGS,
                           per_image_n_regions=PER_IMAGE_R, rows=rows,
                           per_image={name: {i: {str(PER_IMAGE_R): dict(zip(KEYS, per[name][i][PER_IMAGE_R]))} for i in ids}
                                      for name in per},
                           tree={name: {i: tree[name][i] for i in ids} for name in tree}), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 24,
         int(sys.argv[3]) if len(sys.argv) > 3 else 4)
