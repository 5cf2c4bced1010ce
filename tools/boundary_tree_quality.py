#!/usr/bin/env python3
"""Quality table of SPEC.md §23 on the CPU: the 24 val fixture images through the restatements (the features of
tests/position_ref.py, tests/superpixel_ref.py, the k-means of the C oracle, tests/component_tree_ref.py for the node maps,
tests/feature_gradient_ref.py for G, tests/boundary_tree_ref.py for the tree) on the colour bank (n_orient 5, color_weight 1/8,
chroma_gain 4), with and without smoothing = 1.0, 10 passes, on three node maps:

  components    300 superpixels, tree_nodes = "components"
  clusters_k16  tree_nodes = "clusters", k = 16
  clusters_k8   tree_nodes = "clusters", k = 8

each cut at R in {4, 6, 8, 12, 16, 32} from one tree per image, plus ODS / OIS of the tree's contour map over R = 1 .. 256. Means of
boundary recall, precision, F, PRI, VoI, covering and regions; per image the nodes, rounds and leaf edges. ``features=1`` adds the
same rows for merge_cost = "features" (the plain-Python tree of §14 takes a second per thousand nodes and round: the slow part).
``smoothing``: the values to run, comma-separated (default both); what an existing out.json holds for other values is kept, so the
two halves may be run one after the other. No GPU is used.
Usage: boundary_tree_quality.py [out.json] [n_images] [jobs] [features] [smoothing]
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
NODES = ("components", "clusters_k16", "clusters_k8")
SMOOTHING = (0.0, 1.0)
N_ITER, N_SUPERPIXELS = 10, 300
RS = (4, 6, 8, 12, 16, 32)
ODS_RS = list(range(1, 257))
KEYS = ("recall", "precision", "fmeasure", "PRI", "VoI", "covering", "regions")


def scores(lab, truth):
    from gabor_color_image_segmentation_amd.evaluate import metrics, region_agreement
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    m = metrics(None, lab, truth)
    m.set_metrics()
    got, ra = m.get_metrics(), region_agreement(lab, truth)
    got.update(PRI=ra["PRI"], VoI=ra["VoI"], covering=ra["covering"])
    return [float(got[k]) for k in KEYS]


def one_job(job):
    import boundary_tree_ref as bt
    import cluster_tree_ref as cl
    import component_tree_ref as ct
    import contour_map_ref as cm
    import position_ref as pr
    import region_tree_ref as rt
    import superpixel_ref as sr
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    i, smoothing, features = job
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]
    x = pr.features(img, BANK["color_weight"], BANK["chroma_gain"], 0, 4, BANK["n_orient"], smoothing)
    g = bt.gradient(x, 4, BANK["n_orient"] + 1)
    out = {}
    for nodes in NODES:
        if nodes == "components":
            lab = sr.superpixels(x, N_SUPERPIXELS, n_iter=N_ITER)
        else:
            lab = cl.kmeans_maps(x[None], int(nodes.split("_k")[1]), N_ITER)[0]
        n_map = ct.nodes(lab, 0)
        k = int(n_map.max()) + 1
        for cost in ("boundary", "features") if features else ("boundary",):
            info = {}
            if cost == "boundary":
                merges, _, alive = bt.build_tree(n_map, k, g, info=info)
            else:
                merges, _, alive = rt.build_tree(x, n_map, k, info=info)
            cuts = {r: scores(rt.cut(n_map, merges, alive, r), truth) for r in RS}
            u = cm.contour_map(n_map, merges, alive)
            f = edge_scores(u, truth, [max(0, alive - r) for r in ODS_RS])["fmeasure"]
            out[f"{nodes}/{cost}"] = dict(cuts=cuts, f_curve=[float(v) for v in f], nodes=int(alive), rounds=int(info["rounds"]),
                                          edges=int(info["edges"][0]) if cost == "boundary" and info["edges"] else None)
    return i, smoothing, out


def main():
    from concurrent.futures import ProcessPoolExecutor
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    ids = [str(i) for i in np.load(os.path.join(GOLD, "bsd_val_images.npz"))["ids"]]
    ids = ids[:int(sys.argv[2])] if len(sys.argv) > 2 else ids
    jobs_n = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    features = len(sys.argv) > 4 and sys.argv[4] not in ("0", "")
    smoothing = tuple(float(v) for v in sys.argv[5].split(",")) if len(sys.argv) > 5 else SMOOTHING
    jobs = [(i, s, features) for s in smoothing for i in ids]
    with ProcessPoolExecutor(jobs_n) as pool:
        done = {(i, s): o for i, s, o in pool.map(one_job, jobs)}
    doc = dict(images=len(ids), ids=ids, bank=BANK, n_iter=N_ITER, n_superpixels=N_SUPERPIXELS, regions=list(RS), ods_regions=[1, 256],
               measured="CPU restatements; no GPU", rows=[], contours=[], tree={})
    if out_path and os.path.exists(out_path):                # the rows of the smoothing values this run leaves out
        old = json.load(open(out_path))
        if old.get("ids") == ids:
            doc["rows"] = [r for r in old["rows"] if r["smoothing"] not in smoothing]
            doc["contours"] = [r for r in old["contours"] if r["smoothing"] not in smoothing]
            doc["tree"] = {k: v for k, v in old["tree"].items() if float(k.rsplit("=", 1)[1]) not in smoothing}
    for s in smoothing:
        for name in sorted(done[(ids[0], s)]):
            nodes, cost = name.split("/")
            per = [done[(i, s)][name] for i in ids]
            for r in RS:
                mean = np.array([p["cuts"][r] for p in per]).mean(axis=0)
                doc["rows"].append(dict(nodes=nodes, merge_cost=cost, smoothing=s, n_regions=r, **{k: float(v) for k, v in zip(KEYS, mean)}))
            oo = ods_ois([p["f_curve"] for p in per], ODS_RS)
            doc["contours"].append(dict(nodes=nodes, merge_cost=cost, smoothing=s, ODS=oo["ODS"], ODS_regions=oo["ODS_regions"], OIS=oo["OIS"],
                                        mean_nodes=float(np.mean([p["nodes"] for p in per])),
                                        mean_rounds=float(np.mean([p["rounds"] for p in per]))))
            doc["tree"][f"{name}/smoothing={s}"] = {i: dict(nodes=p["nodes"], rounds=p["rounds"], edges=p["edges"]) for i, p in zip(ids, per)}
    for c in doc["contours"]:
        print(c)
    for row in doc["rows"]:
        if row["n_regions"] == 8:
            print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
    if out_path:
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
