#!/usr/bin/env python3
"""What the regulariser of SPEC.md §30 does to the scores and to the shape of the k-means map, on the CPU through the restatements
(tests/colour_ref.py for the features, the k-means of tools/kmeans_model_quality.py, tests/label_relax_ref.py for the sweeps,
tests/cluster_tree_ref.py for the tree), on the 24 val fixture images (landscape ones transposed to 481 x 321 with their annotator
maps), for the three plans of tools/kmeans_model_quality.py, per-image codebooks, n_iter = 10. No GPU is used.

    label_relax_quality.py [out.json] [n_images] [jobs]

(a) ``maps``, per plan: boundary F, PRI, VoI, covering and the number of 4-connected components (mean and max over the images) of
    the map as delivered (``base``) and after 1, 2, 4 and 8 sweeps at lambda in {1/64, 1/16, 1/4, 1, 4} over 4 and 8 neighbours
    (``l<q>_n<neighbours>_s<sweeps>``, q = round(256 lambda)), the mean number of labels every sweep changed, and on how many images
    F rose or fell against ``base``.
(b) ``tree``, for the colour bank at k = 8 and 16: tree_nodes = "clusters" cut at R = 8, without the option and with lambda = 1/4,
    4 sweeps, 8 neighbours: node count and rounds (mean and max) and the four scores of the cut."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kmeans_model_quality import GOLD, H, W, PLANS, _features, assign, distances  # noqa: E402

QS = (4, 16, 64, 256, 1024)                # round(256 lambda) of lambda = 1/64, 1/16, 1/4, 1, 4
SWEEPS = (1, 2, 4, 8)
NEIGHBOURS = (4, 8)
N_ITER = 10
TREE_SETTING = (64, 8, 4)                  # q, neighbours, sweeps of part (b)
NAMES = ["fmeasure", "PRI", "VoI", "covering"]


def kmeans(x, k, n_iter):
    """SPEC.md §4's schedule on x (P, D) int64 -> (labels of the last pass, its distances (P, k) int64)."""
    from oracle import spec_oracle as so
    c = so.kmeans_init(x, k)
    xf = x.astype(np.float64)
    x2 = (xf * xf).sum(axis=1)
    for t in range(n_iter):
        lab, _ = assign(xf, x2, c)
        if t < n_iter - 1:
            c = so.kmeans_update(x, lab, c)[0]
    return lab, distances(xf, x2, c)


def components(lab):
    from scipy import ndimage
    return int(sum(ndimage.label(lab == j)[1] for j in np.unique(lab)))


def image_job(job):
    """One image under one plan -> (image, plan, {setting: [F, PRI, VoI, covering, components]}, {l<q>_n<nb>: changed per sweep},
    {tree variant: [F, PRI, VoI, covering, nodes, rounds]})."""
    import cluster_tree_ref as cl
    import label_relax_ref as lr
    from gabor_color_image_segmentation_amd.evaluate import boundary_scores, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    i, plan = job
    bank, k = PLANS[plan]
    feats = _features(i, bank)                                  # (D, P)
    x = feats.T.astype(np.int64)
    lab, d = kmeans(x, k, N_ITER)
    cost = np.ascontiguousarray(d.T.reshape(k, H, W))
    lab = lab.reshape(H, W).astype(np.int64)
    m = int(d.min(axis=1).sum()) // (H * W)
    truth = [t if t.shape == (H, W) else np.ascontiguousarray(t.T) for t in PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]]

    def scores(mp):
        mp = np.ascontiguousarray(mp, np.int32)
        bs, ra = boundary_scores(mp, truth), region_agreement(mp, truth)
        return [bs["fmeasure"], ra["PRI"], ra["VoI"], ra["covering"]]
    rows, changed, kept = {"base": scores(lab) + [components(lab)]}, {}, None
    for q in QS:
        beta = (q * m) >> 8
        for nb in NEIGHBOURS:
            cur, seen = lab, []
            for s in range(1, max(SWEEPS) + 1):
                cur, ch, _ = lr.relax(cost, cur, beta, 1, nb)
                seen.append(ch[0])
                if s in SWEEPS:
                    rows["l%d_n%d_s%d" % (q, nb, s)] = scores(cur) + [components(cur)]
                    if (q, nb, s) == TREE_SETTING:
                        kept = cur
            changed["l%d_n%d" % (q, nb)] = seen
    tree = {}
    if plan.startswith("colour"):
        canon = feats.reshape(-1, H, W).astype(np.int64)
        for name, mp in (("plain", lab), ("regularised", kept)):
            info = {}
            cut = cl.regions(canon, mp.astype(np.int32), 8, 0, info=info)
            tree[name] = scores(cut) + [info["nodes"], info["rounds"]]
    return i, plan, rows, changed, tree


def main(out_path=None, n_images=24, jobs=8):
    from multiprocessing import Pool
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"][:n_images]]
    res = dict(images=len(ids), shape=[H, W], n_iter=N_ITER, q=list(QS), sweeps=list(SWEEPS), neighbours=list(NEIGHBOURS),
               tree_setting=dict(q=TREE_SETTING[0], neighbours=TREE_SETTING[1], sweeps=TREE_SETTING[2], n_regions=8),
               plans={n: dict(bank=b, k=k) for n, (b, k) in PLANS.items()}, maps={}, tree={})
    with Pool(jobs) as pool:
        got = pool.map(image_job, [(i, plan) for plan in PLANS for i in ids], chunksize=1)
    for plan in PLANS:
        mine = [g for g in got if g[1] == plan]
        base_f = np.array([g[2]["base"][0] for g in mine])
        table = {}
        for setting in mine[0][2]:
            v = np.array([g[2][setting] for g in mine], np.float64)             # (images, 5)
            table[setting] = dict(zip(NAMES, v[:, :4].mean(axis=0).tolist()), components_mean=float(v[:, 4].mean()),
                                  components_max=int(v[:, 4].max()), f_up=int((v[:, 0] > base_f).sum()),
                                  f_down=int((v[:, 0] < base_f).sum()))
        res["maps"][plan] = dict(settings=table, changed_per_sweep={
            n: np.array([g[3][n] for g in mine], np.float64).mean(axis=0).tolist() for n in mine[0][3]})
        best = max((n for n in table if n != "base"), key=lambda n: table[n]["fmeasure"])
        print(json.dumps({plan: dict(base=table["base"], best_f=best, best=table[best])}), flush=True)
        if mine[0][4]:
            res["tree"][plan] = {}
            for name in mine[0][4]:
                v = np.array([g[4][name] for g in mine], np.float64)            # (images, 6)
                res["tree"][plan][name] = dict(zip(NAMES, v[:, :4].mean(axis=0).tolist()), nodes_mean=float(v[:, 4].mean()),
                                               nodes_max=int(v[:, 4].max()), rounds_mean=float(v[:, 5].mean()),
                                               rounds_max=int(v[:, 5].max()))
            print(json.dumps({plan: res["tree"][plan]}), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(a[0] if a else None, int(a[1]) if len(a) > 1 else 24, int(a[2]) if len(a) > 2 else 8)
