#!/usr/bin/env python3
"""Quality table of SPEC.md §24 on the CPU: on the 24 val fixture images, through the restatements (the features and
the k-means map of tests/position_ref.py, tests/feature_gradient_ref.py, tests/texton_gradient_ref.py), the boundary scores
(``evaluate.edge_scores`` at ABSOLUTE thresholds) of

  G    the texture gradient of §22                             per (bank, smoothing)
  TG   the texton gradient of the k-means map, n = 8           per (bank, smoothing, k, r), k in {8, 16}, r in {4, 8, 12}
  E    floor(sqrt(TG * G))                                     per (bank, smoothing, k, r)

for the banks of tools/feature_gradient_quality.py (default, colour) and smoothing 0 and 1.0. Per map: step = ceil((largest value
of the 24 maps + 1) / 256), thresholds step (tau + 1) - 1 for tau = 0 .. 255 (the levels of ``evaluate_gpu.edge_sweep_resident`` on
the whole set as one batch), ODS with its threshold and OIS; for the rows of PER_IMAGE (the recommended setting) also per image its
best F with that threshold, its scores at the ODS threshold and the largest value of its map (tests/test_texton_gradient.py
reproduces the first six). The JSON keeps one row per line. No GPU is used.
Usage: texton_gradient_quality.py [out.json] [n_images] [jobs]
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
KS = (8, 16)
RADII = (4, 8, 12)
N_DIRECTIONS = 8
LEVELS = 256
PER_IMAGE = ("E_colour_s0_k8_r8",)                            # rows whose per-image figures are kept


def row_name(kind, bank, smoothing, k=None, r=None):
    return f"{kind}_{bank}_s{smoothing:g}" + ("" if kind == "G" else f"_k{k}_r{r}")


def image_maps(img, bank, smoothing, ks=KS, radii=RADII):
    """Every map of one image under one (bank, smoothing): {row name: (H, W) int32}. The features are made once, the k-means map
    once per k."""
    from oracle import c_oracle as co
    import feature_gradient_ref as fg
    import position_ref as pr
    import texton_gradient_ref as tg
    b = BANKS[bank]
    x = pr.features(img, b["color_weight"], b["chroma_gain"], 0, 4, b["n_orient"], smoothing=smoothing)
    h, w = img.shape[:2]
    g = fg.gradient(x, 4, pr.n_slots(b["n_orient"], b["color_weight"], 0))
    out = {row_name("G", bank, smoothing): g}
    for k in ks:
        lab = co.kmeans(x.reshape(1, -1, h * w), k, 10)[0].reshape(h, w)       # position_ref.segment on features at hand
        for r in radii:
            t = tg.texton_gradient(lab, k, r, N_DIRECTIONS)[0]
            out[row_name("TG", bank, smoothing, k, r)] = t
            out[row_name("E", bank, smoothing, k, r)] = tg.joined(t, g)
    return out


def thresholds(step):
    return [step * (tau + 1) - 1 for tau in range(LEVELS)]


def map_job(job):
    i, bank, smoothing = job
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    return i, image_maps(img, bank, smoothing)


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
    maps = {}
    with Pool(jobs) as pool:
        for i, per in pool.imap_unordered(map_job, [(i, bank, s) for bank in BANKS for s in SMOOTHINGS for i in ids]):
            for name, m in per.items():
                maps.setdefault(name, {})[i] = m
            print("maps", i, sorted(per)[0], flush=True)
        steps = {name: -(-(max(int(m.max()) for m in per.values()) + 1) // LEVELS) for name, per in maps.items()}
        table = {}
        for i, name, sc in pool.imap_unordered(score_job, [(i, name, maps[name][i], steps[name]) for name in maps for i in ids],
                                               chunksize=8):
            table.setdefault(name, {})[i] = sc
    rows, per_image = [], {}
    for name in sorted(maps):
        kind, bank, s = name.split("_")[:3]
        th = thresholds(steps[name])
        f = [table[name][i]["fmeasure"] for i in ids]
        res = ods_ois(f, th)                                # (its "regions" axis is the threshold: ties go to the lowest)
        j = th.index(res["ODS_regions"])
        row = dict(row=name, map=kind, bank=bank, smoothing=float(s[1:]), step=steps[name], ODS=res["ODS"],
                   ODS_threshold=res["ODS_regions"], OIS=res["OIS"],
                   recall_at_ODS=float(np.mean([table[name][i]["recall"][j] for i in ids])),
                   precision_at_ODS=float(np.mean([table[name][i]["precision"][j] for i in ids])))
        if kind != "G":
            row.update(k=int(name.split("_")[3][1:]), radius=int(name.split("_")[4][1:]), n_directions=N_DIRECTIONS)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if name in PER_IMAGE:
            per_image[name] = {i: dict(best_f=table[name][i]["fmeasure"][th.index(t)], best_threshold=t,
                                       f_at_ods=table[name][i]["fmeasure"][j], recall_at_ods=table[name][i]["recall"][j],
                                       precision_at_ods=table[name][i]["precision"][j], map_max=int(maps[name][i].max()))
                               for i, t in zip(ids, res["OIS_regions"])}
    if out_path:
        head = dict(images=len(ids), ids=ids, levels=LEVELS, banks=BANKS, smoothings=list(SMOOTHINGS), ks=list(KS),
                    radii=list(RADII), n_directions=N_DIRECTIONS)
        line = lambda items: ",\n".join("  " + json.dumps(v) if k is None else "  %s: %s" % (json.dumps(k), json.dumps(v))
                                        for k, v in items)
        with open(out_path, "w") as fh:                     # one row, and one image, per line
            fh.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in head.items()))
            fh.write(' "rows": [\n' + line((None, r) for r in rows) + '\n ],\n "per_image": {\n')
            fh.write(",\n".join(' %s: {\n%s\n }' % (json.dumps(name), line(per.items())) for name, per in per_image.items()))
            fh.write("\n }\n}\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 24,
         int(sys.argv[3]) if len(sys.argv) > 3 else 4)
