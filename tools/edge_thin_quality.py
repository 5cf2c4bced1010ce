#!/usr/bin/env python3
"""Quality table of SPEC.md §26 on the CPU: on the 24 val fixture images, through the restatements (the inputs of
tools/cue_gradient_quality.py, tests/texton_gradient_ref.py, tests/cue_gradient_ref.py, tests/edge_thin_ref.py), four maps of the
colour bank at k = 8, r = 8, n = 8, 16 bins, weights (2, 2, 1, 1):

  Ep_thick   E' = floor(sqrt(PB * G)) of §25 as delivered          Ep_thin   E' thinned along its direction map (§26)
  E_thick    E  = floor(sqrt(TG * G)) of §24 as delivered          E_thin    E thinned along its direction map

each under two metrics: the thick-boundary metric of §22 (``evaluate.edge_scores``, 5 x 5 dilation, many-to-one) at the 256 levels
of the sweep, and the one-to-one matching metric of §26 (``evaluate.match_scores``, annotator means) at 32 of them (tau = 8 j + 3).
Per map: step = ceil((largest value of the 24 maps + 1) / 256), thresholds step (tau + 1) - 1; ODS with its threshold, OIS, recall
and precision at ODS, per metric. ``thin_minus_thick``: the difference of the matching ODS, for E' and for E - the acceptance
condition of §26 is that both are positive. For the two E' rows also per image the matching scores at the row's ODS threshold and
at the image's best threshold, and the largest value of its map (tests/test_edge_thin.py reproduces the first three images).
The JSON keeps one row per line. No GPU is used.
Usage: edge_thin_quality.py [out.json] [n_images] [jobs]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")

BANK = "colour"
K, RADIUS, N_DIRECTIONS, BINS, WEIGHTS = 8, 8, 8, 16, (2, 2, 1, 1)
LEVELS = 256
MATCH_TAUS = tuple(8 * j + 3 for j in range(32))
ROWS = ("Ep_thick", "Ep_thin", "E_thick", "E_thin")
PER_IMAGE = ("Ep_thick", "Ep_thin")


def image_maps(img):
    """The four maps of one image: {row: (H, W) int32}."""
    import cue_gradient_quality as inputs
    import cue_gradient_ref as cg
    import edge_thin_ref as et
    import texton_gradient_ref as tg
    lab, i0, g = inputs.cue_inputs(img, BANK)
    cache = {}
    pb, pb_dir = cg.cue_gradient(lab, i0, K, BINS, WEIGHTS, RADIUS, N_DIRECTIONS, cache=cache)
    t, t_dir = cg.cue_gradient(lab, None, K, BINS, (1, 0, 0, 0), RADIUS, N_DIRECTIONS, cache=cache)     # §24 bit for bit (§25)
    ep, e = tg.joined(pb, g), tg.joined(t, g)
    return {"Ep_thick": ep, "Ep_thin": et.thin_fast(ep, pb_dir, N_DIRECTIONS),
            "E_thick": e, "E_thin": et.thin_fast(e, t_dir, N_DIRECTIONS)}


def thresholds(step, taus=range(LEVELS)):
    return [step * (tau + 1) - 1 for tau in taus]


def map_job(i):
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    return i, image_maps(img)


def score_job(job):
    from gabor_color_image_segmentation_amd.evaluate import edge_scores, match_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    i, name, g, step = job
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]
    thick = edge_scores(g, truth, thresholds(step))
    match = match_scores(g, truth, thresholds(step, MATCH_TAUS))
    return i, name, {k: v.tolist() for k, v in thick.items()}, {k: v.tolist() for k, v in match.items()}


def summary(table, ids, th):
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    res = ods_ois([table[i]["fmeasure"] for i in ids], th)      # (its "regions" axis is the threshold: ties go to the lowest)
    j = th.index(res["ODS_regions"])
    return res, j, dict(ODS=res["ODS"], ODS_threshold=res["ODS_regions"], OIS=res["OIS"],
                        recall_at_ODS=float(np.mean([table[i]["recall"][j] for i in ids])),
                        precision_at_ODS=float(np.mean([table[i]["precision"][j] for i in ids])))


def main(out_path=None, n_images=24, jobs=4):
    from multiprocessing import Pool
    ids = [str(i) for i in np.load(os.path.join(GOLD, "bsd_val_images.npz"))["ids"][:n_images]]
    maps, thick, match = {}, {}, {}
    with Pool(jobs) as pool:
        for i, per in pool.imap_unordered(map_job, ids):
            for name, m in per.items():
                maps.setdefault(name, {})[i] = m
            print("maps", i, flush=True)
        steps = {name: -(-(max(int(m.max()) for m in per.values()) + 1) // LEVELS) for name, per in maps.items()}
        for i, name, a, b in pool.imap_unordered(score_job, [(i, name, maps[name][i], steps[name]) for name in ROWS for i in ids]):
            thick.setdefault(name, {})[i] = a
            match.setdefault(name, {})[i] = b
    rows, per_image = [], {}
    for name in ROWS:
        kind, form = name.split("_")
        _, _, by_thick = summary(thick[name], ids, thresholds(steps[name]))
        th = thresholds(steps[name], MATCH_TAUS)
        res, j, by_match = summary(match[name], ids, th)
        row = dict(row=name, map=kind, form=form, step=steps[name], thick=by_thick, match=by_match, k=K, radius=RADIUS,
                   n_directions=N_DIRECTIONS, weights=list(WEIGHTS) if kind == "Ep" else [1, 0, 0, 0], bins=BINS)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if name in PER_IMAGE:
            t = match[name]
            per_image[name] = {i: dict(best_f=t[i]["fmeasure"][th.index(best)], best_threshold=best, f_at_ods=t[i]["fmeasure"][j],
                                       recall_at_ods=t[i]["recall"][j], precision_at_ods=t[i]["precision"][j],
                                       map_max=int(maps[name][i].max()))
                               for i, best in zip(ids, res["OIS_regions"])}
    by = {r["row"]: r for r in rows}
    gain = {kind: by[kind + "_thin"]["match"]["ODS"] - by[kind + "_thick"]["match"]["ODS"] for kind in ("Ep", "E")}
    if out_path:
        head = dict(images=len(ids), ids=ids, levels=LEVELS, match_taus=list(MATCH_TAUS), bank=BANK, k=K, radius=RADIUS,
                    n_directions=N_DIRECTIONS, bins=BINS, weights=list(WEIGHTS), thin_minus_thick=gain,
                    thin_above_thick=bool(min(gain.values()) > 0))
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
