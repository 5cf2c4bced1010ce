#!/usr/bin/env python3
"""Quality table of SPEC.md §25 on the CPU: on the 24 val fixture images, through the restatements (the features and
the k-means map of tests/position_ref.py, tests/feature_gradient_ref.py, tests/texton_gradient_ref.py, tests/cue_gradient_ref.py),
the boundary scores (``evaluate.edge_scores`` at ABSOLUTE thresholds) of

  E     floor(sqrt(TG * G)) of §24, r = 8                               per bank
  Ep    E' = floor(sqrt(PB * G)) of §25                                 colour bank: every weight set of WEIGHTS at bins 8 and 16
                                                                        and r 8 and 12; default bank (R, G, B cues): bins 16, r 8
  PB    PB alone (no join with G)                                       colour bank, (0, 1, 1, 1), bins 16, r 8 and 12
  SM    floor(sqrt(S * G)), S = sum_c w_c max_i chi_{c,i}               colour bank, (2, 2, 1, 1), bins 16, r 8 and 12: the ablation
                                                                        of the per-direction join (not what §25 defines)

k = 8, no smoothing, n = 8 directions. Per map: step = ceil((largest value of the 24 maps + 1) / 256), thresholds step (tau + 1) - 1
for tau = 0 .. 255 (the levels of ``evaluate_gpu.edge_sweep_resident`` on the whole set as one batch), ODS with its threshold, OIS,
recall and precision at ODS. ``ranking_r_le_8``: the Ep rows of the colour bank with r <= 8 (the mask table stays §24's) by falling
ODS; the first is the default of ``cue_edges_device``. ``spread``: the largest ODS difference between two Ep rows that differ in
one of (bins, radius) only - what "neighbouring rows" differ by. For the rows of PER_IMAGE also per image its best F with that
threshold, its scores at the ODS threshold and the largest value of its map (tests/test_cue_gradient.py reproduces the first two).
The JSON keeps one row per line. No GPU is used.
Usage: cue_gradient_quality.py [out.json] [n_images] [jobs]
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
WEIGHTS = ((2, 2, 1, 1), (1, 1, 0, 0), (1, 1, 1, 1), (0, 1, 1, 1))
BINS = (8, 16)
RADII = (8, 12)
K = 8
N_DIRECTIONS = 8
LEVELS = 256
PER_IMAGE = ("Ep_colour_w2-2-1-1_b16_r8",)                    # rows whose per-image figures are kept


def row_name(kind, bank, weights=None, bins=None, r=None):
    if kind == "E":
        return f"E_{bank}_k{K}_r{r}"
    return f"{kind}_{bank}_w" + "-".join(str(v) for v in weights) + f"_b{bins}_r{r}"


def cue_inputs(img, bank):
    """What every row of one image under one bank is made of: (labels, I_0, G). I_0: the image the Gabor stage sees."""
    from oracle import c_oracle as co
    import colour_ref
    import feature_gradient_ref as fg
    import position_ref as pr
    b = BANKS[bank]
    h, w = img.shape[:2]
    x = pr.features(img, b["color_weight"], b["chroma_gain"], 0, 4, b["n_orient"], smoothing=0.0)
    g = fg.gradient(x, 4, pr.n_slots(b["n_orient"], b["color_weight"], 0))
    lab = co.kmeans(x.reshape(1, -1, h * w), K, 10)[0].reshape(h, w)
    i0 = colour_ref.opponent(img, b["chroma_gain"]) if b["chroma_gain"] else img
    return lab.astype(np.int32), np.ascontiguousarray(i0).astype(np.uint8), g


def image_maps(img, bank, only=None):
    """Every map of one image under one bank: {row name: (H, W) int32} (``only``: these rows). A cue's chi-squares are made once
    per (bins, r) and shared by the weight sets."""
    import cue_gradient_ref as cg
    import texton_gradient_ref as tg
    lab, i0, g = cue_inputs(img, bank)
    grid = [(nb, r) for nb in BINS for r in RADII] if bank == "colour" else [(16, 8)]
    out = {}
    want = lambda name: only is None or name in only
    for r in sorted({r for _, r in grid}):
        need_r = [nb for nb, rr in grid if rr == r]
        names = [row_name(kind, bank, wts, nb, r) for nb in need_r for wts in WEIGHTS for kind in ("Ep", "PB", "SM")]
        if not any(want(nm) for nm in names + [row_name("E", bank, r=r)]):
            continue
        chi_t = tg.chi_squares(lab, K, r, N_DIRECTIONS)
        if r == 8 and want(row_name("E", bank, r=r)):
            out[row_name("E", bank, r=r)] = tg.joined(chi_t.max(axis=0), g)
        for nb in need_r:
            chi = [chi_t] + [tg.chi_squares(cg.quantise(i0[..., c], nb), nb, r, N_DIRECTIONS) for c in range(3)]
            for wts in WEIGHTS:
                pb = sum(v * x for v, x in zip(wts, chi) if v).max(axis=0)
                if want(row_name("Ep", bank, wts, nb, r)):
                    out[row_name("Ep", bank, wts, nb, r)] = tg.joined(pb, g)
                if bank == "colour" and nb == 16 and wts == (0, 1, 1, 1) and want(row_name("PB", bank, wts, nb, r)):
                    out[row_name("PB", bank, wts, nb, r)] = pb.astype(np.int32)
                if bank == "colour" and nb == 16 and wts == (2, 2, 1, 1) and want(row_name("SM", bank, wts, nb, r)):
                    out[row_name("SM", bank, wts, nb, r)] = tg.joined(sum(v * x.max(axis=0) for v, x in zip(wts, chi) if v), g)
    return out


def thresholds(step):
    return [step * (tau + 1) - 1 for tau in range(LEVELS)]


def map_job(job):
    i, bank = job
    img = np.load(os.path.join(GOLD, "bsd_val_images.npz"))["img_" + i]
    return i, image_maps(img, bank)


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
        for i, per in pool.imap_unordered(map_job, [(i, bank) for bank in ("colour", "default") for i in ids]):
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
        kind, bank = name.split("_")[:2]
        th = thresholds(steps[name])
        f = [table[name][i]["fmeasure"] for i in ids]
        res = ods_ois(f, th)                                # (its "regions" axis is the threshold: ties go to the lowest)
        j = th.index(res["ODS_regions"])
        row = dict(row=name, map=kind, bank=bank, step=steps[name], ODS=res["ODS"], ODS_threshold=res["ODS_regions"], OIS=res["OIS"],
                   recall_at_ODS=float(np.mean([table[name][i]["recall"][j] for i in ids])),
                   precision_at_ODS=float(np.mean([table[name][i]["precision"][j] for i in ids])),
                   k=K, radius=int(name.rsplit("_r", 1)[1]), n_directions=N_DIRECTIONS)
        if kind != "E":
            row.update(weights=[int(v) for v in name.split("_w")[1].split("_")[0].split("-")], bins=int(name.split("_b")[1].split("_")[0]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if name in PER_IMAGE:
            per_image[name] = {i: dict(best_f=table[name][i]["fmeasure"][th.index(t)], best_threshold=t,
                                       f_at_ods=table[name][i]["fmeasure"][j], recall_at_ods=table[name][i]["recall"][j],
                                       precision_at_ods=table[name][i]["precision"][j], map_max=int(maps[name][i].max()))
                               for i, t in zip(ids, res["OIS_regions"])}
    ep = [r for r in rows if r["map"] == "Ep" and r["bank"] == "colour"]
    ranking = [r["row"] for r in sorted((r for r in ep if r["radius"] <= 8), key=lambda r: (-r["ODS"], r["row"]))]
    near = lambda a, b: a["weights"] == b["weights"] and ((a["bins"] != b["bins"]) + (a["radius"] != b["radius"])) == 1
    spread = max([abs(a["ODS"] - b["ODS"]) for a in ep for b in ep if near(a, b)] or [0.0])
    e_ods = next(r["ODS"] for r in rows if r["row"] == row_name("E", "colour", r=8))
    first = next(r for r in ep if r["row"] == ranking[0])
    if out_path:
        head = dict(images=len(ids), ids=ids, levels=LEVELS, banks=BANKS, k=K, weight_sets=[list(w) for w in WEIGHTS], bins=list(BINS),
                    radii=list(RADII), n_directions=N_DIRECTIONS, ranking_r_le_8=ranking, spread=spread,
                    first_minus_E=first["ODS"] - e_ods, first_beats_E_by_more_than_the_spread=bool(first["ODS"] - e_ods > spread))
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
