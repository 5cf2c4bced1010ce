#!/usr/bin/env python3
"""The reference's driver loop (/root/reference/BSD_metrics/script.py:19-38) with the MI355X segmenter
in the slot, on the packed BSD fixtures (no JPEG / .mat decoding, no /root/reference needed):

    load image -> labels = segment(img) -> load ground truth -> metrics -> print

Iterates an explicit sorted id list (script.py:21-22 takes os.listdir order, which is not stable).
`--gpu-scoring`: the label map never leaves the device; gcs_boundary_counts / gcs_region_counts produce the integer
tables and the same numbers are printed (evaluate_gpu.all_scores_device).
`--val`: the data-set form of the same loop on the 24 packed images of the BSD500 val split: batches per image shape through
the device path, the batched GPU scorer against the packed ground truth of all 500 ids, mean recall / precision / F beside the
numbers the reference's own metrics class gave for the same label maps (tests/golden/bsd_val_scores.json).
`--val --agreement`: also the region metrics PRI / VoI / covering (SPEC.md §8) of the same maps, as segmented and as
4-connected regions, with their means beside the scikit-learn / scikit-image numbers (tests/golden/region_agreement_golden.json).
`--min-region-size N[,N...]`: the same 24 images through Segmenter(min_region_size=N) (SPEC.md §9: regions below N pixels
merged into their largest neighbour), one row per N of mean recall / precision / F / PRI / VoI / covering and the range of
regions per image, all from the GPU path.
`--smoothing K[,K...]`: the same through Segmenter(smoothing=K) (SPEC.md §10: the Gabor magnitudes smoothed with a Gaussian of
K half-periods before k-means); with `--min-region-size N` as well, every K is combined with every N.
`--color-weight W[,W...]`, `--chroma-gain G[,G...]`, `--n-orient N`: the same table through Segmenter(n_orient=N, color_weight=W,
chroma_gain=G) (SPEC.md §11: a low-pass slot per scale, clustering in opponent colours), every W with every G (and every K and m);
`--val --n-orient 5 --color-weight 0.125 --chroma-gain 4` is the recommended colour setting.
`--position-weight MU[,MU...]`: the same table through Segmenter(position_weight=MU) (SPEC.md §12: a coordinate slot per scale),
every MU with every other option; `--n-orient 4 --color-weight 0.125 --chroma-gain 4 --position-weight 6` is the recommended
setting.
`--superpixels N [--spatial-weight L]`: the same 24 images through Segmenter(n_superpixels=N, spatial_weight=L) (SPEC.md §13:
grid-local k-means instead of the Lloyd stage) with the other options of the table (`--n-orient`, `--color-weight`, `--chroma-gain`,
`--min-region-size`, taken as single values; `--min-region-size auto` = S * S // 4 per image shape): mean boundary recall, underseg,
undersegNP, compactness and regions from the GPU path; `--superpixels 300 --n-orient 5 --color-weight 0.125 --chroma-gain 4
--min-region-size auto` is the recommended setting.
`--regions R[,R...]` beside `--superpixels`: the superpixels merged to R regions (SPEC.md §14); one tree per batch
(`Segmenter.region_tree_device`), one cut per R (`cut_regions_device`), `--min-region-size` applied to every cut: a row per R with mean
boundary recall, precision, F, PRI, VoI, covering and regions; `--superpixels 300 --regions 8 --n-orient 5 --color-weight 0.125
--chroma-gain 4` is the recommended setting.
`--regions R[,R...] --sweep`: boundary recall, precision and F of every listed R from ONE contour map per batch (SPEC.md §15:
`Segmenter.contour_map_device`) and one pass over it (`evaluate_gpu.boundary_sweep_resident`) instead of a cut and a scorer call per R,
then OIS (every image at its own best R) and ODS (one R for the whole set) over the list; the map describes the raw cuts, so
`--min-region-size` is not applied.
`--regions R[,R...] --sweep --agreement`: PRI, VoI and covering columns beside them, from the same tree (SPEC.md §16: the contingency
tables of the superpixels once per batch, the table of every cut from the merge list, `evaluate_gpu.region_sweep_resident`), and the ODS /
OIS of each of the three (VoI: the lowest). Without `--sweep` the per-cut path above stays: `--min-region-size` needs the label maps.
`--regions R[,R...] --sweep --reference-metrics`: the reference's other columns beside them - underseg, undersegNP, compactness,
density and regions - of every listed R from the same tree and contour map (SPEC.md §17: `evaluate_gpu.under_sweep_resident`,
`cut_shapes_device`, `sweep_reference_scores`); combines with `--agreement`.
`--tree-nodes components` beside `--regions` (with or without `--sweep`): the tree on the connected regions of the superpixel map
(SPEC.md §18: `Segmenter(tree_nodes="components")`): every cut at R is R connected regions, `--min-region-size` goes into the node
map instead of running behind every cut, and the sweeps describe the delivered maps.
`--merge-cost boundary` beside `--regions` (any `--tree-nodes`): the tree merges the pair of regions whose common boundary is weakest
on average in the texture-gradient map (SPEC.md §23: `Segmenter(merge_cost="boundary")`); the default, `features`, is the tree of §14.
`--tree-nodes clusters [--k K]` beside `--regions` (with or without `--sweep`; no `--superpixels`): the tree on the connected regions
of the k-means map of K clusters (SPEC.md §21: `Segmenter(tree_nodes="clusters", k=K)`, default K = 16), the rest as for `components`
(the n and lambda columns print 0): `--tree-nodes clusters --k 16 --regions 4,6,8,12,16,32 --sweep --agreement --reference-metrics
--n-orient 5 --color-weight 0.125 --chroma-gain 4` prints the mode's table of `DESIGN.md` §7 from one tree per batch.
`--edges [--smoothing K] [--n-orient N --color-weight W --chroma-gain G]`: the texture-gradient edge map of the 24 images (SPEC.md
§22: `Segmenter.edges_device`, no clustering) swept at 256 absolute thresholds (`evaluate_gpu.edge_sweep_resident`, one step for the
whole set): ODS with its threshold and OIS of the map.
`--texton-edges [--radius R] [--k K] [--smoothing S] [--n-orient N --color-weight W --chroma-gain G]`: the same sweep for the three maps
of SPEC.md §24 on the plan's k-means map (default R = 8, K = 8, 8 directions): E = floor(sqrt(TG * G))
(`Segmenter.texton_edges_device`), TG alone (`joined=False`) and G (`edges_device`), one row each.
`--cue-edges [--bins N] [--weights a,b,c,d] [--radius R] [--k K] [--n-orient N --color-weight W --chroma-gain G]`: the same sweep for
the maps of SPEC.md §25 (defaults: 16 bins, weights 2,2,1,1 for textons and the three channels, R = 8, K = 8, 8 directions):
E' = floor(sqrt(PB * G)) (`Segmenter.cue_edges_device`), PB alone (`joined=False`) and, beside them, E of §24; with a first weight of 0 no
k-means runs. `--cue-edges --n-orient 5 --color-weight 0.125 --chroma-gain 4` prints the default row of `DESIGN.md` §7.
`--thin` beside `--texton-edges` / `--cue-edges`: the maps thinned along their direction map (SPEC.md §26; G of §22 has none and stays).
`--match [N]` beside them: two more columns, the ODS / OIS of the one-to-one matching score of §26 (`evaluate.match_scores`, on the
host, minutes for the 24 images) at N of the 256 thresholds (32 when N is left out).
`--match-device` beside them: two more columns, the ODS / OIS of the same score at ALL 256 thresholds from the device matcher (SPEC.md
§27: `evaluate_gpu.edge_match_resident`, seconds); with `--match N` as well, a line per map says whether the two paths give the same
floats at the N thresholds.
`--regularize LAMBDA [--regularize-sweeps N --regularize-neighbours 4|8]` beside the label tables (`--min-region-size`, `--smoothing`,
the colour and position options) and beside `--regions ... --tree-nodes clusters`: the same rows through
Segmenter(regularize=LAMBDA, ...) (SPEC.md §30: ICM sweeps of a Potts prior on the k-means map, in front of every later stage).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _regularize_kw():
    """The plan options of SPEC.md §30 from the command line: none without `--regularize`."""
    arg = lambda name, kind: {name.strip("-").replace("-", "_"): kind(sys.argv[sys.argv.index(name) + 1])} if name in sys.argv else {}
    if "--regularize" not in sys.argv:
        return {}
    return dict(**arg("--regularize", float), **arg("--regularize-sweeps", int), **arg("--regularize-neighbours", int))

from gabor_color_image_segmentation_amd import segment                      # noqa: E402  (script.py:11)
from gabor_color_image_segmentation_amd.evaluate import metrics             # noqa: E402  (script.py:14)
from gabor_color_image_segmentation_amd.groundtruth import load_packed      # noqa: E402  (script.py:13)

def val_split(agreement=False):
    import json
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    ref = json.load(open(os.path.join(gold, "bsd_val_scores.json")))["per_id"]
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    seg = Segmenter()
    ids = [str(i) for i in pack["ids"]]
    rows = {}
    agree = {"stored": {}, "connected": {}}
    for shape in sorted({pack["img_" + i].shape[:2] for i in ids}):
        group = [i for i in ids if pack["img_" + i].shape[:2] == shape]
        labels = seg.segment_device(torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda())
        # ground truth resident on the device in the scorer's form (prepared once per shape group; a data-set loop keeps it)
        dt = truth.to_device(group)
        for i, s in zip(group, all_scores_batch_device(labels, dt, n_segments=seg.k, agreement=agreement)):
            rows[i] = s
            if agreement:
                agree["stored"][i] = s
            print("%-8s Regions: %d Recall: %.4f Precision: %.4f F-measure: %.4f   (reference class: %.4f)"
                  % (i, s["regions"], s["recall"], s["precision"], s["fmeasure"], ref[i]["v2"]["fmeasure"]))
        if agreement:                                    # the same maps as connected regions (Segmenter(connectivity=True))
            conn = Segmenter(connectivity=True).segment_device(
                torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda())
            for i, s in zip(group, all_scores_batch_device(conn, dt, agreement=True)):
                agree["connected"][i] = s
    for key in ("recall", "precision", "fmeasure"):
        print("mean %-9s %.4f   reference class on the same maps: %.4f" % (
            key, float(np.mean([rows[i][key] for i in ids])), float(np.mean([ref[i]["v2"][key] for i in ids]))))
    if agreement:
        gold_agr = json.load(open(os.path.join(gold, "region_agreement_golden.json")))
        for kind in ("stored", "connected"):
            for key, gkey in (("PRI", "PRI"), ("VoI", "VoI"), ("covering", "covering_mean")):
                print("mean %-8s %-9s %.6f   scikit-learn / scikit-image on the same maps: %.6f" % (
                    key, kind, float(np.mean([agree[kind][i][key] for i in ids])),
                    float(np.mean([gold_agr["val/%s/%s" % (i, kind)][gkey] for i in ids]))))


def merge_table(sizes, smoothings=(0.0,), weights=(0.0,), gains=(0,), n_orient=None, positions=(0,)):
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    groups = [[i for i in ids if pack["img_" + i].shape[:2] == shape] for shape in sorted({pack["img_" + i].shape[:2] for i in ids})]
    keys = ("recall", "precision", "fmeasure", "PRI", "VoI", "covering")
    position = tuple(positions) != (0,)                                                    # the mu column, when asked for
    colour = n_orient is not None or tuple(weights) != (0.0,) or tuple(gains) != (0,) or position    # the colour columns, when asked for
    n_orient = 6 if n_orient is None else n_orient
    print(("| n_orient | w | g " if colour else "") + ("| mu " if position else "") + "| K | m | R | P | F | PRI | VoI | covering | regions / image |")
    print(("|---|---|---" if colour else "") + ("|---" if position else "") + "|---|---|---|---|---|---|---|---|---|")
    for cw, g, mu, K, m in [(cw, g, mu, K, m) for cw in weights for g in gains for mu in positions for K in smoothings for m in sizes]:
        seg = Segmenter(n_orient=n_orient, min_region_size=m, smoothing=K, color_weight=cw, chroma_gain=g, position_weight=mu,
                        **_regularize_kw())
        rows = []
        for group in groups:
            labels = seg.segment_device(torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda())
            rows += all_scores_batch_device(labels, truth.to_device(group), agreement=True)
        mean = [float(np.mean([r[k] for r in rows])) for k in keys]
        regions = [r["regions"] for r in rows]
        print(("| %d | %g | %d " % (n_orient, cw, g) if colour else "") + ("| %d " % mu if position else "") +
              "| %g | %d | %s | %d - %d |" % (K, m, " | ".join("%.4f" % v for v in mean), min(regions), max(regions)))


def superpixel_row(n, lam, n_orient, cw, g, merge):
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, superpixel_grid
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    rows = []
    for shape in sorted({pack["img_" + i].shape[:2] for i in ids}):
        group = [i for i in ids if pack["img_" + i].shape[:2] == shape]
        m = superpixel_grid(shape[0], shape[1], n)[0] ** 2 // 4 if merge == "auto" else int(merge)
        seg = Segmenter(n_orient=n_orient, color_weight=cw, chroma_gain=g, n_superpixels=n, spatial_weight=lam, min_region_size=m)
        labels = seg.segment_device(torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda())
        rows += all_scores_batch_device(labels, truth.to_device(group))
    print("| n | lambda | n_orient | w | g | m | boundary recall | underseg | undersegNP | compactness | regions |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    print("| %d | %d | %d | %g | %d | %s | %s | %.1f |" % (n, lam, n_orient, cw, g, merge, " | ".join(
        "%.4f" % float(np.mean([r[k] for r in rows])) for k in ("recall", "underseg", "undersegNP", "compactness")),
        float(np.mean([r["regions"] for r in rows]))))


def region_plan(n, lam, n_orient, cw, g, tree_nodes, k, m=0):
    """The plan of `--regions`: on superpixels (SPEC.md §14, §18) or, with `--tree-nodes clusters`, on the k-means map (§21)."""
    from gabor_color_image_segmentation_amd import Segmenter
    cost = sys.argv[sys.argv.index("--merge-cost") + 1] if "--merge-cost" in sys.argv else "features"    # SPEC.md §23
    if tree_nodes == "clusters":
        return Segmenter(n_orient=n_orient, color_weight=cw, chroma_gain=g, k=k, tree_nodes=tree_nodes, min_region_size=m,
                         merge_cost=cost, **_regularize_kw())
    return Segmenter(n_orient=n_orient, color_weight=cw, chroma_gain=g, n_superpixels=n, spatial_weight=lam, tree_nodes=tree_nodes,
                     min_region_size=m, merge_cost=cost)


def region_rows(n, lam, n_orient, cw, g, merge, regions, tree_nodes="superpixels", k=16):
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, superpixel_grid
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    rows = {r: [] for r in regions}
    components = tree_nodes in ("components", "clusters")
    seg = None if components else region_plan(n, lam, n_orient, cw, g, "superpixels", k)
    for shape in sorted({pack["img_" + i].shape[:2] for i in ids}):
        group = [i for i in ids if pack["img_" + i].shape[:2] == shape]
        m = superpixel_grid(shape[0], shape[1], n or 300)[0] ** 2 // 4 if merge == "auto" else int(merge)
        if components:                                   # m is part of the node map (SPEC.md §18, §21): nothing runs behind a cut
            seg = region_plan(n, lam, n_orient, cw, g, tree_nodes, k, m)
            m = 0
        labels, merges, _, alive = seg.region_tree_device(torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda())
        dt = truth.to_device(group)
        for r in regions:                                # one tree, a relabel per R
            cut = seg.cut_regions_device(labels, merges, alive, r)
            if m > 0:
                post = torch.empty_like(cut)
                seg.ops.merge_small_regions(cut, m, post)
                cut = post
            rows[r] += all_scores_batch_device(cut, dt, agreement=True)
    keys = ("recall", "precision", "fmeasure", "PRI", "VoI", "covering")
    print("| n | lambda | n_orient | w | g | R | m | R | P | F | PRI | VoI | covering | regions |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in regions:
        print("| %d | %d | %d | %g | %d | %d | %s | %s | %.1f |" % (n, lam, n_orient, cw, g, r, merge, " | ".join(
            "%.4f" % float(np.mean([x[k] for x in rows[r]])) for k in keys), float(np.mean([x["regions"] for x in rows[r]]))))


def sweep_rows(n, lam, n_orient, cw, g, regions, agreement=False, reference=False, tree_nodes="superpixels", k=16):
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    from gabor_color_image_segmentation_amd.evaluate_gpu import (boundary_sweep_resident, cut_shapes_device, region_sweep_resident,
                                                                  sweep_agreement, sweep_reference_scores, sweep_scores,
                                                                  under_sweep_resident)
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    seg = region_plan(n, lam, n_orient, cw, g, tree_nodes, k)
    rows, agree, ref = [], [], []
    for shape in sorted({pack["img_" + i].shape[:2] for i in ids}):
        group = [i for i in ids if pack["img_" + i].shape[:2] == shape]
        labels, merges, _, alive = seg.region_tree_device(torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda())
        contours = seg.contour_map_device(labels, merges, alive)
        dt = truth.to_device(group)                      # one map and one pass over it per batch, whatever the number of R
        rows += sweep_scores(boundary_sweep_resident(contours, alive, dt), alive.cpu().numpy(), dt.bd_counts.cpu().numpy(), dt.first,
                             regions)
        if agreement:                                    # the leaf tables once, every coarser table from the merge list (SPEC.md §16)
            agree += sweep_agreement(*region_sweep_resident(labels, merges, alive, dt, regions), dt.first, shape[0] * shape[1], regions)
        if reference:                                    # the undersegmentation sums and the shape counts of every cut (SPEC.md §17)
            ref += sweep_reference_scores(under_sweep_resident(labels, merges, alive, dt, regions),
                                          *cut_shapes_device(labels, contours, merges, alive, regions), alive.cpu().numpy(), dt.first,
                                          shape[0], shape[1], regions)
    keys = ("recall", "precision", "fmeasure") + (("PRI", "VoI", "covering") if agreement else ()) + \
        (("underseg", "undersegNP", "compactness", "density", "regions") if reference else ())
    for extra in ([agree] if agreement else []) + ([ref] if reference else []):
        rows = [[dict(s, **a) for s, a in zip(row, arow)] for row, arow in zip(rows, extra)]
    print("| n | lambda | n_orient | w | g | R | R | P | F |" + (" PRI | VoI | covering |" if agreement else "") +
          (" underseg | undersegNP | compactness | density | regions |" if reference else ""))
    print("|---|---|---|---|---|---|---|---|---|" + ("---|---|---|" if agreement else "") + ("---|---|---|---|---|" if reference else ""))
    for j, r in enumerate(regions):
        print("| %d | %d | %d | %g | %d | %d | %s |" % (n, lam, n_orient, cw, g, r, " | ".join(
            "%.4f" % float(np.mean([row[j][k] for row in rows])) for k in keys)))
    best = ods_ois([[s["fmeasure"] for s in row] for row in rows], regions)
    print("ODS %.4f at R = %d   OIS %.4f   (%d images, R in %s)" % (best["ODS"], best["ODS_regions"], best["OIS"], len(rows),
                                                                    ",".join(str(r) for r in regions)))
    for key in keys[3:6] if agreement else ():           # VoI: lower is better
        best = ods_ois([[s[key] for s in row] for row in rows], regions, best="min" if key == "VoI" else "max")
        print("%-8s ODS %.4f at R = %d   OIS %.4f" % (key, best["ODS"], best["ODS_regions"], best["OIS"]))


def edge_rows(n_orient, cw, g, smoothing, levels=256):
    """`--edges`: the texture-gradient edge map (SPEC.md §22) of the 24 val images at `levels` absolute thresholds."""
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    seg = Segmenter(n_orient=n_orient, color_weight=cw, chroma_gain=g, smoothing=smoothing)
    groups = [[i for i in ids if pack["img_" + i].shape[:2] == shape] for shape in sorted({pack["img_" + i].shape[:2] for i in ids})]
    maps = [seg.edges_device(torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda()) for group in groups]
    step = -(-(max(int(m.max()) for m in maps) + 1) // levels)             # one step for the set: the thresholds are absolute
    table = []
    for group, m in zip(groups, maps):
        table += edge_sweep_resident(m, truth.to_device(group), levels=levels, step=step)[2].tolist()
    best = ods_ois(table, [step * (tau + 1) - 1 for tau in range(levels)])
    print("| n_orient | w | g | K | levels | step | ODS | threshold | OIS |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("| %d | %g | %d | %g | %d | %d | %.4f | G > %d | %.4f |" % (n_orient, cw, g, smoothing, levels, step, best["ODS"],
                                                                    best["ODS_regions"], best["OIS"]))


def _match_cells(maps, groups, truth, step, levels, match, device=False):
    """`--match [N]`: " ODS | OIS |" of the one-to-one matching score (SPEC.md §26, `evaluate.match_scores`, on the host) at N of
    the `levels` thresholds of the sweep; nothing when `match` is 0. `--match-device`: " ODS | OIS |" of the same score at all
    `levels` thresholds from the device (§27, `evaluate_gpu.edge_match_resident`), and with both a second line: whether the host's
    floats are the device's at the N thresholds."""
    from gabor_color_image_segmentation_amd.evaluate import match_scores, ods_ois
    cells, taus, table = "", [], []
    if match:
        taus = [(2 * j + 1) * levels // (2 * match) for j in range(match)]
        th = [step * (tau + 1) - 1 for tau in taus]
        for group, m in zip(groups, maps):
            host = m.cpu().numpy()
            table += [match_scores(host[j], truth[i], th)["fmeasure"].tolist() for j, i in enumerate(group)]
        best = ods_ois(table, th)
        cells += " %.4f | %.4f |" % (best["ODS"], best["OIS"])
    if device:
        from gabor_color_image_segmentation_amd.evaluate_gpu import edge_match_resident
        dev = []
        for group, m in zip(groups, maps):
            dev += edge_match_resident(m, truth.to_device(group), levels=levels, step=step)[2].tolist()
        best = ods_ois(dev, [step * (tau + 1) - 1 for tau in range(levels)])
        cells += " %.4f | %.4f |" % (best["ODS"], best["OIS"])
        if match:
            same = all(row[tau] == want for row, wants in zip(dev, table) for tau, want in zip(taus, wants))
            cells += "\n  host and device F at tau = %s: %s" % (",".join(str(t) for t in taus), "the same floats" if same else "DIFFERENT")
    return cells


def _match_header(match, device):
    return (" match ODS | match OIS |" if match else "") + (" device match ODS | device match OIS |" if device else ""), \
        ("---|---|" if match else "") + ("---|---|" if device else "")


def texton_edge_rows(n_orient, cw, g, smoothing, k, radius, levels=256, thin=False, match=0, match_device=False):
    """`--texton-edges`: E, TG and G (SPEC.md §24, §22) of the 24 val images at `levels` absolute thresholds each. `thin`: E and TG
    thinned along their direction map (§26; G has none)."""
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    seg = Segmenter(n_orient=n_orient, color_weight=cw, chroma_gain=g, smoothing=smoothing, k=k)
    groups = [[i for i in ids if pack["img_" + i].shape[:2] == shape] for shape in sorted({pack["img_" + i].shape[:2] for i in ids})]
    batches = [torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda() for group in groups]
    print("| map | n_orient | w | g | K | k | radius | levels | step | ODS | threshold | OIS |" + _match_header(match, match_device)[0])
    print("|---|---|---|---|---|---|---|---|---|---|---|---|" + _match_header(match, match_device)[1])
    mark = " thin" if thin else ""
    for name, make in (("E" + mark, lambda d: seg.texton_edges_device(d, radius=radius, thin=thin)),
                       ("TG" + mark, lambda d: seg.texton_edges_device(d, radius=radius, joined=False, thin=thin)),
                       ("G", lambda d: seg.edges_device(d))):
        maps = [make(d) for d in batches]
        step = -(-(max(int(m.max()) for m in maps) + 1) // levels)          # one step for the set: the thresholds are absolute
        table = []
        for group, m in zip(groups, maps):
            table += edge_sweep_resident(m, truth.to_device(group), levels=levels, step=step)[2].tolist()
        best = ods_ois(table, [step * (tau + 1) - 1 for tau in range(levels)])
        print("| %s | %d | %g | %d | %g | %d | %d | %d | %d | %.4f | %s > %d | %.4f |" % (
            name, n_orient, cw, g, smoothing, k, radius, levels, step, best["ODS"], name, best["ODS_regions"], best["OIS"])
            + _match_cells(maps, groups, truth, step, levels, match, match_device))


def cue_edge_rows(n_orient, cw, g, k, radius, bins, weights, levels=256, thin=False, match=0, match_device=False):
    """`--cue-edges`: E' and PB (SPEC.md §25) and E (§24) of the 24 val images at `levels` absolute thresholds each. `thin`: every
    map thinned along its direction map (§26)."""
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    gold = os.path.join(ROOT, "tests", "golden")
    pack = np.load(os.path.join(gold, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(gold, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    seg = Segmenter(n_orient=n_orient, color_weight=cw, chroma_gain=g, k=k)
    groups = [[i for i in ids if pack["img_" + i].shape[:2] == shape] for shape in sorted({pack["img_" + i].shape[:2] for i in ids})]
    batches = [torch.from_numpy(np.stack([pack["img_" + i] for i in group])).cuda() for group in groups]
    print("| map | n_orient | w | g | k | radius | bins | weights | levels | step | ODS | threshold | OIS |" + _match_header(match, match_device)[0])
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|" + _match_header(match, match_device)[1])
    cue = dict(radius=radius, bins=bins, weights=weights, thin=thin)
    mark = " thin" if thin else ""
    for name, cues, make in (("E'" + mark, True, lambda d: seg.cue_edges_device(d, **cue)),
                             ("PB" + mark, True, lambda d: seg.cue_edges_device(d, joined=False, **cue)),
                             ("E" + mark, False, lambda d: seg.texton_edges_device(d, radius=radius, thin=thin))):
        maps = [make(d) for d in batches]
        step = -(-(max(int(m.max()) for m in maps) + 1) // levels)          # one step for the set: the thresholds are absolute
        table = []
        for group, m in zip(groups, maps):
            table += edge_sweep_resident(m, truth.to_device(group), levels=levels, step=step)[2].tolist()
        best = ods_ois(table, [step * (tau + 1) - 1 for tau in range(levels)])
        print("| %s | %d | %g | %d | %d | %d | %s | %s | %d | %d | %.4f | %s > %d | %.4f |" % (
            name, n_orient, cw, g, k, radius, bins if cues else "-", ",".join(str(v) for v in weights) if cues else "-",
            levels, step, best["ODS"], name, best["ODS_regions"], best["OIS"]) + _match_cells(maps, groups, truth, step, levels, match, match_device))


def _match_levels():
    """`--match [N]`: N thresholds (32 when N is left out), 0 without the option."""
    if "--match" not in sys.argv:
        return 0
    at = sys.argv.index("--match") + 1
    return int(sys.argv[at]) if at < len(sys.argv) and sys.argv[at].isdigit() else 32


if __name__ == '__main__':
    if "--cue-edges" in sys.argv:
        def opt(name, conv, default):
            return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
        cue_edge_rows(opt("--n-orient", int, 6), opt("--color-weight", float, 0.0), opt("--chroma-gain", int, 0), opt("--k", int, 8),
                      opt("--radius", int, 8), opt("--bins", int, 16),
                      tuple(int(v) for v in opt("--weights", str, "2,2,1,1").split(",")), thin="--thin" in sys.argv,
                      match=_match_levels(), match_device="--match-device" in sys.argv)
        sys.exit(0)
    if "--texton-edges" in sys.argv:
        def opt(name, conv, default):
            return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
        texton_edge_rows(opt("--n-orient", int, 6), opt("--color-weight", float, 0.0), opt("--chroma-gain", int, 0),
                         opt("--smoothing", float, 0.0), opt("--k", int, 8), opt("--radius", int, 8), thin="--thin" in sys.argv,
                         match=_match_levels(), match_device="--match-device" in sys.argv)
        sys.exit(0)
    if "--edges" in sys.argv:
        def opt(name, conv, default):
            return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
        edge_rows(opt("--n-orient", int, 6), opt("--color-weight", float, 0.0), opt("--chroma-gain", int, 0),
                  opt("--smoothing", float, 0.0))
        sys.exit(0)
    clusters ="--tree-nodes" in sys.argv and sys.argv[sys.argv.index("--tree-nodes") + 1] == "clusters"
    if "--superpixels" in sys.argv or (clusters and "--regions" in sys.argv):
        def one(name, conv, default):
            return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
        if clusters and "--superpixels" in sys.argv:
            sys.exit("--tree-nodes clusters takes the k-means map: leave --superpixels out")
        if clusters:                                     # (no superpixel stage: its two columns print 0)
            sys.argv += ["--superpixels", "0", "--spatial-weight", "0"]
        if "--regions" in sys.argv and "--sweep" in sys.argv:
            sweep_rows(one("--superpixels", int, 300), one("--spatial-weight", int, 576), one("--n-orient", int, 6),
                       one("--color-weight", float, 0.0), one("--chroma-gain", int, 0),
                       [int(v) for v in one("--regions", str, "8").split(",")], agreement="--agreement" in sys.argv,
                       reference="--reference-metrics" in sys.argv, tree_nodes=one("--tree-nodes", str, "superpixels"),
                       k=one("--k", int, 16))
            sys.exit(0)
        if "--regions" in sys.argv:
            region_rows(one("--superpixels", int, 300), one("--spatial-weight", int, 576), one("--n-orient", int, 6),
                        one("--color-weight", float, 0.0), one("--chroma-gain", int, 0), one("--min-region-size", str, "0"),
                        [int(v) for v in one("--regions", str, "8").split(",")], one("--tree-nodes", str, "superpixels"),
                        one("--k", int, 16))
            sys.exit(0)
        superpixel_row(one("--superpixels", int, 300), one("--spatial-weight", int, 576), one("--n-orient", int, 6),
                       one("--color-weight", float, 0.0), one("--chroma-gain", int, 0), one("--min-region-size", str, "0"))
        sys.exit(0)
    if any(o in sys.argv for o in ("--min-region-size", "--smoothing", "--color-weight", "--chroma-gain", "--n-orient", "--position-weight",
                                   "--regularize")):
        def arg(name, conv, default):
            return [conv(v) for v in sys.argv[sys.argv.index(name) + 1].split(",")] if name in sys.argv else default
        merge_table(arg("--min-region-size", int, [0]), arg("--smoothing", float, [0.0]), arg("--color-weight", float, [0.0]),
                    arg("--chroma-gain", int, [0]), arg("--n-orient", int, [None])[0], arg("--position-weight", int, [0]))
        sys.exit(0)
    if "--val" in sys.argv:
        val_split(agreement="--agreement" in sys.argv)
        sys.exit(0)
    data = load_packed(os.path.join(ROOT, "tests", "golden", "bsd_inputs.npz"))
    for name in sorted(data):
        img, segments = data[name]                       # script.py:25, :33
        print("Processing image " + name)
        if "--gpu-scoring" in sys.argv:
            import torch
            from gabor_color_image_segmentation_amd import Segmenter
            from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_device
            seg = Segmenter()
            s = all_scores_device(seg.segment_device(torch.from_numpy(img[None]).cuda())[0], segments)
            print("Regions: %d Recall: %r Precision: %r F-measure: %r Undersegmentation: %r Undersegmentation (NP) %r "
                  "Compactness %r Density %r" % (s["regions"], s["recall"], s["precision"], s["fmeasure"], s["underseg"],
                                                 s["undersegNP"], s["compactness"], s["density"]))
            continue
        labels = segment(img)                            # script.py:30 — the slot
        m = metrics(img, labels, segments)               # script.py:36
        m.set_metrics()
        m.display_metrics()
