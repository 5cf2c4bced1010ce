"""Region agreement golden: PRI / VoI / covering per annotator map from third-party code (SPEC.md §8).

Run once in the build container, under the Python that has scikit-learn 0.24.2 and scikit-image 0.18.3 (the interpreter of
the other make_*.py scripts), from the repository root:

    python3.9 -W ignore tests/golden/make_region_golden.py tests/golden

Per annotator map G of an image and label map S:
  rand      sklearn.metrics.rand_score(G, S)                      (unordered pairs of distinct pixels)
  voi       sum(skimage.metrics.variation_of_information(G, S))   (bits)
  covering  (1/N) sum over regions R of G of |R| * max over regions R' of S meeting R of |R & R'| / |R | R'|, by region
            sets (np.unique of S[G == r], pixel masks): no contingency table, independent of the product code
Maps:
  scoring/<id>/<name>   the 12 maps of scoring_golden.json (oracle, halves, 16x16 blocks, SLIC) for the 3 bsd_inputs ids,
                        built as make_scoring_golden.py builds them
  val/<id>/stored       the 24 packed val oracle maps (bsd_val_images.npz) against bsd500_truth.npz
  val/<id>/connected    the same maps as 4-connected components (skimage.measure.label, connectivity=1)
Writes region_agreement_golden.json: per map the per-annotator lists and their means (PRI, VoI, covering).
"""
import json
import sys

import numpy as np
from skimage.measure import label as cc_label
from skimage.metrics import variation_of_information
from skimage.segmentation import slic
from sklearn.metrics import rand_score

golden_dir = sys.argv[1]


def covering(s, g):
    s, g = s.ravel(), g.ravel()
    order = np.argsort(s, kind="stable")
    keys, starts = np.unique(s[order], return_index=True)
    ends = np.append(starts[1:], s.size)
    pix = {int(k): order[a:b] for k, a, b in zip(keys, starts, ends)}      # region sets of S
    total = 0.0
    for r in np.unique(g):
        mask = g == r
        size_r = int(mask.sum())
        best = 0.0
        for q in np.unique(s[mask]):
            inter = int(np.count_nonzero(g[pix[int(q)]] == r))
            best = max(best, inter / (size_r + pix[int(q)].size - inter))
        total += size_r * best
    return total / s.size


def score(s, segs):
    rows = {"rand": [], "voi": [], "covering": []}
    for g in segs:
        g = np.asarray(g).astype(np.int64)
        rows["rand"].append(float(rand_score(g.ravel(), s.ravel())))
        rows["voi"].append(float(np.sum(variation_of_information(g, s))))
        rows["covering"].append(float(covering(s, g)))
    rows["PRI"] = float(np.mean(rows["rand"]))
    rows["VoI"] = float(np.mean(rows["voi"]))
    rows["covering_mean"] = float(np.mean(rows["covering"]))
    return rows


res = {}
inp = np.load(golden_dir + "/bsd_inputs.npz")
path = np.load(golden_dir + "/path_golden.npz")
stored = np.load(golden_dir + "/scoring_maps.npz")
for i in inp["ids"]:
    i = str(i)
    img = inp["img_" + i]
    segs = [inp["seg_%s_%d" % (i, a)] for a in range(int(inp["nseg_" + i]))]
    h, w = img.shape[:2]
    cand = {
        "oracle": path["labels_" + i].astype(np.int32),
        "halves": (np.arange(w)[None, :] >= w // 2).astype(np.int32) * np.ones((h, 1), np.int32),
        "blocks": ((np.arange(h)[:, None] // 16) * ((w + 15) // 16) + np.arange(w)[None, :] // 16).astype(np.int32),
        "slic": slic(img, n_segments=300, compactness=10.0).astype(np.int32),
    }
    assert np.array_equal(cand["slic"], stored["slic_" + i].astype(np.int32))
    for name, lab in cand.items():
        res["scoring/%s/%s" % (i, name)] = score(lab.astype(np.int64), segs)
        print(i, name, res["scoring/%s/%s" % (i, name)]["PRI"])

val = np.load(golden_dir + "/bsd_val_images.npz")
tp = np.load(golden_dir + "/bsd500_truth.npz")
index = {str(k): n for n, k in enumerate(tp["ids"])}
for i in val["ids"]:
    i = str(i)
    n = index[i]
    h, w = (int(x) for x in tp["hw"][n])
    segs = [tp["data"][tp["offs"][t]:tp["offs"][t + 1]].reshape(h, w) for t in range(tp["first"][n], tp["first"][n + 1])]
    lab = val["labels_" + i].astype(np.int64)
    conn = cc_label(lab + 1, background=0, connectivity=1).astype(np.int64) - 1
    res["val/%s/stored" % i] = score(lab, segs)
    res["val/%s/connected" % i] = score(conn, segs)
    res["val/%s/connected" % i]["regions"] = int(conn.max()) + 1
    print(i, res["val/%s/stored" % i]["PRI"], res["val/%s/connected" % i]["PRI"], int(conn.max()) + 1)
json.dump(res, open(golden_dir + "/region_agreement_golden.json", "w"), indent=1, sort_keys=True)
