#!/usr/bin/env python3
"""What the k-means model of SPEC.md §28 says about the Lloyd loop and about frozen codebooks, on the CPU through the oracles
(tests/colour_ref.py for the features, the C oracle for whole loops, oracle/spec_oracle.py for the update), on the 24 val fixture
images (landscape ones transposed to 481 x 321 with their annotator maps, as a batch of one shape would hold them). No GPU is used.

    kmeans_model_quality.py [out.json] [n_images] [jobs]

(a) convergence, per plan (the default bank at k = 8, the colour bank - n_orient 5, color_weight 1/8, chroma_gain 4 - at k = 8 and
    16), per-image codebooks: ``mse[n - 1]`` = sum_p best(p) / (P D) under the centroids a loop of n_iter = n ends on, n = 1 .. 20,
    and ``changed[t - 1]`` = the share of pixels whose label differs between pass t and pass t + 1, t = 1 .. 19; means over the
    images, and the per-image extremes at n = 10.
(b) frozen codebooks, per plan at k = 8, n_iter = 10: recall, precision, boundary F, PRI, VoI and covering of the raw cluster labels
    with per-image codebooks, against ONE codebook fitted (mode "global") on the other half of the images - the first twelve label
    the last twelve and the other way round - with refine = 0, 1 and 2 (per image); on how many images F rose.

A pass assigns with one float64 matrix product, which is exact here: x c <= 65535^2 < 2^32 per term and D <= 72 terms stay below
2^39 < 2^53, as do |x|^2 and |c|^2; the labels of the twentieth pass are held to the C oracle's loop on every image."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
H, W = 481, 321
PASSES = 20
COLOUR = dict(n_orient=5, w=0.125, g=4)
PLANS = {"default_k8": (dict(n_orient=6, w=0.0, g=0), 8), "colour_k8": (COLOUR, 8), "colour_k16": (COLOUR, 16)}


def _image(i):
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    im = val["img_" + i]
    return im if im.shape[:2] == (H, W) else np.ascontiguousarray(im.transpose(1, 0, 2))


def _features(i, bank):
    import colour_ref as cr
    f = cr.features(_image(i), bank["w"], bank["g"], 4, bank["n_orient"])          # (D, H, W) uint16
    return f.reshape(f.shape[0], -1)


def distances(xf, x2, c):
    """xf (P, D) float64, x2 = |x|^2 (P,), c (k, D) int64 -> (P, k) int64, exact (see the module's text)."""
    cf = c.astype(np.float64)
    return (x2[:, None] - 2.0 * (xf @ cf.T) + (cf * cf).sum(axis=1)[None, :]).astype(np.int64)


def assign(xf, x2, c):
    d = distances(xf, x2, c)
    lab = d.argmin(axis=1)                                     # the first minimum: ties to the lowest j
    return lab.astype(np.int32), d[np.arange(len(lab)), lab]


def loop(x, c, n_iter):
    """SPEC.md §4's schedule from centroids c on x (P, D) int64 -> (labels of the last pass, per pass: inertia, labels changed)."""
    from oracle import spec_oracle as so
    xf = x.astype(np.float64)
    x2 = (xf * xf).sum(axis=1)
    inertia, changed, prev = [], [], None
    for t in range(n_iter):
        lab, best = assign(xf, x2, c)
        inertia.append(int(best.sum()))
        if prev is not None:
            changed.append(int((lab != prev).sum()))
        prev = lab
        if t < n_iter - 1:
            c = so.kmeans_update(x, lab, c)[0]
    return lab, inertia, changed


def convergence_job(job):
    from oracle import c_oracle as co
    from oracle import spec_oracle as so
    i, plan = job
    bank, k = PLANS[plan]
    co.set_threads(1)
    f = _features(i, bank)
    x = f.T.astype(np.int64)
    lab, inertia, changed = loop(x, so.kmeans_init(x, k), PASSES)
    assert np.array_equal(lab, co.kmeans(f[None], k, PASSES)[0][0]), (i, plan, "the float64 assign left the C oracle's loop")
    p, d = x.shape
    return i, plan, [v / (p * d) for v in inertia], [v / p for v in changed]


def frozen_job(job):
    """One half of the images under the codebook of the other half, and under their own: rows of
    (image, variant, recall, precision, F, PRI, VoI, covering)."""
    from oracle import c_oracle as co
    from gabor_color_image_segmentation_amd.evaluate import boundary_scores, region_agreement
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    plan, fit_ids, ids = job
    bank, k = PLANS[plan]
    pt = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    model = co.kmeans(np.stack([_features(i, bank) for i in fit_ids]), k, 10)[1].astype(np.int64)
    rows = []
    for i in ids:
        f = _features(i, bank)
        x = f.T.astype(np.int64)
        truth = [m if m.shape == (H, W) else np.ascontiguousarray(m.T) for m in pt[i]]
        maps = {"per_image": co.kmeans(f[None], k, 10)[0][0]}
        for m in (0, 1, 2):
            maps["frozen_refine%d" % m] = loop(x, model, m + 1)[0]
        for name, lab in maps.items():
            lab = lab.reshape(H, W).astype(np.int32)
            bs, ra = boundary_scores(lab, truth), region_agreement(lab, truth)
            rows.append([i, name, bs["recall"], bs["precision"], bs["fmeasure"], ra["PRI"], ra["VoI"], ra["covering"]])
    return plan, rows


def main(out_path=None, n_images=24, jobs=8):
    from multiprocessing import Pool
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"][:n_images]]
    res = dict(images=len(ids), shape=[H, W], passes=PASSES, plans={n: dict(bank=b, k=k) for n, (b, k) in PLANS.items()},
               convergence={}, frozen={})
    with Pool(jobs) as pool:
        got = pool.map(convergence_job, [(i, plan) for plan in PLANS for i in ids], chunksize=1)
        half = len(ids) // 2
        halves = [(ids[:half], ids[half:]), (ids[half:], ids[:half])]
        frozen = pool.map(frozen_job, [(plan, a, b) for plan in ("default_k8", "colour_k8") for a, b in halves], chunksize=1)
    for plan in PLANS:
        mse = np.array([m for _, p, m, _ in got if p == plan])
        chg = np.array([c for _, p, _, c in got if p == plan])
        row = dict(mse=mse.mean(axis=0).tolist(), changed=chg.mean(axis=0).tolist(),
                   mse_10_over_20=float((mse[:, 9] / mse[:, 19]).mean()), mse_10_over_20_worst=float((mse[:, 9] / mse[:, 19]).max()),
                   mse_1_over_20=float((mse[:, 0] / mse[:, 19]).mean()),
                   changed_at_10=float(chg[:, 8].mean()), changed_at_10_worst=float(chg[:, 8].max()),
                   changed_at_20=float(chg[:, 18].mean()), mse_not_falling=int((np.diff(mse, axis=1) > 0).sum()))
        res["convergence"][plan] = row
        print(json.dumps({plan: {n: v for n, v in row.items() if not isinstance(v, list)}}), flush=True)
    names = ["recall", "precision", "fmeasure", "PRI", "VoI", "covering"]
    for plan in ("default_k8", "colour_k8"):
        rows = [r for p, rs in frozen if p == plan for r in rs]
        table = {}
        base = {r[0]: r[4] for r in rows if r[1] == "per_image"}
        for variant in ("per_image", "frozen_refine0", "frozen_refine1", "frozen_refine2"):
            per = np.array([r[2:] for r in rows if r[1] == variant], np.float64)
            table[variant] = dict(zip(names, per.mean(axis=0).tolist()),
                                  f_up=int(sum(r[4] > base[r[0]] for r in rows if r[1] == variant)))
        res["frozen"][plan] = table
        print(json.dumps({plan: table}), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(a[0] if a else None, int(a[1]) if len(a) > 1 else 24, int(a[2]) if len(a) > 2 else 8)
