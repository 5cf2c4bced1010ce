#!/usr/bin/env python3
"""What k-means++ seeding (SPEC.md §29) does to the Lloyd loop's objective and to the scores of its label maps, on the CPU through
the oracles (tests/colour_ref.py for the features, tests/kmeans_seed_ref.py for the seeds, oracle/spec_oracle.py for the update),
on the 24 val fixture images (landscape ones transposed to 481 x 321 with their annotator maps), for the three plans of
tools/kmeans_model_quality.py, per-image codebooks, seeds 0 .. 3. No GPU is used.

    kmeans_seed_quality.py [out.json] [n_images] [jobs]

(a) ``mse``, per plan: the mse (sum_p best(p) / (P D)) after n_iter = 10 from the seeds, relative to the init of SPEC.md §4 at
    n_iter = 10 (``vs_spec10``) and at n_iter = 20 (``vs_spec20``): mean over images and seeds, the worst single image and seed, and
    the share of (image, seed) pairs that improved - for strides 8, 16 and 32 with 1 and 4 trials (n_init = 1), and for
    n_init = 1, 2 and 4 at stride 8 with 4 trials (restart i uses seed s + i; the restart with the least final inertia is kept;
    starting seeds 0 .. 3 for n_init 1, 0 and 2 for n_init 2, 0 for n_init 4). ``spec20_vs_spec10`` is the yardstick: what ten more
    passes buy.
(b) ``scores``, for the two k = 8 plans: recall, precision, boundary F, PRI, VoI and covering of the raw cluster labels after
    n_iter = 10 - the init of §4 (``spec10``), §4 at n_iter = 20 (``spec20``), the seeds at stride 8 with 4 trials (``seeded``: mean
    over seeds 0 .. 3) and the best of those four restarts (``n_init4``) - and on how many images F rose against ``spec10``."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kmeans_model_quality import GOLD, H, W, PLANS, _features, loop  # noqa: E402

SEEDS = (0, 1, 2, 3)
STRIDES = (8, 16, 32)
TRIALS = (1, 4)
N_ITER = 10
NAMES = ["recall", "precision", "fmeasure", "PRI", "VoI", "covering"]


def image_job(job):
    """One image under one plan -> (image, plan, spec inertia at 10 and 20, {(stride, trials, seed): inertia at 10},
    score rows [variant, recall, precision, F, PRI, VoI, covering] for the k = 8 plans)."""
    import kmeans_seed_ref as ks
    from oracle import spec_oracle as so
    i, plan = job
    bank, k = PLANS[plan]
    x = _features(i, bank).T.astype(np.int64)
    lab20, inertia, _ = loop(x, so.kmeans_init(x, k), 2 * N_ITER)
    lab10 = loop(x, so.kmeans_init(x, k), N_ITER)[0]
    seeded, maps = {}, {}
    for stride in STRIDES:
        cand = x[ks.candidates(H, W, stride)]
        for trials in TRIALS:
            for seed in SEEDS:
                lab, ins, _ = loop(x, ks.seed_set(cand, k, seed, trials)[0], N_ITER)
                seeded["%d,%d,%d" % (stride, trials, seed)] = ins[-1]
                if stride == 8 and trials == 4:
                    maps[seed] = lab
    rows = []
    if k == 8:
        from gabor_color_image_segmentation_amd.evaluate import boundary_scores, region_agreement
        from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
        truth = [m if m.shape == (H, W) else np.ascontiguousarray(m.T) for m in PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i]]
        best = min(SEEDS, key=lambda s: (seeded["8,4,%d" % s], s))
        variants = [("spec10", lab10), ("spec20", lab20)] + [("seeded", maps[s]) for s in SEEDS] + [("n_init4", maps[best])]
        for name, lab in variants:
            lab = lab.reshape(H, W).astype(np.int32)
            bs, ra = boundary_scores(lab, truth), region_agreement(lab, truth)
            rows.append([name, bs["recall"], bs["precision"], bs["fmeasure"], ra["PRI"], ra["VoI"], ra["covering"]])
    return i, plan, inertia[N_ITER - 1], inertia[2 * N_ITER - 1], seeded, rows


def _ratio_row(r):
    r = np.asarray(r, np.float64)
    return dict(mean=float(r.mean()), worst=float(r.max()), improved=float((r < 1).mean()), n=int(r.size))


def main(out_path=None, n_images=24, jobs=8):
    from multiprocessing import Pool
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"][:n_images]]
    res = dict(images=len(ids), shape=[H, W], n_iter=N_ITER, seeds=list(SEEDS), strides=list(STRIDES), trials=list(TRIALS),
               plans={n: dict(bank=b, k=k) for n, (b, k) in PLANS.items()}, mse={}, scores={})
    with Pool(jobs) as pool:
        got = pool.map(image_job, [(i, plan) for plan in PLANS for i in ids], chunksize=1)
    for plan in PLANS:
        mine = [g for g in got if g[1] == plan]
        s10 = np.array([g[2] for g in mine], np.float64)
        s20 = np.array([g[3] for g in mine], np.float64)
        table = dict(spec20_vs_spec10=_ratio_row(s20 / s10))
        for stride in STRIDES:
            for trials in TRIALS:
                v = np.array([[g[4]["%d,%d,%d" % (stride, trials, s)] for s in SEEDS] for g in mine], np.float64)     # (images, seeds)
                table["stride%d_trials%d" % (stride, trials)] = dict(vs_spec10=_ratio_row(v / s10[:, None]), vs_spec20=_ratio_row(v / s20[:, None]))
        v = np.array([[g[4]["8,4,%d" % s] for s in SEEDS] for g in mine], np.float64)
        for n_init, starts in ((1, (0, 1, 2, 3)), (2, (0, 2)), (4, (0,))):
            kept = np.stack([v[:, s:s + n_init].min(axis=1) for s in starts], axis=1)
            table["n_init%d" % n_init] = dict(vs_spec10=_ratio_row(kept / s10[:, None]), vs_spec20=_ratio_row(kept / s20[:, None]))
        res["mse"][plan] = table
        print(json.dumps({plan: {n: (r["vs_spec10"]["mean"] if "vs_spec10" in r else r["mean"]) for n, r in table.items()}}), flush=True)
        if PLANS[plan][1] != 8:
            continue
        scores = {}
        base = {g[0]: [r for r in g[5] if r[0] == "spec10"][0][3] for g in mine}
        for variant in ("spec10", "spec20", "seeded", "n_init4"):
            per = np.array([np.mean([r[1:] for r in g[5] if r[0] == variant], axis=0) for g in mine], np.float64)   # (images, 6)
            scores[variant] = dict(zip(NAMES, per.mean(axis=0).tolist()),
                                   f_up=int(sum(p[2] > base[g[0]] for p, g in zip(per, mine))),
                                   f_down=int(sum(p[2] < base[g[0]] for p, g in zip(per, mine))))
        res["scores"][plan] = scores
        print(json.dumps({plan: scores}), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(a[0] if a else None, int(a[1]) if len(a) > 1 else 24, int(a[2]) if len(a) > 2 else 8)
