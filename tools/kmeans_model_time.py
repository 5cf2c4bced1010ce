#!/usr/bin/env python3
"""Cost of the k-means model (SPEC.md §28) at batch 64 x 481x321 on the 24 val fixture images (landscape ones transposed, repeated
to 64), for two plans: the default bank (4 x 6, D = 72) at k = 8 and the colour bank (n_orient 5, color_weight 1/8, chroma_gain 4,
D = 72 with its low-pass slots) at k = 16, one codebook per image (the plan's own centroids after its Lloyd loop). GPU only.

    kmeans_model_time.py [out.json] --parent path/to/parent/libgcs.so [--variant shared_levels=path/to/libgcs.so]

Medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs; calls
that are compared take turns, call by call (the method of tools/cue_gradient_time.py):
  <plan>_stats_ms, <plan>_all_ms, <plan>_all_again_ms
                            (a) the gcs_kmeans_evaluate launch with the table alone and with every output; the second twice in the
                                rotation (<plan>_all_self_spread_ms)
  <plan>_<variant>_all_ms       the same launch through every --variant library (a -DGCS_KE_SHARED_LEVELS build), taking turns with this
                                library's (…_equal: the same outputs)
  <plan>_assign_raster_ms       one gcs_kmeans_assign_raster launch with the same centroids, for scale (…_labels_equal)
  <plan>_unpack_ms, <plan>_torch_ms
                            (b) what a user can do without the kernel: gcs_features_unpack alone, and unpack plus a torch
                                formulation of §28 with equal outputs (``torch_evaluate``; <plan>_torch_equal). The ONE condition
                                on time: <plan>_all_faster_than_torch. <plan>_all_over_unpack is recorded
  <plan>_segment_ms, <plan>_predict0_ms, <plan>_predict2_ms
                            (c) Segmenter.segment_device against predict_device(refine = 0 / 2) under a one-codebook model fitted
                                on the batch, end to end; <plan>_fit_ms
  step_<what>_ms / parent_<what>_ms
                            (d) "off means unchanged": segment_device of the default plan and cue_edges_device() of the colour plan
                                with this library and with the PARENT commit's library in this process, taking turns (…_equal: the
                                same output, …_inside_parent_range: the new median lies in the parent's min - max)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cue_gradient_time import _turns, COLOUR  # noqa: E402
from feature_gradient_time import _batch, _stats, _timed, _with_library, BATCH, H, W, WARM  # noqa: E402

PLANS = dict(default=dict(k=8), colour=dict(k=16, **COLOUR))
NAMES = ("labels", "best", "second", "stats")


def torch_evaluate(torch, canon, cent):
    """SPEC.md §28 in torch operations on the canonical (B, D, H, W) int16 tensor and (B, k, D) int16 centroids, image by image in
    int64: (labels int32, best, second int64 (B, H, W), stats (B, k, 2) int64)."""
    b, d, h, w = canon.shape
    k = cent.shape[1]
    labels = torch.empty((b, h, w), dtype=torch.int32, device=canon.device)
    best = torch.empty((b, h, w), dtype=torch.int64, device=canon.device)
    second = torch.empty_like(best)
    stats = torch.zeros((b, k, 2), dtype=torch.int64, device=canon.device)
    top = torch.iinfo(torch.int64).max
    for i in range(b):
        x = (canon[i].reshape(d, -1).to(torch.int64) & 0xFFFF)
        c = (cent[i].to(torch.int64) & 0xFFFF)
        dist = torch.stack([((x - c[j][:, None]) ** 2).sum(0) for j in range(k)])         # (k, P)
        bs, lab = dist.min(dim=0)                              # the first minimum: ties to the lowest j
        if k > 1:
            sc = dist.scatter(0, lab[None], top).min(dim=0).values
        else:
            sc = bs
        labels[i], best[i], second[i] = lab.reshape(h, w).to(torch.int32), bs.reshape(h, w), sc.reshape(h, w)
        stats[i, :, 0] = torch.bincount(lab, minlength=k)
        stats[i, :, 1].scatter_add_(0, lab, bs)
    return labels, best, second, stats


def _outs(torch, k):
    new = lambda dt: torch.full((BATCH, H, W), -1, dtype=dt, device="cuda")
    return dict(labels=new(torch.int32), best=new(torch.int64), second=new(torch.int64),
                stats=torch.full((BATCH, k, 2), -1, dtype=torch.int64, device="cuda"))


def _same(torch, a, b):
    return bool(all(torch.equal(a[n], b[n]) for n in NAMES))


def main(out_path, parent, variants):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.segmenter import HipOps
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], plans=PLANS, variants=sorted(variants),
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    plans = {}
    for plan, kw in PLANS.items():
        seg = plans[plan] = Segmenter(**kw)
        ops, k, d = seg.ops, kw["k"], seg.bank.n_features
        want = seg.segment_device(imgs)
        ws = seg._workspace(BATCH, H, W, "per_image")          # the step's slab and the centroids its loop ended on
        feats, cent = ws["feats"], ws["cent"].clone()
        res[f"{plan}_features"] = d
        res[f"{plan}_slab_bytes"] = int(feats.numel())
        # (a)
        outs = {name: _outs(torch, k) for name in ["all", "all_again"] + [v + "_all" for v in variants]}
        table = torch.full((BATCH, k, 2), -1, dtype=torch.int64, device="cuda")
        raster = torch.full((BATCH, H, W), -1, dtype=torch.int32, device="cuda")
        vops = {v: _with_library(path, lambda: HipOps(seg.bank, "cuda:0", seg.smoothing, seg.chroma_gain)) for v, path in variants.items()}
        calls = dict(stats=lambda: ops.kmeans_evaluate(feats, cent, BATCH, H, W, k, BATCH, stats=table),
                     all=lambda: ops.kmeans_evaluate(feats, cent, BATCH, H, W, k, BATCH, **outs["all"]),
                     assign_raster=lambda: ops.assign_raster(feats, cent, BATCH, H, W, k, BATCH, raster, scratch_labels=ws["labels"]),
                     all_again=lambda: ops.kmeans_evaluate(feats, cent, BATCH, H, W, k, BATCH, **outs["all_again"]))
        for v in variants:
            calls[v + "_all"] = (lambda n: lambda: vops[n].kmeans_evaluate(feats, cent, BATCH, H, W, k, BATCH, **outs[n + "_all"]))(v)
        for name, ts in _turns(torch, calls).items():
            res.update(_stats(f"{plan}_{name}", ts))
        res[f"{plan}_all_self_spread_ms"] = abs(res[f"{plan}_all_ms"] - res[f"{plan}_all_again_ms"])
        for v in variants:
            res[f"{plan}_{v}_equal"] = _same(torch, outs["all"], outs[v + "_all"])
            res[f"{plan}_{v}_over_default"] = res[f"{plan}_{v}_all_ms"] / res[f"{plan}_all_ms"]
        res[f"{plan}_stats_equal"] = bool(torch.equal(table, outs["all"]["stats"]))
        res[f"{plan}_labels_equal"] = bool(torch.equal(raster, outs["all"]["labels"]) and torch.equal(raster, want))
        res[f"{plan}_all_over_assign_raster"] = res[f"{plan}_all_ms"] / res[f"{plan}_assign_raster_ms"]
        total = outs["all"]["stats"].cpu().numpy()
        res[f"{plan}_mse_mean"] = float((total[:, :, 1].sum(axis=1) / (total[:, :, 0].sum(axis=1) * d)).mean())
        del outs["all_again"], vops
        # (b)
        canon = torch.empty((BATCH, d, H, W), dtype=torch.int16, device="cuda")
        held = {}
        res.update(_stats(f"{plan}_unpack", _turns(torch, dict(u=lambda: ops.features_unpack(feats, BATCH, H, W, out=canon)))["u"]))

        def via_torch():
            ops.features_unpack(feats, BATCH, H, W, out=canon)
            held["t"] = dict(zip(NAMES, torch_evaluate(torch, canon, cent)))
        res.update(_stats(f"{plan}_torch", [_timed(torch, via_torch) for _ in range(WARM + 5)][WARM:]))
        res[f"{plan}_torch_equal"] = _same(torch, outs["all"], held["t"])
        res[f"{plan}_all_faster_than_torch"] = bool(res[f"{plan}_all_ms"] < res[f"{plan}_torch_ms"])
        res[f"{plan}_torch_over_all"] = res[f"{plan}_torch_ms"] / res[f"{plan}_all_ms"]
        res[f"{plan}_all_over_unpack"] = res[f"{plan}_all_ms"] / res[f"{plan}_unpack_ms"]
        del canon, held, outs, table, raster
        torch.cuda.empty_cache()
        # (c)
        model = seg.fit_device(imgs, "global")
        res.update(_stats(f"{plan}_fit", [_timed(torch, lambda: seg.fit_device(imgs, "global")) for _ in range(WARM + 5)][WARM:]))
        times = _turns(torch, dict(segment=lambda: seg.segment_device(imgs), predict0=lambda: seg.predict_device(imgs, model),
                                   predict2=lambda: seg.predict_device(imgs, model, refine=2)))
        for name, ts in times.items():
            res.update(_stats(f"{plan}_{name}", ts))
        res[f"{plan}_predict0_over_segment"] = res[f"{plan}_predict0_ms"] / res[f"{plan}_segment_ms"]
        res[f"{plan}_predict2_over_segment"] = res[f"{plan}_predict2_ms"] / res[f"{plan}_segment_ms"]
        res[f"{plan}_model_mse"] = float(model.mse[0])
        seg._ws.clear()
        del ws, feats, model
        torch.cuda.empty_cache()
        print(json.dumps({n: v for n, v in res.items() if n.startswith(plan)}), flush=True)
    # (d) "off means unchanged": the existing steps against the parent commit's library
    old = dict(parent=(_with_library(parent, lambda: Segmenter()), _with_library(parent, lambda: Segmenter(k=8, **COLOUR))),
               step=(Segmenter(), Segmenter(k=8, **COLOUR)))
    assert not hasattr(old["parent"][0].ops.lib, "gcs_kmeans_evaluate")
    runs = dict(default=lambda pair: pair[0].segment_device(imgs), cue_edges=lambda pair: pair[1].cue_edges_device(imgs))
    for what, fn in runs.items():
        got = {}
        times = _turns(torch, {name: (lambda nm: lambda: got.__setitem__(nm, fn(old[nm])))(name) for name in ("parent", "step")})
        for name, ts in times.items():
            res.update(_stats(f"{name}_{what}", ts))
        res[what + "_equal"] = bool(torch.equal(got["step"], got["parent"]))
        res[what + "_inside_parent_range"] = bool(res[f"parent_{what}_ms_min"] <= res[f"step_{what}_ms"] <= res[f"parent_{what}_ms_max"])
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    args = sys.argv[1:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    variants = dict(a.split("=", 1) for i, a in enumerate(args) if i and args[i - 1] == "--variant")
    if parent is None:
        sys.exit("the parent commit's libgcs.so is needed: --parent path")
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in ("--parent", "--variant"))]
    main(paths[0] if paths else None, parent, variants)
