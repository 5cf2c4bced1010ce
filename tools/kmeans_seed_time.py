#!/usr/bin/env python3
"""Cost of k-means++ seeding (SPEC.md §29) at batch 64 x 481x321 on the 24 val fixture images (landscape ones transposed, repeated
to 64), for two plans: the default bank (4 x 6, D = 72) at k = 8 and the colour bank (n_orient 5, color_weight 1/8, chroma_gain 4)
at k = 16. GPU only.

    kmeans_seed_time.py [out.json] --parent path/to/parent/libgcs.so

Medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs; calls
that are compared take turns, call by call (the method of tools/cue_gradient_time.py):
  <plan>_seed_per_image_ms, <plan>_seed_global_ms
                            (a) the gcs_kmeans_seed launch on the step's slab: 64 sets at the rule's stride 8 (2501 candidates
                                each, 64 workgroups), one set at stride 64 (3072 candidates, ONE workgroup); per-image also with
                                1 and 8 trials (<plan>_seed_per_image_t1_ms, _t8_ms) and at strides 16 and 32 (_s16_ms, _s32_ms:
                                651 and 176 candidates), which the host's rule never picks for one image of this shape
  <plan>_segment_ms, <plan>_segment_seeded_ms, <plan>_segment_20_ms
                            (b) Segmenter.segment_device with the init of SPEC.md §4, with init="kmeans++", and with §4's init at
                                n_iter = 20 - ten more passes, the alternative that buys about the same mse; per-image codebooks.
                                <plan>_seeded_over_segment, <plan>_20_over_segment; the same three in mode "global"
                                (<plan>_global_...)
  <plan>_mse, <plan>_mse_seeded, <plan>_mse_20
                                the mean mse of the batch after each of the three (evaluate_device), for the record
  step_default_ms / parent_default_ms
                            (c) "off means unchanged": segment_device of the default plan with this library and with the PARENT
                                commit's library in this process, taking turns (default_equal: the same labels,
                                default_inside_parent_range: the new median lies in the parent's min - max)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cue_gradient_time import _turns, COLOUR, REPS, WARM  # noqa: E402
from feature_gradient_time import _batch, _stats, _with_library, BATCH, H, W  # noqa: E402

PLANS = dict(default=dict(k=8), colour=dict(k=16, **COLOUR))


def main(out_path, parent):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, seed_stride
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], plans=PLANS, reps=REPS, warm=WARM,
               stride_per_image=seed_stride(1, H, W), stride_global=seed_stride(BATCH, H, W),
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    for plan, kw in PLANS.items():
        k = kw["k"]
        segs = dict(spec=Segmenter(**kw), seeded=Segmenter(init="kmeans++", **kw), spec20=Segmenter(n_iter=20, **kw))
        seg = segs["spec"]
        ops, d = seg.ops, seg.bank.n_features
        seg.segment_device(imgs)
        feats = seg._workspace(BATCH, H, W, "per_image")["feats"]      # the step's slab
        # (a)
        cent_b = torch.empty((BATCH, k, d), dtype=torch.int16, device="cuda")
        cent_1 = torch.empty((1, k, d), dtype=torch.int16, device="cuda")
        s1, sg = res["stride_per_image"], res["stride_global"]
        calls = dict(seed_per_image=lambda: ops.kmeans_seed(feats, BATCH, H, W, k, BATCH, cent_b, s1, 4, 0),
                     seed_per_image_t1=lambda: ops.kmeans_seed(feats, BATCH, H, W, k, BATCH, cent_b, s1, 1, 0),
                     seed_per_image_t8=lambda: ops.kmeans_seed(feats, BATCH, H, W, k, BATCH, cent_b, s1, 8, 0),
                     seed_per_image_s16=lambda: ops.kmeans_seed(feats, BATCH, H, W, k, BATCH, cent_b, 16, 4, 0),
                     seed_per_image_s32=lambda: ops.kmeans_seed(feats, BATCH, H, W, k, BATCH, cent_b, 32, 4, 0),
                     seed_global=lambda: ops.kmeans_seed(feats, BATCH, H, W, k, 1, cent_1, sg, 4, 0))
        for name, ts in _turns(torch, calls).items():
            res.update(_stats(f"{plan}_{name}", ts))
        del feats
        # (b)
        for mode, tag in (("per_image", ""), ("global", "global_")):
            times = _turns(torch, {name: (lambda s: lambda: s.segment_device(imgs, mode))(s) for name, s in segs.items()})
            for name, key in (("spec", "segment"), ("seeded", "segment_seeded"), ("spec20", "segment_20")):
                res.update(_stats(f"{plan}_{tag}{key}", times[name]))
            base = res[f"{plan}_{tag}segment_ms"]
            res[f"{plan}_{tag}seeded_over_segment"] = res[f"{plan}_{tag}segment_seeded_ms"] / base
            res[f"{plan}_{tag}20_over_segment"] = res[f"{plan}_{tag}segment_20_ms"] / base
            res[f"{plan}_{tag}seeding_ms"] = res[f"{plan}_{tag}segment_seeded_ms"] - base
            res[f"{plan}_{tag}ten_passes_ms"] = res[f"{plan}_{tag}segment_20_ms"] - base
            for name, key in (("spec", "mse"), ("seeded", "mse_seeded"), ("spec20", "mse_20")):
                st = segs[name].evaluate_device(imgs, mode=mode, labels=False)["stats"].cpu().numpy()
                res[f"{plan}_{tag}{key}"] = float((st[:, :, 1].sum(axis=1) / (st[:, :, 0].sum(axis=1) * d)).mean())
        for s in segs.values():
            s._ws.clear()
        del segs, seg
        torch.cuda.empty_cache()
        print(json.dumps({n: v for n, v in res.items() if n.startswith(plan)}), flush=True)
    # (c) "off means unchanged": the default step against the parent commit's library
    old = dict(parent=_with_library(parent, lambda: Segmenter()), step=Segmenter())
    assert not hasattr(old["parent"].ops.lib, "gcs_kmeans_seed")
    got = {}
    times = _turns(torch, {name: (lambda nm: lambda: got.__setitem__(nm, old[nm].segment_device(imgs)))(name) for name in ("parent", "step")})
    for name, ts in times.items():
        res.update(_stats(f"{name}_default", ts))
    res["default_equal"] = bool(torch.equal(got["step"], got["parent"]))
    res["default_inside_parent_range"] = bool(res["parent_default_ms_min"] <= res["step_default_ms"] <= res["parent_default_ms_max"])
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    args = sys.argv[1:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    if parent is None:
        sys.exit("the parent commit's libgcs.so is needed: --parent path")
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
    main(paths[0] if paths else None, parent)
