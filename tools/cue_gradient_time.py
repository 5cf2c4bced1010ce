#!/usr/bin/env python3
"""Cost of the cue gradient (SPEC.md §25) at batch 64 x 481x321 on the 24 val fixture images (landscape ones transposed, repeated
to 64), colour bank (n_orient 5, color_weight 1/8, chroma_gain 4), k = 8, r = 8, n = 8, 16 bins. GPU only.

    cue_gradient_time.py [out.json] --parent path/to/parent/libgcs.so

Medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs; calls
that are compared take turns, call by call:
  texton_ms / texton_again_ms, cue_1000_ms
                            (a) gcs_texton_gradient on the plan's k-means map, TWICE in the rotation (the spread of the existing
                                kernel against itself: texton_self_spread_ms = |difference of the two medians|), and
                                gcs_cue_gradient at weights (1, 0, 0, 0) on the same labels (cue_1000_equal: the same map;
                                cue_1000_inside_texton_range: its median lies in the min - max of the existing kernel's calls)
  cue_2211_ms, cue_0111_ms, …_joined_ms
                            (b) the launch at (2, 2, 1, 1) and (0, 1, 1, 1), without / with grad
  four_2211_ms, four_0111_ms, …_joined_ms
                            (c) what the existing entry point can do over the same planes: one gcs_texton_gradient launch per cue
                                of non-zero weight (the channels quantised and widened to int32 by torch beforehand, not timed),
                                timed as one group. These launches cannot produce PB (no join per direction); they do the same
                                popcount work. fused_no_slower_than_four_<w>: cue_<w>_ms <= four_<w>_ms
  bins_per_tile_<cue>           mean number of bins an 8 x 32 tile's window holds (what the skip leaves to walk), per cue
  cue_edges_2211_ms, cue_edges_0111_ms, texton_edges_ms
                            (d) Segmenter.cue_edges_device at both weight sets and Segmenter.texton_edges_device, end to end
  step_<what>_ms / parent_<what>_ms
                            (e) Segmenter.segment_device of the default plan, texton_edges_device, gcs_texton_gradient and
                                gcs_cue_gradient at (2, 2, 1, 1), joined, with this library and with the PARENT commit's library in
                                this process, taking turns (…_equal: the same output, …_inside_parent_range: the new median lies in
                                the parent's min - max; a parent that does not export gcs_cue_gradient has no arm in that call)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from feature_gradient_time import _batch, _stats, _timed, _with_library, BATCH, H, W  # noqa: E402

REPS, WARM = 15, 3
RADIUS, N_DIR, BINS, K = 8, 8, 16, 8
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
SETS = {"2211": (2, 2, 1, 1), "0111": (0, 1, 1, 1)}


def _turns(torch, calls, reps=REPS, warm=WARM):
    """Every call of ``calls`` in turn, round after round: {name: times of the rounds after the warm-up}."""
    times = {name: [] for name in calls}
    for rnd in range(warm + reps):
        for name, fn in calls.items():
            t = _timed(torch, fn)
            if rnd >= warm:
                times[name].append(t)
    return times


def main(out_path, parent):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], reps=REPS, warm=WARM, radius=RADIUS, n_directions=N_DIR, bins=BINS, k=K, bank=COLOUR,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    new = lambda: torch.full((BATCH, H, W), -1, dtype=torch.int32, device="cuda")
    seg = Segmenter(k=K, **COLOUR)
    ops = seg.ops
    labels, grad = seg.segment_device(imgs), seg.edges_device(imgs)
    i0 = torch.empty_like(imgs)
    ops.colour_opponent(imgs, i0)
    shift = 8 - (BINS.bit_length() - 1)
    planes = [labels] + [(i0[..., c] >> shift).to(torch.int32).contiguous() for c in range(3)]
    outs = {name: new() for name in ("texton", "texton_again", "cue_1000")}
    tex = lambda lab, k, g, out: ops.texton_gradient(lab, BATCH, H, W, k, RADIUS, N_DIR, g, out, None)
    cue = lambda wts, g, out: ops.cue_gradient(labels, i0, BATCH, H, W, K, BINS, wts, RADIUS, N_DIR, g, out, None)
    # (a)
    times = _turns(torch, dict(texton=lambda: tex(labels, K, None, outs["texton"]), cue_1000=lambda: cue((1, 0, 0, 0), None, outs["cue_1000"]),
                               texton_again=lambda: tex(labels, K, None, outs["texton_again"])))
    for name, ts in times.items():
        res.update(_stats(name, ts))
    res["texton_self_spread_ms"] = abs(res["texton_ms"] - res["texton_again_ms"])
    res["cue_1000_equal"] = bool(torch.equal(outs["texton"], outs["cue_1000"]))
    lo = min(res["texton_ms_min"], res["texton_again_ms_min"])
    hi = max(res["texton_ms_max"], res["texton_again_ms_max"])
    res["cue_1000_inside_texton_range"] = bool(lo <= res["cue_1000_ms"] <= hi)
    # (b), (c)
    four_out = [new() for _ in range(4)]
    for tag, wts in SETS.items():
        for suffix, g in (("", None), ("_joined", grad)):
            fused = new()

            def four():
                for c in range(4):
                    if wts[c]:
                        tex(planes[c], K if c == 0 else BINS, g, four_out[c])
            times = _turns(torch, {f"cue_{tag}{suffix}": lambda: cue(wts, g, fused), f"four_{tag}{suffix}": four})
            for name, ts in times.items():
                res.update(_stats(name, ts))
            res[f"fused_no_slower_than_four_{tag}{suffix}"] = bool(res[f"cue_{tag}{suffix}_ms"] <= res[f"four_{tag}{suffix}_ms"])
            res[f"cue_over_four_{tag}{suffix}"] = res[f"cue_{tag}{suffix}_ms"] / res[f"four_{tag}{suffix}_ms"]
            res[f"cue_{tag}{suffix}_map_max"] = int(fused.max())
    for c, name in enumerate(("labels", "Y", "Co", "Cg")):
        kc = K if c == 0 else BINS
        seen = torch.zeros((BATCH, kc, -(-H // 8), -(-W // 32)), dtype=torch.bool, device="cuda")
        for j in range(kc):                                   # (clipped instead of mirrored: a close count)
            pl = torch.nn.functional.max_pool2d((planes[c] == j).to(torch.float32)[:, None], (8 + 2 * RADIUS, 32 + 2 * RADIUS),
                                                stride=(8, 32), padding=(RADIUS, RADIUS), ceil_mode=True)
            seen[:, j] = pl[:, 0, :seen.shape[2], :seen.shape[3]] > 0
        res["bins_per_tile_" + name] = float(seen.sum(1).to(torch.float32).mean())
    del seen, four_out, planes
    # (d)
    times = _turns(torch, dict(cue_edges_2211=lambda: seg.cue_edges_device(imgs, weights=SETS["2211"]),
                               cue_edges_0111=lambda: seg.cue_edges_device(imgs, weights=SETS["0111"]),
                               texton_edges=lambda: seg.texton_edges_device(imgs)))
    for name, ts in times.items():
        res.update(_stats(name, ts))
    res["cue_edges_0111_saves_ms"] = res["texton_edges_ms"] - res["cue_edges_0111_ms"]
    print(json.dumps(res), flush=True)
    # (e) "off means unchanged": the existing steps against the parent commit's library
    plans = dict(parent=(_with_library(parent, lambda: Segmenter()), _with_library(parent, lambda: Segmenter(k=K, **COLOUR))),
                 step=(Segmenter(), seg))
    held = {name: new() for name in plans}

    def texton_launch(pair, name):
        pair[1].ops.texton_gradient(labels, BATCH, H, W, K, RADIUS, N_DIR, grad, held[name], None)
        return held[name]

    def cue_launch(pair, name):
        pair[1].ops.cue_gradient(labels, i0, BATCH, H, W, K, BINS, SETS["2211"], RADIUS, N_DIR, grad, held[name], None)
        return held[name]
    runs = dict(default=lambda pair, name: pair[0].segment_device(imgs), texton_edges=lambda pair, name: pair[1].texton_edges_device(imgs),
                texton_gradient=texton_launch, cue_gradient=cue_launch)
    for what, fn in runs.items():
        got = {}
        arms = ("parent", "step") if what != "cue_gradient" or hasattr(plans["parent"][1].ops.lib, "gcs_cue_gradient") else ("step",)
        times = _turns(torch, {name: (lambda nm: lambda: got.__setitem__(nm, fn(plans[nm], nm)))(name) for name in arms})
        for name, ts in times.items():
            res.update(_stats(f"{name}_{what}", ts))
        if "parent" in arms:
            res[what + "_equal"] = bool(torch.equal(got["step"], got["parent"]))
            res[what + "_inside_parent_range"] = bool(res[f"parent_{what}_ms_min"] <= res[f"step_{what}_ms"] <= res[f"parent_{what}_ms_max"])
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
