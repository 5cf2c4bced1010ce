#!/usr/bin/env python3
"""Cost of thin boundary maps (SPEC.md §26) at batch 64 x 481x321 on the 24 val fixture images (landscape ones transposed, repeated
to 64), colour bank (n_orient 5, color_weight 1/8, chroma_gain 4), k = 8, r = 8, n = 8, 16 bins, weights (2, 2, 1, 1). GPU only.

    edge_thin_time.py [out.json] --parent path/to/parent/libgcs.so
    edge_thin_time.py trace       (under `rocprofv3 --kernel-trace --stats -f csv -d <dir> -o run --`: the chain once, then TRAIN
                                   launches of gcs_edge_thin alone; et_kernel's row of the stats is the kernel's own time)

Medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs; calls
that are compared take turns, call by call (the method of tools/cue_gradient_time.py):
  thin_ms, thin_again_ms, torch_thin_ms
                            (a) the gcs_edge_thin launch on E' and its direction map, TWICE in the rotation (thin_self_spread_ms),
                                against the same rule in torch operations (``torch_thin``: per direction two shifted sums on the
                                whole batch in int64, selected by dir; torch_thin_equal: the same map); thin_over_torch.
                                thin_train_ms: TRAIN launches between ONE pair of events, divided by TRAIN - a pair of events
                                around one launch of tens of microseconds measures the events as much as the kernel
  thin_bytes, hbm_floor_ms, thin_over_hbm_floor
                            (b) the launch against its traffic, 9 bytes per pixel (E read, dir read, T written), at the achievable
                                HBM rate of an MI355X, 6.3 TB/s (HBM_TBPS)
  cue_edges_ms / cue_edges_thin_ms, texton_edges_ms / texton_edges_thin_ms
                            (c) Segmenter.cue_edges_device and texton_edges_device without and with ``thin``, end to end;
                                …_thin_adds_ms
  step_<what>_ms / parent_<what>_ms
                            (d) "off means unchanged": cue_edges_device() and texton_edges_device() (no ``thin``) and
                                segment_device of the default plan with this library and with the PARENT commit's library in this
                                process, taking turns (…_equal: the same output, …_inside_parent_range: the new median lies in the
                                parent's min - max)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cue_gradient_time import _turns, COLOUR, K, N_DIR, RADIUS  # noqa: E402
from feature_gradient_time import _batch, _stats, _timed, _with_library, BATCH, H, W  # noqa: E402

HBM_TBPS = 6.3
TRAIN = 50


def torch_thin(torch, edges, dirs, steps):
    """SPEC.md §26 in torch operations: (B,H,W) int32. ``steps``: the (n, 8) table as a list of rows on the host."""
    v = edges.clamp(min=0).to(torch.int64)
    h, w = v.shape[1:]
    iy, ix = torch.arange(h, device=v.device), torch.arange(w, device=v.device)
    tap = lambda dy, dx: v[:, (iy + dy).clamp(0, h - 1)][:, :, (ix + dx).clamp(0, w - 1)]
    keep = torch.zeros_like(v, dtype=torch.bool)
    for i, (dy1, dx1, dy2, dx2, w1, w2, _, _) in enumerate(steps):
        plus = w1 * tap(dy1, dx1) + w2 * tap(dy2, dx2)
        minus = w1 * tap(-dy1, -dx1) + w2 * tap(-dy2, -dx2)
        mv = (w1 + w2) * v
        keep |= (dirs == i) & (mv > minus) & (mv >= plus)
    return torch.where(keep & (v > 0), v, torch.zeros_like(v)).to(torch.int32)


def _inputs(torch):
    """(imgs, the colour plan, E', dir) of the batch."""
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _batch(torch)
    seg = Segmenter(k=K, **COLOUR)
    labels, grad = seg.segment_device(imgs), seg.edges_device(imgs)
    i0 = torch.empty_like(imgs)
    seg.ops.colour_opponent(imgs, i0)
    ep, dirs = seg.cue_gradient_device(labels, i0, K=K, gradient=grad, directions=True)
    return imgs, seg, ep, dirs


def trace():
    sys.path.insert(0, ROOT)
    import torch
    imgs, seg, ep, dirs = _inputs(torch)
    out = torch.empty_like(ep)
    for _ in range(TRAIN):
        seg.ops.edge_thin(ep, dirs, BATCH, H, W, N_DIR, out)
    torch.cuda.synchronize()
    print("kept", int(torch.count_nonzero(out)), "of", int(torch.count_nonzero(ep)))


def main(out_path, parent):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    imgs, seg, ep, dirs = _inputs(torch)
    res = dict(batch=BATCH, shape=[H, W], radius=RADIUS, n_directions=N_DIR, k=K, bank=COLOUR, hbm_tbps=HBM_TBPS,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    ops = seg.ops
    steps = ops.thin_steps(N_DIR).cpu().tolist()
    new = lambda: torch.full((BATCH, H, W), -1, dtype=torch.int32, device="cuda")
    outs = dict(thin=new(), thin_again=new())
    held = {}
    # (a)
    times = _turns(torch, dict(thin=lambda: ops.edge_thin(ep, dirs, BATCH, H, W, N_DIR, outs["thin"]),
                               torch_thin=lambda: held.__setitem__("torch", torch_thin(torch, ep, dirs, steps)),
                               thin_again=lambda: ops.edge_thin(ep, dirs, BATCH, H, W, N_DIR, outs["thin_again"])))
    for name, ts in times.items():
        res.update(_stats(name, ts))
    res["thin_self_spread_ms"] = abs(res["thin_ms"] - res["thin_again_ms"])
    res["torch_thin_equal"] = bool(torch.equal(outs["thin"], held["torch"]) and torch.equal(outs["thin"], outs["thin_again"]))
    res["thin_over_torch"] = res["thin_ms"] / res["torch_thin_ms"]
    def train():
        for _ in range(TRAIN):
            ops.edge_thin(ep, dirs, BATCH, H, W, N_DIR, outs["thin_again"])
    res.update(_stats("thin_train", [_timed(torch, train) / TRAIN for _ in range(8)][3:]))
    res["thin_kept_fraction"] = float(torch.count_nonzero(outs["thin"])) / float(torch.count_nonzero(ep))
    # (b)
    res["thin_bytes"] = 9 * BATCH * H * W
    res["hbm_floor_ms"] = res["thin_bytes"] / (HBM_TBPS * 1e12) * 1e3
    res["thin_over_hbm_floor"] = res["thin_ms"] / res["hbm_floor_ms"]
    res["thin_train_over_hbm_floor"] = res["thin_train_ms"] / res["hbm_floor_ms"]
    del held["torch"]
    # (c)
    times = _turns(torch, dict(cue_edges=lambda: seg.cue_edges_device(imgs), cue_edges_thin=lambda: seg.cue_edges_device(imgs, thin=True),
                               texton_edges=lambda: seg.texton_edges_device(imgs),
                               texton_edges_thin=lambda: seg.texton_edges_device(imgs, thin=True)))
    for name, ts in times.items():
        res.update(_stats(name, ts))
    for what in ("cue_edges", "texton_edges"):
        res[what + "_thin_adds_ms"] = res[what + "_thin_ms"] - res[what + "_ms"]
    res["cue_edges_thin_equal"] = bool(torch.equal(seg.cue_edges_device(imgs, thin=True), outs["thin"]))
    print(json.dumps(res), flush=True)
    # (d) "off means unchanged": the existing steps against the parent commit's library
    plans = dict(parent=(_with_library(parent, lambda: Segmenter()), _with_library(parent, lambda: Segmenter(k=K, **COLOUR))),
                 step=(Segmenter(), seg))
    runs = dict(default=lambda pair: pair[0].segment_device(imgs), cue_edges=lambda pair: pair[1].cue_edges_device(imgs),
                texton_edges=lambda pair: pair[1].texton_edges_device(imgs))
    for what, fn in runs.items():
        got = {}
        times = _turns(torch, {name: (lambda nm: lambda: got.__setitem__(nm, fn(plans[nm])))(name) for name in ("parent", "step")})
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
    if args[:1] == ["trace"]:
        trace()
        sys.exit(0)
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    if parent is None:
        sys.exit("the parent commit's libgcs.so is needed: --parent path")
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
    main(paths[0] if paths else None, parent)
