#!/usr/bin/env python3
"""Cost of the texton gradient (SPEC.md §24) at batch 64 x 481x321 on the 24 val fixture images (landscape ones transposed,
repeated to 64), colour bank (n_orient 5, color_weight 1/8, chroma_gain 4), r = 8, n = 8. GPU only.

    texton_gradient_time.py [out.json] --parent path/to/parent/libgcs.so [--variant no_skip=path/to/libgcs.so]

Medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs; calls
that are compared take turns, call by call:
  k<k>_tg_ms / k<k>_joined_ms   (a) gcs_texton_gradient on the plan's own k-means map of the batch (k = 8, 16), without / with grad
  k<k>_<name>_tg_ms                 the same launch through every --variant library (a -DGCS_TG_NO_SKIP build: every label walked),
                                    taking turns with this library's (…_equal: the same map)
  k<k>_labels_per_tile              mean number of labels an 8 x 32 tile's window holds (what the skip leaves to walk)
  k<k>_torch_ms                 (b) a torch formulation with equal results: one-hot planes, reflect padding, conv2d with the half
                                    discs, integer chi-square (in chunks of 8 images: its planes at 64 would take 5 GB);
                                    k<k>_torch_equal: the same map, every value; k<k>_kernel_no_slower_than_torch
  feature_gradient_ms           (c) gcs_feature_gradient on the same batch's slab, for scale
  texton_edges_device_ms        (d) Segmenter.texton_edges_device end to end (features, G, Lloyd loop, labels, the kernel), k = 8;
                                    texton_alone_device_ms: joined=False
  step_default_ms / parent_default_ms, step_edges_ms / parent_edges_ms
                                (e) Segmenter.segment_device of the default plan and Segmenter.edges_device, this library's calls
                                    taking turns with the PARENT commit's library in this process (…_equal: the same output,
                                    …_inside_parent_range: the new median lies in the parent's min - max); the parent may itself
                                    export gcs_texton_gradient: only these two existing calls go through it
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from feature_gradient_time import _batch, _stats, _timed, _with_library, BATCH, H, W  # noqa: E402

REPS, WARM = 15, 3
RADIUS, N_DIR = 8, 8
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
CHUNK = 8


def torch_texton(torch, labels, K, masks, r, grad=None):
    """SPEC.md §24 in torch ops: (B,H,W) int32 labels, masks (n,2,2r+1) int32 -> TG or E, (B,H,W) int32."""
    import torch.nn.functional as F
    n, width = masks.shape[0], 2 * r + 1
    bits = torch.arange(width, device=labels.device, dtype=torch.int32)
    kern = ((masks.reshape(2 * n, width, 1) >> bits) & 1).to(torch.float32).reshape(2 * n, 1, width, width)
    out = []
    for c0 in range(0, labels.shape[0], CHUNK):
        lab = labels[c0:c0 + CHUNK]
        b, h, w = lab.shape
        planes = (lab[:, None] == torch.arange(K, device=lab.device, dtype=torch.int32)[None, :, None, None]).to(torch.float32)
        planes = F.pad(planes.reshape(b * K, 1, h, w), (r, r, r, r), mode="reflect")
        cnt = F.conv2d(planes, kern).to(torch.int32).reshape(b, K, n, 2, h, w)          # counts <= 961: exact in float32
        g, hh = cnt[:, :, :, 0], cnt[:, :, :, 1]
        chi = torch.div(64 * (g - hh) ** 2, (g + hh).clamp(min=1), rounding_mode="floor").sum(1)      # the floor is per bin
        tg = chi.max(1).values
        if grad is not None:
            e = tg.to(torch.int64) * grad[c0:c0 + CHUNK].to(torch.int64)
            root = e.to(torch.float64).sqrt().to(torch.int64)
            root -= (root * root > e).to(torch.int64)
            root += ((root + 1) * (root + 1) <= e).to(torch.int64)
            tg = root
        out.append(tg.to(torch.int32))
    return torch.cat(out)


def main(out_path, parent, variants):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.segmenter import HipOps, _step_features
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], reps=REPS, warm=WARM, radius=RADIUS, n_directions=N_DIR, bank=COLOUR,
               variants=sorted(variants), torch_chunk=CHUNK,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    new = lambda: torch.full((BATCH, H, W), -1, dtype=torch.int32, device="cuda")
    for k in (8, 16):
        seg = Segmenter(k=k, **COLOUR)
        ops = seg.ops
        labels = seg.segment_device(imgs)
        grad = seg.edges_device(imgs)
        masks = ops.texton_masks(RADIUS, N_DIR)
        vops = {name: _with_library(path, lambda: HipOps(seg.bank, "cuda:0")) for name, path in variants.items()}
        outs = dict(tg=new(), joined=new(), **{name + "_tg": new() for name in variants})
        calls = dict(tg=lambda: ops.texton_gradient(labels, BATCH, H, W, k, RADIUS, N_DIR, None, outs["tg"], None),
                     joined=lambda: ops.texton_gradient(labels, BATCH, H, W, k, RADIUS, N_DIR, grad, outs["joined"], None))
        for name in variants:
            calls[name + "_tg"] = (lambda nm: lambda: vops[nm].texton_gradient(labels, BATCH, H, W, k, RADIUS, N_DIR, None,
                                                                                outs[nm + "_tg"], None, masks=masks))(name)
        times = {name: [] for name in calls}
        for rnd in range(WARM + REPS):
            for name, fn in calls.items():
                t = _timed(torch, fn)
                if rnd >= WARM:
                    times[name].append(t)
        for name, ts in times.items():
            res.update(_stats(f"k{k}_{name}", ts))
        for name in variants:
            res[f"k{k}_{name}_equal"] = bool(torch.equal(outs["tg"], outs[name + "_tg"]))
        # labels in the window of a tile (rows 8 + 2r, columns 32 + 2r, clipped instead of mirrored: a close count)
        seen = torch.zeros((BATCH, k, -(-H // 8), -(-W // 32)), dtype=torch.bool, device="cuda")
        for j in range(k):
            pl = torch.nn.functional.max_pool2d((labels == j).to(torch.float32)[:, None], (8 + 2 * RADIUS, 32 + 2 * RADIUS),
                                                stride=(8, 32), padding=(RADIUS, RADIUS), ceil_mode=True)
            seen[:, j] = pl[:, 0, :seen.shape[2], :seen.shape[3]] > 0
        res[f"k{k}_labels_per_tile"] = float(seen.sum(1).to(torch.float32).mean())
        via = {}
        for key, g in (("torch", None), ("torch_joined", grad)):
            ts = [_timed(torch, lambda: via.__setitem__(key, torch_texton(torch, labels, k, masks, RADIUS, g)))
                  for _ in range(2 + 3)][2:]
            res.update(_stats(f"k{k}_{key}", ts))
        res[f"k{k}_torch_equal"] = bool(torch.equal(outs["tg"], via["torch"]) and torch.equal(outs["joined"], via["torch_joined"]))
        res[f"k{k}_kernel_no_slower_than_torch"] = res[f"k{k}_tg_ms"] <= res[f"k{k}_torch_ms"]
        res[f"k{k}_map_max"] = int(outs["tg"].max())
        if k == 8:
            ws = seg._tail_workspace(BATCH, H, W, "per_image", slab_only=True)
            _step_features(ops, seg._opt, ws, imgs, BATCH, H, W)
            res.update(_stats("feature_gradient", [_timed(torch, lambda: ops.feature_gradient(ws["feats"], BATCH, H, W, outs["joined"]))
                                                   for _ in range(WARM + REPS)][WARM:]))
            del ws
            res.update(_stats("texton_edges_device", [_timed(torch, lambda: seg.texton_edges_device(imgs))
                                                      for _ in range(WARM + REPS)][WARM:]))
            res.update(_stats("texton_alone_device", [_timed(torch, lambda: seg.texton_edges_device(imgs, joined=False))
                                                      for _ in range(WARM + REPS)][WARM:]))
        del seg, ops, labels, grad, outs, via, calls, vops, seen
        torch.cuda.empty_cache()
        print(json.dumps({key: v for key, v in res.items() if key.startswith(f"k{k}_")}), flush=True)
    # "off means unchanged": the existing steps against the parent commit's library
    plans = dict(parent=_with_library(parent, lambda: Segmenter()), step=Segmenter())
    runs = dict(default=lambda s: s.segment_device(imgs), edges=lambda s: s.edges_device(imgs))
    for what, fn in runs.items():
        times, outs = dict(parent=[], step=[]), {}
        for rnd in range(WARM + REPS):
            for name in ("parent", "step"):
                t = _timed(torch, lambda: outs.__setitem__(name, fn(plans[name])))
                if rnd >= WARM:
                    times[name].append(t)
        for name, ts in times.items():
            res.update(_stats(f"{name}_{what}", ts))
        res[what + "_equal"] = bool(torch.equal(outs["step"], outs["parent"]))
        res[what + "_inside_parent_range"] = res[f"parent_{what}_ms_min"] <= res[f"step_{what}_ms"] <= res[f"parent_{what}_ms_max"]
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
