#!/usr/bin/env python3
"""Cost of the texture-gradient edge map (SPEC.md §22) at batch 64 x 481x321 on the 24 val fixture images (landscape ones
transposed, repeated to 64), on the default bank (4 x 6, D = 72, split slab) and on a wide-slab bank (4 x 7, D = 84). GPU only.

    feature_gradient_time.py [out.json] --parent path/to/parent/libgcs.so [--variant name=path/to/libgcs.so ...]

Medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs; the calls
of one bank take turns, call by call:
  <bank>_gradient_ms          gcs_feature_gradient on the slab of the batch (one launch)
  <bank>_unpack_ms            gcs_features_unpack of the same slab alone: the first step of any formulation without the kernel
  <bank>_torch_ms             a torch formulation of §22 on the unpacked tensor (<bank>_torch_equal: the same map, every value)
  <bank>_gradient_over_unpack the ratio of the two medians; <bank>_gradient_no_slower_than_unpack is the condition of DESIGN.md §4.20
  <bank>_<name>_gradient_ms   the same launch through every --variant library (e.g. a -DGCS_FG_PER_PIXEL build), taking turns
                              with this library's (…_equal: the same map)
  edges_device_ms             Segmenter.edges_device on the default bank (Gabor stage + the launch)
  edge_sweep_ms               evaluate_gpu.edge_sweep_resident at 256 levels on the batch's map and its resident annotator maps
                              (device work, one download and the host arithmetic; a host clock around the call)
  step_default_ms / parent_default_ms, step_components_ms / parent_components_ms
                              Segmenter.segment_device of the default plan and of Segmenter(n_superpixels=300, n_regions=8,
                              tree_nodes="components") on the colour bank, this library's calls taking turns with the PARENT
                              commit's library in this process: "off means unchanged" (…_labels_equal, …_inside_parent_range: the
                              new median lies in the parent's min - max)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 15, 3
BATCH, H, W, LEVELS = 64, 481, 321, 256
BANKS = dict(default=dict(n_scales=4, n_orient=6), wide=dict(n_scales=4, n_orient=7))
COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(name, ts):
    return {name + "_ms": statistics.median(ts), name + "_ms_min": min(ts), name + "_ms_max": max(ts)}


def _val():
    import numpy as np
    val = np.load(os.path.join(ROOT, "tests", "golden", "bsd_val_images.npz"))
    return val, [str(i) for i in val["ids"]]


def _batch(torch):
    import numpy as np
    val, ids = _val()
    imgs = [val["img_" + i] for i in ids]
    imgs = [im if im.shape[:2] == (H, W) else np.ascontiguousarray(im.transpose(1, 0, 2)) for im in imgs]
    return torch.from_numpy(np.stack([imgs[i % len(imgs)] for i in range(BATCH)])).cuda()


def _truth():
    """The resident annotator maps of the batch (landscape maps transposed like their images)."""
    import numpy as np
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    _, ids = _val()
    packed = PackedTruth(os.path.join(ROOT, "tests", "golden", "bsd500_truth.npz"))
    maps, first, img_of = [], [0], []
    for b in range(BATCH):
        for m in packed[ids[b % len(ids)]]:
            maps.append(m if m.shape == (H, W) else np.ascontiguousarray(m.T))
            img_of.append(b)
        first.append(len(maps))
    return DeviceTruth(np.stack(maps), first, img_of, [int(m.max()) + 1 for m in maps])


def _with_library(path, make):
    """``make()`` with the package bound to another build of the library (tools/ab.py: one process, several builds)."""
    import ctypes
    from gabor_color_image_segmentation_amd import _lib
    here, sigs = _lib.LIB_PATH, dict(_lib.SIGNATURES)
    raw = ctypes.CDLL(os.path.abspath(path))
    _lib.LIB_PATH, _lib._lib = os.path.abspath(path), None
    _lib.SIGNATURES = {k: v for k, v in sigs.items() if hasattr(raw, k)}
    try:
        return make()
    finally:
        _lib.LIB_PATH, _lib._lib, _lib.SIGNATURES = here, None, sigs


def torch_edges(torch, canon, n_scales, slots):
    """SPEC.md §22 in torch ops on the canonical (B, D, H, W) int16 tensor: (B, H, W) int32."""
    b, d, h, w = canon.shape
    f_n = n_scales * slots
    e = torch.zeros((b, h, w), dtype=torch.int64, device=canon.device)
    for lv in range((n_scales + 1) // 2):
        planes = [c * f_n + s * slots + o for c in range(3) for s in (2 * lv, 2 * lv + 1) if s < n_scales for o in range(slots)]
        g = canon[:, planes][:, :, ::1 << lv, ::1 << lv].to(torch.int32) & 0xFFFF
        hl, wl = g.shape[2:]
        ix, iy = torch.arange(wl, device=canon.device), torch.arange(hl, device=canon.device)
        dx = (g[..., (ix + 1).clamp(max=wl - 1)] - g[..., (ix - 1).clamp(min=0)]).to(torch.int64).pow(2).sum(1) >> (2 * lv)
        dy = (g[:, :, (iy + 1).clamp(max=hl - 1)] - g[:, :, (iy - 1).clamp(min=0)]).to(torch.int64).pow(2).sum(1) >> (2 * lv)
        t = dx + dy
        if lv:
            t = t.repeat_interleave(1 << lv, 1).repeat_interleave(1 << lv, 2)[:, :h, :w]
        e += t
    r = e.to(torch.float64).sqrt().to(torch.int64)
    r -= (r * r > e).to(torch.int64)
    r += ((r + 1) * (r + 1) <= e).to(torch.int64)
    return r.to(torch.int32)


def main(out_path, parent, variants):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.segmenter import HipOps, _step_features
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], levels=LEVELS, reps=REPS, warm=WARM, variants=sorted(variants),
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    for bank, kw in BANKS.items():
        seg = Segmenter(**kw)
        ops, ns, no = seg.ops, kw["n_scales"], kw["n_orient"]
        ws = seg._tail_workspace(BATCH, H, W, "per_image", slab_only=True)
        _step_features(ops, seg._opt, ws, imgs, BATCH, H, W)
        feats = ws["feats"]
        out = torch.full((BATCH, H, W), -1, dtype=torch.int32, device="cuda")
        canon = torch.empty((BATCH, seg.bank.n_features, H, W), dtype=torch.int16, device="cuda")
        outs = {name: torch.full((BATCH, H, W), -1, dtype=torch.int32, device="cuda") for name in variants}
        vops = {name: _with_library(path, lambda: HipOps(seg.bank, "cuda:0")) for name, path in variants.items()}
        calls = dict(gradient=lambda: ops.feature_gradient(feats, BATCH, H, W, out),
                     unpack=lambda: ops.features_unpack(feats, BATCH, H, W, out=canon))
        for name in variants:
            calls[name + "_gradient"] = (lambda n: lambda: vops[n].feature_gradient(feats, BATCH, H, W, outs[n]))(name)
        times = {name: [] for name in calls}
        for rnd in range(WARM + REPS):
            for name, fn in calls.items():
                t = _timed(torch, fn)
                if rnd >= WARM:
                    times[name].append(t)
        for name, ts in times.items():
            res.update(_stats(f"{bank}_{name}", ts))
        for name in variants:
            res[f"{bank}_{name}_equal"] = bool(torch.equal(out, outs[name]))
        res[f"{bank}_gradient_over_unpack"] = res[f"{bank}_gradient_ms"] / res[f"{bank}_unpack_ms"]
        res[f"{bank}_gradient_no_slower_than_unpack"] = res[f"{bank}_gradient_ms"] <= res[f"{bank}_unpack_ms"]
        via = {}
        res.update(_stats(f"{bank}_torch", [_timed(torch, lambda: via.__setitem__("g", torch_edges(torch, canon, ns, no)))
                                            for _ in range(WARM + 5)][WARM:]))
        res[f"{bank}_torch_equal"] = bool(torch.equal(out, via["g"]))
        res[f"{bank}_map_max"] = int(out.max())
        res[f"{bank}_slab_bytes"] = int(feats.numel())
        res[f"{bank}_canonical_tensor_bytes"] = int(canon.numel()) * 2
        if bank == "default":
            res.update(_stats("edges_device", [_timed(torch, lambda: seg.edges_device(imgs)) for _ in range(WARM + REPS)][WARM:]))
            truth = _truth()
            ts = []
            for _ in range(WARM + 5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = edge_sweep_resident(out, truth, levels=LEVELS)[2]
                ts.append((time.perf_counter() - t0) * 1e3)
            res.update(_stats("edge_sweep", ts[WARM:]))
            res["edge_sweep_annotator_maps"] = truth.t
            res["edge_sweep_best_mean_f"] = float(f.mean(axis=0).max())
            del truth
        del ws, feats, canon, out, outs, via, calls, vops, seg
        torch.cuda.empty_cache()
        print(json.dumps({k: v for k, v in res.items() if k.startswith(bank)}), flush=True)
    # "off means unchanged": the existing steps against the parent commit's library
    comp = dict(n_superpixels=300, spatial_weight=576, n_regions=8, tree_nodes="components", **COLOUR)
    plans = dict(parent_default=_with_library(parent, lambda: Segmenter()), step_default=Segmenter(),
                 parent_components=_with_library(parent, lambda: Segmenter(**comp)), step_components=Segmenter(**comp))
    assert not hasattr(plans["parent_default"].ops.lib, "gcs_feature_gradient")
    times, outs = {name: [] for name in plans}, {}
    for group in (["parent_default", "step_default"], ["parent_components", "step_components"]):
        for rnd in range(WARM + REPS):
            for name in group:
                t = _timed(torch, lambda: outs.__setitem__(name, plans[name].segment_device(imgs)))
                if rnd >= WARM:
                    times[name].append(t)
        for name in group:
            plans[name]._ws.clear()
        torch.cuda.empty_cache()
    for name, ts in times.items():
        res.update(_stats(name, ts))
    for what in ("default", "components"):
        res[what + "_labels_equal"] = bool(torch.equal(outs["step_" + what], outs["parent_" + what]))
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
