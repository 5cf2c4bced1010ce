#!/usr/bin/env python3
"""Cost of the region tree on k-means clusters (SPEC.md §21) at batch 64 x 481x321, colour bank (5, 1/8, 4; D = 72), R = 8, on the
24 val fixture images (landscape ones transposed, repeated to 64).

    cluster_tree_time.py time  [out.json] --parent path/to/parent/libgcs.so
    cluster_tree_time.py trace --parent path/to/parent/libgcs.so     (under rocprofv3 --kernel-trace -f csv -d <dir> -o run --)
    cluster_tree_time.py split <run_kernel_trace.csv> <out.json>

``time``: medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs:
  step_clusters_k16_ms, _k12_ms, _k8_ms       Segmenter(tree_nodes="clusters", n_regions=8, k=k).segment_device
  step_kmeans_k16_ms                          the same plan without the option (the Lloyd loop the mode runs in front of the tree)
  step_default_ms / parent_default_ms         the k = 8 plan of the same bank, this library's calls taking turns with the PARENT
  step_components_ms / parent_components_ms   commit's library in this process, and Segmenter(n_superpixels=300, n_regions=8,
                                              tree_nodes="components") likewise: "off means unchanged" (…_labels_equal,
                                              …_inside_parent_range: the new median lies in the parent's min - max)
  nodes_ms, cut_ms                            gcs_region_nodes on the batch's k = 16 maps; gcs_region_tree_cut at R = 8
  tree_slab_ms                                gcs_region_tree_slab at K = 4096 on the slab and the node maps
  parent_unpack_ms, parent_tree_ms            gcs_features_unpack of that slab and gcs_region_tree on its tensor and the same node
                                              maps, through the parent's library (trees_equal: the same merges, costs and alive)
``trace`` runs the last three a few times; ``split`` adds the median time of rt_stats_slab_kernel, rt_stats_kernel and unpack_kernel
per launch (and of rt_zero_kernel, rt_merge_kernel) to the JSON: the statistics launch against unpack + statistics.
"""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 15, 3
BANK = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
BATCH, H, W, R, K_CAP = 64, 481, 321, 8, 4096
KERNELS = ("rt_stats_slab_kernel", "rt_stats_kernel", "unpack_kernel", "rt_zero_kernel", "rt_merge_kernel")


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(name, ts):
    return {name + "_ms": statistics.median(ts), name + "_ms_min": min(ts), name + "_ms_max": max(ts)}


def _batch(torch):
    import numpy as np
    val = np.load(os.path.join(ROOT, "tests", "golden", "bsd_val_images.npz"))
    imgs = [val["img_" + str(i)] for i in val["ids"]]
    imgs = [im if im.shape[:2] == (H, W) else np.ascontiguousarray(im.transpose(1, 0, 2)) for im in imgs]
    return torch.from_numpy(np.stack([imgs[i % len(imgs)] for i in range(BATCH)])).cuda()


def _with_parent(parent, make):
    """``make()`` with the package bound to the parent commit's library (tools/ab.py: one process, both builds)."""
    import ctypes
    from gabor_color_image_segmentation_amd import _lib
    here, sigs = _lib.LIB_PATH, dict(_lib.SIGNATURES)
    raw = ctypes.CDLL(os.path.abspath(parent))
    _lib.LIB_PATH, _lib._lib = os.path.abspath(parent), None
    _lib.SIGNATURES = {k: v for k, v in sigs.items() if hasattr(raw, k)}
    try:
        return make()
    finally:
        _lib.LIB_PATH, _lib._lib, _lib.SIGNATURES = here, None, sigs


def _pieces(torch, imgs, parent):
    """The slab, the node maps of the k = 16 maps and the three calls on them: (this library's plan, dict of name -> call, outputs)."""
    from gabor_color_image_segmentation_amd import Segmenter
    plan = Segmenter(tree_nodes="clusters", n_regions=R, k=16, **BANK)
    old = _with_parent(parent, lambda: Segmenter(k=16, **BANK))
    assert not hasattr(old.ops.lib, "gcs_region_tree_slab") and hasattr(plan.ops.lib, "gcs_region_tree_slab")
    ops, pops = plan.ops, old.ops
    n_map, ws = plan._cluster_maps(imgs, tree=False)
    feats = ws["feats"]
    new_bufs, old_bufs = ops.region_tree_buffers(BATCH, H, W, K_CAP), pops.region_tree_buffers(BATCH, H, W, K_CAP)
    canon = torch.empty((BATCH, plan.bank.n_features, H, W), dtype=torch.int16, device="cuda")
    calls = dict(tree_slab=lambda: ops.region_tree_slab(feats, n_map, BATCH, H, W, K_CAP, *new_bufs),
                 parent_unpack=lambda: pops.features_unpack(feats, BATCH, H, W, out=canon),
                 parent_tree=lambda: pops.region_tree(canon, n_map, BATCH, H, W, K_CAP, *old_bufs))
    return plan, ws, n_map, calls, new_bufs, old_bufs


def time_main(out_path, parent):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    imgs = _batch(torch)
    comp = dict(n_superpixels=300, spatial_weight=576, n_regions=R, tree_nodes="components", **BANK)
    plans = dict(parent_default=_with_parent(parent, lambda: Segmenter(**BANK)), step_default=Segmenter(**BANK),
                 parent_components=_with_parent(parent, lambda: Segmenter(**comp)), step_components=Segmenter(**comp),
                 step_kmeans_k16=Segmenter(k=16, **BANK),
                 step_clusters_k16=Segmenter(tree_nodes="clusters", n_regions=R, k=16, **BANK),
                 step_clusters_k12=Segmenter(tree_nodes="clusters", n_regions=R, k=12, **BANK),
                 step_clusters_k8=Segmenter(tree_nodes="clusters", n_regions=R, k=8, **BANK))
    res = dict(batch=BATCH, shape=[H, W], n_regions=R, K_cap=K_CAP, D=plans["step_default"].bank.n_features, reps=REPS, warm=WARM,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    times, outs = {name: [] for name in plans}, {}
    for group in (["parent_default", "step_default"], ["parent_components", "step_components"], ["step_kmeans_k16"],
                  ["step_clusters_k16"], ["step_clusters_k12"], ["step_clusters_k8"]):      # a pair takes turns, call by call, with nothing else between
        for rnd in range(WARM + REPS):
            for name in group:
                t = _timed(torch, lambda: outs.__setitem__(name, plans[name].segment_device(imgs)))
                if rnd >= WARM:
                    times[name].append(t)
        for name in group:
            if not name.endswith(("default", "components")):
                outs[name] = outs[name].amax(dim=(1, 2)) + 1         # (the label count is all that is kept of these)
            plans[name]._ws.clear()
        torch.cuda.empty_cache()
    for name, ts in times.items():
        res.update(_stats(name, ts))
    for what in ("default", "components"):
        res[what + "_labels_equal"] = bool(torch.equal(outs["step_" + what], outs["parent_" + what]))
        res[what + "_inside_parent_range"] = res[f"parent_{what}_ms_min"] <= res[f"step_{what}_ms"] <= res[f"parent_{what}_ms_max"]
    res["labels_per_image_k16"] = sorted({int(v) for v in outs["step_clusters_k16"]})
    res["clusters_faster_than_components"] = res["step_clusters_k16_ms"] < res["step_components_ms"]
    del plans, outs
    torch.cuda.empty_cache()
    plan, ws, n_map, calls, new_bufs, old_bufs = _pieces(torch, imgs, parent)
    ops = plan.ops
    ndws, raw, n_nodes = ws["nd"]
    out = torch.empty_like(n_map)
    calls = dict(calls, nodes=lambda: ops.region_nodes(raw, 0, out, n_nodes, scratch=ndws),
                 cut=lambda: ops.region_tree_cut(n_map, new_bufs[1], new_bufs[3], BATCH, H, W, K_CAP, R, out))
    for name in ("nodes", "tree_slab", "parent_unpack", "parent_tree", "cut"):
        res.update(_stats(name, [_timed(torch, calls[name]) for _ in range(WARM + REPS)][WARM:]))
    res["trees_equal"] = all(bool(torch.equal(a, b)) for a, b in zip(new_bufs[1:], old_bufs[1:]))
    res["tree_slab_minus_unpack_and_tree_ms"] = res["tree_slab_ms"] - res["parent_unpack_ms"] - res["parent_tree_ms"]
    counts = n_nodes.cpu().numpy()
    res["nodes_per_image"] = dict(min=int(counts.min()), mean=float(counts.mean()), max=int(counts.max()))
    res["canonical_tensor_bytes"] = BATCH * plan.bank.n_features * H * W * 2
    res["slab_bytes"] = int(ws["feats"].numel())
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def trace_main(parent):
    sys.path.insert(0, ROOT)
    import torch
    imgs = _batch(torch)
    _, _, _, calls, _, _ = _pieces(torch, imgs, parent)
    for _ in range(WARM + REPS):
        for name in ("tree_slab", "parent_unpack", "parent_tree"):
            calls[name]()
        torch.cuda.current_stream().synchronize()


def split_main(trace, out_path):
    with open(trace) as f:
        rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in csv.DictReader(f)]
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    for key in KERNELS:                                  # ("rt_stats_kernel" is no substring of "rt_stats_slab_kernel")
        ts = [t for name, t in rows if key in name][-REPS:]
        res["trace_" + key + "_ms"] = statistics.median(ts)
    res["stats_slab_no_slower_than_unpack_and_stats"] = \
        res["trace_rt_stats_slab_kernel_ms"] <= res["trace_unpack_kernel_ms"] + res["trace_rt_stats_kernel_ms"]
    print(json.dumps({k: v for k, v in res.items() if k.startswith(("trace_", "stats_slab"))}))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    args = sys.argv[2:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    if mode == "split":
        split_main(args[0], args[1])
    elif parent is None:
        sys.exit("the parent commit's libgcs.so is needed: --parent path")
    elif mode == "trace":
        trace_main(parent)
    else:
        paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
        time_main(paths[0] if paths else None, parent)
