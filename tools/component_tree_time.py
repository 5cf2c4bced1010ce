#!/usr/bin/env python3
"""Cost of the region tree on connected regions (SPEC.md §18) at batch 64 x 481x321, colour bank (5, 1/8, 4; D = 72), n = 300,
lambda = 576, R = 8, on the 24 val fixture images (landscape ones transposed, repeated to 64): the node count is what the mode costs,
and the photographs' is the one that matters.

    component_tree_time.py time  [out.json] [--parent path/to/parent/libgcs.so]
    component_tree_time.py trace                      (under rocprofv3 --kernel-trace -f csv -d <dir> -o run --)
    component_tree_time.py split <run_kernel_trace.csv> <out.json>

``time``: medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs:
  step_components_ms   Segmenter(n_superpixels=300, n_regions=8, tree_nodes="components").segment_device
  step_superpixels_ms  the same plan with tree_nodes="superpixels", its calls taking turns with ...
  parent_step_ms       (--parent) ... the same plan through the PARENT commit's library, in this process: "off means unchanged"
                       (parent_labels_equal; superpixels_inside_parent_range: the new median lies in the parent's min - max)
  nodes_ms             gcs_region_nodes on the batch's superpixel maps (one call, m = 0)
  tree_ms, cut_ms      gcs_region_tree at K = 4096 on the node maps; gcs_region_tree_cut at R = 8
  small_first_call_ms  by the host's clock: the first one-image segment_batch of a fresh plan (warm-up step on an all-zero image - its
                       nodes are the grid cells, the K - 1-round case of §14 at K = 4096 capacity -, capture, first replay), per mode
  small_replay_ms      by the host's clock: the median of the replays that follow
``trace`` runs warm + reps steps of the components plan; ``split`` adds, per kernel, the median over those steps of the time the
kernel's launches take in one step (the node map's kernels summed as ``nodes_kernels_ms``) to the JSON.
"""
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 25, 4
BANK = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
BATCH, H, W, N, LAM, R, K_CAP = 64, 481, 321, 300, 576, 8, 4096
NODE_KERNELS = ("mr_init_kernel", "cc_union_kernel", "rn_count_kernel", "mr_flatten_kernel", "mr_size_kernel", "rn_best_kernel",
                "mr_union_kernel", "cc_rank_kernel", "cc_relabel_kernel")
TREE_KERNELS = ("rt_zero_kernel", "rt_stats_kernel", "rt_merge_kernel", "rt_cut_kernel")


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


def _plan(tree_nodes):
    from gabor_color_image_segmentation_amd import Segmenter
    return Segmenter(n_superpixels=N, spatial_weight=LAM, n_regions=R, tree_nodes=tree_nodes, **BANK)


def time_main(out_path=None, parent=None):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    plans = {}
    if parent:                                           # the parent's library first (tools/ab.py: one process, both builds)
        import ctypes
        here, sigs = _lib.LIB_PATH, dict(_lib.SIGNATURES)
        raw = ctypes.CDLL(os.path.abspath(parent))
        _lib.LIB_PATH, _lib._lib = os.path.abspath(parent), None
        _lib.SIGNATURES = {k: v for k, v in sigs.items() if hasattr(raw, k)}
        plans["parent_step"] = Segmenter(n_superpixels=N, spatial_weight=LAM, n_regions=R, **BANK)
        _lib.LIB_PATH, _lib._lib, _lib.SIGNATURES = here, None, sigs
    imgs = _batch(torch)
    plans["step_superpixels"] = _plan("superpixels")
    plans["step_components"] = comp = _plan("components")
    res = dict(batch=BATCH, shape=[H, W], n_superpixels=N, spatial_weight=LAM, n_regions=R, K_cap=K_CAP, D=comp.bank.n_features,
               reps=REPS, warm=WARM, images="24 val fixture images, landscape ones transposed, repeated to 64",
               tree_workspace_bytes_per_image=comp.ops.lib.gcs_region_tree_workspace_bytes(1, H, W, comp.bank.n_features, K_CAP),
               tree_workspace_bytes=comp.ops.lib.gcs_region_tree_workspace_bytes(BATCH, H, W, comp.bank.n_features, K_CAP))
    times, outs = {name: [] for name in plans}, {}
    turns = [[n for n in plans if n != "step_components"], ["step_components"]]
    for group in turns:                                  # this library's "superpixels" step and the parent's take turns, call by
        for rnd in range(WARM + REPS):                   # call, with nothing else between them; the new mode runs behind them
            for name in group:
                t = _timed(torch, lambda: outs.__setitem__(name, plans[name].segment_device(imgs)))
                if rnd >= WARM:
                    times[name].append(t)
    for name, ts in times.items():
        res.update(_stats(name, ts))
    if parent:
        res["parent_labels_equal"] = bool(torch.equal(outs["step_superpixels"], outs["parent_step"]))
        res["superpixels_inside_parent_range"] = res["parent_step_ms_min"] <= res["step_superpixels_ms"] <= res["parent_step_ms_max"]
    res["added_ms"] = res["step_components_ms"] - res["step_superpixels_ms"]
    res["labels_per_image"] = sorted({int(v) for v in outs["step_components"].amax(dim=(1, 2)) + 1})
    # the pieces, on the batch's own maps
    raw, _ = comp.superpixels_device(imgs)
    canon = comp.features_device(imgs)
    ops = comp.ops
    ndws, n_map, n_nodes = ops.region_nodes_buffers(BATCH, H, W)
    rtws, merges, costs, alive = ops.region_tree_buffers(BATCH, H, W, K_CAP)
    out = torch.empty_like(n_map)
    pieces = (("nodes", lambda: ops.region_nodes(raw, 0, n_map, n_nodes, scratch=ndws)),
              ("tree", lambda: ops.region_tree(canon, n_map, BATCH, H, W, K_CAP, rtws, merges, costs, alive)),
              ("cut", lambda: ops.region_tree_cut(n_map, merges, alive, BATCH, H, W, K_CAP, R, out)))
    for name, fn in pieces:
        res.update(_stats(name, [_timed(torch, fn) for _ in range(WARM + REPS)][WARM:]))
    counts = n_nodes.cpu().numpy()
    res["nodes_per_image"] = dict(min=int(counts.min()), mean=float(counts.mean()), max=int(counts.max()))
    host = imgs[:1].cpu().numpy()
    for mode in ("superpixels", "components"):           # the small call: first use (zeros warm-up, capture, replay), then replays
        plan = _plan(mode)
        t0 = time.perf_counter()
        plan.segment_batch(host)
        res["small_first_call_ms_" + mode] = (time.perf_counter() - t0) * 1e3
        ts = []
        for _ in range(WARM + REPS):
            t0 = time.perf_counter()
            plan.segment_batch(host)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["small_replay_ms_" + mode] = statistics.median(ts[WARM:])
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def trace_main():
    sys.path.insert(0, ROOT)
    import torch
    imgs, plan = _batch(torch), _plan("components")
    out = torch.empty((BATCH, H, W), dtype=torch.int32, device="cuda")
    for _ in range(WARM + REPS):
        plan.segment_device(imgs, out=out)
        torch.cuda.current_stream().synchronize()


def split_main(trace, out_path):
    with open(trace) as f:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    # a step = the launches between two rt_cut_kernel launches (the cut ends every step)
    steps, cur = [], {}
    for t0, t1, name in ks:
        key = next((k for k in NODE_KERNELS + TREE_KERNELS if k in name), "other")
        cur[key] = cur.get(key, 0.0) + (t1 - t0) / 1e6
        if key == "rt_cut_kernel":
            steps.append(cur)
            cur = {}
    steps = steps[-REPS:]
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    for key in NODE_KERNELS + TREE_KERNELS + ("other",):
        res["trace_" + key + "_ms"] = statistics.median([s.get(key, 0.0) for s in steps])
    res["trace_nodes_kernels_ms"] = statistics.median([sum(s.get(k, 0.0) for k in NODE_KERNELS) for s in steps])
    res["trace_step_kernels_ms"] = statistics.median([sum(s.values()) for s in steps])
    print(json.dumps({k: v for k, v in res.items() if k.startswith("trace_")}))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "trace":
        trace_main()
    elif mode == "split":
        split_main(sys.argv[2], sys.argv[3])
    else:
        args = sys.argv[2:]
        parent = args[args.index("--parent") + 1] if "--parent" in args else None
        paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
        time_main(paths[0] if paths else None, parent)
