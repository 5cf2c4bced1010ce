#!/usr/bin/env python3
"""Cost of the region tree merged by boundary strength (SPEC.md §23) at batch 64 x 481x321, colour bank (5, 1/8, 4; D = 72), R = 8, on
the 24 val fixture images (landscape ones transposed, repeated to 64).

    boundary_tree_time.py time [out.json] --parent path/to/parent/libgcs.so [--dump maps.npz]
    boundary_tree_time.py rounds maps.npz out.json          (CPU: the restatement's rounds and live edges per image, into the JSON)

``time``: medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs:
  step_<mode>_features_ms / step_<mode>_boundary_ms   Segmenter(..., n_regions=8, merge_cost=...).segment_device, <mode> = components
                                              (300 superpixels), clusters_k16, clusters_k8
  step_default_ms / parent_default_ms         the k = 8 plan, Segmenter(n_superpixels=300, n_regions=8, tree_nodes="components") and
  step_components_ms / parent_components_ms   Segmenter(tree_nodes="clusters", n_regions=8, k=16), all with merge_cost="features", this
  step_clusters_ms / parent_clusters_ms       library's calls taking turns with the PARENT commit's library in this process: "off
                                              means unchanged" (…_labels_equal, …_inside_parent_range)
  <mode>_gradient_ms, _used_ms, _adjacency_ms, _tree_edges_ms      the four launches of §23 on the mode's node maps, one by one
  <mode>_tree_features_ms                     the statistics + merge launches of §14 on the same node maps (gcs_region_tree on the
                                              canonical tensor for components, gcs_region_tree_slab for clusters), at K = 4096
  <mode>_edges_per_image                      the leaf table's count per image (the first 24)
``--dump``: the node maps and planes of the 24 distinct images, for ``rounds``.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 15, 3
BANK = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
BATCH, H, W, R, K_CAP = 64, 481, 321, 8, 4096
MODES = {"components": dict(n_superpixels=300, spatial_weight=576, tree_nodes="components"),
         "clusters_k16": dict(tree_nodes="clusters", k=16), "clusters_k8": dict(tree_nodes="clusters", k=8)}


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
    return torch.from_numpy(np.stack([imgs[i % len(imgs)] for i in range(BATCH)])).cuda(), len(imgs)


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


def _turns(torch, plans, groups, imgs, times, outs):
    for group in groups:                                 # a group takes turns, call by call, with nothing else between
        for rnd in range(WARM + REPS):
            for name in group:
                t = _timed(torch, lambda: outs.__setitem__(name, plans[name].segment_device(imgs)))
                if rnd >= WARM:
                    times[name].append(t)
        for name in group:
            plans[name]._ws.clear()
        torch.cuda.empty_cache()


def time_main(out_path, parent, dump):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    imgs, distinct = _batch(torch)
    off = dict(default=dict(), components=dict(n_regions=R, **MODES["components"]), clusters=dict(n_regions=R, **MODES["clusters_k16"]))
    plans = {}
    for what, kw in off.items():
        plans["parent_" + what] = _with_parent(parent, lambda: Segmenter(**kw, **BANK))
        plans["step_" + what] = Segmenter(merge_cost="features", **kw, **BANK)
        assert not hasattr(plans["parent_" + what].ops.lib, "gcs_region_tree_edges")
    for mode, kw in MODES.items():
        for cost in ("features", "boundary"):
            plans[f"step_{mode}_{cost}"] = Segmenter(n_regions=R, merge_cost=cost, **kw, **BANK)
    res = dict(batch=BATCH, shape=[H, W], n_regions=R, K_cap=K_CAP, D=plans["step_default"].bank.n_features, reps=REPS, warm=WARM,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    times, outs = {name: [] for name in plans}, {}
    _turns(torch, plans, [["parent_" + w, "step_" + w] for w in off] + [[f"step_{m}_features", f"step_{m}_boundary"] for m in MODES],
           imgs, times, outs)
    for name, ts in times.items():
        res.update(_stats(name, ts))
    for what in off:
        res[what + "_labels_equal"] = bool(torch.equal(outs["step_" + what], outs["parent_" + what]))
        res[what + "_inside_parent_range"] = res[f"parent_{what}_ms_min"] <= res[f"step_{what}_ms"] <= res[f"parent_{what}_ms_max"]
    for mode in MODES:
        res[mode + "_labels_per_image"] = sorted({int(v) for m in ("features", "boundary")
                                                  for v in outs[f"step_{mode}_{m}"].amax(dim=(1, 2)) + 1})
    del plans, outs
    torch.cuda.empty_cache()
    saved = {}
    for mode, kw in MODES.items():                       # the launches one by one, on the mode's own node maps
        plan = Segmenter(merge_cost="boundary", **kw, **BANK)
        ops = plan.ops
        if mode == "components":
            n_map, ws, _ = plan._superpixel_maps(imgs, tree=False)
        else:
            n_map, ws = plan._cluster_maps(imgs, tree=False)
        st, merges, costs, alive = ops.region_tree_edges_buffers(BATCH, H, W, K_CAP)
        old = ops.region_tree_buffers(BATCH, H, W, K_CAP)
        feats = ws["feats"]
        calls = dict(gradient=lambda: ops.feature_gradient(feats, BATCH, H, W, st["grad"]),
                     used=lambda: ops.label_used(n_map, BATCH, H, W, K_CAP, st["used"]),
                     adjacency=lambda: ops.region_adjacency(n_map, None, st["grad"], BATCH, H, W, K_CAP, st["adj"], st["edges"],
                                                            st["vals"], st["count"]),
                     tree_edges=lambda: ops.region_tree_edges(st["edges"], st["vals"], st["count"], st["used"], BATCH, K_CAP, st["tree"],
                                                              merges, costs, alive),
                     tree_features=(lambda: ops.region_tree(ws["sp"][0], n_map, BATCH, H, W, K_CAP, *old)) if mode == "components"
                     else (lambda: ops.region_tree_slab(feats, n_map, BATCH, H, W, K_CAP, *old)))
        for name in ("gradient", "used", "adjacency", "tree_edges", "tree_features"):
            res.update(_stats(f"{mode}_{name}", [_timed(torch, calls[name]) for _ in range(WARM + REPS)][WARM:]))
        res[mode + "_boundary_launches_ms"] = sum(res[f"{mode}_{n}_ms"] for n in ("gradient", "used", "adjacency", "tree_edges"))
        res[mode + "_edges_per_image"] = st["count"][:distinct].cpu().tolist()
        res[mode + "_nodes_per_image"] = alive[:distinct].cpu().tolist()
        res[mode + "_alive_equal"] = bool(torch.equal(alive, old[3]))
        saved[mode + "_maps"] = n_map[:distinct].cpu().numpy().astype(np.int16 if K_CAP <= 32767 else np.int32)
        saved[mode + "_planes"] = st["grad"][:distinct].cpu().numpy()
        saved[mode + "_merges"] = merges[:distinct].cpu().numpy()
        del plan, ws, st, old, calls
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    if dump:
        np.savez_compressed(dump, **saved)


def rounds_main(dump, out_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import boundary_tree_ref as bt
    doc = np.load(dump)
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    for mode in MODES:
        rounds, same = [], True
        for lab, plane, merges in zip(doc[mode + "_maps"], doc[mode + "_planes"], doc[mode + "_merges"]):
            info = {}
            m, _, _ = bt.build_tree(lab.astype(np.int32), K_CAP, plane, info=info)
            rounds.append(info["rounds"])
            same = same and bool(np.array_equal(m, merges))
        res[mode + "_rounds_per_image"] = rounds
        res[mode + "_merges_equal_restatement"] = same
    print(json.dumps({k: v for k, v in res.items() if "rounds" in k or "restatement" in k}))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    args = sys.argv[2:]
    if mode == "rounds":
        rounds_main(args[0], args[1])
        sys.exit(0)
    opts = {}
    for flag in ("--parent", "--dump"):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    if "--parent" not in opts:
        sys.exit("the parent commit's libgcs.so is needed: --parent path")
    time_main(args[0] if args else None, opts["--parent"], opts.get("--dump"))
