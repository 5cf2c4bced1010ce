#!/usr/bin/env python3
"""Time of the region adjacency graph (SPEC.md §20) at batch 64 x 481x321 on the 24 val fixture images (landscape ones transposed,
repeated to 64), colour bank (5, 1/8, 4), n = 300, lambda = 576: on the leaf map of the tree on superpixels (K = 294) and on the node
map of the tree on connected regions (SPEC.md §18), six cuts. The method of tools/region_props_time.py.

    region_adjacency_time.py time  [out.json] [--parent path/to/parent/libgcs.so]
    region_adjacency_time.py trace                    (under rocprofv3 --kernel-trace -f csv -d <dir> -o run --)
    region_adjacency_time.py split <run_kernel_trace.csv> <out.json>

``time``: every ``*_ms`` figure is the median of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the
stream, on device-resident inputs, outputs and workspace; per tree ``<tree>_``:
  capacity, edges_max   E_cap of the leaf call (default_capacity, the Segmenter's default for K, where the batch's largest count
                        edges_max fits it, else the power of two at or above edges_max); cut_capacity:
                        E_out_cap of the cuts call, max(64, R (R - 1) / 2) for the largest R
  leaf_ms               gcs_region_adjacency with the image and the contour map as the plane; leaf_img_ms: image only; leaf_none_ms:
                        neither
  props_ms              the yardstick: gcs_region_props at D = 0, the same pixel pass with per-label rows; leaf_ratio = leaf_ms / props_ms
  cuts_ms               gcs_region_adjacency_cuts for REGIONS from that leaf table, group from gcs_region_props_cuts
  percut_ms             what a caller does without these calls, for REGIONS: per R gcs_region_tree_cut, pair keys from shifted label
                        comparisons, torch.unique(return_inverse=True), one index_add_ per column; 7 calls after 2
  cuts_ratio            percut_ms / (leaf_ms + cuts_ms): the leaf pass is paid once, for every cut
  routes_equal          the two routes give the same tables (asserted), for every R; leaf_routes_equal: the same for the leaf map
                        itself against leaf_ms' output
With --parent, "off means unchanged": the default step and the n_superpixels=300, n_regions=8 step through this build, through the
PARENT commit's library and through a second plan on the parent's library, the three taking turns call by call (the fields of
tools/region_props_time.py), asserted: labels equal, and this build's time inside the spread the parent shows against itself.
``trace`` runs, after all set-up, warm + reps calls each of gcs_region_props (D = 0), the leaf call and the cuts call, first on the
superpixel tree, then on the component tree; ``split`` adds the median time of each kernel in each phase to the JSON (the fill and
finish kernels once for the leaf call, once for the cuts call).
"""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from component_tree_time import BATCH, H, LAM, N, REPS, W, WARM, BANK, _batch, _stats, _timed  # noqa: E402
from contour_map_time import REGIONS  # noqa: E402
from region_props_time import PERCUT_REPS, PHASES, _cases, _median, _parent_plans  # noqa: E402

ONCE = ("rp_stats_kernel", "ra_pixels_kernel", "ra_cuts_kernel")       # launched by one of the three calls
TWICE = ("ra_fill_kernel", "ra_finish_kernel")                          # by the leaf call and by the cuts call


def _setup(torch, c, imgs):
    """Buffers and closures of one tree: the leaf call in its three forms, the yardstick, the cuts call."""
    ops, k, n = c["seg"].ops, c["k"], len(REGIONS)
    # the Segmenter's default capacity where it holds the batch's largest graph (one call at full capacity to learn it), else the
    # power of two at or above that
    edges_max = int(c["seg"].region_adjacency_device(c["lab"], K=k, capacity=16384)[2].max())
    cap = min(16384, max(64, 4 * k))
    while cap < edges_max:
        cap = min(16384, 1 << cap.bit_length())
    dev = dict(device="cuda")
    srt = sorted(REGIONS, reverse=True)
    rsum = sum(min(k, r) for r in srt)
    cut_cap = min(cap, max(64, srt[0] * (srt[0] - 1) // 2))            # a cut at R has at most R (R - 1) / 2 edges
    b = dict(cap=cap, cut_cap=cut_cap, srt=srt, edges_max=edges_max, plane=c["seg"].contour_map_device(c["lab"], c["merges"], c["alive"]),
             edges=torch.empty((BATCH, cap, 2), dtype=torch.int32, **dev), vals=torch.empty((BATCH, cap, 3), dtype=torch.int64, **dev),
             count=torch.empty((BATCH,), dtype=torch.int32, **dev), ws=ops.adjacency_buffers(BATCH, cap),
             sums=torch.empty((BATCH, k, 6), dtype=torch.int64, **dev), bbox=torch.empty((BATCH, k, 4), dtype=torch.int32, **dev),
             regs=torch.tensor(srt, dtype=torch.int32, **dev), group=torch.empty((n, BATCH, k), dtype=torch.int32, **dev),
             sums_out=torch.empty((BATCH, rsum, 6), dtype=torch.int64, **dev), bbox_out=torch.empty((BATCH, rsum, 4), dtype=torch.int32, **dev),
             cut_edges=torch.empty((n, BATCH, cut_cap, 2), dtype=torch.int32, **dev),
             cut_vals=torch.empty((n, BATCH, cut_cap, 3), dtype=torch.int64, **dev), cut_count=torch.empty((n, BATCH), dtype=torch.int32, **dev),
             cut_ws=ops.adjacency_buffers(n * BATCH, cut_cap))
    leaf = lambda im=imgs, pl=b["plane"]: ops.region_adjacency(c["lab"], im, pl, BATCH, H, W, k, b["ws"], b["edges"], b["vals"], b["count"])
    props = lambda: ops.region_props(c["lab"], imgs, None, BATCH, H, W, k, b["sums"], b["bbox"])
    group = lambda: ops.region_props_cuts(b["sums"], b["bbox"], c["merges"], c["alive"], b["regs"], BATCH, H, W, k, b["group"],
                                          b["sums_out"], b["bbox_out"])
    cuts = lambda: ops.region_adjacency_cuts(b["edges"], b["vals"], b["count"], b["group"], BATCH, k, k, b["cut_ws"], b["cut_edges"],
                                             b["cut_vals"], b["cut_count"])
    return b, leaf, props, group, cuts


def _pair_table(torch, lab, imgs, plane, r):
    """The graph of a (B,H,W) map with labels in 0 .. r-1 by torch alone: (keys = (image r + a) r + b, sorted; vals int64 [n][3])."""
    image = torch.arange(BATCH, device="cuda").view(BATCH, 1, 1)
    rgb, pl = imgs.to(torch.int64), plane.clamp(min=0).to(torch.int64)
    keys, cols = [], []
    for p, q in (((slice(None), slice(None), slice(0, -1)), (slice(None), slice(None), slice(1, None))),
                 ((slice(None), slice(0, -1), slice(None)), (slice(None), slice(1, None), slice(None)))):
        la, lb = lab[p].to(torch.int64), lab[q].to(torch.int64)
        m = la != lb
        keys.append((((image * r + torch.minimum(la, lb)) * r) + torch.maximum(la, lb))[m])
        cols.append(torch.stack([torch.ones_like(la)[m], ((rgb[p] - rgb[q]) ** 2).sum(-1)[m], (pl[p] + pl[q])[m]], 1))
    uniq, inv = torch.unique(torch.cat(keys), return_inverse=True)
    cols = torch.cat(cols)
    vals = torch.zeros((uniq.shape[0], 3), dtype=torch.int64, device="cuda")
    for e in range(3):
        vals[:, e].index_add_(0, inv, cols[:, e])
    return uniq, vals


def _flat(torch, edges, vals, count, r):
    """A device table [B][cap] in the form of ``_pair_table``."""
    assert int(count.min()) >= 0, "a table overflowed its capacity"
    cap = edges.shape[1]
    mask = torch.arange(cap, device="cuda").view(1, cap) < count.view(-1, 1)
    image = torch.arange(BATCH, device="cuda").view(BATCH, 1)
    keys = (image * r + edges[..., 0].to(torch.int64)) * r + edges[..., 1].to(torch.int64)
    return keys[mask], vals[mask]


def time_main(out_path=None, parent=None):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    steps = {"default_step": {}, "tree_step": dict(n_superpixels=N, spatial_weight=LAM, n_regions=8, **BANK)}
    parents = {name: _parent_plans(parent, kw) for name, kw in steps.items()} if parent else {}
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], n_superpixels=N, spatial_weight=LAM, regions=REGIONS, reps=REPS, warm=WARM,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    for name, c in _cases(torch, imgs).items():
        pre = name + "_"
        k, ops = c["k"], c["seg"].ops
        b, leaf, props, group, cuts = _setup(torch, c, imgs)
        res[pre + "K"], res[pre + "capacity"], res[pre + "cut_capacity"] = k, b["cap"], b["cut_cap"]
        res.update(_stats(pre + "leaf_none", _median(torch, lambda: leaf(None, None))))
        res.update(_stats(pre + "leaf_img", _median(torch, lambda: leaf(imgs, None))))
        res.update(_stats(pre + "leaf", _median(torch, leaf)))
        res.update(_stats(pre + "props", _median(torch, props)))
        res[pre + "leaf_ratio"] = res[pre + "leaf_ms"] / res[pre + "props_ms"]
        res[pre + "edges_max"], res[pre + "default_capacity"] = b["edges_max"], min(16384, max(64, 4 * k))
        assert int(b["count"].max()) == b["edges_max"] and int(b["count"].min()) >= 0
        group()
        res.update(_stats(pre + "cuts", _median(torch, cuts)))
        cut = torch.empty_like(c["lab"])

        def percut(keep=None):
            for r in REGIONS:
                ops.region_tree_cut(c["lab"], c["merges"], c["alive"], BATCH, H, W, k, r, cut)
                table = _pair_table(torch, cut, imgs, b["plane"], r)
                if keep is not None:
                    keep[r] = table
        res.update(_stats(pre + "percut", _median(torch, percut, PERCUT_REPS, 2)))
        res[pre + "cuts_ratio"] = res[pre + "percut_ms"] / (res[pre + "leaf_ms"] + res[pre + "cuts_ms"])
        tables = {}
        percut(tables)
        same = True
        for r in REGIONS:
            at = b["srt"].index(r)
            mine = _flat(torch, b["cut_edges"][at], b["cut_vals"][at], b["cut_count"][at], r)
            same = same and torch.equal(mine[0], tables[r][0]) and torch.equal(mine[1], tables[r][1])
        res[pre + "routes_equal"] = bool(same)
        mine, theirs = _flat(torch, b["edges"], b["vals"], b["count"], k), _pair_table(torch, c["lab"], imgs, b["plane"], k)
        res[pre + "leaf_routes_equal"] = bool(torch.equal(mine[0], theirs[0]) and torch.equal(mine[1], theirs[1]))
        assert res[pre + "routes_equal"] and res[pre + "leaf_routes_equal"], "the two routes give different tables"
        assert res[pre + "cuts_ratio"] >= 1.0, "the new route is the slower one"
        del b, tables, mine, theirs
        torch.cuda.empty_cache()
    for name, kw in steps.items():
        plans = {name: Segmenter(**kw)}
        if parent:
            plans[name + "_parent"], plans[name + "_parent2"] = parents[name]
        times, outs = {p: [] for p in plans}, {}
        for rnd in range(WARM + REPS):
            for p, plan in plans.items():
                t = _timed(torch, lambda: outs.__setitem__(p, plan.segment_device(imgs)))
                if rnd >= WARM:
                    times[p].append(t)
        for p, ts in times.items():
            res.update(_stats(p, ts))
        if parent:
            a, b1, b2 = res[name + "_ms"], res[name + "_parent_ms"], res[name + "_parent2_ms"]
            spread = max(abs(b1 - b2), res[name + "_parent_ms_max"] - res[name + "_parent_ms_min"])
            res[name + "_parent_spread_ms"] = spread
            res[name + "_labels_equal"] = bool(torch.equal(outs[name], outs[name + "_parent"]))
            res[name + "_inside_parent_spread"] = abs(a - b1) <= spread
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    if parent:
        assert all(res[name + "_labels_equal"] and res[name + "_inside_parent_spread"] for name in steps), "the step changed"


def trace_main():
    sys.path.insert(0, ROOT)
    import torch
    imgs = _batch(torch)
    work = []
    for name, c in _cases(torch, imgs).items():          # every buffer first: nothing but the timed calls runs behind this loop
        b, leaf, props, group, cuts = _setup(torch, c, imgs)
        leaf(), props(), group()
        work.append((b, props, leaf, cuts))
    torch.cuda.synchronize()
    for _, *fns in work:
        for fn in fns:
            for _ in range(WARM + REPS):
                fn()
                torch.cuda.current_stream().synchronize()


def split_main(trace, out_path):
    with open(trace) as f:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    per = WARM + REPS
    for key in ONCE + TWICE:
        calls = 2 if key in TWICE else 1
        mine = [(t1 - t0) / 1e6 for t0, t1, name in ks if key in name][-2 * calls * per:]     # set-up launches come first: dropped
        assert len(mine) == 2 * calls * per, (key, len(mine))
        for i, phase in enumerate(PHASES):
            for j, call in enumerate(("leaf", "cuts")[:calls]):
                at = (i * calls + j) * per
                tag = "trace_%s_%s%s_ms" % (phase, key, "_" + call if calls == 2 else "")
                res[tag] = statistics.median(mine[at:at + per][WARM:])
    print(json.dumps({k: v for k, v in res.items() if k.startswith("trace_")}))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    args = sys.argv[2:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
    if mode == "trace":
        trace_main()
    elif mode == "split":
        split_main(paths[0], paths[1])
    else:
        time_main(paths[0] if paths else None, parent)
