#!/usr/bin/env python3
"""Time of the region descriptors and mean-colour pictures (SPEC.md §19) at batch 64 x 481x321 on the 24 val fixture images (landscape
ones transposed, repeated to 64), colour bank (5, 1/8, 4; D = 72), n = 300, lambda = 576: on the tree on superpixels (K = 294) and on
the tree on connected regions (SPEC.md §18; K = the batch's largest node count rounded up to 64), each with D = 0 and D = 72, six cuts.

    region_props_time.py time  [out.json] [--parent path/to/parent/libgcs.so]
    region_props_time.py trace [--parent path/to/parent/libgcs.so]   (under rocprofv3 --kernel-trace -f csv -d <dir> -o run --)
    region_props_time.py split <run_kernel_trace.csv> <out.json>
    region_props_time.py same  <out.json> --parent path/to/parent/libgcs.so

``time``: every ``*_ms`` figure is the median of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the
stream, on device-resident inputs and outputs; per case ``<tree>_d<D>_``:
  props_ms       gcs_region_props (fill + the pass over the pixels)
  cuts_ms        gcs_region_props_cuts for REGIONS from that leaf table
  paint_ms       gcs_region_paint of the cut at R = 8 (group table + the cut's rows); paint_leaf_ms: of the leaf table itself
  percut_ms      what a caller does without these calls, for REGIONS: per R gcs_region_tree_cut and the table of the relabelled map
                 by torch.index_add_ (one call per column on prepared int64 columns) and scatter_reduce_ (the four box columns);
                 7 calls after 2
  cuts_ratio     percut_ms / (props_ms + cuts_ms): the leaf pass is paid once, for every cut
With --parent, "off means unchanged": the default step and the n_superpixels=300, n_regions=8 step through this build, through the
PARENT commit's library and through a second plan on the parent's library, the three taking turns call by call:
  <step>_ms, <step>_parent_ms, <step>_parent2_ms, <step>_labels_equal, and <step>_inside_parent_spread = |this - parent| <=
  max(|parent - parent2|, the parent's own max - min).
``trace`` runs, after all set-up, warm + reps calls each of: gcs_region_tree through the parent's library (the yardstick of the D = 72
leaf pass: its rt_stats_kernel does the same accumulation), then the three calls at D = 72, first on the superpixel tree, then on
the component tree; ``split`` adds the median time of each kernel in each of the two phases to the JSON, and ``leaf_ratio`` =
rp_stats_kernel / rt_stats_kernel per phase.
``same``: gcs_region_props, gcs_region_props_cuts (both per case) and gcs_region_tree_cut at R = 8 (per tree) through this build and
twice through the PARENT's library on the SAME device buffers in one process, the three taking turns call by call, SAME_REPS calls
after ``warm``: separate ``time`` runs place their buffers independently, which moves a latency-bound kernel by a few per cent
whichever library runs it. Adds ``same_buffers`` to the JSON: per figure parent, parent2, this, the parent's min and max, the
spread max(|parent - parent2|, parent max - min) and ``inside``.
"""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from component_tree_time import BANK, BATCH, H, LAM, N, REPS, W, WARM, _batch, _stats, _timed  # noqa: E402
from contour_map_time import REGIONS  # noqa: E402

KERNELS = ("rt_stats_kernel", "rp_fill_kernel", "rp_stats_kernel", "rp_cuts_kernel", "rp_paint_kernel")
PHASES = ("superpixels", "components")
SAME_REPS = 60
PERCUT_REPS = 7                                          # the caller's route of today: hundreds of launches per call


def _median(torch, fn, reps=REPS, warm=WARM):
    return [_timed(torch, fn) for _ in range(warm + reps)][warm:]


def _cases(torch, imgs):
    """Per tree: the plan, its leaf map, merge list, alive, K and the canonical features of the batch."""
    from gabor_color_image_segmentation_amd import Segmenter
    out = {}
    for name in PHASES:
        seg = Segmenter(n_superpixels=N, spatial_weight=LAM, tree_nodes=name, **BANK)
        lab, merges, _, alive = seg.region_tree_device(imgs)
        out[name] = dict(seg=seg, lab=lab, merges=merges, alive=alive, k=merges.shape[1] + 1, canon=seg.features_device(imgs))
    return out


def _buffers(torch, c, d):
    k, n = c["k"], len(REGIONS)
    srt = sorted(REGIONS, reverse=True)
    rsum = sum(min(k, r) for r in srt)
    dev = dict(device="cuda")
    return dict(sums=torch.empty((BATCH, k, 6 + d), dtype=torch.int64, **dev), bbox=torch.empty((BATCH, k, 4), dtype=torch.int32, **dev),
                regs=torch.tensor(srt, dtype=torch.int32, **dev), group=torch.empty((n, BATCH, k), dtype=torch.int32, **dev),
                sums_out=torch.empty((BATCH, rsum, 6 + d), dtype=torch.int64, **dev),
                bbox_out=torch.empty((BATCH, rsum, 4), dtype=torch.int32, **dev),
                rgb=torch.empty((BATCH, H, W, 3), dtype=torch.uint8, **dev), srt=srt)


def _calls(c, imgs, d, buf):
    """The three calls of one case as closures; paint: the cut at R = 8."""
    ops, k = c["seg"].ops, c["k"]
    canon = c["canon"] if d else None
    at = buf["srt"].index(8)
    off = sum(min(k, r) for r in buf["srt"][:at])
    rows8 = buf["sums_out"][:, off:off + 8]
    props = lambda: ops.region_props(c["lab"], imgs, canon, BATCH, H, W, k, buf["sums"], buf["bbox"])
    cuts = lambda: ops.region_props_cuts(buf["sums"], buf["bbox"], c["merges"], c["alive"], buf["regs"], BATCH, H, W, k, buf["group"],
                                         buf["sums_out"], buf["bbox_out"])
    paint = lambda: ops.region_paint(c["lab"], buf["group"][at], rows8, BATCH, H, W, k, buf["rgb"])
    leaf = lambda: ops.region_paint(c["lab"], None, buf["sums"], BATCH, H, W, k, buf["rgb"])
    return props, cuts, paint, leaf


def _per_cut(torch, c, imgs, d):
    """The caller's route today for one R, as a closure over prepared columns: relabel, then one index_add_ per column."""
    ops, k = c["seg"].ops, c["k"]
    hw = H * W
    yy = torch.arange(H, device="cuda").repeat_interleave(W).repeat(BATCH)
    xx = torch.arange(W, device="cuda").repeat(H * BATCH)
    cols = [torch.ones(BATCH * hw, dtype=torch.int64, device="cuda"), yy.to(torch.int64), xx.to(torch.int64)]
    cols += [imgs[..., ch].reshape(-1).to(torch.int64) for ch in range(3)]
    if d:
        cols += [(c["canon"][:, p].reshape(-1).to(torch.int64) & 0xffff) for p in range(d)]
    image = torch.arange(BATCH, device="cuda").repeat_interleave(hw)
    cut = torch.empty_like(c["lab"])
    y32, x32 = yy.to(torch.int32), xx.to(torch.int32)

    def run():
        for r in REGIONS:
            ops.region_tree_cut(c["lab"], c["merges"], c["alive"], BATCH, H, W, k, r, cut)
            idx = image * r + cut.reshape(-1)
            table = torch.zeros((len(cols), BATCH * r), dtype=torch.int64, device="cuda")
            for e, v in enumerate(cols):
                table[e].index_add_(0, idx, v)
            box = torch.empty((4, BATCH * r), dtype=torch.int32, device="cuda")
            box[0].fill_(H), box[1].fill_(W), box[2].fill_(-1), box[3].fill_(-1)
            box[0].scatter_reduce_(0, idx, y32, "amin"), box[1].scatter_reduce_(0, idx, x32, "amin")
            box[2].scatter_reduce_(0, idx, y32, "amax"), box[3].scatter_reduce_(0, idx, x32, "amax")
        return table, box
    return run


def _parent_plans(parent, kw):
    """Two plans on the PARENT commit's library (tools/ab.py: one process, both builds)."""
    import ctypes
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    here, sigs = _lib.LIB_PATH, dict(_lib.SIGNATURES)
    raw = ctypes.CDLL(os.path.abspath(parent))
    _lib.LIB_PATH, _lib._lib = os.path.abspath(parent), None
    _lib.SIGNATURES = {k: v for k, v in sigs.items() if hasattr(raw, k)}
    plans = [Segmenter(**kw), Segmenter(**kw)]
    _lib.LIB_PATH, _lib._lib, _lib.SIGNATURES = here, None, sigs
    return plans


def time_main(out_path=None, parent=None):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    steps = {"default_step": {}, "tree_step": dict(n_superpixels=N, spatial_weight=LAM, n_regions=8, **BANK)}
    parents = {name: _parent_plans(parent, kw) for name, kw in steps.items()} if parent else {}
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], n_superpixels=N, spatial_weight=LAM, regions=REGIONS, reps=REPS, warm=WARM,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    cases = _cases(torch, imgs)
    for name, c in cases.items():
        res["K_" + name] = c["k"]
        for d in (0, 72):
            assert d in (0, c["seg"].bank.n_features)
            pre = "%s_d%d_" % (name, d)
            buf = _buffers(torch, c, d)
            props, cuts, paint, leaf = _calls(c, imgs, d, buf)
            for key, fn in (("props", props), ("cuts", cuts), ("paint", paint), ("paint_leaf", leaf)):
                res.update(_stats(pre + key, _median(torch, fn)))
            run = _per_cut(torch, c, imgs, d)
            res.update(_stats(pre + "percut", _median(torch, run, PERCUT_REPS, 2)))
            res[pre + "cuts_ratio"] = res[pre + "percut_ms"] / (res[pre + "props_ms"] + res[pre + "cuts_ms"])
            # the two routes give the same table for the last R
            table, box = run()
            r = REGIONS[-1]
            at = buf["srt"].index(r)
            off = sum(min(c["k"], q) for q in buf["srt"][:at])
            same = torch.equal(table.reshape(-1, BATCH, r).permute(1, 2, 0), buf["sums_out"][:, off:off + r]) and \
                torch.equal(box.reshape(4, BATCH, r).permute(1, 2, 0), buf["bbox_out"][:, off:off + r])
            res[pre + "routes_equal"] = bool(same)
            del buf, run, table, box
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
            a, b, c2 = res[name + "_ms"], res[name + "_parent_ms"], res[name + "_parent2_ms"]
            spread = max(abs(b - c2), res[name + "_parent_ms_max"] - res[name + "_parent_ms_min"])
            res[name + "_labels_equal"] = bool(torch.equal(outs[name], outs[name + "_parent"]))
            res[name + "_inside_parent_spread"] = abs(a - b) <= spread
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def trace_main(parent=None):
    sys.path.insert(0, ROOT)
    import ctypes
    import torch
    from gabor_color_image_segmentation_amd import _lib
    imgs = _batch(torch)
    cases = _cases(torch, imgs)
    lib = _lib.load()
    tree_lib = lib
    if parent:
        tree_lib = ctypes.CDLL(os.path.abspath(parent))
        for name in ("gcs_region_tree", "gcs_region_tree_workspace_bytes"):
            getattr(tree_lib, name).restype, getattr(tree_lib, name).argtypes = _lib.SIGNATURES[name]
    work = []
    for name in PHASES:                                  # every buffer first: nothing but the timed calls runs behind this loop
        c = cases[name]
        buf = _buffers(torch, c, 72)
        ws = torch.empty(tree_lib.gcs_region_tree_workspace_bytes(BATCH, H, W, 72, c["k"]), dtype=torch.uint8, device="cuda")
        merges, alive = torch.empty_like(c["merges"]), torch.empty_like(c["alive"])
        tree = lambda c=c, ws=ws, merges=merges, alive=alive: tree_lib.gcs_region_tree(
            c["canon"].data_ptr(), c["lab"].data_ptr(), BATCH, H, W, 72, c["k"], ws.data_ptr(), merges.data_ptr(), None,
            alive.data_ptr(), torch.cuda.current_stream().cuda_stream)
        work.append((tree,) + _calls(c, imgs, 72, buf)[:3])
    torch.cuda.synchronize()
    for fns in work:
        for fn in fns:
            for _ in range(WARM + REPS):
                fn()
                torch.cuda.current_stream().synchronize()


def same_main(out_path, parent):
    sys.path.insert(0, ROOT)
    import torch
    p1, p2 = _parent_plans(parent, dict(n_superpixels=N, spatial_weight=LAM, **BANK))
    imgs = _batch(torch)
    cases = _cases(torch, imgs)
    same = {}

    def turns(key, call):
        """``call(ops)`` -> a closure; the three plans' closures take turns."""
        fns = {"parent": call(p1.ops), "this": call(c["seg"].ops), "parent2": call(p2.ops)}
        times = {who: [] for who in fns}
        for rnd in range(WARM + SAME_REPS):
            for who, fn in fns.items():
                t = _timed(torch, fn)
                if rnd >= WARM:
                    times[who].append(t)
        m = {who: statistics.median(ts) for who, ts in times.items()}
        lo, hi = min(times["parent"]), max(times["parent"])
        spread = max(abs(m["parent"] - m["parent2"]), hi - lo)
        same[key] = dict(m, parent_min=lo, parent_max=hi, spread=spread, inside=abs(m["this"] - m["parent"]) <= spread)
        print(key, json.dumps(same[key]), flush=True)

    for name, c in cases.items():
        k = c["k"]
        for d in (0, 72):
            buf = _buffers(torch, c, d)
            canon = c["canon"] if d else None
            turns("%s_d%d_props_ms" % (name, d),
                  lambda ops: lambda: ops.region_props(c["lab"], imgs, canon, BATCH, H, W, k, buf["sums"], buf["bbox"]))
            turns("%s_d%d_cuts_ms" % (name, d),
                  lambda ops: lambda: ops.region_props_cuts(buf["sums"], buf["bbox"], c["merges"], c["alive"], buf["regs"], BATCH, H, W, k,
                                                            buf["group"], buf["sums_out"], buf["bbox_out"]))
            del buf
            torch.cuda.empty_cache()
        out = torch.empty_like(c["lab"])
        turns("%s_cut_ms" % name, lambda ops: lambda: ops.region_tree_cut(c["lab"], c["merges"], c["alive"], BATCH, H, W, k, 8, out))
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["same_buffers"] = dict(same, reps=SAME_REPS, warm=WARM)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


def split_main(trace, out_path):
    with open(trace) as f:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    per = WARM + REPS
    for key in KERNELS:
        mine = [(t1 - t0) / 1e6 for t0, t1, name in ks if key in name][-2 * per:]     # set-up launches come first: dropped
        assert len(mine) == 2 * per, (key, len(mine))
        for i, phase in enumerate(PHASES):
            res["trace_%s_%s_ms" % (phase, key)] = statistics.median(mine[i * per:(i + 1) * per][WARM:])
    for phase in PHASES:
        res["trace_%s_leaf_ratio" % phase] = res["trace_%s_rp_stats_kernel_ms" % phase] / res["trace_%s_rt_stats_kernel_ms" % phase]
    print(json.dumps({k: v for k, v in res.items() if k.startswith("trace_")}))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    args = sys.argv[2:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
    if mode == "trace":
        trace_main(parent)
    elif mode == "split":
        split_main(paths[0], paths[1])
    elif mode == "same":
        same_main(paths[0], parent)
    else:
        time_main(paths[0] if paths else None, parent)
