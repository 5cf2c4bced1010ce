#!/usr/bin/env python3
"""Time of the region tree (SPEC.md §14) at batch 64 x 481x321 behind the superpixel stage (n = 300, lambda = 576, colour bank 5, 1/8,
4; D = 72), R = 8.

    region_tree_time.py time  [out.json] [--parent path/to/parent/libgcs.so]
    region_tree_time.py trace                      (under rocprofv3 --kernel-trace -f csv -d <dir> -o run --)
    region_tree_time.py split <run_kernel_trace.csv> <out.json>

``time``: every figure is the median of ``reps`` calls after ``warm`` warm-up calls, each call bracketed by two events on the stream,
on device-resident inputs:
  tree_ms            gcs_region_tree on the batch's superpixel maps: zero + statistics/adjacency + the merge kernel (one call)
  tree_constant_ms   the same call on a constant batch (every cost 0: alive - 1 rounds, one pair per round) and its own superpixel maps
  cut_ms             gcs_region_tree_cut at R = 8, in place
  step_ms            Segmenter(n_superpixels=300, n_regions=8).segment_device: Gabor stage, unpack, superpixel stage, tree, cut
  step0_ms           the same plan with n_regions = 0
  parent_step0_ms    (--parent) the n_regions = 0 step through the PARENT commit's library on the same box, its rounds taking turns with
                     step0's inside this process: the yardstick for "nothing changed when the option is off"
``trace`` runs warm + reps tree calls on the real batch, then on the constant batch, then the cuts; ``split`` reads the kernel trace
of that run and adds the median time of each kernel (zero, statistics + adjacency, merge, cut) to the JSON: a call enqueues its
launches itself, so events cannot get between them.
"""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 25, 4
BANK = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
BATCH, H, W, N, LAM, R = 64, 481, 321, 300, 576, 8


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median_ms(torch, fn, reps=REPS, warm=WARM):
    times = [_timed(torch, fn) for _ in range(warm + reps)][warm:]
    return statistics.median(times), min(times), max(times)


def _setup(torch):
    """The plan, the batch's canonical features and superpixel maps, and the same for a constant batch."""
    from gabor_color_image_segmentation_amd import Segmenter, superpixel_grid
    from gabor_color_image_segmentation_amd.segmenter import _step_cluster, _step_features
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = torch.from_numpy(synthetic_batch(BATCH, H, W, seed=0)).cuda()
    seg = Segmenter(n_superpixels=N, spatial_weight=LAM, n_regions=R, **BANK)
    _, ny, nx = superpixel_grid(H, W, N)
    cases = {}
    for name, batch in (("real", imgs), ("constant", torch.full_like(imgs, 128))):
        ws = seg._tail_workspace(BATCH, H, W, "per_image")
        _step_features(seg.ops, seg._opt, ws, batch, BATCH, H, W)
        lab = torch.empty((BATCH, H, W), dtype=torch.int32, device="cuda")
        _step_cluster(seg.ops, seg._opt, ws, lab, BATCH, H, W, "per_image", seg.debug, tree=False)      # the §13 map alone
        cases[name] = (ws["sp"][0], lab, seg.ops.region_tree_buffers(BATCH, H, W, ny * nx))
    return seg, imgs, ny * nx, cases


def _tree(seg, k, case):
    canon, lab, (rtws, merges, costs, alive) = case
    seg.ops.region_tree(canon, lab, BATCH, H, W, k, rtws, merges, costs, alive)


def _cut(seg, k, case, out):
    _, lab, (_, merges, _, alive) = case
    seg.ops.region_tree_cut(lab, merges, alive, BATCH, H, W, k, R, out)


def time_main(out_path=None, parent=None):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    parent_seg = None
    if parent:                                           # the parent's library first (tools/ab.py: one process, both builds)
        import ctypes
        here, sigs = _lib.LIB_PATH, dict(_lib.SIGNATURES)
        raw = ctypes.CDLL(os.path.abspath(parent))
        _lib.LIB_PATH, _lib._lib = os.path.abspath(parent), None
        _lib.SIGNATURES = {k: v for k, v in sigs.items() if hasattr(raw, k)}
        parent_seg = Segmenter(n_superpixels=N, spatial_weight=LAM, **BANK)
        _lib.LIB_PATH, _lib._lib, _lib.SIGNATURES = here, None, sigs
    seg, imgs, k, cases = _setup(torch)
    out = torch.empty((BATCH, H, W), dtype=torch.int32, device="cuda")
    res = dict(batch=BATCH, shape=[H, W], n_superpixels=N, spatial_weight=LAM, n_regions=R, K=k, D=seg.bank.n_features, reps=REPS,
               warm=WARM, feature_bytes=BATCH * seg.bank.n_features * H * W * 2)
    for name, fn in (("tree", lambda: _tree(seg, k, cases["real"])), ("tree_constant", lambda: _tree(seg, k, cases["constant"])),
                     ("cut", lambda: _cut(seg, k, cases["real"], out)), ("step", lambda: seg.segment_device(imgs, out=out))):
        m = _median_ms(torch, fn)
        res.update({name + "_ms": m[0], name + "_ms_min": m[1], name + "_ms_max": m[2]})
    res["alive"] = [int(cases[c][2][3].min()) for c in ("real", "constant")] + [int(cases[c][2][3].max()) for c in ("real", "constant")]
    off = Segmenter(n_superpixels=N, spatial_weight=LAM, **BANK)
    plans = {"step0": off}
    if parent_seg is not None:
        plans["parent_step0"] = parent_seg
    times = {name: [] for name in plans}
    outs = {}
    for rnd in range(WARM + REPS):                       # the builds take turns inside each round
        for name, plan in plans.items():
            t = _timed(torch, lambda: outs.__setitem__(name, plan.segment_device(imgs)))
            if rnd >= WARM:
                times[name].append(t)
    for name, ts in times.items():
        res.update({name + "_ms": statistics.median(ts), name + "_ms_min": min(ts), name + "_ms_max": max(ts)})
    if parent_seg is not None:
        res["parent_labels_equal"] = bool(torch.equal(outs["step0"], outs["parent_step0"]))
    res["added_ms"] = res["step_ms"] - res["step0_ms"]
    res["step_Mpix_per_s"] = BATCH * H * W / res["step_ms"] / 1e3
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def trace_main():
    sys.path.insert(0, ROOT)
    import torch
    seg, imgs, k, cases = _setup(torch)
    out = torch.empty((BATCH, H, W), dtype=torch.int32, device="cuda")
    for case in ("real", "constant"):
        for _ in range(WARM + REPS):
            _tree(seg, k, cases[case])
        torch.cuda.synchronize()
    for _ in range(WARM + REPS):
        _cut(seg, k, cases["real"], out)
    torch.cuda.synchronize()


def split_main(trace, out_path):
    with open(trace) as f:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    per = {}
    for t0, t1, name in ks:
        for key in ("rt_zero_kernel", "rt_stats_kernel", "rt_merge_kernel", "rt_cut_kernel"):
            if key in name:
                per.setdefault(key, []).append((t1 - t0) / 1e6)
    n = WARM + REPS
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    for key, ts in per.items():
        ts = ts[-n:] if key == "rt_cut_kernel" else ts[-2 * n:]          # (the set-up runs no tree or cut; be safe about extra launches)
        short = key[3:-7]
        res[short + "_kernel_ms"] = statistics.median(ts[WARM:n])
        if key != "rt_cut_kernel":
            res[short + "_kernel_constant_ms"] = statistics.median(ts[n + WARM:])
    print(json.dumps({k: v for k, v in res.items() if "_kernel_" in k}))
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
