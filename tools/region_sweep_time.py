#!/usr/bin/env python3
"""Time of the region metrics of every cut at once (SPEC.md §16) at batch 64 x 481x321 behind the superpixel stage and the tree
(n = 300, lambda = 576, colour bank 5, 1/8, 4; K = 294; 5 synthetic annotator maps per image, T = 320), beside the per-cut path it
replaces: the batch, the bank and the annotator maps of tools/contour_map_time.py.

    region_sweep_time.py time   [out.json] [--parent path/to/parent/libgcs.so]
    region_sweep_time.py percut [out.json] --parent path/to/parent/libgcs.so     (a process of its own: only the parent's library is loaded)
    region_sweep_time.py trace                      (under rocprofv3 --kernel-trace -f csv -d <dir> -o run --)
    region_sweep_time.py split <run_kernel_trace.csv> <out.json>

``time``: every ``*_ms`` figure is the median of ``reps`` calls after ``warm`` warm-up calls, each call bracketed by two events on the
stream, on device-resident inputs (``*_wall_ms``: host calls that end with a copy to the host, by the host's clock):
  leaf_ms            gcs_region_counts_batch_u8 with n_segments = K: the leaf tables [T][K][stride], zeroing included
  sweep_ms           gcs_region_sweep for REGIONS on those tables (restored from a copy before every call, outside the events: the
                     call consumes them)
  sweep_wall_ms      evaluate_gpu.region_sweep_resident + sweep_agreement for REGIONS: all region metrics of all R
  *_4096_*           the same three on one 64 x 64 image of one-pixel labels with the chain (K-2, K-1), ..., (0, 1): K = 4096
  cut_ms_R, score_ms_R, score_wall_ms_R   per R of REGIONS: gcs_region_tree_cut; submit_scores_batch_resident(agreement=True) on that
                     cut between two events (kernels and the result copy); all_scores_batch_resident(agreement=True) by the host's clock
  per_cut_path_ms / per_cut_path_wall_ms   their sums over REGIONS: the path the sweep replaces
  step0 / step8      Segmenter(n_superpixels=300[, n_regions=8]).segment_device here and (--parent) through the PARENT commit's
                     library in the same process, the builds taking turns call by call: "nothing changed when the calls are not made"
``percut`` writes the per-cut figures alone, prefixed ``parent_``, measured through the parent commit's library: the yardstick.
``trace`` runs warm + reps leaf and sweep calls on the batch, then on the K = 4096 case; ``split`` adds the median time of each kernel.
"""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contour_map_time import ANNOTATORS, BANK, BATCH, H, LAM, N, R, REGIONS, REPS, W, WARM, _median_ms, _timed, _truth, _wall_ms  # noqa: E402


def _use_parent(parent):
    """Point the package at the parent commit's library (which lacks this commit's entry points) before anything loads it."""
    import ctypes
    from gabor_color_image_segmentation_amd import _lib
    state = _lib.LIB_PATH, dict(_lib.SIGNATURES)
    raw = ctypes.CDLL(os.path.abspath(parent))
    _lib.LIB_PATH, _lib._lib = os.path.abspath(parent), None
    _lib.SIGNATURES = {k: v for k, v in state[1].items() if hasattr(raw, k)}
    return state


def _setup(torch, big=True):
    import numpy as np
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = torch.from_numpy(synthetic_batch(BATCH, H, W, seed=0)).cuda()
    seg = Segmenter(n_superpixels=N, spatial_weight=LAM, **BANK)
    lab, merges, _, alive = seg.region_tree_device(imgs)
    s = dict(seg=seg, imgs=imgs, lib=_lib.load(), cases={})
    s["cases"][""] = dict(lab=lab, merges=merges, alive=alive, k=merges.shape[1] + 1, truth=_truth(np), b=BATCH, h=H, w=W)
    if big:
        k = 4096
        rng = np.random.default_rng(2)
        t = np.zeros((ANNOTATORS, 64, 64), np.uint16)
        for m in t:
            for _ in range(6):
                y, x = int(rng.integers(0, 50)), int(rng.integers(0, 50))
                m[y:y + int(rng.integers(8, 40)), x:x + int(rng.integers(8, 40))] += 1
        dt = DeviceTruth(t, [0, ANNOTATORS], [0] * ANNOTATORS, [int(m.max()) + 1 for m in t])
        s["cases"]["_4096"] = dict(lab=torch.arange(k, dtype=torch.int32, device="cuda").reshape(1, 64, 64),
                                   merges=torch.tensor([(q - 1, q) for q in range(k - 1, 0, -1)], dtype=torch.int32,
                                                       device="cuda").reshape(1, k - 1, 2),
                                   alive=torch.tensor([k], dtype=torch.int32, device="cuda"), k=k, truth=dt, b=1, h=64, w=64)
    return s


def _raw_calls(torch, lib, c):
    """-> (leaf(), sweep(), restore()) on buffers of their own for case ``c``."""
    dt, k, b = c["truth"], c["k"], c["b"]
    n = len(REGIONS)
    hist = torch.empty(dt.t * k * dt.stride, dtype=torch.int32, device="cuda")
    side = torch.empty(2 * b * k, dtype=torch.int32, device="cuda")
    regs = torch.tensor(sorted(REGIONS, reverse=True), dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.gcs_region_sweep_workspace_bytes(dt.t, k, dt.stride, n), dtype=torch.uint8, device="cuda")
    out = torch.empty(2 * n * dt.t * 4, dtype=torch.int64, device="cuda")
    counts = lib.gcs_region_counts_batch_u8 if dt.u8 else lib.gcs_region_counts_batch

    def leaf():
        assert counts(c["lab"].data_ptr(), dt.maps.data_ptr(), dt.first_d.data_ptr(), b, dt.t, dt.a_max, c["h"], c["w"], k, dt.stride,
                      hist.data_ptr(), side.data_ptr(), side.data_ptr() + 4 * b * k, torch.cuda.current_stream().cuda_stream) == 0

    def sweep():
        assert lib.gcs_region_sweep(hist.data_ptr(), c["merges"].data_ptr(), c["alive"].data_ptr(), dt.img_of_d.data_ptr(),
                                    regs.data_ptr(), b, dt.t, k, dt.stride, n, ws.data_ptr(), out.data_ptr(),
                                    out.data_ptr() + n * dt.t * 32, torch.cuda.current_stream().cuda_stream) == 0
    leaf()
    saved = hist.clone()
    return leaf, sweep, lambda: hist.copy_(saved)


def _per_cut(torch, s, res, prefix="", agreement=True):
    """The path the sweep replaces, per R: the cut, the scoring call with ``agreement`` (device time and host clock)."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_resident, submit_scores_batch_resident
    c = s["cases"][""]
    cut = torch.empty_like(c["lab"])
    dev = wall = 0.0
    for r in REGIONS:
        m = _median_ms(torch, lambda: s["seg"].ops.region_tree_cut(c["lab"], c["merges"], c["alive"], BATCH, H, W, c["k"], r, cut))
        res.update({"%scut_ms_%d" % (prefix, r): m[0], "%scut_ms_%d_min" % (prefix, r): m[1], "%scut_ms_%d_max" % (prefix, r): m[2]})
        times = []
        for _ in range(WARM + REPS):                     # the second event goes in behind the result copy, before the host waits for it
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pending = submit_scores_batch_resident(cut, c["truth"], n_segments=r, agreement=agreement)
            e1.record()
            pending.result()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        sc = (statistics.median(times[WARM:]),)
        wl = _wall_ms(torch, lambda: all_scores_batch_resident(cut, c["truth"], n_segments=r, agreement=agreement))
        res.update({"%sscore_ms_%d" % (prefix, r): sc[0], "%sscore_wall_ms_%d" % (prefix, r): wl[0]})
        dev += m[0] + sc[0]
        wall += m[0] + wl[0]
    res[prefix + "per_cut_path_ms"] = dev
    res[prefix + "per_cut_path_wall_ms"] = wall


def _write(res, out_path, merge=False):
    print(json.dumps(res), flush=True)
    if out_path:
        if merge and os.path.exists(out_path):
            res = dict(json.load(open(out_path)), **res)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def percut_main(out_path, parent):
    sys.path.insert(0, ROOT)
    import torch
    _use_parent(parent)
    s = _setup(torch, big=False)
    res = {}
    _per_cut(torch, s, res, "parent_")
    _write(res, out_path, merge=True)


def time_main(out_path=None, parent=None):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    from gabor_color_image_segmentation_amd.evaluate_gpu import region_sweep_resident, sweep_agreement
    parent_plans = {}
    if parent:                                           # the parent's library first (one process, both builds)
        here, sigs = _use_parent(parent)
        parent_plans = {"parent_step0": Segmenter(n_superpixels=N, spatial_weight=LAM, **BANK),
                        "parent_step8": Segmenter(n_superpixels=N, spatial_weight=LAM, n_regions=R, **BANK)}
        _lib.LIB_PATH, _lib._lib, _lib.SIGNATURES = here, None, sigs
    s = _setup(torch)
    main = s["cases"][""]
    res = dict(batch=BATCH, shape=[H, W], n_superpixels=N, K=main["k"], annotators=main["truth"].t, stride=main["truth"].stride,
               regions=REGIONS, reps=REPS, warm=WARM)
    for tag, c in s["cases"].items():
        leaf, sweep, restore = _raw_calls(torch, s["lib"], c)
        m = _median_ms(torch, leaf)
        res.update({"leaf%s_ms" % tag: m[0], "leaf%s_ms_min" % tag: m[1], "leaf%s_ms_max" % tag: m[2]})
        times = []
        for _ in range(WARM + REPS):
            restore()
            times.append(_timed(torch, sweep))
        times = times[WARM:]
        res.update({"sweep%s_ms" % tag: statistics.median(times), "sweep%s_ms_min" % tag: min(times), "sweep%s_ms_max" % tag: max(times)})
        dt = c["truth"]
        m = _wall_ms(torch, lambda: sweep_agreement(*region_sweep_resident(c["lab"], c["merges"], c["alive"], dt, REGIONS), dt.first,
                                                    c["h"] * c["w"], REGIONS))
        res.update({"sweep%s_wall_ms" % tag: m[0], "sweep%s_wall_ms_min" % tag: m[1], "sweep%s_wall_ms_max" % tag: m[2]})
    res["one_pass_path_ms"] = res["leaf_ms"] + res["sweep_ms"]
    _per_cut(torch, s, res)
    plans = {"step0": Segmenter(n_superpixels=N, spatial_weight=LAM, **BANK),
             "step8": Segmenter(n_superpixels=N, spatial_weight=LAM, n_regions=R, **BANK)}
    plans.update(parent_plans)
    times, outs = {name: [] for name in plans}, {}
    for rnd in range(WARM + REPS):                       # the builds take turns inside each round
        for name, plan in plans.items():
            t = _timed(torch, lambda: outs.__setitem__(name, plan.segment_device(s["imgs"])))
            if rnd >= WARM:
                times[name].append(t)
    for name, ts in times.items():
        res.update({name + "_ms": statistics.median(ts), name + "_ms_min": min(ts), name + "_ms_max": max(ts)})
    for q in ("0", "8"):
        if "parent_step" + q in outs:
            a, p = "step" + q, "parent_step" + q
            res["parent_labels_equal_" + q] = bool(torch.equal(outs[a], outs[p]))
            res["medians_within_ranges_" + q] = bool(res[p + "_ms_min"] <= res[a + "_ms"] <= res[p + "_ms_max"]
                                                     and res[a + "_ms_min"] <= res[p + "_ms"] <= res[a + "_ms_max"])
    _write(res, out_path, merge=True)


def trace_main():
    sys.path.insert(0, ROOT)
    import torch
    s = _setup(torch)
    for c in s["cases"].values():
        leaf, sweep, restore = _raw_calls(torch, s["lib"], c)
        for _ in range(WARM + REPS):
            leaf()
            sweep()
        torch.cuda.synchronize()


def split_main(trace, out_path):
    with open(trace) as f:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    per = {}
    for t0, t1, name in ks:
        for key in ("region_counts_kernel", "region_sweep_kernel"):
            if key in name:
                per.setdefault(key, []).append((t1 - t0) / 1e6)
    n = WARM + REPS
    res = {}
    tags = ("", "_4096")                        # the order of _setup's cases
    for key, ts in per.items():
        extra = 1 if key == "region_counts_kernel" else 0    # _raw_calls makes the tables once before the timed calls of each case
        ts = ts[-len(tags) * (n + extra):]
        for j, tag in enumerate(tags):
            mine = ts[j * (n + extra) + extra:(j + 1) * (n + extra)]
            res[key + tag + "_ms"] = statistics.median(mine[WARM:])
    _write(res, out_path, merge=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    args = sys.argv[2:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
    if mode == "trace":
        trace_main()
    elif mode == "split":
        split_main(sys.argv[2], sys.argv[3])
    elif mode == "percut":
        percut_main(paths[0] if paths else None, parent)
    else:
        time_main(paths[0] if paths else None, parent)
