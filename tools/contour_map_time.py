#!/usr/bin/env python3
"""Time of the contour map and the sweep over all cuts (SPEC.md §15) at batch 64 x 481x321 behind the superpixel stage and the tree
(n = 300, lambda = 576, colour bank 5, 1/8, 4; K = 294), beside one cut and one scoring call on a cut.

    contour_map_time.py time  [out.json] [--parent path/to/parent/libgcs.so]
    contour_map_time.py trace                      (under rocprofv3 --kernel-trace -f csv -d <dir> -o run --)
    contour_map_time.py split <run_kernel_trace.csv> <out.json>

``time``: every ``*_ms`` figure is the median of ``reps`` calls after ``warm`` warm-up calls, each call bracketed by two events on the
stream, on device-resident inputs (``*_wall_ms``: host calls that end with a copy to the host, by the host's clock):
  contours_ms        gcs_region_tree_contours on the batch's superpixel maps and trees (prepare + pixels, one call)
  contours_4096_ms   the same call on one 64 x 64 image of one-pixel labels with the chain (K-2, K-1), ..., (0, 1): K = 4096
  sweep_ms           gcs_boundary_sweep_resident on the batch's contour maps against 5 synthetic annotator maps per image
  cut_ms             gcs_region_tree_cut at R = 8
  counts_ms          gcs_boundary_counts_resident on that cut (the three launches the sweep replaces, per R)
  score_wall_ms      evaluate_gpu.all_scores_batch_resident on that cut (all scores of one R, counts and region tables)
  sweep_wall_ms      boundary_sweep_resident + sweep_scores for REGIONS (all boundary scores of all R)
  step0 / step8      Segmenter(n_superpixels=300[, n_regions=8]).segment_device here and (--parent) through the PARENT commit's
                     library in the same process, the builds taking turns call by call: "nothing changed when the calls are not made"
``trace`` runs warm + reps contour calls on the batch, then on the K = 4096 case, then the sweeps; ``split`` reads the kernel trace of
that run and adds the median time of each kernel to the JSON.
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
BATCH, H, W, N, LAM, R = 64, 481, 321, 300, 576, 8
REGIONS = [4, 6, 8, 12, 16, 32]
ANNOTATORS = 5


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


def _wall_ms(torch, fn, reps=REPS, warm=WARM):
    times = []
    for _ in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    times = times[warm:]
    return statistics.median(times), min(times), max(times)


def _truth(np):
    """ANNOTATORS synthetic annotator maps per image: a few rectangles each."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth
    rng = np.random.default_rng(1)
    t = np.zeros((BATCH * ANNOTATORS, H, W), np.uint16)
    for m in t:
        for _ in range(6):
            y, x = int(rng.integers(0, H - 40)), int(rng.integers(0, W - 40))
            m[y:y + int(rng.integers(30, 200)), x:x + int(rng.integers(30, 200))] += 1
    first = np.arange(BATCH + 1, dtype=np.int32) * ANNOTATORS
    return DeviceTruth(t, first, np.repeat(np.arange(BATCH), ANNOTATORS).astype(np.int32), [int(m.max()) + 1 for m in t])


def _setup(torch):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = torch.from_numpy(synthetic_batch(BATCH, H, W, seed=0)).cuda()
    seg = Segmenter(n_superpixels=N, spatial_weight=LAM, **BANK)
    lab, merges, _, alive = seg.region_tree_device(imgs)
    k = merges.shape[1] + 1
    s = dict(seg=seg, imgs=imgs, lab=lab, merges=merges, alive=alive, k=k, lib=_lib.load(), truth=_truth(np),
             ws=seg.ops.contour_buffers(BATCH, k), out=torch.empty_like(lab))
    big = 4096
    s["big"] = dict(lab=torch.arange(big, dtype=torch.int32, device="cuda").reshape(1, 64, 64),
                    merges=torch.tensor([(q - 1, q) for q in range(big - 1, 0, -1)], dtype=torch.int32, device="cuda").reshape(1, big - 1, 2),
                    alive=torch.tensor([big], dtype=torch.int32, device="cuda"), ws=seg.ops.contour_buffers(1, big),
                    out=torch.empty((1, 64, 64), dtype=torch.int32, device="cuda"))
    s["hist"] = torch.empty((BATCH + 2 * s["truth"].t, k + 1), dtype=torch.int32, device="cuda")
    return s


def _contours(s):
    s["seg"].ops.region_tree_contours(s["lab"], s["merges"], s["alive"], BATCH, H, W, s["k"], s["ws"], s["out"])


def _contours_big(s):
    b = s["big"]
    s["seg"].ops.region_tree_contours(b["lab"], b["merges"], b["alive"], 1, 64, 64, 4096, b["ws"], b["out"])


def _sweep(torch, s):
    dt = s["truth"]
    rc = s["lib"].gcs_boundary_sweep_resident(s["out"].data_ptr(), dt.planes.data_ptr(), dt.img_of_d.data_ptr(), BATCH, dt.t, H, W, s["k"],
                                              s["hist"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0


def time_main(out_path=None, parent=None):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    from gabor_color_image_segmentation_amd.evaluate_gpu import (all_scores_batch_resident, boundary_sweep_resident, sweep_scores)
    parent_plans = {}
    if parent:                                           # the parent's library first (one process, both builds)
        import ctypes
        here, sigs = _lib.LIB_PATH, dict(_lib.SIGNATURES)
        raw = ctypes.CDLL(os.path.abspath(parent))
        _lib.LIB_PATH, _lib._lib = os.path.abspath(parent), None
        _lib.SIGNATURES = {k: v for k, v in sigs.items() if hasattr(raw, k)}
        parent_plans = {"parent_step0": Segmenter(n_superpixels=N, spatial_weight=LAM, **BANK),
                        "parent_step8": Segmenter(n_superpixels=N, spatial_weight=LAM, n_regions=R, **BANK)}
        _lib.LIB_PATH, _lib._lib, _lib.SIGNATURES = here, None, sigs
    s = _setup(torch)
    seg, dt, lib = s["seg"], s["truth"], s["lib"]
    res = dict(batch=BATCH, shape=[H, W], n_superpixels=N, K=s["k"], annotators=dt.t, regions=REGIONS, reps=REPS, warm=WARM)
    cut = torch.empty_like(s["lab"])
    scratch = torch.empty(lib.gcs_bit_planes_bytes(BATCH, H, W), dtype=torch.uint8, device="cuda")
    counts = torch.empty(BATCH + 3 * dt.t, dtype=torch.int64, device="cuda")

    def counts_call():
        assert lib.gcs_boundary_counts_resident(cut.data_ptr(), dt.planes.data_ptr(), dt.bd_counts.data_ptr(), dt.img_of_d.data_ptr(),
                                                BATCH, dt.t, H, W, scratch.data_ptr(), counts.data_ptr(), None,
                                                torch.cuda.current_stream().cuda_stream) == 0
    for name, fn in (("contours", lambda: _contours(s)), ("contours_4096", lambda: _contours_big(s)), ("sweep", lambda: _sweep(torch, s)),
                     ("cut", lambda: seg.ops.region_tree_cut(s["lab"], s["merges"], s["alive"], BATCH, H, W, s["k"], R, cut)),
                     ("counts", counts_call)):
        m = _median_ms(torch, fn)
        res.update({name + "_ms": m[0], name + "_ms_min": m[1], name + "_ms_max": m[2]})
    bd = dt.bd_counts.cpu().numpy()
    for name, fn in (("score_wall", lambda: all_scores_batch_resident(cut, dt, n_segments=R, agreement=True)),
                     ("sweep_wall", lambda: sweep_scores(boundary_sweep_resident(s["out"], s["alive"], dt), s["alive"].cpu().numpy(), bd,
                                                         dt.first, REGIONS))):
        m = _wall_ms(torch, fn)
        res.update({name + "_ms": m[0], name + "_ms_min": m[1], name + "_ms_max": m[2]})
    res["boundary_fraction"] = float((s["out"] > 0).float().mean())
    res["per_cut_path_ms"] = len(REGIONS) * (res["cut_ms"] + res["counts_ms"])
    res["one_pass_path_ms"] = res["contours_ms"] + res["sweep_ms"]
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
            res["parent_labels_equal_" + q] = bool(torch.equal(outs["step" + q], outs["parent_step" + q]))
            a, p = "step" + q, "parent_step" + q
            res["medians_within_ranges_" + q] = bool(res[p + "_ms_min"] <= res[a + "_ms"] <= res[p + "_ms_max"]
                                                     and res[a + "_ms_min"] <= res[p + "_ms"] <= res[a + "_ms_max"])
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def trace_main():
    sys.path.insert(0, ROOT)
    import torch
    s = _setup(torch)
    for fn in (lambda: _contours(s), lambda: _contours_big(s), lambda: _sweep(torch, s)):
        for _ in range(WARM + REPS):
            fn()
        torch.cuda.synchronize()


def split_main(trace, out_path):
    with open(trace) as f:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    per = {}
    for t0, t1, name in ks:
        for key in ("rt_contour_prepare_kernel", "rt_contour_kernel", "boundary_sweep_kernel"):
            if key in name:
                per.setdefault(key, []).append((t1 - t0) / 1e6)
    n = WARM + REPS
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    for key, ts in per.items():
        if key == "boundary_sweep_kernel":
            res["sweep_kernel_ms"] = statistics.median(ts[-n:][WARM:])
            continue
        ts = ts[-2 * n:]                                 # (the set-up ran no contour call)
        short = "prepare" if "prepare" in key else "pixels"
        res[short + "_kernel_ms"] = statistics.median(ts[WARM:n])
        res[short + "_kernel_4096_ms"] = statistics.median(ts[n + WARM:])
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
