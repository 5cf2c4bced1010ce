#!/usr/bin/env python3
"""Time of the reference's region and shape metrics of every cut at once (SPEC.md §17) at batch 64 x 481x321 behind the superpixel
stage and the tree (n = 300, lambda = 576, colour bank 5, 1/8, 4; K = 294; 5 synthetic annotator maps per image, T = 320), beside the
per-cut path it replaces: the batch, the bank, the annotator maps and the six R of tools/region_sweep_time.py.

    cut_metrics_time.py time   [out.json]
    cut_metrics_time.py percut [out.json] --parent path/to/parent/libgcs.so     (a process of its own: only the parent's library is loaded)

``time``: every ``*_ms`` figure is the median of ``reps`` calls after ``warm`` warm-up calls, each call bracketed by two events on the
stream, on device-resident inputs (``*_wall_ms``: host calls that end with a copy to the host, by the host's clock):
  leaf_ms            gcs_region_counts_batch_u8 with n_segments = K: the leaf tables, zeroing included (as in region_sweep_time.py)
  shapes_ms          gcs_cut_shapes for REGIONS (its three launches)
  under_ms           gcs_region_sweep_under for REGIONS without the agreement outputs (the leaf tables restored from a copy before
                     every call, outside the events: the call consumes them)
  under_agree_ms     the same call with the agreement outputs; sweep_ms: gcs_region_sweep alone on the same tables
  new_route_ms       leaf_ms + under_ms + shapes_ms: the four metrics of all R
  metrics_wall_ms    evaluate_gpu.metrics_sweep_resident for REGIONS (boundary scores included), by the host's clock
``percut`` writes, measured through the PARENT commit's library: per R of REGIONS gcs_region_tree_cut (parent_cut_ms_R) and
submit_scores_batch_resident on that cut between two events, kernels and the result copy (parent_score_ms_R); their sum over REGIONS
(parent_per_cut_path_ms) and the same with all_scores_batch_resident by the host's clock (parent_per_cut_path_wall_ms).
Whichever mode runs second adds ``ratio`` = parent_per_cut_path_ms / new_route_ms.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contour_map_time import BATCH, H, REGIONS, REPS, W, WARM, _median_ms, _timed, _wall_ms  # noqa: E402
from region_sweep_time import _per_cut, _setup, _use_parent  # noqa: E402


def _write(res, out_path):
    if out_path and os.path.exists(out_path):
        res = dict(json.load(open(out_path)), **res)
    if "parent_per_cut_path_ms" in res and "new_route_ms" in res:
        res["ratio"] = res["parent_per_cut_path_ms"] / res["new_route_ms"]
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def percut_main(out_path, parent):
    if not parent:
        sys.exit("cut_metrics_time.py percut [out.json] --parent path/to/parent/libgcs.so")
    sys.path.insert(0, ROOT)
    import torch
    _use_parent(parent)
    res = {}
    _per_cut(torch, _setup(torch, big=False), res, "parent_", agreement=False)
    _write(res, out_path)


def time_main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd.evaluate_gpu import metrics_sweep_resident
    s = _setup(torch, big=False)
    lib, c = s["lib"], s["cases"][""]
    dt, k, n = c["truth"], c["k"], len(REGIONS)
    contours = s["seg"].contour_map_device(c["lab"], c["merges"], c["alive"])
    stream = lambda: torch.cuda.current_stream().cuda_stream
    regs = torch.tensor(sorted(REGIONS, reverse=True), dtype=torch.int32, device="cuda")
    hist = torch.empty(dt.t * k * dt.stride, dtype=torch.int32, device="cuda")
    side = torch.empty(2 * BATCH * k, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.gcs_region_sweep_under_workspace_bytes(dt.t, k, dt.stride, n), dtype=torch.uint8, device="cuda")
    out = torch.empty(n * dt.t * 11, dtype=torch.int64, device="cuda")
    agr = out.data_ptr() + n * dt.t * 24
    ws2 = torch.empty(lib.gcs_cut_shapes_workspace_bytes(BATCH, k, n), dtype=torch.uint8, device="cuda")
    out2 = torch.empty(n * BATCH * (2 * k + 1), dtype=torch.int32, device="cuda")
    counts = lib.gcs_region_counts_batch_u8 if dt.u8 else lib.gcs_region_counts_batch

    def leaf():
        assert counts(c["lab"].data_ptr(), dt.maps.data_ptr(), dt.first_d.data_ptr(), BATCH, dt.t, dt.a_max, H, W, k, dt.stride,
                      hist.data_ptr(), side.data_ptr(), side.data_ptr() + 4 * BATCH * k, stream()) == 0

    def under(agreement):
        assert lib.gcs_region_sweep_under(hist.data_ptr(), c["merges"].data_ptr(), c["alive"].data_ptr(), dt.img_of_d.data_ptr(),
                                          regs.data_ptr(), BATCH, dt.t, k, dt.stride, n, ws.data_ptr(), out.data_ptr(),
                                          agr if agreement else None, agr + n * dt.t * 32 if agreement else None, stream()) == 0

    def sweep():
        assert lib.gcs_region_sweep(hist.data_ptr(), c["merges"].data_ptr(), c["alive"].data_ptr(), dt.img_of_d.data_ptr(),
                                    regs.data_ptr(), BATCH, dt.t, k, dt.stride, n, ws.data_ptr(), agr, agr + n * dt.t * 32, stream()) == 0

    def shapes():
        assert lib.gcs_cut_shapes(c["lab"].data_ptr(), contours.data_ptr(), c["merges"].data_ptr(), c["alive"].data_ptr(),
                                  regs.data_ptr(), BATCH, H, W, k, n, ws2.data_ptr(), out2.data_ptr(),
                                  out2.data_ptr() + 4 * n * BATCH * k, out2.data_ptr() + 8 * n * BATCH * k, stream()) == 0

    res = dict(batch=BATCH, shape=[H, W], K=k, annotators=dt.t, stride=dt.stride, regions=REGIONS, reps=REPS, warm=WARM)
    for name, fn in (("leaf", leaf), ("shapes", shapes)):
        m = _median_ms(torch, fn)
        res.update({name + "_ms": m[0], name + "_ms_min": m[1], name + "_ms_max": m[2]})
    saved = hist.clone()
    for name, fn in (("under", lambda: under(False)), ("under_agree", lambda: under(True)), ("sweep", sweep)):
        times = []
        for _ in range(WARM + REPS):
            hist.copy_(saved)
            times.append(_timed(torch, fn))
        times = times[WARM:]
        res.update({name + "_ms": statistics.median(times), name + "_ms_min": min(times), name + "_ms_max": max(times)})
    res["new_route_ms"] = res["leaf_ms"] + res["under_ms"] + res["shapes_ms"]
    m = _wall_ms(torch, lambda: metrics_sweep_resident(c["lab"], c["merges"], c["alive"], contours, dt, REGIONS))
    res.update({"metrics_wall_ms": m[0], "metrics_wall_ms_min": m[1], "metrics_wall_ms_max": m[2]})
    _write(res, out_path)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    args = sys.argv[2:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
    if mode == "percut":
        percut_main(paths[0] if paths else None, parent)
    else:
        time_main(paths[0] if paths else None)
