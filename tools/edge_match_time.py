#!/usr/bin/env python3
"""Cost and quality of the device matcher (SPEC.md §27) on the 24 val fixture images: the four maps of DESIGN.md §7's table of §26
(E' and E of the colour bank at k = 8, r = 8, n = 8, 16 bins, weights (2, 2, 1, 1), as delivered and thinned), made on the device
(``Segmenter.cue_edges_device`` / ``texton_edges_device``), one step per map for the whole set. GPU only.

    edge_match_time.py [out.json] [jobs]

  rows[<map>]   device_ms: ``evaluate_gpu.edge_match_resident`` at all 256 levels, both shape groups one after the other, between two
                events on the stream (host arithmetic and the result copy included: the call ends in a synchronise); the median of
                REPS calls after a warm-up call, with min and max. kernel_ms: the seven launches alone (``gcs_edge_match`` between two
                events). ODS / OIS / recall and precision at ODS over all 256 levels, and over the 32 levels tau = 8 j + 3 of
                tools/edge_thin_quality.py from the same integers. per_map: per annotator map |Q_t|, #{q > 0}, M at level 0 and
                the kernel's counters (search steps, 64-lane probes, deepest stack, failed searches); their totals, probes_per_step
                and the steps of the slowest map, which bounds the launch: the maps run side by side.
  host          for the two E' maps: ``evaluate.match_scores`` (the host path: one Hopcroft-Karp matching per level and annotator)
                at the 32 levels on ``jobs`` processes (default 16), wall seconds; host_equals_device: every float of the host's
                recall / precision / F is the device's at that level.
  device_over_host   device wall time of the two E' maps (256 levels) over the host's (32 levels).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4)
K, LEVELS, REPS = 8, 256, 5
MATCH_TAUS = tuple(8 * j + 3 for j in range(32))
ROWS = ("Ep_thick", "Ep_thin", "E_thick", "E_thin")
HOST_ROWS = ("Ep_thick", "Ep_thin")


def host_job(job):
    from gabor_color_image_segmentation_amd.evaluate import match_scores
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    i, name, edges, th = job
    sc = match_scores(edges, PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))[i], th)
    return i, name, {k: v.tolist() for k, v in sc.items()}


def _summary(f, rec, prec, th):
    from gabor_color_image_segmentation_amd.evaluate import ods_ois
    best = ods_ois(f, th)
    j = th.index(best["ODS_regions"])
    return dict(ODS=best["ODS"], ODS_threshold=best["ODS_regions"], OIS=best["OIS"], recall_at_ODS=float(np.mean([r[j] for r in rec])),
                precision_at_ODS=float(np.mean([p[j] for p in prec])))


def _events(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def write(res, out_path):
    """The JSON with one annotator map per line."""
    res = json.loads(json.dumps(res))
    per = {name: row.pop("per_map") for name, row in res["rows"].items()}
    for name, row in res["rows"].items():
        row["per_map"] = "@" + name
    taus, res["match_taus"] = res["match_taus"], "@taus"
    text = json.dumps(res, indent=1).replace(json.dumps("@taus"), json.dumps(taus))
    for name, maps in per.items():
        text = text.replace(json.dumps("@" + name), "[\n" + ",\n".join("    " + json.dumps(p) for p in maps) + "\n   ]")
    with open(out_path, "w") as fh:
        fh.write(text + "\n")


def main(out_path=None, jobs=16):
    import torch
    from multiprocessing import get_context
    from gabor_color_image_segmentation_amd import Segmenter, _lib
    from gabor_color_image_segmentation_amd.evaluate import match_distance2
    from gabor_color_image_segmentation_amd.evaluate_gpu import _match_offsets, edge_match_counts_resident, edge_match_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    pack = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    ids = [str(i) for i in pack["ids"]]
    groups = [[i for i in ids if pack["img_" + i].shape[:2] == shape] for shape in sorted({pack["img_" + i].shape[:2] for i in ids})]
    order = [i for g in groups for i in g]
    seg = Segmenter(k=K, **COLOUR)
    batches = [torch.from_numpy(np.stack([pack["img_" + i] for i in g])).cuda() for g in groups]
    resident = [truth.to_device(g) for g in groups]
    make = {"Ep_thick": lambda d: seg.cue_edges_device(d), "Ep_thin": lambda d: seg.cue_edges_device(d, thin=True),
            "E_thick": lambda d: seg.texton_edges_device(d), "E_thin": lambda d: seg.texton_edges_device(d, thin=True)}
    lib = _lib.load()
    res = dict(images=len(ids), levels=LEVELS, match_taus=list(MATCH_TAUS), bank=COLOUR, k=K, reps=REPS, jobs=jobs,
               annotator_maps=int(sum(r.t for r in resident)), rows={})
    host_jobs, device_f = [], {}
    for name in ROWS:
        maps = [make[name](d) for d in batches]
        step = -(-(max(int(m.max()) for m in maps) + 1) // LEVELS)
        th = [step * (tau + 1) - 1 for tau in range(LEVELS)]

        def sweep():
            out = [edge_match_resident(m, r, levels=LEVELS, step=step) for m, r in zip(maps, resident)]
            return [np.concatenate([o[k] for o in out]) for k in range(3)]
        sweep()                                              # warm-up: code objects, the thin planes, the allocator
        times, walls = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            ms, (rec, prec, f) = _events(torch, sweep)
            walls.append(time.perf_counter() - t0)
            times.append(ms)
        # the launches alone, and the kernel's counters
        kernel_ms, per_map = 0.0, []
        for m, r in zip(maps, resident):
            q = torch.clamp(torch.div(m, step, rounding_mode="floor"), max=LEVELS).to(torch.int32).contiguous()
            thin, _, n_thin = r.thin_planes()
            offs = torch.from_numpy(_match_offsets(lib, match_distance2(r.h, r.w))).cuda()
            cap = int(n_thin.max()) + 1
            ws = torch.empty(lib.gcs_edge_match_bytes(r.b, r.t, r.h, r.w, cap), dtype=torch.uint8, device="cuda")
            out = torch.empty((r.t + r.b, LEVELS), dtype=torch.int32, device="cuda")
            call = lambda: _lib.check(lib.gcs_edge_match(q.data_ptr(), thin.data_ptr(), r.img_of_d.data_ptr(), r.b, r.t, r.h, r.w, LEVELS,
                                                         offs.data_ptr(), len(offs), cap, ws.data_ptr(), out.data_ptr(),
                                                         out[r.t:].data_ptr(), torch.cuda.current_stream().cuda_stream), "gcs_edge_match")
            call()
            torch.cuda.synchronize()
            kernel_ms += float(np.median([_events(torch, call)[0] for _ in range(REPS)]))
            matched, above, n, counters = edge_match_counts_resident(q, r, LEVELS, stats=True)
            assert np.array_equal(matched, out[:r.t].cpu().numpy())
            for t in range(r.t):
                per_map.append(dict(n_thin=int(n[t]), map_pixels=int(above[r.img_of[t], 0]), matched=int(matched[t, 0]),
                                    steps=int(counters[t, 0]), probes=int(counters[t, 1]), deepest=int(counters[t, 2]),
                                    failed=int(counters[t, 3])))
        pick = lambda table: [[row[tau] for tau in MATCH_TAUS] for row in table.tolist()]
        row = dict(step=step, device_ms=float(np.median(times)), device_ms_min=min(times), device_ms_max=max(times),
                   device_wall_s=float(np.median(walls)), kernel_ms=kernel_ms,
                   all_levels=_summary(f.tolist(), rec.tolist(), prec.tolist(), th),
                   levels_32=_summary(pick(f), pick(rec), pick(prec), [th[tau] for tau in MATCH_TAUS]),
                   steps_total=sum(p["steps"] for p in per_map), failed_total=sum(p["failed"] for p in per_map),
                   probes_per_step=sum(p["probes"] for p in per_map) / max(1, sum(p["steps"] for p in per_map)),
                   deepest=max(p["deepest"] for p in per_map), slowest_map_steps=max(p["steps"] for p in per_map), per_map=per_map)
        res["rows"][name] = row
        print(json.dumps({k: v for k, v in row.items() if k != "per_map"}), flush=True)
        if name in HOST_ROWS:
            device_f[name] = dict(recall=pick(rec), precision=pick(prec), fmeasure=pick(f))
            host_jobs += [(i, name, m.cpu().numpy()[j], [th[tau] for tau in MATCH_TAUS]) for g, m in zip(groups, maps)
                          for j, i in enumerate(g)]
    # the host path on the same maps: 32 levels, `jobs` fresh processes that never open the device
    t0 = time.perf_counter()
    host = {}
    with get_context("spawn").Pool(jobs) as pool:
        for i, name, sc in pool.imap_unordered(host_job, host_jobs):
            host.setdefault(name, {})[i] = sc
    host_s = time.perf_counter() - t0
    same = all(host[name][i][key] == device_f[name][key][order.index(i)] for name in HOST_ROWS for i in order
               for key in ("recall", "precision", "fmeasure"))
    device_s = sum(res["rows"][name]["device_wall_s"] for name in HOST_ROWS)
    res["host"] = dict(rows=list(HOST_ROWS), levels=len(MATCH_TAUS), jobs=jobs, wall_s=host_s, host_equals_device=bool(same))
    res["device_over_host"] = device_s / host_s
    res["device_within_a_tenth_of_host"] = bool(device_s <= host_s / 10)
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    if out_path:
        write(res, out_path)
    return res


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, int(sys.argv[2]) if len(sys.argv) > 2 else 16)
