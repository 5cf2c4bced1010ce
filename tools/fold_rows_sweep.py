"""Per-pass times of the self-updating loop (B=64, 321x481, global and per_image) for the GCS_KP_FOLD_ROWS of the environment,
beside the init / pass / reduce loop of the same library."""
import os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gabor_color_image_segmentation_amd import Segmenter
from gabor_color_image_segmentation_amd.segmenter import lloyd
from gabor_color_image_segmentation_amd.synthetic import synthetic_shard
B, H, W, K, N = 64, 321, 481, 8, 10
imgs = torch.from_numpy(synthetic_shard(0, B, H, W)).cuda()
R = os.environ.get("GCS_KP_FOLD_ROWS", "default")
for mode in ("global", "per_image"):
    seg = Segmenter()
    ws = seg._workspace(B, H, W, mode)
    seg.ops.gabor_features(imgs, ws["feats"])
    out = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    n_sets = B if mode == "per_image" else 1
    ops = seg.ops
    per = [[] for _ in range(N)]
    loop_new, loop_old = [], []
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for rnd in range(14):
        e = [ev() for _ in range(N + 1)]
        e[0].record()
        for t in range(N):
            rev = not (t & 1)
            if t == N - 1:
                ops.assign_raster(ws["feats"], ws["cent"], B, H, W, K, n_sets, out, reverse=rev, fused=(ws["fold"], t))
            else:
                ops.assign_accumulate(ws["feats"], ws["cent"], B, H, W, K, n_sets, None, None, reverse=rev, fused=(ws["fold"], t))
            e[t + 1].record()
        a, b = ev(), ev()
        a.record(); lloyd(ops, ws["feats"], B, H, W, K, N, mode, ws["labels"], ws["partials"], ws["cent"], ws["sums"], raster=out, fold=ws["fold"]); b.record()
        c, d = ev(), ev()
        c.record(); lloyd(ops, ws["feats"], B, H, W, K, N, mode, ws["labels"], ws["partials"], ws["cent"], ws["sums"], raster=out, fold=None); d.record()
        torch.cuda.synchronize()
        if rnd >= 2:
            for t in range(N):
                per[t].append(e[t].elapsed_time(e[t + 1]) * 1e3)
            loop_new.append(a.elapsed_time(b) * 1e3); loop_old.append(c.elapsed_time(d) * 1e3)
    med = [statistics.median(p) for p in per]
    print(f"rows={R:>7s} {mode:9s} loop new {statistics.median(loop_new):7.1f} us  old {statistics.median(loop_old):7.1f} us | "
          f"pass0 {med[0]:.1f} mid {statistics.mean(med[1:-1]):.1f} last {med[-1]:.1f} (with events)", flush=True)
