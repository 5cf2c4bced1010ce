#!/usr/bin/env python3
"""Cost of the regulariser of SPEC.md §30 at batch 64 x 481x321 on the 24 val fixture images (landscape ones transposed, repeated
to 64), colour bank (n_orient 5, color_weight 1/8, chroma_gain 4; D = 72) at k = 8 and k = 16. GPU only.

    label_relax_time.py [out.json] --parent path/to/parent/libgcs.so

Medians of ``reps`` calls after ``warm`` warm-up calls, each call between two events on the stream, device-resident inputs; calls
that are compared take turns, call by call (the method of tools/cue_gradient_time.py):
  copy_gbps                     the yardstick of the byte floors: a device-to-device copy of 1 GiB on this box (bytes read + written)
  k<k>_costs_ms                 (a) the gcs_kmeans_costs launch on the step's slab; k<k>_costs_torch_ms: gcs_features_unpack plus
                                    a float64 torch formulation with equal outputs (x^2 - 2 x.c + c^2, exact below 2^53);
                                    k<k>_costs_floor_ms: slab bytes + B k H W 8 bytes at copy_gbps
  k<k>_relax_ms                 (b) gcs_label_relax, 4 sweeps, 8 neighbours, beta of lambda = 1/4, no optional output;
                                    k<k>_relax_torch_ms: the sub-passes in torch operations with equal outputs;
                                    k<k>_relax_floor_ms: the copy plus 4 x (the volume once + the map read and written) at copy_gbps;
                                    k<k>_relax_sweeps<n>_ms for n = 1, 2, 8; k<k>_relax_n4_ms (4 neighbours)
  k<k>_segment_ms, k<k>_segment_regularised_ms
                                (c) Segmenter.segment_device without and with regularize = 0.25
  k<k>_clusters_ms, k<k>_clusters_regularised_ms
                                (d) the same with tree_nodes = "clusters", n_regions = 8, and the node counts of both
                                    (k<k>_nodes, k<k>_nodes_regularised: min / mean / max over the batch)
  step_default_ms / parent_default_ms, step_predict_ms / parent_predict_ms, step_evaluate_ms / parent_evaluate_ms
                                (e) "off means unchanged": the default plan's segment_device, predict_device(refine=0) and the
                                    gcs_kmeans_evaluate launch with this library and with the PARENT commit's library in this
                                    process, taking turns (…_equal: the same outputs; …_inside_parent_range)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cue_gradient_time import _timed, _turns, COLOUR, REPS, WARM  # noqa: E402
from feature_gradient_time import _batch, _stats, _with_library, BATCH, H, W  # noqa: E402

LAM, Q = 0.25, 64
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def torch_costs(torch, ops, feats, cent, k):
    """unpack + float64: (B, k, H, W) int64."""
    canon = ops.features_unpack(feats, BATCH, H, W)                       # (B, D, H, W) int16 holding uint16
    out = torch.empty((BATCH, k, H, W), dtype=torch.int64, device="cuda")
    for b in range(BATCH):
        x = (canon[b].reshape(canon.shape[1], -1).to(torch.int32) & 0xFFFF).to(torch.float64)      # (D, P)
        c = (cent[b].to(torch.int32) & 0xFFFF).to(torch.float64)                                  # (k, D)
        d = (x * x).sum(dim=0)[None] - 2.0 * (c @ x) + (c * c).sum(dim=1)[:, None]
        out[b] = d.to(torch.int64).reshape(k, H, W)
    return out


def torch_relax(torch, costs, labels, beta, sweeps, neighbours):
    """SPEC.md §30 in torch operations for start maps inside 0..k-1: (B, H, W) int32."""
    b, k, h, w = costs.shape
    lab = labels.to(torch.int64).clone()
    ar = torch.arange(k, device=costs.device).view(1, k, 1, 1)
    bt = beta.view(b, 1, 1, 1)
    for _ in range(sweeps):
        for cy in (0, 1):
            for cx in (0, 1):
                hc, wc = (h - cy + 1) // 2, (w - cx + 1) // 2
                pad = torch.nn.functional.pad(lab, (1, 1, 1, 1), value=-2)
                same = torch.zeros((b, k, hc, wc), dtype=torch.int64, device=costs.device)
                n = torch.zeros((b, 1, hc, wc), dtype=torch.int64, device=costs.device)
                for dy, dx in OFFSETS[:neighbours]:
                    y0, x0 = 1 + cy + dy, 1 + cx + dx
                    q = pad[:, y0:y0 + 2 * hc - 1:2, x0:x0 + 2 * wc - 1:2].unsqueeze(1)
                    same += q == ar
                    n += q != -2
                e = costs[:, :, cy::2, cx::2] + bt * (n - same)
                best = e.min(dim=1, keepdim=True).values
                arg = torch.where(e == best, ar, k).min(dim=1).values          # the lowest j attaining the minimum
                own = lab[:, cy::2, cx::2]
                keep = e.gather(1, own.unsqueeze(1)) == best
                lab[:, cy::2, cx::2] = torch.where(keep.squeeze(1), own, arg)
    return lab.to(torch.int32)


def main(out_path, parent):
    sys.path.insert(0, ROOT)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.segmenter import relax_beta
    imgs = _batch(torch)
    res = dict(batch=BATCH, shape=[H, W], bank=COLOUR, reps=REPS, warm=WARM, regularize=LAM,
               images="24 val fixture images, landscape ones transposed, repeated to 64")
    src = torch.empty(1 << 27, dtype=torch.int64, device="cuda").zero_()
    dst = torch.empty_like(src)
    ts = _turns(torch, dict(copy=lambda: dst.copy_(src)))["copy"]
    res["copy_gbps"] = 2 * src.numel() * 8 / (sorted(ts)[len(ts) // 2] * 1e-3) / 1e9
    del src, dst
    gbps = res["copy_gbps"]
    for k in (8, 16):
        tag = f"k{k}"
        seg = Segmenter(k=k, **COLOUR)
        ops = seg.ops
        labels = seg.segment_device(imgs)
        ws = seg._workspace(BATCH, H, W, "per_image")
        feats, cent = ws["feats"], ws["cent"]
        costs = torch.empty((BATCH, k, H, W), dtype=torch.int64, device="cuda")
        # (a)
        for name, t in _turns(torch, dict(costs=lambda: ops.kmeans_costs(feats, cent, BATCH, H, W, k, BATCH, costs))).items():
            res.update(_stats(f"{tag}_{name}", t))
        ref = torch_costs(torch, ops, feats, cent, k)
        res[f"{tag}_costs_torch_equal"] = bool(torch.equal(ref, costs))
        del ref
        res.update(_stats(f"{tag}_costs_torch", [_timed(torch, lambda: torch_costs(torch, ops, feats, cent, k)) for _ in range(3)]))
        res[f"{tag}_costs_bytes"] = int(feats.numel() + costs.numel() * 8)
        res[f"{tag}_costs_floor_ms"] = res[f"{tag}_costs_bytes"] / gbps / 1e6
        res[f"{tag}_costs_over_floor"] = res[f"{tag}_costs_ms"] / res[f"{tag}_costs_floor_ms"]
        res[f"{tag}_costs_torch_over_kernel"] = res[f"{tag}_costs_torch_ms"] / res[f"{tag}_costs_ms"]
        # (b)
        stats = torch.empty((BATCH, k, 2), dtype=torch.int64, device="cuda")
        ops.kmeans_evaluate(feats, cent, BATCH, H, W, k, BATCH, stats=stats)
        beta = relax_beta(stats, Q).contiguous()
        out, work = torch.empty_like(labels), torch.empty_like(labels)
        relax = lambda sweeps, nb: (lambda: ops.label_relax(costs, beta, BATCH, H, W, k, nb, sweeps, labels, out, workspace=work))
        calls = dict(relax=relax(4, 8), relax_sweeps1=relax(1, 8), relax_sweeps2=relax(2, 8), relax_sweeps8=relax(8, 8), relax_n4=relax(4, 4))
        for name, t in _turns(torch, calls).items():
            res.update(_stats(f"{tag}_{name}", t))
        changed = torch.empty((BATCH, 4), dtype=torch.int32, device="cuda")
        ops.label_relax(costs, beta, BATCH, H, W, k, 8, 4, labels, out, workspace=work, changed=changed)
        res[f"{tag}_changed_per_sweep_mean"] = changed.to(torch.float64).mean(dim=0).tolist()
        ref = torch_relax(torch, costs, labels, beta, 4, 8)
        res[f"{tag}_relax_torch_equal"] = bool(torch.equal(ref, out))
        del ref
        res.update(_stats(f"{tag}_relax_torch", [_timed(torch, lambda: torch_relax(torch, costs, labels, beta, 4, 8)) for _ in range(3)]))
        maps = labels.numel() * 4
        res[f"{tag}_relax_bytes"] = int(2 * maps + 4 * (costs.numel() * 8 + 2 * maps))
        res[f"{tag}_relax_floor_ms"] = res[f"{tag}_relax_bytes"] / gbps / 1e6
        res[f"{tag}_relax_over_floor"] = res[f"{tag}_relax_ms"] / res[f"{tag}_relax_floor_ms"]
        res[f"{tag}_relax_torch_over_kernel"] = res[f"{tag}_relax_torch_ms"] / res[f"{tag}_relax_ms"]
        del costs, out, work, feats, cent, ws
        seg._ws.clear()
        torch.cuda.empty_cache()
        # (c), (d)
        for key, kw in (("segment", {}), ("clusters", dict(tree_nodes="clusters", n_regions=8))):
            plans = {key: Segmenter(k=k, **COLOUR, **kw), key + "_regularised": Segmenter(k=k, regularize=LAM, **COLOUR, **kw)}
            for name, t in _turns(torch, {n: (lambda s: lambda: s.segment_device(imgs))(s) for n, s in plans.items()}).items():
                res.update(_stats(f"{tag}_{name}", t))
            res[f"{tag}_{key}_regularised_over_plain"] = res[f"{tag}_{key}_regularised_ms"] / res[f"{tag}_{key}_ms"]
            if kw:
                for name, s in plans.items():
                    counts = s._cluster_maps(imgs, tree=False)[1]["nd"][2].cpu().numpy()
                    res[f"{tag}_nodes" + name[len(key):]] = dict(min=int(counts.min()), mean=float(counts.mean()), max=int(counts.max()))
            for s in plans.values():
                s._ws.clear()
            del plans
            torch.cuda.empty_cache()
        print(json.dumps({n: v for n, v in res.items() if n.startswith(tag)}), flush=True)
    # (e) "off means unchanged"
    both = dict(parent=_with_library(parent, lambda: Segmenter()), step=Segmenter())
    assert not hasattr(both["parent"].ops.lib, "gcs_label_relax")
    model = both["step"].fit_device(imgs[:8], "global")
    got = {}

    def evaluate(s):
        ws = s._workspace(BATCH, H, W, "per_image")
        lab = torch.empty((BATCH, H, W), dtype=torch.int32, device="cuda")
        best, second = (torch.empty((BATCH, H, W), dtype=torch.int64, device="cuda") for _ in range(2))
        stats = torch.empty((BATCH, s.k, 2), dtype=torch.int64, device="cuda")
        return lambda: (s.ops.kmeans_evaluate(ws["feats"], ws["cent"], BATCH, H, W, s.k, BATCH, lab, best, second, stats),
                        (lab, best, second, stats))[1]
    for what, make in (("default", lambda s: lambda: s.segment_device(imgs)), ("predict", lambda s: lambda: s.predict_device(imgs, model)),
                       ("evaluate", evaluate)):
        fns = {n: make(s) for n, s in both.items()}
        times = _turns(torch, {n: (lambda n: lambda: got.__setitem__(n, fns[n]()))(n) for n in ("parent", "step")})
        for n, t in times.items():
            res.update(_stats(f"{n}_{what}", t))
        a, b = got["step"], got["parent"]
        res[f"{what}_equal"] = bool(all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else torch.equal(a, b))
        res[f"{what}_inside_parent_range"] = bool(res[f"parent_{what}_ms_min"] <= res[f"step_{what}_ms"] <= res[f"parent_{what}_ms_max"])
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    args = sys.argv[1:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    if parent is None:
        sys.exit("the parent commit's libgcs.so is needed: --parent path")
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--parent")]
    main(paths[0] if paths else None, parent)
