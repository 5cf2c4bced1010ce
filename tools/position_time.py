#!/usr/bin/env python3
"""Cost of the coordinate slot (gcs_position_features, SPEC.md §12) at batch 64 x 481x321, mu = 6.

The kernel reads nothing but its arguments on full runs of slots and writes the slot's bytes: ``bytes_written`` below is computed
from the slab geometry (two planes per scale, 2 bytes per slot in either slab format). The yardstick is ``torch.Tensor.copy_`` of a
device tensor of exactly that many bytes, timed the same way in the same run: every call bracketed by two events on the stream,
median of ``reps`` calls after ``warm`` warm-up calls - once on an idle queue and once behind queued device work (``queued_*``: the
span is then device time; see tools/colour_time.py). Under `rocprofv3 --kernel-trace --stats -f csv -d <dir> -o run --` (a run of
its own, ``--kernel-only``) the trace has the kernels' own times.
Then the whole segment_device step per plan, ``rounds`` times over the plans (20 steps after 5 warm-up steps each): the default, the
colour plan (5, 1/8, 4), the position plan (4, 1/8, 4, mu = 6; D = 72) and (5, 1/8, 4, mu = 6; D = 84, wide slab).
``--default-only``: the default plan's rounds alone (what an older tree can run too: ``--root DIR`` imports the package from DIR).
Usage: position_time.py [--kernel-only | --default-only] [--root DIR] [out.json]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median_ms(torch, fn, reps, warm, filler=None):
    times = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if filler is not None:
            filler.zero_()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def slot_bytes(batch, h, w, n_scales):
    """Bytes of the coordinate planes in a slab of either format: 2 channels x 2 bytes per slot of every scale's slot plane, over the
    tiles of csrc/common.h (8x8 blocks, four per tile; one- and two-pixel edges packed for banks of at most two levels)."""
    n_levels = (n_scales + 1) // 2
    pack = n_levels <= 2 and h >= 8 and w >= 8
    pack_r, pack_b = pack and (w & 7) in (1, 2), pack and (h & 7) in (1, 2)
    bx, by = (w // 8 if pack_r else (w + 7) // 8), (h // 8 if pack_b else (h + 7) // 8)
    wb = 8 * bx if pack_r else w
    nblk = bx * by + (((h + 1) // 2 + 15) // 16 if pack_r else 0) + (((wb + 1) // 2 + 15) // 16 if pack_b else 0)
    ntiles = (nblk + 3) // 4
    per_tile = sum(2 * min(2, n_scales - 2 * lv) * (256 >> (2 * lv)) * 2 for lv in range(n_levels))
    return batch * ntiles * per_tile


def step_rounds(torch, Segmenter, imgs, plans, rounds, reps, warm):
    batch, h, w, _ = imgs.shape
    out = {name: [] for name, _ in plans}
    for _ in range(rounds):
        for name, kw in plans:
            s = Segmenter(**kw)
            lab = torch.empty((batch, h, w), dtype=torch.int32, device="cuda")
            for _ in range(warm):
                s.segment_device(imgs, out=lab)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                s.segment_device(imgs, out=lab)
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps)
            del s, lab
    return {name + "_step_ms": v for name, v in out.items()}


def main(batch=64, h=321, w=481, reps=20, warm=5, mu=6, rounds=6, mode="all", root=ROOT):
    sys.path.insert(0, root)
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = torch.from_numpy(synthetic_batch(batch, h, w, seed=0)).cuda()
    res = {"batch": batch, "shape": [h, w], "reps": reps, "warm": warm, "rounds": rounds, "root": os.path.relpath(root, ROOT)}
    if mode == "default":
        res.update(step_rounds(torch, Segmenter, imgs, (("default", {}),), rounds, reps, warm))
        print(json.dumps(res), flush=True)
        return res
    rec = dict(n_orient=4, color_weight=0.125, chroma_gain=4, position_weight=mu)
    seg = Segmenter(**rec)
    ops = seg.ops
    n_bytes = slot_bytes(batch, h, w, seg.bank.n_scales)
    feats = ops.feature_slab(batch, h, w)
    ops.gabor_features(imgs, feats)
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res.update(position_weight=mu, bytes_written=n_bytes, slab_bytes=feats.numel())
    k = _median_ms(torch, lambda: ops.position_features(feats, batch, h, w), reps, warm)
    c = _median_ms(torch, lambda: dst.copy_(src), reps, warm)
    filler = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    kf = _median_ms(torch, lambda: ops.position_features(feats, batch, h, w), reps, warm, filler)
    cf = _median_ms(torch, lambda: dst.copy_(src), reps, warm, filler)
    del filler
    res.update(queued_kernel_ms=kf[0], queued_kernel_ms_min=kf[1], queued_kernel_ms_max=kf[2], queued_copy_ms=cf[0],
               queued_copy_ms_min=cf[1], queued_copy_ms_max=cf[2], queued_kernel_over_copy=kf[0] / cf[0],
               queued_kernel_write_TBps=n_bytes / kf[0] / 1e9, queued_copy_write_TBps=n_bytes / cf[0] / 1e9,
               kernel_ms=k[0], kernel_ms_min=k[1], kernel_ms_max=k[2], copy_ms=c[0], copy_ms_min=c[1], copy_ms_max=c[2])
    # the D = 84 plan's launch (wide slab) behind queued work, for the record
    seg84 = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4, position_weight=mu)
    feats84 = seg84.ops.feature_slab(batch, h, w)
    seg84.ops.gabor_features(imgs, feats84)
    filler = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    w84 = _median_ms(torch, lambda: seg84.ops.position_features(feats84, batch, h, w), reps, warm, filler)
    del filler, feats84, seg84
    res.update(queued_kernel_wide_ms=w84[0], queued_kernel_wide_ms_min=w84[1], queued_kernel_wide_ms_max=w84[2])
    print(json.dumps(res), flush=True)
    if mode == "kernel":
        return res
    del feats, src, dst, seg
    plans = (("default", {}), ("colour_no5_w0.125_g4", dict(n_orient=5, color_weight=0.125, chroma_gain=4)),
             ("position_no4_w0.125_g4_mu%d" % mu, rec),
             ("position_no5_w0.125_g4_mu%d_D84" % mu, dict(n_orient=5, color_weight=0.125, chroma_gain=4, position_weight=mu)))
    steps = step_rounds(torch, Segmenter, imgs, plans, rounds, reps, warm)
    res.update(steps)
    print(json.dumps(steps), flush=True)
    return res


if __name__ == "__main__":
    argv = sys.argv[1:]
    root = ROOT
    if "--root" in argv:
        i = argv.index("--root")
        root = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    mode = "kernel" if "--kernel-only" in argv else "default" if "--default-only" in argv else "all"
    args = [a for a in argv if not a.startswith("--")]
    r = main(mode=mode, root=root)
    if args:
        with open(args[0], "w") as f:
            json.dump(r, f, indent=1)
