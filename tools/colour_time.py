#!/usr/bin/env python3
"""Cost of the opponent-colour transform (gcs_colour_opponent, SPEC.md §11) at batch 64 x 481x321.

The kernel moves exactly the bytes of a device-to-device copy of the batch (3 B read + 3 B written per pixel), so the yardstick is
``torch.Tensor.copy_`` of the same tensor, timed the same way in the same run: every call bracketed by two events on the stream,
median of ``reps`` calls after ``warm`` warm-up calls - once on an idle queue and once behind queued device work (``queued_*``: see
``_median_ms``; under `rocprofv3 --kernel-trace --stats -f csv -d <dir> -o run --` the trace has the kernels' own times). The kernel is also timed at a source 7 and a destination 5 bytes off
16-byte alignment (inside larger buffers). Then the whole segment_device step per plan: the default, n_orient=5 with the low-pass
slot, the same with chroma_gain=4, and n_orient=6 with the slot (D = 84, wide slab).
Usage: colour_time.py [--kernel-only] [out.json]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(torch, fn, reps, warm, filler=None):
    """``filler``: a tensor zeroed on the stream in front of every timed call. A 20 us kernel is shorter than the host's way to
    its launch: on an idle queue the first event is stamped at once and the span between the events is mostly the host getting to
    the launch; behind ~100 us of queued device work both events and the call are enqueued before the device reaches them, and the
    span is device time."""
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


def main(batch=64, h=321, w=481, reps=20, warm=5, gain=4, steps=True):
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    imgs = torch.from_numpy(synthetic_batch(batch, h, w, seed=0)).cuda()
    n_bytes = imgs.numel()
    seg = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=gain)
    ops = seg.ops
    out = ops.colour_scratch(batch, h, w)
    res = {"batch": batch, "shape": [h, w], "gain": gain, "bytes_read": n_bytes, "bytes_written": n_bytes, "reps": reps}
    k = _median_ms(torch, lambda: ops.colour_opponent(imgs, out), reps, warm)
    c = _median_ms(torch, lambda: out.copy_(imgs), reps, warm)
    big_in = torch.empty(n_bytes + 32, dtype=torch.uint8, device="cuda")
    big_out = torch.empty(n_bytes + 32, dtype=torch.uint8, device="cuda")
    big_in[7:7 + n_bytes].copy_(imgs.view(-1))
    u = _median_ms(torch, lambda: ops.colour_opponent(big_in[7:7 + n_bytes], big_out[5:5 + n_bytes]), reps, warm)
    filler = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    kf = _median_ms(torch, lambda: ops.colour_opponent(imgs, out), reps, warm, filler)
    cf = _median_ms(torch, lambda: out.copy_(imgs), reps, warm, filler)
    uf = _median_ms(torch, lambda: ops.colour_opponent(big_in[7:7 + n_bytes], big_out[5:5 + n_bytes]), reps, warm, filler)
    res.update(queued_kernel_ms=kf[0], queued_kernel_ms_min=kf[1], queued_kernel_ms_max=kf[2], queued_copy_ms=cf[0],
               queued_copy_ms_min=cf[1], queued_copy_ms_max=cf[2], queued_kernel_over_copy=kf[0] / cf[0],
               queued_kernel_TBps=2 * n_bytes / kf[0] / 1e9, queued_copy_TBps=2 * n_bytes / cf[0] / 1e9,
               queued_kernel_unaligned_ms=uf[0], queued_kernel_unaligned_over_copy=uf[0] / cf[0])
    del filler
    res.update(kernel_ms=k[0], kernel_ms_min=k[1], kernel_ms_max=k[2], copy_ms=c[0], copy_ms_min=c[1], copy_ms_max=c[2],
               kernel_over_copy=k[0] / c[0], kernel_TBps=2 * n_bytes / k[0] / 1e9, copy_TBps=2 * n_bytes / c[0] / 1e9,
               kernel_unaligned_ms=u[0], kernel_unaligned_over_copy=u[0] / c[0])
    print(json.dumps(res), flush=True)
    if not steps:
        return res
    steps = {}
    plans = (("default", {}), ("no5_w0.125", dict(n_orient=5, color_weight=0.125)),
             ("no5_w0.125_g4", dict(n_orient=5, color_weight=0.125, chroma_gain=gain)),
             ("no6_w0.125_D84", dict(n_orient=6, color_weight=0.125)))
    for rnd in range(2):                                   # two rounds over the plans: the second one is reported
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
            steps[name + "_step_ms"] = e0.elapsed_time(e1) / reps
            del s, lab
    res.update(steps)
    print(json.dumps(steps), flush=True)
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--kernel-only"]
    r = main(steps="--kernel-only" not in sys.argv)
    if args:
        with open(args[0], "w") as f:
            json.dump(r, f, indent=1)
