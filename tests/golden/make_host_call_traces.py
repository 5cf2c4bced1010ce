"""Records tests/golden/host_call_traces.json: what every host path of the Segmenter asks of its ops, call by call.

The fixture pins the launch sequence of the commit BEFORE the per-batch step was folded into two functions
(tests/test_gpu_host_call_trace.py compares the code under test with it, entry by entry, with ``==``). It was recorded once, on
the GPU, from a worktree of that parent commit:

    python tests/golden/make_host_call_traces.py tests/golden/host_call_traces.json

It is NEVER regenerated from the code under test: a path that gains, loses or reorders a launch, or passes another scalar,
must fail the test, not rewrite the fixture. A later change that alters a launch sequence ON PURPOSE edits the entries it
means to change by hand, or records from the commit that made the change after review of the diff of the two files.

What is logged, per call made through ``seg.ops`` on the calling thread: the method's name and its arguments bound to the
method's parameter names (so that passing an argument by position or by keyword, or leaving a default out, reads the same) -
ints, bools, strings and None as they are, tensors as dtype and shape only, tuples as lists. A path that refuses its arguments
is recorded by the exception's type and message. The captured replay of a small ``segment_batch`` runs on a helper thread and
is not logged: the eager warm-up call made when the graph entry is built is.
"""
import inspect
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PLANS = {
    "default": dict(n_iter=3),
    "all_on": dict(n_iter=3, n_orient=4, smoothing=1.0, chroma_gain=4, color_weight=0.125, position_weight=6),
    "regions": dict(n_iter=3, n_superpixels=300, n_regions=8),                   # K = 14 * 21 = 294 > 256: uint8 only through R
    "regions_min_size": dict(n_iter=3, n_superpixels=300, n_regions=8, min_region_size=12),
}
# Lloyd plans: both sides odd, so both packed edge strips occur; superpixel plans: the shape of the uint8 rule above
SHAPES = {"default": (5, 41, 57), "all_on": (5, 41, 57), "regions": (2, 72, 104), "regions_min_size": (2, 72, 104)}


def _code(v):
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, (np.integer, np.bool_)):
        return v.item()
    if hasattr(v, "data_ptr") and hasattr(v, "dtype"):
        return {"dtype": str(v.dtype), "shape": list(v.shape)}
    if isinstance(v, (tuple, list)):
        return [_code(x) for x in v]
    return {"type": type(v).__name__}


class Recorder:
    """Stands where ``seg.ops`` stood and forwards everything; calls made on the thread that built it are logged."""

    def __init__(self, ops):
        self._ops, self.log, self._thread = ops, [], threading.get_ident()

    def __getattr__(self, name):
        attr = getattr(self._ops, name)
        if not inspect.ismethod(attr):
            return attr

        def call(*a, **kw):
            if threading.get_ident() == self._thread:
                bound = inspect.signature(attr).bind(*a, **kw)
                bound.apply_defaults()
                self.log.append([name, {k: _code(v) for k, v in bound.arguments.items()}])
            return attr(*a, **kw)
        return call


def _images(b, h, w, seed=5):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    return synthetic_batch(b, h, w, seed=seed)


def _dev(seg, imgs):
    import torch
    return torch.from_numpy(imgs).to(seg.ops._ops.device)


def _no_graph(seg, imgs):
    from gabor_color_image_segmentation_amd.segmenter import DebugSwitches
    seg.debug = DebugSwitches("no_graph")
    seg.segment_batch(imgs)


def _stream(seg, imgs):
    n = sum(1 for _ in seg.segment_stream([imgs, imgs[::-1].copy(), imgs, imgs[::-1].copy()], depth=2))
    assert n == 4


def _bsd_images(seg, imgs):
    big = _images(8, 481, 321)            # 8 x 481 x 321 > 2^20 pixels: the smallest batch that is pipelined
    assert sum(1 for _ in seg.segment_images(list(big), batch=8)) == 8


PATHS = {
    "segment_device": lambda seg, imgs: seg.segment_device(_dev(seg, imgs)),
    "segment_device_global": lambda seg, imgs: seg.segment_device(_dev(seg, imgs), mode="global"),
    "segment_device_groups": lambda seg, imgs: seg.segment_device(_dev(seg, imgs), group=2 if len(imgs) > 2 else 1),
    "segment_batch_graph": lambda seg, imgs: seg.segment_batch(imgs),
    "segment_batch_graph_u8": lambda seg, imgs: seg.segment_batch(imgs, out_dtype=np.uint8),
    "segment_batch_chunked": _no_graph,
    "segment_stream": _stream,
    "segment_images": _bsd_images,
    "region_tree_device": lambda seg, imgs: seg.region_tree_device(_dev(seg, imgs)),
    "superpixels_device": lambda seg, imgs: seg.superpixels_device(_dev(seg, imgs)),
    "contours_device": lambda seg, imgs: seg.contours_device(_dev(seg, imgs)),
    "features_device": lambda seg, imgs: seg.features_device(_dev(seg, imgs)),
}


def record(plan, path):
    """The ops calls of ``path`` on a fresh Segmenter of ``plan``: a list of [name, arguments], or {"raises": ...}."""
    import torch
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(**PLANS[plan])
    seg.ops = rec = Recorder(seg.ops)
    try:
        PATHS[path](seg, _images(*SHAPES[plan]))
    except ValueError as e:
        assert not rec.log, "a path that refuses its arguments must do so before its first launch"
        return {"raises": f"{type(e).__name__}: {e}"}
    torch.cuda.current_stream(rec._ops.device).synchronize()
    return rec.log


if __name__ == "__main__":
    traces = {plan: {path: record(plan, path) for path in PATHS} for plan in PLANS}
    with open(sys.argv[1], "w") as f:            # one call per line: a changed launch reads as a one-line diff
        plans = []
        for plan, paths in traces.items():
            cases = [f' "{path}": ' + (json.dumps(log) if isinstance(log, dict) else
                                      "[\n" + ",\n".join("  " + json.dumps(c) for c in log) + "\n ]") for path, log in paths.items()]
            plans.append(f'"{plan}": {{\n' + ",\n".join(cases) + "\n}")
        f.write("{\n" + ",\n".join(plans) + "\n}\n")
    for plan, paths in traces.items():
        for path, log in paths.items():
            print(plan, path, log["raises"] if isinstance(log, dict) else f"{len(log)} calls")
