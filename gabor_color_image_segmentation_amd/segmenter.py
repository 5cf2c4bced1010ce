"""Host side of the segmenter slot: ``labels = segment(img)``.

Mirrors the only interface the reference has for this path — the positional call at
/root/reference/BSD_metrics/script.py:30 (``labels = slic(img, ...)``): ``img`` is the
(H,W,3) uint8 array from script.py:25, the result is a fresh (H,W) integer array for
metrics.__init__ (/root/reference/BSD_metrics/metrics.py:43-51). Errors are plain Python
exceptions (script.py:19-38 catches nothing).

PyTorch is plumbing only: device memory, the current HIP stream and torch.distributed
(RCCL). All arithmetic runs in libgcs.so (one csrc/*.hip file per stage, csrc/abi.hip for the
entry points) through the C ABI (include/gcs.h). There is no CPU fallback.

Every host path runs the same per-batch step, ``_step_features`` then ``_step_cluster``, around its own buffers,
streams and events (DESIGN.md §1 lists which path wraps them with what).
"""
from __future__ import annotations

import collections
import contextlib
import math
import os

import numpy as np

from . import _lib
from .bank import GaborBank, check_color_weight, check_position_range, check_position_weight, make_bank, smoothing_taps
from .kmeans_model import KMeansModel, confidence_of

# Feature-slab bytes per group of a per-image batch. Large on purpose: measured in round 4 with the current kernels
# (tools/cache_resident_pass.py, profiles/r4_notes.md "Infinity-Cache-resident groups"): a pass that re-reads a slab small enough
# to stay in the 256 MiB Infinity Cache (8 images, 112 MB) streams it at 3.8 TB/s, 16 images (224 MB) at 4.9 TB/s, the
# 64-image slab (895 MB, from HBM) at 5.9 TB/s - a pass costs ~12 us of launch, prologue and fold however few bytes it reads,
# and what remains is the same 6.4-6.6 TB/s per byte in all three cases (the staging structure, not HBM, sets the rate). 64
# images in cache-sized groups of 16 take 2.45 ms against 2.04 ms in one group.
_SLAB_BUDGET = 16 << 30
# host calls up to this many pixels replay a captured HIP graph of the whole step
_GRAPH_MAX_PIXELS = 1 << 20


class DebugSwitches:
    """The ONE set of measurement / test switches of the host side; none of them changes a result.

    Set from the environment, ``GCS_DEBUG=no_reverse,no_graph,force_collectives,slab_candidates=2`` (any subset), or per
    plan through ``Segmenter.debug``:

    * ``no_reverse``: every Lloyd pass sweeps the slab in the same direction (tools/pass_direction_probe.py);
    * ``no_graph``: small host calls launch eagerly instead of replaying their captured HIP graph;
    * ``force_collectives``: ``lloyd`` takes the multi-rank branch (reduce, all-reduce, finalize) even in a one-rank
      group, so that one GPU can exercise the RCCL path end to end (tests/test_distributed.py, tools/rccl_overhead.py);
    * ``slab_candidates=N``: overrides ``Segmenter(slab_candidates=...)`` (see ``Segmenter._place_slab``)."""

    def __init__(self, spec=""):
        self.no_reverse = self.no_graph = self.force_collectives = False
        self.slab_candidates = None
        for item in filter(None, (x.strip() for x in spec.split(","))):
            name, _, val = item.partition("=")
            if name == "slab_candidates" and val.isdigit():
                self.slab_candidates = int(val)
            elif name in ("no_reverse", "no_graph", "force_collectives") and not val:
                setattr(self, name, True)
            else:
                raise ValueError(f"GCS_DEBUG: unknown switch {item!r}")


_ENV_DEBUG = DebugSwitches(os.environ.get("GCS_DEBUG", ""))


class _CaptureGuard:
    """Process-wide order for HIP graph captures of this module.

    A torch ``CUDAGraph`` destroyed while a stream capture is open throws out of its destructor and ``std::terminate`` ends the
    process (profiles/r4_notes.md). Three rules keep that from happening through this module, whatever threads use it:

    * captures are SERIALISED: one lock is held from the garbage collection in front of a capture to its end, so the cyclic
      collector - a process-global switch - is turned off by the one capturer there is and turned back on (if it was on) when
      that capture has ended, never inside another thread's open capture;
    * graph entries are never dropped where a capture might be open: evicted entries and the entries of a Segmenter that is
      being finalised go through ``retire``, which frees them at once when no capture is open and parks them otherwise
      (drained at the end of the capture, under the lock);
    * a capture that fails is not silent: ``fell_back`` warns once per plan key;
    * a graph whose capture failed is never destroyed: torch 2.10's ``~CUDAGraph`` throws for it too ("The graph should be
      registered to the state", tools/dbg/capture_probe.py) - the few hundred bytes stay in ``_failed`` for the life of the process.

    What a thread that is NOT capturing may do beside an open capture was measured on the box (tools/dbg/capture_probe.py,
    profiles/r5_notes.md): kernel launches, stream / event synchronisation, hipMalloc, pinned allocation and copies are all
    fine; ``hipDeviceSynchronize`` is refused with hipErrorStreamCaptureUnsupported AND invalidates the other thread's
    capture - so no path of this package calls ``torch.cuda.synchronize``: every wait is on a stream or an event. A CALLER's
    thread still can: ``capture`` therefore runs on a helper thread (see there), which confines the damage of an invalidated
    capture to a thread and a stream nobody uses again."""

    def __init__(self):
        import threading
        self._lock = threading.Lock()      # not re-entrant: a plan finalised BY the capturing thread must park its graphs too
        self._parked = []            # retired graph entries waiting for the open capture to end
        self._failed = []            # graphs whose capture was refused or invalidated: kept alive on purpose (see above)
        self._warned = set()

    def capture(self, torch, graph, body, device=None):
        """Capture ``body()`` into ``graph`` (thread_local error mode). Returns True, or False when the capture was refused or
        invalidated (the caller then launches eagerly).

        The capture runs on a HELPER THREAD, and on a stream of its own. Measured on the box (tools/dbg/invalidated_capture_probe.py,
        capture_helper_thread_probe.py, profiles/r6_notes.md): a device-wide synchronize from ANY other thread - a caller's loader, a
        logger - is refused by HIP while a capture is open in whatever mode AND invalidates that capture, and an invalidated capture
        leaves the thread that opened it unable to launch another kernel (hipErrorStreamCaptureInvalidated from every later launch;
        hipStreamEndCapture does not clear it) and its capture stream in the invalidated state for good. Bound to the helper, that
        damage dies with it: the caller's thread and streams stay usable, the shape runs as eager launches, and the next capture
        gets a fresh helper and a fresh stream."""
        import gc
        import threading
        with self._lock:
            gc.collect()             # dead cycles that hold graphs: finalise them NOW, not between capture_begin and capture_end
            was_enabled = gc.isenabled()
            gc.disable()
            result = {}
            stream = torch.cuda.Stream(device=device)

            def run():
                try:
                    if device is not None:
                        torch.cuda.set_device(device)
                    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
                        body()
                    result["ok"] = True
                except RuntimeError as e:          # (GcsError and torch.AcceleratorError are RuntimeErrors)
                    result["err"] = e
                except BaseException as e:         # anything else is the caller's to see
                    result["raise"] = e

            try:
                helper = threading.Thread(target=run, name="gcs-graph-capture")
                helper.start()
                helper.join()
                if "raise" in result:
                    self._failed.append((graph, stream))
                    raise result["raise"]
                if result.get("ok"):
                    return True
                self._failed.append((graph, stream))      # never destroyed, never reused (see the class docstring)
                return False
            finally:
                if was_enabled:
                    gc.enable()
                self._drain()

    def retire(self, entries):
        """Drop graph entries (dicts holding a CUDAGraph and its buffers): now if no capture is open, else after it. ``entries``
        is a LIST the caller gives up: it is emptied here, so that the last references die inside the locked region (or move to
        the parking list) and not later, when the caller's frame unwinds and another thread may have opened a capture."""
        if self._lock.acquire(blocking=False):
            try:
                self._drain()
                entries.clear()      # (the last references: the graphs are destroyed here, under the lock, outside any capture)
            finally:
                self._lock.release()
        else:
            self._parked.extend(e for e in entries if e is not None)      # drained by the capturer, under the lock
            entries.clear()

    def _drain(self):
        while self._parked:
            self._parked.pop()

    def fell_back(self, key, err):
        if key not in self._warned:
            self._warned.add(key)
            import warnings
            warnings.warn(f"gabor_color_image_segmentation_amd: HIP graph capture refused for plan {key} ({err}); this shape runs "
                          "as eager kernel launches for the life of the plan (slower one-image calls, same results)",
                          RuntimeWarning, stacklevel=3)


_CAPTURES = _CaptureGuard()


def _torch():
    import torch
    return torch


def _on_device(fn):
    """Run a HipOps entry point with the plan's device current (a Segmenter on cuda:1 used while cuda:0 is current
    would otherwise launch on the wrong device) after checking where its tensor arguments live."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kw):
        self._check_dev(*[a for a in list(args) + list(kw.values()) if hasattr(a, "data_ptr") and hasattr(a, "device")])
        with self.torch.cuda.device(self.device):
            return fn(self, *args, **kw)
    return wrapper


EDGES_MAX = 16384             # SPEC.md §20: the largest capacity of an edge table (§23 builds its leaf table at it)
NODES_MAX = 4096              # SPEC.md §18: K_cap, the most nodes an image's tree can have (= §14's largest K)


class HipOps:
    """Thin pointer-passer over the C ABI for one device. Stateless apart from the bank."""

    def __init__(self, bank: GaborBank, device, smoothing=0.0, chroma_gain=0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.GcsError("no HIP device visible: the segmenter has no CPU fallback")
        self.lib = _lib.load()
        self.torch = torch
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.bank = bank
        ns, no = bank.n_scales, bank.n_orient
        self._bk = (ns, no)                      # the bank as the C ABI describes it
        packed = np.zeros(self.lib.gcs_bank_packed_bytes(ns, no), np.int8)
        bias = np.zeros(self.lib.gcs_bank_bias_count(ns, no), np.int32)
        tapq = np.ascontiguousarray(bank.tapq, np.int16)
        _lib.check(self.lib.gcs_bank_pack(tapq.ctypes.data, ns, no, bank.ksize, packed.ctypes.data,
                                          bias.ctypes.data), "gcs_bank_pack")
        self.packed = torch.from_numpy(packed).to(self.device)
        self.bias = torch.from_numpy(bias).to(self.device)
        self._gabor_ws = None
        self._texton_masks = {}                  # SPEC.md §24: the half-disc tables on the device, per (r, n)
        self._thin_steps = {}                    # SPEC.md §26: the step tables on the device, per n
        self.chroma_gain = _check_chroma_gain(chroma_gain)        # SPEC.md §11 (0: colour_opponent is never called)
        # SPEC.md §10: the smoothing taps of every scale on the device (K = 0: none, and smooth_features is never called)
        self.smoothing = _check_smoothing(smoothing, bank)
        self._smooth_ws = self.smooth_taps = self.smooth_radius = None
        if self.smoothing > 0:
            taps, radius = smoothing_taps(self.smoothing, ns, no, bank.f_max, bank.ratio)
            self.smooth_taps = torch.from_numpy(taps).to(self.device)
            self.smooth_radius = torch.from_numpy(radius).to(self.device)
        # the self-updating Lloyd passes: only with a library that exports them (tools/ab.py loads older builds in one process)
        self.has_fused = all(n in _lib.SIGNATURES and hasattr(self.lib, n)
                             for n in ("gcs_kmeans_fused_workspace_bytes", "gcs_kmeans_pass_fused"))

    # ---- allocation helpers (bytes buffers; layouts are opaque, see gcs.h)
    def empty_bytes(self, n):
        return self.torch.empty(int(n), dtype=self.torch.uint8, device=self.device)

    def feature_slab(self, b, h, w):
        return self.empty_bytes(self.lib.gcs_feature_slab_bytes(b, h, w, *self._bk))

    def label_slab(self, b, h, w):
        return self.empty_bytes(self.lib.gcs_label_slab_bytes(b, h, w))

    def partial_slab(self, b, h, w, k):
        return self.empty_bytes(self.lib.gcs_kmeans_partial_bytes(b, h, w, self.bank.n_features, k))

    def fused_workspace(self, b, h, w, k, n_sets):
        """The workspace of the self-updating Lloyd passes (``lloyd(fold=...)``), zeroed as gcs.h asks, or None when the library
        or this bank / k has no such pass."""
        n = self.lib.gcs_kmeans_fused_workspace_bytes(b, h, w, *self._bk, k, n_sets) if self.has_fused else 0
        return self.torch.zeros(int(n), dtype=self.torch.uint8, device=self.device) if n else None

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _check_dev(self, *tensors):
        """Launches go through ctypes on the calling thread's CURRENT device: every tensor must live on this plan's
        device, and the calls below run inside ``torch.cuda.device(self.device)`` (see ``_on_device``)."""
        for t in tensors:
            if t.device != self.device:
                raise ValueError(f"tensor on {t.device}, this Segmenter's kernels run on {self.device}")

    @staticmethod
    def _need(t, dtypes, shape, what):
        """The ONE tensor-argument check: ``t`` (None passes: an optional output) is a contiguous tensor of ``shape`` and of one
        of ``dtypes`` (a dtype or a tuple of them), or ValueError(``what``)."""
        if t is not None and (t.dtype not in (dtypes if isinstance(dtypes, tuple) else (dtypes,)) or tuple(t.shape) != shape
                              or not t.is_contiguous()):
            raise ValueError(what)

    def _need_tree(self, b, h, w, K, merges, alive, **maps):
        """What the entry points of SPEC.md §14 and §15 share: (B,H,W) int32 maps by name, the merge list and ``alive``."""
        for name, t in maps.items():
            self._need(t, self.torch.int32, (b, h, w), f"{name} must be a contiguous (B,H,W) int32 tensor")
        self._need(merges, self.torch.int32, (b, K - 1, 2), "merges must be a contiguous (B, K - 1, 2) int32 tensor")
        self._need(alive, self.torch.int32, (b,), "alive must be a contiguous (B,) int32 tensor")

    def _scratch(self, shared, scratch, need, what):
        """The caller's ``scratch`` when it gave one (checked), else the shared, growing workspace this HipOps keeps in the
        attribute ``shared`` (see ``gabor_features`` for who may use which)."""
        if scratch is None:
            if getattr(self, shared) is None or getattr(self, shared).numel() < need:
                setattr(self, shared, self.empty_bytes(need))
            return getattr(self, shared)
        if scratch.numel() < need or scratch.device != self.device:
            raise ValueError(f"{what} scratch too small or on another device")
        return scratch

    # ---- device entry points
    def gabor_scratch(self, b, h, w):
        """A private Gabor workspace for one (batch, shape): what a captured graph must own (see ``gabor_features``)."""
        return self.empty_bytes(self.lib.gcs_gabor_workspace_bytes(b, h, w, self.bank.n_scales))

    @_on_device
    def gabor_features(self, imgs, feats, scratch=None):
        """``scratch``: a workspace the CALLER owns (``gabor_scratch``). Without it the call uses the shared, growing
        workspace of this HipOps - fine for eager launches (torch's allocator hands a replaced block to later work of the
        same stream only), NOT for a captured graph: a replay would keep writing through the raw pointer of a block that
        a later, larger call has meanwhile given back to the allocator."""
        b, h, w, _ = imgs.shape
        scratch = self._scratch("_gabor_ws", scratch, self.lib.gcs_gabor_workspace_bytes(b, h, w, self.bank.n_scales), "gabor")
        _lib.check(self.lib.gcs_gabor_features(imgs.data_ptr(), b, h, w, self.packed.data_ptr(),
                                               self.bias.data_ptr(), *self._bk,
                                               self.bank.ksize, self.bank.shift, scratch.data_ptr(),
                                               feats.data_ptr(), self._stream()),
                   "gcs_gabor_features")

    def colour_scratch(self, b, h, w):
        """The (B,H,W,3) uint8 buffer ``colour_opponent`` writes the transformed batch to (a captured graph must own it)."""
        return self.torch.empty((b, h, w, 3), dtype=self.torch.uint8, device=self.device)

    @_on_device
    def colour_opponent(self, imgs, out):
        """SPEC.md §11: ``out`` = T_g of ``imgs`` with this plan's ``chroma_gain``; both contiguous uint8 tensors of the same
        number of whole pixels (any byte alignment: slices of a batch qualify), not the same memory."""
        if self.chroma_gain == 0:
            raise ValueError("colour_opponent needs HipOps(chroma_gain=g) with g > 0")
        torch = self.torch
        if imgs.dtype != torch.uint8 or out.dtype != torch.uint8 or imgs.numel() != out.numel() or imgs.numel() % 3 \
                or not imgs.is_contiguous() or not out.is_contiguous():
            raise ValueError("colour_opponent needs two contiguous uint8 tensors of the same number of RGB pixels")
        _lib.check(self.lib.gcs_colour_opponent(imgs.data_ptr(), imgs.numel() // 3, self.chroma_gain, out.data_ptr(),
                                                self._stream()), "gcs_colour_opponent")

    def smooth_scratch(self, b, h, w):
        """A private smoothing workspace for one (batch, shape): the level planes (see ``smooth_features``)."""
        return self.empty_bytes(self.lib.gcs_smooth_workspace_bytes(b, h, w, *self._bk))

    @_on_device
    def smooth_features(self, feats, b, h, w, scratch=None):
        """SPEC.md §10 in place on a slab that ``gabor_features`` has filled, with this plan's ``smoothing``. ``scratch``: as in
        ``gabor_features`` (a captured graph must own its workspace; eager calls may share the growing one of this HipOps)."""
        if self.smooth_taps is None:
            raise ValueError("smooth_features needs HipOps(smoothing=K) with K > 0")
        scratch = self._scratch("_smooth_ws", scratch, self.lib.gcs_smooth_workspace_bytes(b, h, w, *self._bk), "smoothing")
        _lib.check(self.lib.gcs_smooth_features(feats.data_ptr(), b, h, w, *self._bk, self.smooth_taps.data_ptr(),
                                                self.smooth_radius.data_ptr(), scratch.data_ptr(), self._stream()),
                   "gcs_smooth_features")

    @_on_device
    def position_features(self, feats, b, h, w, y0=0):
        """SPEC.md §12 in place on a slab that ``gabor_features`` (and ``smooth_features``, when smoothing is on) has filled: the
        coordinate slot of every scale, with this plan's bank's ``position_weight``. ``y0``: the global row of the slab's row 0
        (row strips of a taller image). One launch, no workspace (capturable as it is)."""
        mu = getattr(self.bank, "position_weight", 0)
        if mu == 0:
            raise ValueError("position_features needs a bank made with position_weight = mu > 0")
        _lib.check(self.lib.gcs_position_features(feats.data_ptr(), b, h, w, *self._bk, mu, int(y0), self._stream()),
                   "gcs_position_features")

    @_on_device
    def features_unpack(self, feats, b, h, w, out=None):
        d = self.bank.n_features
        if out is None:
            out = self.torch.empty((b, d, h, w), dtype=self.torch.int16, device=self.device)
        self._need(out, self.torch.int16, (b, d, h, w), "out must be a contiguous (B,D,H,W) int16 tensor")
        _lib.check(self.lib.gcs_features_unpack(feats.data_ptr(), b, h, w, *self._bk, out.data_ptr(),
                                                self._stream()), "gcs_features_unpack")
        return out

    @_on_device
    def kmeans_init(self, feats, b, h, w, k, n_sets, cent):
        _lib.check(self.lib.gcs_kmeans_init(feats.data_ptr(), b, h, w, *self._bk, k, n_sets,
                                            cent.data_ptr(), self._stream()), "gcs_kmeans_init")

    def _pass_fused(self, feats, cent, b, h, w, k, n_sets, fused, reverse, out=None):
        fold, t = fused
        self._check_dev(fold)
        _lib.check(self.lib.gcs_kmeans_pass_fused(
            feats.data_ptr(), b, h, w, *self._bk, k, n_sets, 1 if reverse else 0, t, 0 if out is None else 1,
            fold.data_ptr(), cent.data_ptr(), None if out is None else out.data_ptr(),
            1 if out is not None and out.dtype == self.torch.uint8 else 0, self._stream()), "gcs_kmeans_pass_fused")

    @_on_device
    def assign_accumulate(self, feats, cent, b, h, w, k, n_sets, labels, partials, rows=None, reverse=False, fused=None):
        """One Lloyd pass. ``labels=None``: the assignment is not stored (every pass but the last); ``partials=None``:
        no sums are accumulated (the last pass). ``fused=(workspace, t)``: pass ``t`` of a self-updating loop (not the last:
        ``assign_raster``) - the sums stay in the workspace, ``cent`` receives the centroids the pass made for itself."""
        if fused is not None:
            if labels is not None or partials is not None or rows is not None:
                raise ValueError("a self-updating pass takes whole images and has no label or partial output")
            return self._pass_fused(feats, cent, b, h, w, k, n_sets, fused, reverse)
        lo, hi = rows if rows is not None else (0, h)
        _lib.check(self.lib.gcs_kmeans_assign_accumulate(
            feats.data_ptr(), cent.data_ptr(), b, h, w, *self._bk, k, n_sets, lo, hi,
            1 if reverse else 0, None if labels is None else labels.data_ptr(),
            None if partials is None else partials.data_ptr(), self._stream()),
            "gcs_kmeans_assign_accumulate")

    @_on_device
    def assign_raster(self, feats, cent, b, h, w, k, n_sets, out, scratch_labels=None, reverse=False, fused=None):
        """The last Lloyd pass with the label map written in raster order: ``out`` (B,H,W) int32 or uint8 device tensor.
        ``fused=(workspace, t)``: as the last pass of a self-updating loop (see ``assign_accumulate``)."""
        torch = self.torch
        self._need(out, (torch.int32, torch.uint8), (b, h, w), "out must be a contiguous (B,H,W) int32 or uint8 tensor")
        if fused is not None:
            return self._pass_fused(feats, cent, b, h, w, k, n_sets, fused, reverse, out=out)
        _lib.check(self.lib.gcs_kmeans_assign_raster(
            feats.data_ptr(), cent.data_ptr(), b, h, w, *self._bk, k, n_sets, 1 if reverse else 0, out.data_ptr(),
            1 if out.dtype == torch.uint8 else 0, None if scratch_labels is None else scratch_labels.data_ptr(),
            self._stream()), "gcs_kmeans_assign_raster")

    def superpixel_buffers(self, b, h, w, n):
        """What the stage of SPEC.md §13 needs beside the slab for one (batch, shape): the canonical (B,D,H,W) tensor the kernels
        read and the workspace of ``gcs_superpixel_segment`` (a captured graph must own both)."""
        need = self.lib.gcs_superpixel_workspace_bytes(b, h, w, self.bank.n_features, int(n))
        if need == 0:
            raise ValueError("no superpixel grid for this shape / bank (H, W <= 4096, D <= 207, 2 <= n <= 4096, ny * nx <= 4096)")
        return (self.torch.empty((b, self.bank.n_features, h, w), dtype=self.torch.int16, device=self.device),
                self.empty_bytes(need))

    @_on_device
    def superpixels(self, canon, b, h, w, ny, nx, spatial_weight, n_iter, out, workspace, centres=None):
        """SPEC.md §13 on canonical features (``features_unpack``): ``out`` (B,H,W) int32 labels in 0 .. ny * nx - 1 of the last of
        ``n_iter`` assigns; ``centres``: None or a (B, ny * nx, D + 2) int32 tensor that receives the centres that assign used
        (D features, cy, cx). ``workspace``: from ``superpixel_buffers``. One call, 2 n_iter launches, capturable."""
        torch, d = self.torch, self.bank.n_features
        self._need(canon, torch.int16, (b, d, h, w), "canon must be the contiguous (B,D,H,W) int16 tensor of features_unpack")
        self._need(out, torch.int32, (b, h, w), "out must be a contiguous (B,H,W) int32 tensor")
        self._need(centres, torch.int32, (b, ny * nx, d + 2), "centres must be a contiguous (B, ny * nx, D + 2) int32 tensor")
        _lib.check(self.lib.gcs_superpixel_segment(canon.data_ptr(), b, h, w, d, int(ny), int(nx), int(spatial_weight), int(n_iter),
                                                   workspace.data_ptr(), out.data_ptr(),
                                                   None if centres is None else centres.data_ptr(), self._stream()),
                   "gcs_superpixel_segment")

    def region_tree_buffers(self, b, h, w, K):
        """What SPEC.md §14 needs for one (batch, shape, K): ``(workspace, merges (B, K-1, 2) int32, costs (B, K-1) int64, alive (B,)
        int32)`` (a captured graph must own them). The costs are unsigned 64-bit values below 2^62: an int64 tensor holds the bits."""
        torch, K = self.torch, int(K)
        need = self.lib.gcs_region_tree_workspace_bytes(b, h, w, self.bank.n_features, K)
        if need == 0:
            raise ValueError("no region tree for this shape / bank (H, W <= 4096, D <= 207, 1 <= K <= 4096)")
        return (self.empty_bytes(need), torch.empty((b, K - 1, 2), dtype=torch.int32, device=self.device),
                torch.empty((b, K - 1), dtype=torch.int64, device=self.device), torch.empty((b,), dtype=torch.int32, device=self.device))

    @_on_device
    def region_tree(self, canon, labels, b, h, w, K, workspace, merges, costs, alive):
        """SPEC.md §14 on canonical features and an int32 (B,H,W) label map in 0 .. K-1: fills ``merges`` (B, K-1, 2) int32, ``costs``
        (None or (B, K-1) int64) and ``alive`` (B,) int32. ``workspace``: from ``region_tree_buffers``. Three launches, capturable."""
        torch, d, K = self.torch, self.bank.n_features, int(K)
        self._need(canon, torch.int16, (b, d, h, w), "canon must be the contiguous (B,D,H,W) int16 tensor of features_unpack")
        self._need_tree(b, h, w, K, merges, alive, labels=labels)
        self._need(costs, torch.int64, (b, K - 1), "costs must be a contiguous (B, K - 1) int64 tensor")
        _lib.check(self.lib.gcs_region_tree(canon.data_ptr(), labels.data_ptr(), b, h, w, d, K, workspace.data_ptr(),
                                            merges.data_ptr() if K > 1 else None,
                                            None if costs is None or K == 1 else costs.data_ptr(), alive.data_ptr(), self._stream()),
                   "gcs_region_tree")

    @_on_device
    def region_tree_slab(self, feats, labels, b, h, w, K, workspace, merges, costs, alive):
        """``region_tree`` with the node statistics taken from the feature slab ``feats`` itself (SPEC.md §21): no canonical tensor.
        Same buffers, same results bit for bit. Three launches, capturable."""
        torch, K = self.torch, int(K)
        self._need_tree(b, h, w, K, merges, alive, labels=labels)
        self._need(costs, torch.int64, (b, K - 1), "costs must be a contiguous (B, K - 1) int64 tensor")
        if feats is None or feats.numel() * feats.element_size() < self.lib.gcs_feature_slab_bytes(b, h, w, *self._bk):
            raise ValueError("feats must be the feature slab of this batch, shape and bank")
        _lib.check(self.lib.gcs_region_tree_slab(feats.data_ptr(), labels.data_ptr(), b, h, w, *self._bk, K, workspace.data_ptr(),
                                                 merges.data_ptr() if K > 1 else None,
                                                 None if costs is None or K == 1 else costs.data_ptr(), alive.data_ptr(),
                                                 self._stream()), "gcs_region_tree_slab")

    @_on_device
    def region_tree_cut(self, labels, merges, alive, b, h, w, K, R, out):
        """The cut of SPEC.md §14 at ``R``: ``out`` (B,H,W) int32 (it may be ``labels``) gets min(alive, R) labels per image. One
        launch, capturable."""
        K = int(K)
        self._need_tree(b, h, w, K, merges, alive, labels=labels, out=out)
        _lib.check(self.lib.gcs_region_tree_cut(labels.data_ptr(), merges.data_ptr() if K > 1 else None, alive.data_ptr(), b, h, w, K,
                                                int(R), out.data_ptr(), self._stream()), "gcs_region_tree_cut")

    def contour_buffers(self, b, K):
        """The workspace of ``gcs_region_tree_contours`` for ``b`` images of ``K`` labels (SPEC.md §15): per image the positions of
        the labels in the tree's leaf order and the range-maximum table over its gaps (a captured graph must own it)."""
        need = self.lib.gcs_region_tree_contours_workspace_bytes(int(b), int(K))
        if need == 0:
            raise ValueError("no contour map for this batch / K (1 <= B <= 65535, 1 <= K <= 4096)")
        return self.empty_bytes(need)

    @_on_device
    def region_tree_contours(self, labels, merges, alive, b, h, w, K, workspace, out):
        """The contour map of SPEC.md §15: ``out`` (B,H,W) int32 (not ``labels``: neighbours are read) gets, per pixel, the level in
        0 .. alive at which its boundary disappears from the tree. ``workspace``: from ``contour_buffers``. Two launches, capturable."""
        K = int(K)
        self._need_tree(b, h, w, K, merges, alive, labels=labels, out=out)
        if out.data_ptr() == labels.data_ptr():
            raise ValueError("out must not be labels: the contour map reads every pixel's neighbours")
        _lib.check(self.lib.gcs_region_tree_contours(labels.data_ptr(), merges.data_ptr() if K > 1 else None, alive.data_ptr(), b, h, w,
                                                     K, workspace.data_ptr(), out.data_ptr(), self._stream()),
                   "gcs_region_tree_contours")

    def _need_table(self, sums, bbox, b, rows):
        """A table of SPEC.md §19: ``sums`` (B, rows, C) int64 (the bits of the uint64 columns), ``bbox`` (B, rows, 4) int32 -> C."""
        torch = self.torch
        if sums is None or sums.dim() != 3 or not 6 <= sums.shape[2] <= 213:
            raise ValueError("sums must be a contiguous (B, rows, 6 + D) int64 tensor, 0 <= D <= 207")
        self._need(sums, torch.int64, (b, rows, sums.shape[2]), "sums must be a contiguous (B, rows, 6 + D) int64 tensor")
        self._need(bbox, torch.int32, (b, rows, 4), "bbox must be a contiguous (B, rows, 4) int32 tensor")
        return int(sums.shape[2])

    @_on_device
    def region_props(self, labels, imgs, canon, b, h, w, K, sums, bbox):
        """The leaf table of SPEC.md §19 of an int32 (B,H,W) label map: ``sums`` (B, K, 6 + D) int64 (the bits of the uint64 columns
        n, sum y, sum x, sum R, sum G, sum B, D feature sums) and ``bbox`` (B, K, 4) int32 are written whole. ``imgs``: None or the
        (B,H,W,3) uint8 images; ``canon``: None (D = 0) or a (B,D,H,W) int16 tensor of ``features_unpack``. Two launches, capturable."""
        torch, K = self.torch, int(K)
        self._need(labels, torch.int32, (b, h, w), "labels must be a contiguous (B,H,W) int32 tensor")
        self._need(imgs, torch.uint8, (b, h, w, 3), "imgs must be a contiguous (B,H,W,3) uint8 tensor")
        d = 0 if canon is None else int(canon.shape[1]) if canon.dim() == 4 else -1
        self._need(canon, torch.int16, (b, d, h, w), "canon must be a contiguous (B,D,H,W) int16 tensor")
        if sums is None or bbox is None or self._need_table(sums, bbox, b, K) != 6 + d:
            raise ValueError("sums must have 6 + D columns")
        _lib.check(self.lib.gcs_region_props(labels.data_ptr(), None if imgs is None else imgs.data_ptr(),
                                             None if canon is None else canon.data_ptr(), b, h, w, d, K, sums.data_ptr(),
                                             bbox.data_ptr(), self._stream()), "gcs_region_props")

    @_on_device
    def region_props_cuts(self, sums, bbox, merges, alive, regions, b, h, w, K, group, sums_out, bbox_out):
        """The tables of the cuts of SPEC.md §19 from the leaf table: ``regions`` (n_cuts,) int32 on the device, decreasing;
        ``group`` (n_cuts, B, K) int32, ``sums_out`` (B, Rsum, C) int64 and ``bbox_out`` (B, Rsum, 4) int32 are written whole
        (Rsum = the caller's sum of min(K, R)). One launch, capturable."""
        torch, K = self.torch, int(K)
        c = self._need_table(sums, bbox, b, K)
        self._need(merges, torch.int32, (b, K - 1, 2), "merges must be a contiguous (B, K - 1, 2) int32 tensor")
        self._need(alive, torch.int32, (b,), "alive must be a contiguous (B,) int32 tensor")
        if regions is None or regions.dim() != 1 or merges is None or alive is None or group is None or sums_out is None:
            raise ValueError("regions must be an (n_cuts,) int32 tensor; merges, alive, group and sums_out are needed")
        n = int(regions.shape[0])
        self._need(regions, torch.int32, (n,), "regions must be a contiguous (n_cuts,) int32 tensor")
        self._need(group, torch.int32, (n, b, K), "group must be a contiguous (n_cuts, B, K) int32 tensor")
        if sums_out.dim() != 3 or bbox_out is None or self._need_table(sums_out, bbox_out, b, int(sums_out.shape[1])) != c:
            raise ValueError("sums_out must be a (B, Rsum, C) int64 tensor with the columns of sums")
        _lib.check(self.lib.gcs_region_props_cuts(sums.data_ptr(), bbox.data_ptr(), merges.data_ptr() if K > 1 else None,
                                                  alive.data_ptr(), regions.data_ptr(), b, h, w, K, c, n, int(sums_out.shape[1]),
                                                  group.data_ptr(), sums_out.data_ptr(), bbox_out.data_ptr(), self._stream()),
                   "gcs_region_props_cuts")

    @_on_device
    def region_paint(self, labels, group, sums, b, h, w, K, out):
        """The mean-colour picture of SPEC.md §19: ``out`` (B,H,W,3) uint8 gets, per pixel of label l, the mean colour of row
        ``group[b][l]`` (``group`` (B, K) int32) or, with ``group`` None, of row l of ``sums`` (B, G, C) int64: a contiguous table or
        a run of rows of one (``sums_out[:, o:o + G]``, read in place). One launch, capturable."""
        torch, K = self.torch, int(K)
        self._need(labels, torch.int32, (b, h, w), "labels must be a contiguous (B,H,W) int32 tensor")
        self._need(group, torch.int32, (b, K), "group must be a contiguous (B, K) int32 tensor")
        if sums is None or sums.dim() != 3 or out is None:
            raise ValueError("sums must be a (B, G, C) int64 tensor and out a (B,H,W,3) uint8 tensor")
        g, c = int(sums.shape[1]), int(sums.shape[2])
        stride = sums.stride(0) // c if b > 1 else g
        if sums.dtype != torch.int64 or sums.shape[0] != b or (g > 1 and sums.stride(1) != c) or sums.stride(2) != 1 or stride < g \
                or (b > 1 and sums.stride(0) != stride * c):
            raise ValueError("sums must be a (B, G, C) int64 tensor, contiguous or a run of rows of a contiguous (B, rows, C) tensor")
        self._need(out, torch.uint8, (b, h, w, 3), "out must be a contiguous (B,H,W,3) uint8 tensor")
        _lib.check(self.lib.gcs_region_paint(labels.data_ptr(), None if group is None else group.data_ptr(), sums.data_ptr(), b, h, w,
                                             K, g, c, stride, out.data_ptr(), self._stream()),
                   "gcs_region_paint")

    def adjacency_buffers(self, tables, capacity):
        """The workspace of ``gcs_region_adjacency`` for ``tables`` images (``gcs_region_adjacency_cuts``: n_cuts * B) at ``capacity``
        edges each (SPEC.md §20): the open-addressing tables the edges are counted in (a captured graph must own it)."""
        need = self.lib.gcs_region_adjacency_workspace_bytes(int(tables), int(capacity))
        if need == 0:
            raise ValueError("no adjacency workspace for this batch / capacity (B >= 1, 1 <= capacity <= 16384)")
        return self.empty_bytes(need)

    def _need_graph(self, edges, vals, count, lead, what):
        """An edge table of SPEC.md §20 over the leading axes ``lead``: edges (.., cap, 2) int32, vals (.., cap, 3) int64 (the bits of
        the uint64 columns), count ``lead`` int32 -> cap."""
        torch = self.torch
        if edges is None or vals is None or count is None or edges.dim() != len(lead) + 2:
            raise ValueError(f"{what}: edges (.., capacity, 2) int32, vals (.., capacity, 3) int64 and count int32 are needed")
        cap = int(edges.shape[-2])
        self._need(edges, torch.int32, lead + (cap, 2), f"{what}: edges must be a contiguous (.., capacity, 2) int32 tensor")
        self._need(vals, torch.int64, lead + (cap, 3), f"{what}: vals must be a contiguous (.., capacity, 3) int64 tensor")
        self._need(count, torch.int32, lead, f"{what}: count must be a contiguous int32 tensor over the leading axes")
        return cap

    @_on_device
    def region_adjacency(self, labels, imgs, strength, b, h, w, K, workspace, edges, vals, count):
        """The edge table of SPEC.md §20 of an int32 (B,H,W) label map: ``edges`` (B, capacity, 2) int32, ``vals`` (B, capacity, 3)
        int64 (the bits of the uint64 columns length, contrast, strength) and ``count`` (B,) int32 are written whole. ``imgs``: None
        or the (B,H,W,3) uint8 images; ``strength``: None or a (B,H,W) int32 plane; ``workspace``: from ``adjacency_buffers(B,
        capacity)``. Three launches, capturable."""
        torch, K = self.torch, int(K)
        self._need(labels, torch.int32, (b, h, w), "labels must be a contiguous (B,H,W) int32 tensor")
        self._need(imgs, torch.uint8, (b, h, w, 3), "imgs must be a contiguous (B,H,W,3) uint8 tensor")
        self._need(strength, torch.int32, (b, h, w), "strength must be a contiguous (B,H,W) int32 tensor")
        cap = self._need_graph(edges, vals, count, (b,), "region_adjacency")
        if labels is None or workspace is None or workspace.numel() * workspace.element_size() < \
                self.lib.gcs_region_adjacency_workspace_bytes(b, cap):
            raise ValueError("labels and a workspace of adjacency_buffers(B, capacity) are needed")
        _lib.check(self.lib.gcs_region_adjacency(labels.data_ptr(), None if imgs is None else imgs.data_ptr(),
                                                 None if strength is None else strength.data_ptr(), b, h, w, K, cap,
                                                 workspace.data_ptr(), edges.data_ptr(), vals.data_ptr(), count.data_ptr(),
                                                 self._stream()), "gcs_region_adjacency")

    @_on_device
    def region_adjacency_cuts(self, edges, vals, count, group, b, K, G, workspace, edges_out, vals_out, count_out):
        """The edge tables of the cuts of SPEC.md §20 from a leaf table: ``group`` (n_cuts, B, K) int32 (``region_props_cuts``' own, or
        any relabelling), ``G`` the number of groups; ``edges_out`` (n_cuts, B, capacity, 2) int32, ``vals_out`` (n_cuts, B, capacity,
        3) int64 and ``count_out`` (n_cuts, B) int32 are written whole; ``workspace``: from ``adjacency_buffers(n_cuts * B,
        capacity)``. Three launches, capturable."""
        torch, K = self.torch, int(K)
        cap = self._need_graph(edges, vals, count, (b,), "region_adjacency_cuts")
        if group is None or group.dim() != 3:
            raise ValueError("group must be a contiguous (n_cuts, B, K) int32 tensor")
        n = int(group.shape[0])
        self._need(group, torch.int32, (n, b, K), "group must be a contiguous (n_cuts, B, K) int32 tensor")
        cap_out = self._need_graph(edges_out, vals_out, count_out, (n, b), "region_adjacency_cuts (outputs)")
        if workspace is None or workspace.numel() * workspace.element_size() < self.lib.gcs_region_adjacency_workspace_bytes(n * b, cap_out):
            raise ValueError("a workspace of adjacency_buffers(n_cuts * B, capacity) is needed")
        _lib.check(self.lib.gcs_region_adjacency_cuts(edges.data_ptr(), vals.data_ptr(), count.data_ptr(), group.data_ptr(), b, K, int(G),
                                                      cap, n, cap_out, workspace.data_ptr(), edges_out.data_ptr(), vals_out.data_ptr(),
                                                      count_out.data_ptr(), self._stream()), "gcs_region_adjacency_cuts")

    @_on_device
    def feature_gradient(self, feats, b, h, w, out):
        """SPEC.md §22: the texture-gradient edge map of the slab ``feats`` (as ``gabor_features`` and the stages behind it left
        it) into ``out``, a contiguous (B,H,W) int32 tensor. One launch, no workspace (capturable as it is)."""
        self._need(out, self.torch.int32, (b, h, w), "out must be a contiguous (B,H,W) int32 tensor")
        if out is None:
            raise ValueError("out must be a contiguous (B,H,W) int32 tensor")
        _lib.check(self.lib.gcs_feature_gradient(feats.data_ptr(), b, h, w, *self._bk, out.data_ptr(), self._stream()),
                   "gcs_feature_gradient")

    @_on_device
    def kmeans_evaluate(self, feats, cent, b, h, w, k, n_sets, labels=None, best=None, second=None, stats=None):
        """SPEC.md §28: the slab ``feats`` measured against the codebooks ``cent``, a contiguous (n_sets, k, D) int16 tensor holding
        the uint16 centroids (what ``kmeans_init`` and the Lloyd loop leave in it), ``n_sets`` 1 or B. Outputs, each optional and
        at least one given: ``labels`` (B,H,W) int32, ``best`` and ``second`` (B,H,W) int64 - the squared distance to the nearest
        and to the second nearest centroid -, ``stats`` (n_sets, k, 2) int64 = (count, inertia) per cluster, zeroed by the call
        itself. One launch (two with ``stats``), no workspace (capturable as it is)."""
        if not hasattr(self.lib, "gcs_kmeans_evaluate"):
            raise _lib.GcsError("the k-means model needs a library that has it (this libgcs.so does not export gcs_kmeans_evaluate)")
        torch = self.torch
        if cent is None or (labels is None and best is None and second is None and stats is None):
            raise ValueError("kmeans_evaluate needs the centroids and at least one of labels, best, second and stats")
        self._need(cent, (torch.int16, torch.uint16), (int(n_sets), int(k), self.bank.n_features),
                   "cent must be a contiguous (n_sets, k, D) int16 tensor")
        self._need(labels, torch.int32, (b, h, w), "labels must be a contiguous (B,H,W) int32 tensor")
        self._need(best, torch.int64, (b, h, w), "best must be a contiguous (B,H,W) int64 tensor")
        self._need(second, torch.int64, (b, h, w), "second must be a contiguous (B,H,W) int64 tensor")
        self._need(stats, torch.int64, (int(n_sets), int(k), 2), "stats must be a contiguous (n_sets, k, 2) int64 tensor")
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.gcs_kmeans_evaluate(feats.data_ptr(), cent.data_ptr(), b, h, w, *self._bk, int(k), int(n_sets),
                                                ptr(labels), ptr(best), ptr(second), ptr(stats), self._stream()),
                   "gcs_kmeans_evaluate")

    @_on_device
    def kmeans_seed(self, feats, b, h, w, k, n_sets, cent, stride, trials=4, seed=0, picks=None, potential=None):
        """SPEC.md §29: k k-means++ seeds per codebook set, drawn among the candidates of the slab ``feats`` at ``stride`` (a power
        of two; at most 4096 candidates per set), into ``cent``, a contiguous (n_sets, k, D) int16 tensor (the uint16 values
        ``kmeans_init`` would write), ``n_sets`` 1 or B. Optional: ``picks`` (n_sets, k) int32, the candidate indices, and
        ``potential`` (n_sets,) int64, the candidates' summed squared distance to their nearest seed. One launch, no workspace
        (capturable as it is)."""
        if not hasattr(self.lib, "gcs_kmeans_seed"):
            raise _lib.GcsError("k-means++ seeding needs a library that has it (this libgcs.so does not export gcs_kmeans_seed)")
        torch = self.torch
        if cent is None:
            raise ValueError("kmeans_seed needs the centroid tensor")
        self._need(cent, (torch.int16, torch.uint16), (int(n_sets), int(k), self.bank.n_features),
                   "cent must be a contiguous (n_sets, k, D) int16 tensor")
        self._need(picks, torch.int32, (int(n_sets), int(k)), "picks must be a contiguous (n_sets, k) int32 tensor")
        self._need(potential, torch.int64, (int(n_sets),), "potential must be a contiguous (n_sets,) int64 tensor")
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.gcs_kmeans_seed(feats.data_ptr(), b, h, w, *self._bk, int(k), int(n_sets), int(stride), int(trials),
                                            int(seed) & _U64, cent.data_ptr(), ptr(picks), ptr(potential), self._stream()),
                   "gcs_kmeans_seed")

    @_on_device
    def kmeans_costs(self, feats, cent, b, h, w, k, n_sets, costs):
        """SPEC.md §30: the cost volume of the slab ``feats`` under the codebooks ``cent`` (as ``kmeans_evaluate`` takes them) into
        ``costs``, a contiguous (B, k, H, W) int64 tensor: the distances d_j(p) of SPEC.md §28. One launch, no workspace."""
        if not hasattr(self.lib, "gcs_kmeans_costs"):
            raise _lib.GcsError("the cost volume needs a library that has it (this libgcs.so does not export gcs_kmeans_costs)")
        torch = self.torch
        if cent is None or costs is None:
            raise ValueError("kmeans_costs needs the centroids and the cost tensor")
        self._need(cent, (torch.int16, torch.uint16), (int(n_sets), int(k), self.bank.n_features),
                   "cent must be a contiguous (n_sets, k, D) int16 tensor")
        self._need(costs, torch.int64, (b, int(k), h, w), "costs must be a contiguous (B, k, H, W) int64 tensor")
        self._check_dev(cent, costs)
        _lib.check(self.lib.gcs_kmeans_costs(feats.data_ptr(), cent.data_ptr(), b, h, w, *self._bk, int(k), int(n_sets),
                                             costs.data_ptr(), self._stream()), "gcs_kmeans_costs")

    @_on_device
    def label_relax(self, costs, beta, b, h, w, k, neighbours, sweeps, labels_in, labels_out, workspace=None, changed=None,
                    energy=None):
        """SPEC.md §30: ``sweeps`` ICM sweeps of the Potts energy of the (B, k, H, W) int64 volume ``costs`` at the weights ``beta``
        ((B,) int64), from the (B,H,W) int32 map ``labels_in`` into ``labels_out`` (another tensor). ``workspace``: at least
        B*H*W*4 bytes, needed for ``sweeps >= 2``. Optional: ``changed`` (B, sweeps) int32, the labels every sweep changed, and
        ``energy`` (B, 2) int64 = (unary, pairs) of the delivered map; both are zeroed by the call itself (capturable as it is)."""
        if not hasattr(self.lib, "gcs_label_relax"):
            raise _lib.GcsError("the label relaxation needs a library that has it (this libgcs.so does not export gcs_label_relax)")
        torch = self.torch
        if costs is None or beta is None or labels_in is None or labels_out is None:
            raise ValueError("label_relax needs costs, beta, labels_in and labels_out")
        self._need(costs, torch.int64, (b, int(k), h, w), "costs must be a contiguous (B, k, H, W) int64 tensor")
        self._need(beta, torch.int64, (b,), "beta must be a contiguous (B,) int64 tensor")
        self._need(labels_in, torch.int32, (b, h, w), "labels_in must be a contiguous (B,H,W) int32 tensor")
        self._need(labels_out, torch.int32, (b, h, w), "labels_out must be a contiguous (B,H,W) int32 tensor")
        self._need(changed, torch.int32, (b, int(sweeps)), "changed must be a contiguous (B, sweeps) int32 tensor")
        self._need(energy, torch.int64, (b, 2), "energy must be a contiguous (B, 2) int64 tensor")
        if workspace is not None and (workspace.numel() * workspace.element_size() < b * h * w * 4 or not workspace.is_contiguous()):
            raise ValueError("workspace must hold at least B*H*W*4 bytes")
        self._check_dev(*(t for t in (costs, beta, labels_in, labels_out, workspace, changed, energy) if t is not None))
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.gcs_label_relax(costs.data_ptr(), beta.data_ptr(), b, h, w, int(k), int(neighbours), int(sweeps),
                                            labels_in.data_ptr(), labels_out.data_ptr(), ptr(workspace), ptr(changed), ptr(energy),
                                            self._stream()), "gcs_label_relax")

    def texton_masks(self, r, n):
        """SPEC.md §24: the half-disc table of radius ``r`` and ``n`` directions, a (n, 2, 2r+1) int32 device tensor holding the
        uint32 rows of gcs_texton_masks; made on the host once per (r, n) and kept (a captured step must find it made)."""
        key = (int(r), int(n))
        if key not in self._texton_masks:
            if not (1 <= key[0] <= 15 and 1 <= key[1] <= 16):
                raise ValueError("the texton gradient takes a radius in 1..15 and 1..16 directions")
            host = np.zeros((key[1], 2, 2 * key[0] + 1), np.uint32)
            _lib.check(self.lib.gcs_texton_masks(key[0], key[1], host.ctypes.data), "gcs_texton_masks")
            self._texton_masks[key] = self.torch.from_numpy(host.view(np.int32)).to(self.device)
        return self._texton_masks[key]

    def _need_half_disc(self, labels, imgs, grad, out, dir_out, masks, b, h, w, r, n, absent):
        """The one check of ``texton_gradient`` and ``cue_gradient``: every tensor that is given, then ``absent`` (the caller's
        message about a tensor that is missing, or None), then the mask table, which is returned (``texton_masks(r, n)`` for None)."""
        i32 = self.torch.int32
        for name, t in (("labels", labels), ("grad", grad), ("out", out)):
            self._need(t, i32, (b, h, w), f"{name} must be a contiguous (B,H,W) int32 tensor")
        self._need(imgs, self.torch.uint8, (b, h, w, 3), "imgs must be a contiguous (B,H,W,3) uint8 tensor")
        self._need(dir_out, self.torch.uint8, (b, h, w), "dir_out must be a contiguous (B,H,W) uint8 tensor")
        if absent:
            raise ValueError(absent)
        if masks is None:
            masks = self.texton_masks(r, n)
        self._need(masks, i32, (int(n), 2, 2 * int(r) + 1), "masks must be a contiguous (n, 2, 2r+1) int32 tensor")
        return masks

    @_on_device
    def texton_gradient(self, labels, b, h, w, K, r, n, grad, out, dir_out, masks=None):
        """SPEC.md §24: the texton gradient of the (B,H,W) int32 label map ``labels`` (values outside 0 .. K-1 count nowhere) at
        radius ``r`` and ``n`` directions into ``out``, a contiguous (B,H,W) int32 tensor: TG, or floor(sqrt(TG * grad)) with
        ``grad`` a (B,H,W) int32 edge map (None: TG). ``dir_out``: (B,H,W) uint8 or None. ``masks``: a (n, 2, 2r+1) int32 device
        tensor in place of ``texton_masks(r, n)`` (any table is exact). One launch, no workspace (capturable as it is)."""
        absent = "labels and out must be contiguous (B,H,W) int32 tensors" if labels is None or out is None else None
        masks = self._need_half_disc(labels, None, grad, out, dir_out, masks, b, h, w, r, n, absent)
        _lib.check(self.lib.gcs_texton_gradient(labels.data_ptr(), b, h, w, int(K), int(r), int(n), masks.data_ptr(),
                                                None if grad is None else grad.data_ptr(), out.data_ptr(),
                                                None if dir_out is None else dir_out.data_ptr(), self._stream()),
                   "gcs_texton_gradient")

    @_on_device
    def cue_gradient(self, labels, imgs, b, h, w, K, bins, weights, r, n, grad, out, dir_out, masks=None):
        """SPEC.md §25: the boundary map of up to four cues - the (B,H,W) int32 label map ``labels`` (K bins, as in
        ``texton_gradient``) and the three channels of the (B,H,W,3) uint8 tensor ``imgs`` quantised to ``bins`` bins - their
        chi-square distances added per direction with the integer ``weights`` (w0, w1, w2, w3) before the maximum is taken, into
        ``out``: PB, or floor(sqrt(PB * grad)). A cue of weight 0 is not read and its tensor may be None. ``dir_out``, ``masks``:
        as in ``texton_gradient``. One launch, no workspace (capturable as it is)."""
        if not hasattr(self.lib, "gcs_cue_gradient"):
            raise ValueError("the cue gradient needs ops that have it (this libgcs.so does not export gcs_cue_gradient)")
        wts = _check_cues(bins, weights)[1]
        absent = None
        if out is None:
            absent = "out must be a contiguous (B,H,W) int32 tensor"
        elif (wts[0] and labels is None) or (any(wts[1:]) and imgs is None):
            absent = "a cue of non-zero weight needs its tensor (labels for weights[0], imgs for weights[1:])"
        masks = self._need_half_disc(labels, imgs, grad, out, dir_out, masks, b, h, w, r, n, absent)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.gcs_cue_gradient(ptr(labels) if wts[0] else None, ptr(imgs) if any(wts[1:]) else None, b, h, w, int(K),
                                             8 - (int(bins).bit_length() - 1), *wts, int(r), int(n), masks.data_ptr(), ptr(grad),
                                             out.data_ptr(), ptr(dir_out), self._stream()), "gcs_cue_gradient")

    def thin_steps(self, n):
        """SPEC.md §26: the step table of ``n`` directions, a (n, 8) int32 device tensor holding the rows of gcs_thin_steps; made
        on the host once per ``n`` and kept (a captured step must find it made)."""
        if not hasattr(self.lib, "gcs_thin_steps"):
            raise ValueError("thin edges need ops that have them (this libgcs.so does not export gcs_thin_steps)")
        key = int(n)
        if key not in self._thin_steps:
            if not 1 <= key <= 16:
                raise ValueError("thin edges take 1..16 directions")
            host = np.zeros((key, 8), np.int32)
            _lib.check(self.lib.gcs_thin_steps(key, host.ctypes.data), "gcs_thin_steps")
            self._thin_steps[key] = self.torch.from_numpy(host).to(self.device)
        return self._thin_steps[key]

    @_on_device
    def edge_thin(self, edges, dirs, b, h, w, n, out, steps=None):
        """SPEC.md §26: the (B,H,W) int32 map ``edges`` thinned along its (B,H,W) uint8 direction map ``dirs`` of ``n`` directions
        into ``out``, a contiguous (B,H,W) int32 tensor: a pixel keeps max(E, 0) when it is the maximum along its direction's
        normal (strict on the minus side, weak on the plus side) and is 0 otherwise. ``steps``: a (n, 8) int32 device tensor in
        place of ``thin_steps(n)`` (any table is exact). One launch, no workspace (capturable as it is)."""
        if not hasattr(self.lib, "gcs_edge_thin"):
            raise ValueError("thin edges need ops that have them (this libgcs.so does not export gcs_edge_thin)")
        if edges is None or dirs is None or out is None:
            raise ValueError("edges and out must be contiguous (B,H,W) int32 tensors and dirs a contiguous (B,H,W) uint8 tensor")
        for name, t in (("edges", edges), ("out", out)):
            self._need(t, self.torch.int32, (b, h, w), f"{name} must be a contiguous (B,H,W) int32 tensor")
        self._need(dirs, self.torch.uint8, (b, h, w), "dirs must be a contiguous (B,H,W) uint8 tensor")
        if steps is None:
            steps = self.thin_steps(n)
        self._need(steps, self.torch.int32, (int(n), 8), "steps must be a contiguous (n, 8) int32 tensor")
        _lib.check(self.lib.gcs_edge_thin(edges.data_ptr(), dirs.data_ptr(), b, h, w, int(n), steps.data_ptr(), out.data_ptr(),
                                          self._stream()), "gcs_edge_thin")

    def region_tree_edges_buffers(self, b, h, w, K, capacity=EDGES_MAX):
        """What SPEC.md §23 needs for one (batch, shape, K): ``(stage, merges (B, K-1, 2) int32, costs (B, K-1) int64, alive (B,)
        int32)``, the shape of ``region_tree_buffers``; ``stage`` is a dict of the plane G (``grad``), the leaf table of SPEC.md §20
        at ``capacity`` (``edges``, ``vals``, ``count``) with its workspace (``adj``), the flags of the labels in use (``used``)
        and the merge kernel's workspace (``tree``) (a captured graph must own them)."""
        torch, K, cap = self.torch, int(K), int(capacity)
        need = self.lib.gcs_region_tree_edges_workspace_bytes(b, K, cap)
        if need == 0 or h > _SP_SIDE_MAX or w > _SP_SIDE_MAX:
            raise ValueError("no region tree for this shape (1 <= B <= 65535, H, W <= 4096, 1 <= K <= 4096, 1 <= capacity <= 16384)")
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
        stage = dict(grad=new((b, h, w), torch.int32), adj=self.adjacency_buffers(b, cap), edges=new((b, cap, 2), torch.int32),
                     vals=new((b, cap, 3), torch.int64), count=new((b,), torch.int32), used=new((b, K), torch.int32),
                     tree=self.empty_bytes(need))
        return stage, new((b, K - 1, 2), torch.int32), new((b, K - 1), torch.int64), new((b,), torch.int32)

    @_on_device
    def label_used(self, labels, b, h, w, K, out):
        """``out`` (B, K) int32 := 1 where a pixel of the int32 (B,H,W) map ``labels`` carries the label, else 0. One launch, capturable."""
        K = int(K)
        self._need(labels, self.torch.int32, (b, h, w), "labels must be a contiguous (B,H,W) int32 tensor")
        self._need(out, self.torch.int32, (b, K), "out must be a contiguous (B, K) int32 tensor")
        if labels is None or out is None:
            raise ValueError("labels and out are needed")
        _lib.check(self.lib.gcs_label_used(labels.data_ptr(), b, h, w, K, out.data_ptr(), self._stream()), "gcs_label_used")

    @_on_device
    def region_tree_edges(self, edges, vals, count, used, b, K, workspace, merges, costs, alive):
        """SPEC.md §23 on a leaf table of SPEC.md §20 (``edges``, ``vals``, ``count`` as ``region_adjacency`` wrote them; the
        strength column weighs the edges) and ``used`` (B, K) int32 (not 0: the label owns a pixel): fills ``merges`` (B, K-1, 2)
        int32, ``costs`` (None or (B, K-1) int64) and ``alive`` (B,) int32 in the format of ``region_tree``. ``workspace``: the
        ``tree`` of ``region_tree_edges_buffers``. One launch, capturable."""
        torch, K = self.torch, int(K)
        cap = self._need_graph(edges, vals, count, (b,), "region_tree_edges")
        self._need(used, torch.int32, (b, K), "used must be a contiguous (B, K) int32 tensor")
        self._need(merges, torch.int32, (b, K - 1, 2), "merges must be a contiguous (B, K - 1, 2) int32 tensor")
        self._need(costs, torch.int64, (b, K - 1), "costs must be a contiguous (B, K - 1) int64 tensor")
        self._need(alive, torch.int32, (b,), "alive must be a contiguous (B,) int32 tensor")
        need = self.lib.gcs_region_tree_edges_workspace_bytes(b, K, cap)
        if used is None or merges is None or alive is None or need == 0 or workspace is None \
                or workspace.numel() * workspace.element_size() < need:
            raise ValueError("used, merges, alive and the workspace of region_tree_edges_buffers are needed (1 <= K <= 4096)")
        _lib.check(self.lib.gcs_region_tree_edges(edges.data_ptr(), vals.data_ptr(), count.data_ptr(), used.data_ptr(), b, K, cap,
                                                  workspace.data_ptr(), merges.data_ptr() if K > 1 else None,
                                                  None if costs is None or K == 1 else costs.data_ptr(), alive.data_ptr(),
                                                  self._stream()), "gcs_region_tree_edges")

    def download(self, dst_pinned, src):
        """Device tensor -> pinned host tensor of the same bytes on the current stream, by SDMA (gcs_download)."""
        self._check_dev(src)
        n = src.numel() * src.element_size()
        if not dst_pinned.is_pinned() or dst_pinned.numel() * dst_pinned.element_size() != n \
                or not src.is_contiguous() or not dst_pinned.is_contiguous():
            raise ValueError("download needs a contiguous device tensor and a pinned host tensor of the same size")
        with self.torch.cuda.device(self.device):
            _lib.check(self.lib.gcs_download(src.data_ptr(), dst_pinned.data_ptr(), n, self._stream()), "gcs_download")

    @_on_device
    def features_gather(self, feats, b, h, w, byx):
        """byx: (n,3) int32 device tensor of (image, row, col); image < 0 -> zero row. -> (n,D) int16."""
        n = byx.shape[0]
        out = self.torch.empty((n, self.bank.n_features), dtype=self.torch.int16, device=self.device)
        _lib.check(self.lib.gcs_features_gather(feats.data_ptr(), b, h, w, *self._bk, n,
                                                byx.data_ptr(), out.data_ptr(), self._stream()),
                   "gcs_features_gather")
        return out

    @_on_device
    def reduce(self, partials, b, h, w, k, n_sets, sums):
        _lib.check(self.lib.gcs_kmeans_reduce(partials.data_ptr(), b, h, w, self.bank.n_features, k,
                                              n_sets, sums.data_ptr(), self._stream()), "gcs_kmeans_reduce")

    @_on_device
    def finalize(self, sums, n_sets, k, cent):
        _lib.check(self.lib.gcs_kmeans_finalize(sums.data_ptr(), n_sets, k, self.bank.n_features,
                                                cent.data_ptr(), self._stream()), "gcs_kmeans_finalize")

    @_on_device
    def reduce_finalize(self, partials, b, h, w, k, n_sets, sums, cent):
        """Single-rank update in one launch (reduce + finalize; no collective in between)."""
        _lib.check(self.lib.gcs_kmeans_reduce_finalize(partials.data_ptr(), b, h, w, self.bank.n_features, k, n_sets,
                                                       sums.data_ptr(), cent.data_ptr(), self._stream()),
                   "gcs_kmeans_reduce_finalize")

    @_on_device
    def connected_regions(self, labels_i32, out):
        """SPEC.md §7 on an int32 (B,H,W) device tensor."""
        b, h, w = labels_i32.shape
        scratch = self.empty_bytes(self.lib.gcs_connected_scratch_bytes(b, h, w))
        _lib.check(self.lib.gcs_connected_regions(labels_i32.data_ptr(), b, h, w, scratch.data_ptr(),
                                                  out.data_ptr(), self._stream()), "gcs_connected_regions")

    @_on_device
    def merge_small_regions(self, labels_i32, min_size, out):
        """SPEC.md §9 on an int32 (B,H,W) device tensor into ``out`` (not the same memory)."""
        b, h, w = labels_i32.shape
        scratch = self.empty_bytes(self.lib.gcs_merge_scratch_bytes(b, h, w, int(min_size)))
        _lib.check(self.lib.gcs_merge_small_regions(labels_i32.data_ptr(), b, h, w, int(min_size), scratch.data_ptr(),
                                                    out.data_ptr(), self._stream()), "gcs_merge_small_regions")

    def region_nodes_buffers(self, b, h, w):
        """What SPEC.md §18 needs for one (batch, shape): ``(scratch, map (B,H,W) int32, n_nodes (B,) int32)`` (a captured graph must
        own them). ``map`` is the second label map of the stage: the step writes the §13 map there and the node map to its output."""
        torch = self.torch
        need = self.lib.gcs_region_nodes_scratch_bytes(b, h, w)
        if need == 0:
            raise ValueError("no node map for this shape (1 <= B <= 65535, 1 <= H, W <= 4096)")
        return (self.empty_bytes(need), torch.empty((b, h, w), dtype=torch.int32, device=self.device),
                torch.empty((b,), dtype=torch.int32, device=self.device))

    @_on_device
    def region_nodes(self, labels_i32, min_size, out, n_nodes, scratch=None, k_cap=NODES_MAX, min_size_used=None):
        """SPEC.md §18 on an int32 (B,H,W) device tensor into ``out`` (not the same memory): the connected regions, merged by §9 at
        ``min_size`` or, in an image that has more than ``k_cap`` of them, at max(min_size, ceil(H W / k_cap)). ``n_nodes`` (B,)
        int32 gets the node counts, ``min_size_used`` (None or (B,) int32) the size each image used. ``scratch``: from
        ``region_nodes_buffers`` (None: a fresh one). Capturable."""
        b, h, w = labels_i32.shape
        self._need(labels_i32, self.torch.int32, (b, h, w), "labels must be a contiguous (B,H,W) int32 tensor")
        self._need(out, self.torch.int32, (b, h, w), "out must be a contiguous (B,H,W) int32 tensor")
        self._need(n_nodes, self.torch.int32, (b,), "n_nodes must be a contiguous (B,) int32 tensor")
        self._need(min_size_used, self.torch.int32, (b,), "min_size_used must be a contiguous (B,) int32 tensor")
        need = self.lib.gcs_region_nodes_scratch_bytes(b, h, w)
        if scratch is None:
            scratch = self.empty_bytes(need)
        elif scratch.numel() < need or scratch.device != self.device:
            raise ValueError("region_nodes scratch too small or on another device")
        _lib.check(self.lib.gcs_region_nodes(labels_i32.data_ptr(), b, h, w, int(min_size), int(k_cap), scratch.data_ptr(),
                                             out.data_ptr(), n_nodes.data_ptr(),
                                             None if min_size_used is None else min_size_used.data_ptr(), self._stream()),
                   "gcs_region_nodes")

    @_on_device
    def labels_widen(self, labels, b, h, w, out):
        _lib.check(self.lib.gcs_labels_widen(labels.data_ptr(), b, h, w, out.data_ptr(), self._stream()),
                   "gcs_labels_widen")

    # centroid / sums tensors are ordinary torch tensors so torch.distributed can move them
    def new_centroids(self, n_sets, k):
        return self.torch.zeros((n_sets, k, self.bank.n_features), dtype=self.torch.int16, device=self.device)

    def new_sums(self, n_sets, k):
        return self.torch.zeros((n_sets, k, self.bank.n_features + 1), dtype=self.torch.int64,
                                device=self.device)


def _collective(fn, t, **kw):
    """Run a torch.distributed collective on a small tensor; gloo gets a host copy of device tensors."""
    import torch.distributed as td
    if t.is_cuda and td.get_backend(kw.get("group")) == "gloo":
        tmp = t.cpu()
        fn(tmp, **kw)
        t.copy_(tmp)
    else:
        fn(t, **kw)


def _as_int(v):
    """``v`` as an int when it is a whole number and not a bool, else None: the test every integer option shares."""
    try:
        i = int(v)
    except (TypeError, ValueError, OverflowError):
        return None
    return i if i == v and not isinstance(v, bool) else None


def _check_chroma_gain(chroma_gain) -> int:
    """SPEC.md §11 parameter: the integer 0 (off) or 1..16."""
    g = _as_int(chroma_gain)
    if g is None or not (0 <= g <= 16):
        raise ValueError(f"chroma_gain must be the integer 0 (off) or 1..16, got {chroma_gain!r}")
    return g


def _check_smoothing(smoothing, bank) -> float:
    """SPEC.md §10 parameter: a finite K >= 0 (0 = off) whose radius is at most 24 on every scale of ``bank``."""
    try:
        K = float(smoothing)
    except (TypeError, ValueError):
        raise ValueError(f"smoothing must be a number, got {smoothing!r}") from None
    if not math.isfinite(K) or K < 0.0:
        raise ValueError(f"smoothing must be finite and >= 0, got {smoothing!r}")
    if K > 0.0:
        smoothing_taps(K, bank.n_scales, bank.n_orient, bank.f_max, bank.ratio)      # raises for a radius outside 1..24
    return K


SUPERPIXELS_MAX = 4096        # SPEC.md §13: centres per image (the option's range and the grid's bound)
_SP_SIDE_MAX, _SP_D_MAX = 4096, 207


def superpixel_grid(height, width, n):
    """SPEC.md §13 grid of ``n_superpixels = n`` on an image of ``height`` x ``width`` pixels: ``(S, ny, nx)`` with
    S = max(1, rint(sqrt(H W / n))), ny = max(1, rint(H / S)), nx = max(1, rint(W / S)); rint is round-half-even on the float64
    value (Python's ``round``). The stage runs K = ny * nx centres."""
    s = max(1, round(math.sqrt(height * width / n)))
    return s, max(1, round(height / s)), max(1, round(width / s))


def _check_superpixels(n_superpixels, spatial_weight):
    """SPEC.md §13 parameters: n the integer 0 (off) or 2..4096, lambda an integer in 1..65535."""
    n, lam = _as_int(n_superpixels), _as_int(spatial_weight)
    if n is None or not (n == 0 or 2 <= n <= SUPERPIXELS_MAX):
        raise ValueError(f"n_superpixels must be the integer 0 (off) or 2..4096, got {n_superpixels!r}")
    if lam is None or not (1 <= lam <= 65535):
        raise ValueError(f"spatial_weight must be an integer in 1..65535, got {spatial_weight!r}")
    return n, lam


REGIONS_MAX = 4096            # SPEC.md §14: the option's range (a cut cannot have more labels than the superpixel grid has centres)


def _check_regions(n_regions, n_superpixels):
    """SPEC.md §14 parameter: R the integer 0 (off) or 1..4096, and only on top of the superpixel stage."""
    r = _as_int(n_regions)
    if r is None or not (0 <= r <= REGIONS_MAX):
        raise ValueError(f"n_regions must be the integer 0 (off) or 1..{REGIONS_MAX}, got {n_regions!r}")
    if r > 0 and n_superpixels == 0:
        raise ValueError('n_regions > 0 merges superpixels: it needs n_superpixels > 0 (or tree_nodes = "clusters", SPEC.md §21)')
    return r


def _check_tree_nodes(tree_nodes, n_superpixels):
    """SPEC.md §18 / §21 parameter: "superpixels" (the tree on the raw §13 map), "components" (on its connected regions; only on top
    of the superpixel stage) or "clusters" (on the connected regions of the k-means map; only without the superpixel stage).
    Returns True for "components"."""
    if not isinstance(tree_nodes, str) or tree_nodes not in ("superpixels", "components", "clusters"):
        raise ValueError(f'tree_nodes must be "superpixels", "components" or "clusters", got {tree_nodes!r}')
    if tree_nodes == "components" and n_superpixels == 0:
        raise ValueError('tree_nodes = "components" takes the components of the superpixel map: it needs n_superpixels > 0')
    if tree_nodes == "clusters" and n_superpixels > 0:
        raise ValueError('tree_nodes = "clusters" takes the components of the k-means map: it needs n_superpixels = 0')
    return tree_nodes == "components"


_U64 = (1 << 64) - 1
SEED_CANDIDATES_MAX = 4096


def seed_stride(b_set, height, width):
    """SPEC.md §29, the host's stride rule: the smallest power of two >= 8 at which a codebook set of ``b_set`` images of
    (height, width) pixels has at most 4096 candidates - 8 for one 481x321 image (61 x 41 = 2501 candidates), 64 for a global
    codebook over 64 of them (3072)."""
    s = 8
    while s <= 4096:
        if b_set * -(-height // s) * -(-width // s) <= SEED_CANDIDATES_MAX:
            return s
        s *= 2
    raise ValueError(f"k-means++ seeding takes at most {SEED_CANDIDATES_MAX} images in one codebook set, got {b_set}")


def _check_seeding(init, seed, seed_trials):
    """The plan's seeding options -> None for the init of SPEC.md §4, (seed, trials) for SPEC.md §29."""
    if init not in ("spec", "kmeans++"):
        raise ValueError(f'init must be "spec" or "kmeans++", got {init!r}')
    s, t = _as_int(seed), _as_int(seed_trials)
    if s is None or not 0 <= s <= _U64:
        raise ValueError(f"seed must be an integer in 0..2^64-1, got {seed!r}")
    if t is None or not 1 <= t <= 8:
        raise ValueError(f"seed_trials must be an integer in 1..8, got {seed_trials!r}")
    return (s, t) if init == "kmeans++" else None


def _check_regularize(regularize, sweeps, neighbours):
    """The plan's options of SPEC.md §30 -> None when ``regularize`` is 0, else (q, sweeps, neighbours), q = round(256 lambda)."""
    try:
        lam = float(regularize)
    except (TypeError, ValueError):
        lam = float("nan")
    if isinstance(regularize, (bool, str, bytes)) or not math.isfinite(lam) or lam < 0:
        raise ValueError(f"regularize must be a finite number >= 0, got {regularize!r}")
    s, n = _as_int(sweeps), _as_int(neighbours)
    if s is None or not 1 <= s <= 64:
        raise ValueError(f"regularize_sweeps must be an integer in 1..64, got {sweeps!r}")
    if n not in (4, 8):
        raise ValueError(f"regularize_neighbours must be 4 or 8, got {neighbours!r}")
    if lam == 0:
        return None
    q = int(math.floor(256.0 * lam + 0.5))
    if not 1 <= q <= 65535:
        raise ValueError(f"regularize: round(256 * lambda) must be in 1..65535, got lambda = {regularize!r}")
    return q, s, n


def relax_beta(stats, q):
    """SPEC.md §30, the weight of a codebook set from the table of SPEC.md §28: ``stats`` (n_sets, k, 2) int64 = (count, inertia)
    -> (n_sets,) int64: beta = (q * m) >> 8 with m = floor(sum_j inertia_j / sum_j count_j). Integer torch operations on the
    tensor's device: no kernel of the library's, no host read."""
    m = stats[:, :, 1].sum(dim=1) // stats[:, :, 0].sum(dim=1)
    return (m * int(q)) >> 8


def _step_relax(ops, opt, ws, km, b, h, w, mode):
    """SPEC.md §30 behind the Lloyd loop, on the slab and the centroids it ended on: the stats table of SPEC.md §28 (for beta
    alone), the cost volume, and ``opt.relax``'s sweeps from a copy of the int32 map ``km`` back into ``km``."""
    q, sweeps, neighbours = opt.relax
    n_sets = b if mode == "per_image" else 1
    rx = _stage_buffers(ops, opt, ws, "rx", b, h, w, n_sets=n_sets, like=km)
    ops.kmeans_evaluate(ws["feats"], ws["cent"], b, h, w, opt.k, n_sets, stats=rx["stats"])
    beta = relax_beta(rx["stats"], q)
    rx["beta"].copy_(beta if n_sets == b else beta.expand(b))             # (global mode: every image gets the set's beta)
    ops.kmeans_costs(ws["feats"], ws["cent"], b, h, w, opt.k, n_sets, rx["costs"])
    rx["start"].copy_(km)
    ops.label_relax(rx["costs"], rx["beta"], b, h, w, opt.k, neighbours, sweeps, rx["start"], km, workspace=rx["work"])


def _seed_init(ops, feats, b, h, w, k, n_sets, seed, trials, stride=None):
    """``lloyd``'s ``init`` for SPEC.md §29: one seed launch into the step's centroids, on the step's stream, at the stride of the
    slab it sees (``seed_stride``) unless one is given."""
    def init(cent):
        ops.kmeans_seed(feats, b, h, w, k, n_sets, cent, stride or seed_stride(b if n_sets == 1 else 1, h, w), trials, seed)
    return init


def lloyd(ops, feats, b, h, w, k, n_iter, mode, labels, partials, cent, sums, dist_group=None,
          rows=None, init=None, raster=None, debug=_ENV_DEBUG, fold=None):
    """SPEC.md §4 schedule on one feature slab. ``mode``: 'per_image' or 'global'.

    In 'global' mode with torch.distributed initialised, the init centroids come from
    rank 0 (its image 0 is image 0 of the global batch) and the int64 sums are all-reduced
    (RCCL on GPU, any order: integer sums are exact). One collective per Lloyd pass.
    ``rows=(lo, hi)``: only these rows of every image vote (row-sharded images, halo rows
    excluded); ``init(cent)``: custom centroid initialisation (row-sharded images).
    ``debug``: the plan's ``DebugSwitches`` (``force_collectives``, ``no_reverse``).
    ``raster``: (B,H,W) int32 / uint8 device tensor: the last pass writes the label map there itself (whole images only,
    ops that have ``assign_raster``) instead of filling the label slab for a separate raster kernel.
    ``fold``: the workspace of ``ops.fused_workspace`` (None: the ops or the library have none for this bank). With it, a
    single-rank loop over whole images that ends in ``raster`` is ``n_iter`` launches: every pass makes its own centroids from the
    sums the previous one left in ``fold`` (no init kernel, no reduce launches; same labels, same ``cent`` afterwards).
    """
    n_sets = b if mode == "per_image" else 1
    dist = None
    if mode == "global":
        import torch.distributed as td
        if td.is_available() and td.is_initialized() and (td.get_world_size(dist_group) > 1 or debug.force_collectives):
            dist = td
    if fold is not None and dist is None and rows is None and init is None and raster is not None and n_iter >= 1:
        for t in range(n_iter):
            rev = not (t & 1) and not debug.no_reverse
            if t == n_iter - 1:
                ops.assign_raster(feats, cent, b, h, w, k, n_sets, raster, scratch_labels=labels, reverse=rev, fused=(fold, t))
            else:
                ops.assign_accumulate(feats, cent, b, h, w, k, n_sets, None, None, reverse=rev, fused=(fold, t))
        return
    if init is not None:
        init(cent)
    else:
        ops.kmeans_init(feats, b, h, w, k, n_sets, cent)
        if dist is not None:
            # RCCL / gloo have no 16-bit integer type: move the centroid bytes
            _collective(dist.broadcast, cent.view(_torch().uint8),
                        src=dist.get_global_rank(dist_group, 0) if dist_group is not None else 0,
                        group=dist_group)
    for t in range(n_iter):
        # alternate the sweep direction: a pass starts where the previous one ended (Infinity Cache reuse); the first
        # pass runs back to front because the Gabor stage, which has just written the slab, finished at its end
        # only the last pass's labels are read, and its sums are not: either output of the kernel is optional
        last = t == n_iter - 1
        rev = not (t & 1) and not debug.no_reverse
        if last and raster is not None:
            ops.assign_raster(feats, cent, b, h, w, k, n_sets, raster, scratch_labels=labels, reverse=rev)
            break
        ops.assign_accumulate(feats, cent, b, h, w, k, n_sets, labels if last else None, None if last else partials, rows,
                              reverse=rev)
        if not last:
            if dist is None:
                ops.reduce_finalize(partials, b, h, w, k, n_sets, sums, cent)
            else:
                ops.reduce(partials, b, h, w, k, n_sets, sums)
                _collective(dist.all_reduce, sums, op=dist.ReduceOp.SUM, group=dist_group)
                ops.finalize(sums, n_sets, k, cent)


# What the per-batch step needs to know of a plan, made once in Segmenter.__init__ (``colour``, ``smooth``, ``position``: is the
# stage on). The two pieces of the step take it, the ops, a workspace and the debug switches as arguments and never the
# Segmenter: a graph entry holds them, and an entry that held its plan would be a reference cycle (see _segment_small).
# ``components``: SPEC.md §18 is on (then ``min_size`` = the plan's min_region_size, the m of the node map); ``clusters``: SPEC.md §21
# is on (the same m). ``boundary``: the tree is SPEC.md §23's (merge_cost = "boundary"). ``seed``: None = the init of SPEC.md §4,
# (seed, trials) = the Lloyd loop starts from the seeds of SPEC.md §29. ``relax``: None = the map as the Lloyd loop leaves it,
# (q, sweeps, neighbours) = the regulariser of SPEC.md §30 behind it, q = round(256 lambda).
_StepOptions = collections.namedtuple("_StepOptions", "k n_iter colour smooth position n_superpixels spatial_weight n_regions "
                                                      "components min_size clusters boundary seed relax",
                                      defaults=(False, False, None, None))


def _opponent(ops, imgs, colour):
    """T_g of ``imgs`` (SPEC.md §11) into the plan-owned buffer ``colour``; returns it. The caller's tensor is not changed."""
    ops.colour_opponent(imgs, colour)
    return colour


def _unpack(ops, ws, b, h, w, out=None):
    """The canonical (B,D,H,W) tensor of the slab ``ws["feats"]``, into ``out`` or a fresh tensor."""
    return ops.features_unpack(ws["feats"], b, h, w, **({} if out is None else {"out": out}))


def _step_features(ops, opt, ws, imgs, b, h, w, y0=0, chunk=None):
    """The first piece of the per-batch step, on the (B,H,W,3) uint8 device tensor ``imgs``: the transform of SPEC.md §11 when
    ``chroma_gain`` is on, the Gabor stage into ``ws["feats"]``, the smoothing of SPEC.md §10 when it is on, then the coordinate
    planes of SPEC.md §12 when ``position_weight`` is on, written behind the Gabor stage and the smoothing (every entry point has
    checked the range rule before its first launch). ``y0``: a row strip's first global row. ``chunk=(g0, g1)``: ``imgs`` holds images [g0, g1) of the ``b`` the slab is for; only their transform and their Gabor stage
    are launched (the chunked upload, which overlaps the next chunk's copy with them). ``imgs=None`` launches the rest: what
    follows the Gabor stage, once for the batch."""
    if imgs is not None:
        feats, colour = ws["feats"], ws.get("colour")
        if chunk is not None:                      # (a chunk of 481 x 321 images starts at any byte)
            feats = feats[chunk[0] * ops.lib.gcs_feature_slab_bytes(1, h, w, *ops._bk):]
            colour = colour[chunk[0]:chunk[1]] if opt.colour else None
        # a private Gabor scratch only where the workspace owns one (a graph entry: see HipOps.gabor_features)
        ops.gabor_features(_opponent(ops, imgs, colour) if opt.colour else imgs, feats,
                           **({"scratch": ws["scratch"]} if "scratch" in ws else {}))
        if chunk is not None:
            return
    if opt.smooth:                                 # (in the chunked upload every chunk's Gabor stage is in front of it)
        ops.smooth_features(ws["feats"], b, h, w, scratch=ws.get("smooth"))
    if opt.position:
        ops.position_features(ws["feats"], b, h, w, y0=y0)


def _stage_buffers(ops, opt, ws, key, b, h, w, n_sets=None, like=None):
    """The one place where the buffers of SPEC.md §13 (``key`` "sp": canonical tensor, workspace), §18 ("nd": scratch, second label
    map, node counts), §14 ("rt": workspace, merges, costs, alive; for K = ny * nx, or K_cap = 4096 on the nodes of §18: about
    5 MB of workspace per image at D = 72, 0.32 GB for a batch of 64) and §30 ("rx": cost volume - B * k * H * W * 8 bytes, 0.63 GB
    for 64 images of 481 x 321 at k = 8 -, stats table, beta, start map and workspace, on the device of ``like``) join a workspace:
    at a stage's first use, or up front for a graph entry. Returns them. A stage that is off leaves no key."""
    if key not in ws:
        _, ny, nx = superpixel_grid(h, w, opt.n_superpixels) if opt.n_superpixels else (0, 0, 0)
        if key == "rx":
            torch, dev = _torch(), like.device
            ws[key] = dict(costs=torch.empty((b, opt.k, h, w), dtype=torch.int64, device=dev),
                           stats=torch.empty((n_sets, opt.k, 2), dtype=torch.int64, device=dev),
                           beta=torch.empty((b,), dtype=torch.int64, device=dev),
                           start=torch.empty((b, h, w), dtype=torch.int32, device=dev),
                           work=torch.empty((b, h, w), dtype=torch.int32, device=dev))
        elif key == "sp":
            ws[key] = ops.superpixel_buffers(b, h, w, opt.n_superpixels)
        elif key == "nd":
            ws[key] = ops.region_nodes_buffers(b, h, w)
        else:
            make = ops.region_tree_edges_buffers if opt.boundary else ops.region_tree_buffers
            ws[key] = make(b, h, w, NODES_MAX if opt.components or opt.clusters else ny * nx)
    return ws[key]


_RELAX_OPS = ("kmeans_evaluate", "kmeans_costs", "label_relax")
_BOUNDARY_OPS = ("region_tree_edges_buffers", "feature_gradient", "label_used", "region_adjacency", "region_tree_edges")


def _check_texton(radius, n_directions):
    """SPEC.md §24: the radius and the number of directions of the texton gradient as integers."""
    r, n = _as_int(radius), _as_int(n_directions)
    if not 1 <= r <= 15:
        raise ValueError(f"radius must be in 1..15, got {radius!r}")
    if not 1 <= n <= 16:
        raise ValueError(f"n_directions must be in 1..16, got {n_directions!r}")
    return r, n


def _check_cues(bins, weights):
    """SPEC.md §25: the number of bins of a quantised channel and the four cue weights (textons, channel 0, 1, 2) as integers."""
    nb = _as_int(bins)
    if nb not in (2, 4, 8, 16, 32, 64):
        raise ValueError(f"bins must be one of 2, 4, 8, 16, 32, 64, got {bins!r}")
    if isinstance(weights, (str, bytes)) or not hasattr(weights, "__len__") or len(weights) != 4:
        raise ValueError(f"weights must be four integers (textons, channel 0, 1, 2), got {weights!r}")
    wts = tuple(_as_int(v) for v in weights)
    if any(v is None or not 0 <= v <= 16 for v in wts) or not any(wts):
        raise ValueError(f"weights must be integers in 0..16, not all zero, got {weights!r}")
    return nb, wts


def _check_merge_cost(merge_cost):
    """SPEC.md §23: which cost the tree merges by."""
    if not isinstance(merge_cost, str) or merge_cost not in ("features", "boundary"):
        raise ValueError(f'merge_cost must be "features" or "boundary", got {merge_cost!r}')
    return merge_cost == "boundary"


def _step_tree(ops, opt, ws, rt, labels, b, h, w, K, canon=None):
    """The tree of the int32 node map ``labels`` into the buffers ``rt`` of ``_stage_buffers``: SPEC.md §14 on the canonical tensor
    ``canon`` or, without one (SPEC.md §21), on the slab; with ``merge_cost = "boundary"`` SPEC.md §23: the edge map of §22 from the
    slab, the labels in use, the leaf table of §20 with that map as its strength plane, and the merges on that table. No node
    statistics are gathered and no feature is read behind the edge map."""
    stage, merges, costs, alive = rt
    if opt.boundary:
        ops.feature_gradient(ws["feats"], b, h, w, stage["grad"])
        ops.label_used(labels, b, h, w, K, stage["used"])
        ops.region_adjacency(labels, None, stage["grad"], b, h, w, K, stage["adj"], stage["edges"], stage["vals"], stage["count"])
        ops.region_tree_edges(stage["edges"], stage["vals"], stage["count"], stage["used"], b, K, stage["tree"], merges, costs, alive)
    elif canon is None:
        ops.region_tree_slab(ws["feats"], labels, b, h, w, K, stage, merges, costs, alive)
    else:
        ops.region_tree(canon, labels, b, h, w, K, stage, merges, costs, alive)


def _step_cluster(ops, opt, ws, out, b, h, w, mode, debug, dist_group=None, rows=None, init=None, centres=None, tree=None,
                  nodes=None):
    """The second piece of the per-batch step, on the slab ``_step_features`` has filled: the labels of ``b`` images into ``out``,
    a contiguous (B,H,W) device tensor. ``n_superpixels = 0``: the Lloyd loop of SPEC.md §4 (``rows``, ``init``, ``dist_group``:
    see ``lloyd``); without a raster pass the label slab is widened into the int32 ``out``. ``n_superpixels > 0`` (SPEC.md §13
    instead of §4): features -> canonical tensor -> the one call that enqueues every pass (``centres``: see
    ``HipOps.superpixels``), then the tree of SPEC.md §14 on the raw §13 map and its cut in place. ``tree``: None = as the plan
    says (tree and cut at ``n_regions`` when that is on), True = the tree without a cut (it stays in ``ws["rt"]``), False = no
    tree. With ``tree_nodes = "components"`` (SPEC.md §18) the §13 map goes to the stage's own buffer, its node map to the output,
    and tree and cut run on that, the tree at K_cap; ``nodes=False`` leaves the §13 map as it is. A uint8 ``out`` is narrowed from
    the int32 map of the workspace (a graph entry). With ``tree_nodes = "clusters"`` (SPEC.md §21) the Lloyd loop writes its int32
    map to the node stage's own buffer, its node map goes to the output, and the tree reads its statistics from the slab
    (``region_tree_slab``: no canonical tensor), at K_cap; ``tree`` as above. ``opt.seed`` (SPEC.md §29): without an ``init`` the
    Lloyd loop starts from the seed launch on this slab instead of the init of SPEC.md §4. ``opt.relax`` (SPEC.md §30): the int32
    k-means map is regularised in place behind the loop (``_step_relax``), in front of the node map; the entry points that
    deliver uint8 maps straight from the loop never run with it."""
    if opt.n_superpixels == 0:
        ndws = raw = n_nodes = None
        if opt.clusters:
            ndws, raw, n_nodes = _stage_buffers(ops, opt, ws, "nd", b, h, w)
        out32 = out
        if opt.clusters and out.dtype != _torch().int32:   # a uint8 result is narrowed from an int32 map the workspace keeps
            if "out32" not in ws:
                ws["out32"] = _torch().empty((b, h, w), dtype=_torch().int32, device=out.device)
            out32 = ws["out32"]
        km = raw if opt.clusters else out
        raster = km if rows is None and hasattr(ops, "assign_raster") else None       # the last pass writes the raster map itself
        if init is None and opt.seed is not None:                                     # SPEC.md §29 (given centroids win)
            init = _seed_init(ops, ws["feats"], b, h, w, opt.k, b if mode == "per_image" else 1, *opt.seed)
        lloyd(ops, ws["feats"], b, h, w, opt.k, opt.n_iter, mode, ws["labels"], ws["partials"], ws["cent"], ws["sums"],
              dist_group, rows=rows, init=init, raster=raster, debug=debug, fold=ws.get("fold"))
        if raster is None:
            ops.labels_widen(ws["labels"], b, h, w, km)
        if opt.relax is not None:                                                     # SPEC.md §30: every later stage sees its map
            _step_relax(ops, opt, ws, km, b, h, w, mode)
        if not opt.clusters:
            return
        ops.region_nodes(raw, opt.min_size, out32, n_nodes, scratch=ndws)
        if opt.n_regions > 0 if tree is None else tree:
            rtws, merges, costs, alive = _stage_buffers(ops, opt, ws, "rt", b, h, w)
            _step_tree(ops, opt, ws, (rtws, merges, costs, alive), out32, b, h, w, NODES_MAX)
            if tree is None:
                ops.region_tree_cut(out32, merges, alive, b, h, w, NODES_MAX, opt.n_regions, out32)
        if out32 is not out:
            out.copy_(out32)                       # (1 <= n_regions <= 256 was checked: the narrowing keeps every label)
        return
    _, ny, nx = superpixel_grid(h, w, opt.n_superpixels)
    (canon, spws), out32 = _stage_buffers(ops, opt, ws, "sp", b, h, w), ws.get("out32", out)
    _unpack(ops, ws, b, h, w, out=canon)
    K = ny * nx
    if opt.components if nodes is None else nodes:
        ndws, raw, n_nodes = _stage_buffers(ops, opt, ws, "nd", b, h, w)
        ops.superpixels(canon, b, h, w, ny, nx, opt.spatial_weight, opt.n_iter, raw, spws, centres)
        ops.region_nodes(raw, opt.min_size, out32, n_nodes, scratch=ndws)
        K = NODES_MAX
    else:
        ops.superpixels(canon, b, h, w, ny, nx, opt.spatial_weight, opt.n_iter, out32, spws, centres)
    if opt.n_regions > 0 if tree is None else tree:
        rtws, merges, costs, alive = _stage_buffers(ops, opt, ws, "rt", b, h, w)
        _step_tree(ops, opt, ws, (rtws, merges, costs, alive), out32, b, h, w, K, canon)
        if tree is None:
            ops.region_tree_cut(out32, merges, alive, b, h, w, K, opt.n_regions, out32)
    if out32 is not out:
        out.copy_(out32)                           # (K, or min(K, R), <= 256 was checked: the narrowing keeps every label)


def halo_rows(n_levels: int = 2, ksize: int = 13) -> int:
    """Real neighbour rows an interior strip edge needs: the reach (ksize - 1) / 2 of the coarsest level's kernel in
    full-resolution rows (12 for the default 13x13 bank on two levels - the defaults here -, 14 for a 15x15 one)."""
    return ((ksize - 1) // 2) << (n_levels - 1)


def shard_rows(height: int, world: int, rank: int, n_levels: int = 2, ksize: int = 13):
    """Row strip of rank ``rank``: owned global rows [r0, r1) and the strip [s0, s1) that also carries real
    neighbour rows on interior edges (BASELINE config 5).

    ``n_levels`` = pyramid levels of the bank (SPEC.md §2), ``ksize`` its kernel size; the defaults are those of the default
    bank (4 scales on 2 levels, 13x13) - for any other bank use ``Segmenter.shard_rows``, which reads them from its bank. Strip and ownership boundaries are multiples of
    ``2**(n_levels-1)`` so that every strip's pyramid is a window of the global pyramid, and the halo is the reach of
    the coarsest level's kernel: ``halo_rows(n_levels, ksize)`` rows."""
    align = 1 << (n_levels - 1)
    halo = halo_rows(n_levels, ksize)
    r0 = (height * rank) // world // align * align
    r1 = height if rank == world - 1 else (height * (rank + 1)) // world // align * align
    return r0, r1, max(0, r0 - halo), min(height, r1 + halo)


def s1_of(bounds, r):
    """End row (exclusive) of rank r's strip, halo included: what its lower neighbour has to send it."""
    return bounds[r][3]


class Segmenter:
    """Reusable plan: bank on device + cached workspaces. ``__call__`` is the slot."""

    def __init__(self, n_scales=4, n_orient=6, k=8, n_iter=10, ksize=13, f_max=0.4,
                 ratio=math.sqrt(2.0), bandwidth=1.0, connectivity=False, device="cuda:0", ops=None,
                 slab_candidates=1, min_region_size=0, smoothing=0.0, color_weight=0.0, chroma_gain=0,
                 position_weight=0, n_superpixels=0, spatial_weight=576, n_regions=0, tree_nodes="superpixels",
                 merge_cost="features", init="spec", seed=0, seed_trials=4, regularize=0.0, regularize_sweeps=4,
                 regularize_neighbours=8):
        """``regularize = lambda > 0`` (SPEC.md §30; needs ``n_superpixels = 0``; 0, the default: every path enqueues what it always
        did): a Potts prior on the k-means map, minimised by ``regularize_sweeps`` (1..64) sweeps of iterated conditional modes over
        ``regularize_neighbours`` (4 or 8) neighbours, behind the Lloyd loop (and behind ``codebook=`` / ``refine=``) and in front
        of ``connectivity``, ``min_region_size`` and the node map of ``tree_nodes = "clusters"``. The weight of a differing
        neighbour is beta = (round(256 lambda) * m) >> 8 with m the mean squared distance of a pixel to its centroid, so lambda
        is in units of the map's own mean cost. Host batches take the plain path. Not with row strips, a ``dist_group``, more than
        one rank or the texton / cue edge chains.

        ``init = "kmeans++"`` (SPEC.md §29; needs ``n_superpixels = 0``): every Lloyd loop of the plan starts from k seeds drawn
        by k-means++ with ``seed_trials`` greedy trials (1..8) among a grid of at most 4096 candidate pixels of its codebook set
        (``seed_stride``), one launch in front of the passes, instead of the k evenly spaced raster pixels of SPEC.md §4
        (``"spec"``, the default: every path enqueues what it always did). The draws depend on ``seed`` (0..2^64-1) alone, not on
        the image: a single image's result is its row of the batch's. A ``codebook=`` wins: no seeding runs. Restarts:
        ``fit_device(n_init=n)``. Not over a ``dist_group``, and not on the row-strip entry points.

        ``n_superpixels = n`` (SPEC.md §13; 0 = off, 2..4096): grid-local k-means instead of the Lloyd stage - about n compact
        superpixels per image (K = ny * nx of ``superpixel_grid``) on the same features; ``k`` and ``mode`` are then unused (centres
        are per image). ``spatial_weight`` = lambda (1..65535, default 576) weighs the squared pixel distance to a centre against
        the squared feature distance: larger = more compact. Recommended pairing: ``min_region_size = S * S // 4`` with S of
        ``superpixel_grid(H, W, n)``, which turns the label map into connected regions and merges the fragments.

        ``n_regions = R`` (SPEC.md §14; 0 = off, 1..4096; needs ``n_superpixels > 0``): the superpixels are merged on their adjacency
        graph, cheapest mutual pair first, until min(R, superpixels in use) regions are left; ``connectivity`` and
        ``min_region_size`` then apply to that map. ``region_tree_device`` / ``cut_regions_device`` give the tree itself and any cut.

        ``tree_nodes = "components"`` (SPEC.md §18; needs ``n_superpixels > 0``): the tree's nodes are the 4-connected components of
        the superpixel map (with ``min_region_size = m > 0``: merged by §9 at m first) instead of its labels, so a cut at R IS
        min(nodes, R) connected regions, numbered in raster order of first pixel, and contour map and sweeps describe the delivered
        maps. ``connectivity`` and ``min_region_size`` are not run again behind the cut. Without ``n_regions`` the node map itself
        is delivered. The default, "superpixels", is the tree on the raw map.

        ``tree_nodes = "clusters"`` (SPEC.md §21; needs ``n_superpixels = 0``): the same tree on the 4-connected components of the
        k-means map (``k``, ``mode`` and ``n_iter`` as without it), cut at ``n_regions``: no superpixel stage, and the tree takes
        its statistics from the feature slab itself. Everything said of "components" holds: min(nodes, R) connected regions in
        raster order, ``min_region_size`` joins the node map, nothing runs behind the cut.

        ``merge_cost = "boundary"`` (SPEC.md §23; wherever a tree is valid, in all three ``tree_nodes`` modes): the tree merges the
        pair of adjacent groups whose common boundary is weakest on average in the texture-gradient map of SPEC.md §22 (the
        UCM rule) instead of the pair of closest mean features: cost = floor(128 strength / length) of the pair's edge in the
        region adjacency graph of SPEC.md §20. Merge list, cuts, contour map and sweeps keep their format and meaning. The
        default, "features", is the tree of SPEC.md §14, bit for bit."""
        if not (1 <= k <= _lib.K_MAX):
            raise ValueError(f"k must be in 1..{_lib.K_MAX}")
        if n_iter < 1:
            raise ValueError("n_iter must be >= 1")
        if int(min_region_size) != min_region_size or min_region_size < 0:
            raise ValueError("min_region_size must be a non-negative integer")
        self.k = int(k)
        self.debug = DebugSwitches(os.environ.get("GCS_DEBUG", ""))     # measurement / test switches (see the class)
        self.connectivity = bool(connectivity)     # SPEC.md §7 post-pass
        self.min_region_size = int(min_region_size)  # SPEC.md §9 post-pass (> 0: connected regions, small ones merged)
        self.color_weight = check_color_weight(color_weight)        # SPEC.md §11: a low-pass slot behind every scale's filters
        self.chroma_gain = _check_chroma_gain(chroma_gain)          # SPEC.md §11: T_g in front of the Gabor stage
        self.position_weight = check_position_weight(position_weight)   # SPEC.md §12: a coordinate slot behind every scale's filters
        self.bank = make_bank(n_scales, n_orient, ksize, f_max, ratio, bandwidth, self.color_weight, self.position_weight)
        self.smoothing = _check_smoothing(smoothing, self.bank)     # SPEC.md §10, between the Gabor stage and k-means
        # SPEC.md §28: what a k-means model must share with the plan that takes it - the feature space and k
        self.model_signature = dict(n_scales=int(n_scales), n_orient=int(n_orient), ksize=int(ksize), f_max=float(f_max),
                                    ratio=float(ratio), bandwidth=float(bandwidth), color_weight=float(self.color_weight),
                                    chroma_gain=int(self.chroma_gain), smoothing=float(self.smoothing),
                                    position_weight=int(self.position_weight), k=self.k)
        self.n_superpixels, self.spatial_weight = _check_superpixels(n_superpixels, spatial_weight)   # SPEC.md §13 (0: §4's Lloyd stage)
        self._seeding = _check_seeding(init, seed, seed_trials)                  # SPEC.md §29 (None: the init of §4)
        self.init, self.seed, self.seed_trials = init, int(seed), int(seed_trials)
        if self._seeding and self.n_superpixels > 0:
            raise ValueError('init = "kmeans++" seeds the Lloyd stage: it needs n_superpixels = 0')
        self._relax = _check_regularize(regularize, regularize_sweeps, regularize_neighbours)   # SPEC.md §30 (None: off)
        self.regularize, self.regularize_sweeps = float(regularize), int(regularize_sweeps)
        self.regularize_neighbours = int(regularize_neighbours)
        if self._relax and self.n_superpixels > 0:
            raise ValueError("regularize > 0 relaxes the k-means map: it needs n_superpixels = 0")
        if self.n_superpixels > 0 and self.bank.n_features > _SP_D_MAX:
            raise ValueError(f"n_superpixels needs a bank of at most {_SP_D_MAX} features, this one has {self.bank.n_features}")
        self._boundary = _check_merge_cost(merge_cost)                          # SPEC.md §23
        self.merge_cost = merge_cost
        if self._boundary and self.n_superpixels == 0 and tree_nodes != "clusters":
            raise ValueError('merge_cost = "boundary" weighs a region tree: it needs n_superpixels > 0 or tree_nodes = "clusters"')
        self.ops = ops if ops is not None else HipOps(self.bank, device, self.smoothing, self.chroma_gain)
        if self.n_superpixels > 0 and not hasattr(self.ops, "superpixels"):
            raise ValueError("Segmenter(n_superpixels=n, ops=...) needs ops that have the superpixel stage")
        if self._seeding and not hasattr(self.ops, "kmeans_seed"):
            raise ValueError('Segmenter(init="kmeans++", ops=...) needs ops that have kmeans_seed')
        if self._relax and not all(hasattr(self.ops, m) for m in _RELAX_OPS):
            raise ValueError("Segmenter(regularize=lambda, ops=...) needs ops that have kmeans_evaluate, kmeans_costs and label_relax")
        self._components = _check_tree_nodes(tree_nodes, self.n_superpixels)    # SPEC.md §18
        self._clusters = tree_nodes == "clusters"                               # SPEC.md §21 (checked: n_superpixels = 0)
        self.tree_nodes = tree_nodes
        if self._clusters and self.bank.n_features > _SP_D_MAX:
            raise ValueError(f'tree_nodes = "clusters" needs a bank of at most {_SP_D_MAX} features, this one has {self.bank.n_features}')
        # SPEC.md §14 (0: the map as it is); the tree merges superpixels or, in the mode of §21, the regions of the k-means map
        self.n_regions = _check_regions(n_regions, 1 if self._clusters else self.n_superpixels)
        tree_ops = ("region_tree_buffers", "region_tree_slab" if self._clusters else "region_tree", "region_tree_cut")
        if self._boundary:
            tree_ops = _BOUNDARY_OPS + ("region_tree_cut",)
            if not all(hasattr(self.ops, m) for m in tree_ops):
                raise ValueError('Segmenter(merge_cost="boundary", ops=...) needs ops that have the stages of SPEC.md §23')
        if self.n_regions > 0 and not all(hasattr(self.ops, m) for m in tree_ops):
            raise ValueError("Segmenter(n_regions=R, ops=...) needs ops that have the region tree")
        if (self._components or self._clusters) and not all(hasattr(self.ops, m) for m in ("region_nodes_buffers", "region_nodes")):
            raise ValueError(f'Segmenter(tree_nodes="{tree_nodes}", ops=...) needs ops that have the node map')
        if self.smoothing > 0 and getattr(self.ops, "smoothing", 0.0) != self.smoothing:
            raise ValueError("Segmenter(smoothing=K, ops=...) needs ops built with the same smoothing")
        if getattr(self.ops, "chroma_gain", 0) != self.chroma_gain:
            raise ValueError("Segmenter(chroma_gain=g, ops=...) needs ops built with the same chroma_gain")
        ops_bank = getattr(self.ops, "bank", None)
        if getattr(ops_bank, "color_weight", 0.0) != self.color_weight or \
                (self.color_weight > 0 and (ops_bank.n_scales, ops_bank.n_orient) != (self.bank.n_scales, self.bank.n_orient)):
            raise ValueError("Segmenter(color_weight=w, ops=...) needs ops built for the same colour bank")
        if getattr(ops_bank, "position_weight", 0) != self.position_weight or \
                (self.position_weight > 0 and ((ops_bank.n_scales, ops_bank.n_orient) != (self.bank.n_scales, self.bank.n_orient)
                                               or not hasattr(self.ops, "position_features"))):
            raise ValueError("Segmenter(position_weight=mu, ops=...) needs ops built for the same position bank")
        # feature-slab allocations to time at first use of a large workspace shape (see _place_slab). 1 = take the first
        # one (the library default: no extra memory, no host synchronisation, graph-capturable); bench.py asks for 2.
        self.slab_candidates = int(self.debug.slab_candidates or slab_candidates)
        self.slab_placement_ms = None
        self._opt = _StepOptions(self.k, int(n_iter), self.chroma_gain > 0, self.smoothing > 0, self.position_weight > 0,
                                 self.n_superpixels, self.spatial_weight, self.n_regions, self._components,
                                 self.min_region_size, self._clusters, self._boundary, self._seeding, self._relax)
        self._ws = {}
        self._host = {}
        self._stream = {}
        self._copy_pair = None
        self._stagers = None
        self._graphs = {}
        self._last_plane = None

    def __del__(self):
        # a plan dropped in one thread while another thread captures: its graphs leave through the guard (parked until that
        # capture has ended) instead of being destroyed wherever the last reference happened to die
        try:
            ents = list(self._graphs.values())
            self._graphs.clear()
            _CAPTURES.retire(ents)
        except Exception:            # interpreter shutdown: module globals may be gone
            pass

    @property
    def native(self):
        """True when the ops are HipOps (libgcs.so). The only other ops are the CPU tests' stand-in for the host logic
        (tests/fake_ops.py), which has no slabs, streams or graphs: the pipelined / captured host paths need ``native``."""
        return hasattr(self.ops, "lib")

    @property
    def _post_passes(self):
        """Do ``connectivity`` / ``min_region_size`` run behind the step? Not in the mode of SPEC.md §18, whose maps are connected."""
        return (self.connectivity or self.min_region_size > 0) and not (self._components or self._clusters)

    @property
    def n_iter(self):
        return self._opt.n_iter

    @n_iter.setter
    def n_iter(self, n):             # (the one option that is changed on a live plan, by tests: the step's record follows)
        self._opt = self._opt._replace(n_iter=int(n))

    @property
    def _model_opt(self):
        """The step of the entry points that describe the k-means model (SPEC.md §28): the plan's, without the regulariser of
        SPEC.md §30, which changes the map and not the model."""
        return self._opt._replace(relax=None)

    def _device(self):
        """Launches go through ctypes on the current stream of ``self.ops.device``: the context that makes that device current
        (the stand-in ops have no device)."""
        return _torch().cuda.device(self.ops.device) if self.native else contextlib.nullcontext()

    # ---- argument rules, path decisions
    def _check_args(self, imgs=None, mode="per_image", out_dtype=None, dist_group=None, kind="array", cluster=True):
        """The ONE set of argument rules of the entry points, applied before an entry point's first launch, in this order: the
        batch ``imgs`` (a (B,H,W,3) uint8 ``kind``; None: no batch is at hand yet, the rules about its shape wait for it), ``mode``,
        ``out_dtype`` (None: the entry point has none) and what it conflicts with, the smallest image, the range rule of SPEC.md
        §12, the rules of SPEC.md §13 (not with ``cluster=False``: an entry point that stops behind the features). Returns
        ``out_dtype`` as a ``np.dtype``."""
        if imgs is not None and (not str(imgs.dtype).endswith("uint8") or imgs.ndim != 4 or imgs.shape[3] != 3):
            raise ValueError(f"imgs must be a (B,H,W,3) uint8 {kind}")
        if mode not in ("per_image", "global"):
            raise ValueError("mode must be 'per_image' or 'global'")
        if out_dtype is not None:
            out_dtype = np.dtype(out_dtype)
            if out_dtype not in (np.dtype(np.int32), np.dtype(np.uint8)):
                raise ValueError("out_dtype must be int32 or uint8")
            if self._components or self._clusters:
                if out_dtype == np.uint8 and not 1 <= self.n_regions <= 256:
                    raise ValueError(f'tree_nodes = "{self.tree_nodes}": uint8 labels need n_regions in 1..256 (the node count is data)')
            elif self.connectivity and out_dtype == np.uint8:
                raise ValueError("connectivity=True needs int32 labels")
            elif self.min_region_size > 0 and out_dtype == np.uint8:
                raise ValueError("min_region_size > 0 needs int32 labels")
        h = w = None
        if imgs is not None:
            h, w = imgs.shape[1:3]
            if h < 8 or w < 8:
                raise ValueError("images must be at least 8x8")
            check_position_range(self.position_weight, h, w)
        if self._seeding and cluster:
            if dist_group is not None:
                raise ValueError('init = "kmeans++" does not run over a dist_group')
            if mode == "global":
                import torch.distributed as td
                if td.is_available() and td.is_initialized() and td.get_world_size() > 1:
                    raise ValueError('init = "kmeans++" does not run over more than one rank (every rank would draw its own seeds)')
                if imgs is not None:
                    seed_stride(imgs.shape[0], h, w)       # (ValueError: more than 4096 images in the one set)
        if self._relax and cluster:
            if dist_group is not None:
                raise ValueError("regularize > 0 does not run over a dist_group")
            if mode == "global":
                import torch.distributed as td
                if td.is_available() and td.is_initialized() and td.get_world_size() > 1:
                    raise ValueError("regularize > 0 does not run over more than one rank (beta would be one rank's)")
        if self.n_superpixels > 0 and cluster:
            self._superpixel_check(h, w, mode, out_dtype, dist_group)
        if self._clusters and cluster:
            self._cluster_check(h, w, mode, dist_group)
        return out_dtype

    def _may_pipeline(self, mode, superpixels=False):
        """May host batches of this plan leave the plain path (``segment_device`` between two blocking copies)? Not the test
        stand-ins, the post-passes, the regulariser of SPEC.md §30 and the collectives; SPEC.md §13 only where the caller says so (``superpixels``: a small call
        replays its graph like any other, but there is no chunked upload and no three-stream pipeline for it)."""
        dist_on = False
        if mode == "global":
            import torch.distributed as td
            dist_on = td.is_available() and td.is_initialized()
        return self.native and not self._post_passes and not dist_on and self._relax is None \
            and not self.debug.force_collectives and (superpixels or self.n_superpixels == 0)

    def _host_path(self, b, h, w, mode):
        """How ``segment_batch`` runs a (b,h,w) batch: "graph" (replay of the captured step: calls of up to _GRAPH_MAX_PIXELS),
        "chunked" (chunked upload, eager launches) or "plain" (see ``_may_pipeline``; a batch of more than one group; a large or
        uncaptured superpixel call)."""
        small = b * h * w <= _GRAPH_MAX_PIXELS and not self.debug.no_graph
        if not self._may_pipeline(mode, superpixels=True) or self.group_size(b, h, w, mode) < b \
                or (self.n_superpixels > 0 and not small):
            return "plain"
        return "graph" if small else "chunked"

    # ---- workspaces
    def _tail_workspace(self, n, h, w, mode, slab_only=False, private=None):
        """The buffers of one step on ``n`` images: the only place that allocates them. A key for a stage that is off stays
        absent. ``slab_only``: no Lloyd buffers and no private smoothing scratch (``features_device``). ``private``: the out
        dtype of a graph entry - a captured graph bakes raw pointers in, so every buffer it touches belongs to the entry and lives
        exactly as long as the graph does: the stage buffers of SPEC.md §13 / §14 up front, the int32 map behind a uint8 superpixel
        result, and the Gabor scratch (the shared scratch of HipOps is replaced, and its block recycled, whenever a later call
        needs a larger one)."""
        ops, opt = self.ops, self._opt
        n_sets = n if mode == "per_image" else 1
        ws = dict(feats=ops.feature_slab(n, h, w))
        if not slab_only:
            ws.update(labels=ops.label_slab(n, h, w), partials=ops.partial_slab(n, h, w, opt.k),
                      cent=ops.new_centroids(n_sets, opt.k), sums=ops.new_sums(n_sets, opt.k))
            if hasattr(ops, "fused_workspace"):
                ws["fold"] = ops.fused_workspace(n, h, w, opt.k, n_sets)
            if opt.smooth:
                ws["smooth"] = ops.smooth_scratch(n, h, w)
        if opt.colour:
            ws["colour"] = ops.colour_scratch(n, h, w)
        if private is not None:
            if opt.n_superpixels > 0:
                _stage_buffers(ops, opt, ws, "sp", n, h, w)
                if opt.components:
                    _stage_buffers(ops, opt, ws, "nd", n, h, w)
                if opt.n_regions > 0:
                    _stage_buffers(ops, opt, ws, "rt", n, h, w)
                if private == np.uint8:
                    ws["out32"] = _torch().empty((n, h, w), dtype=_torch().int32, device=ops.device)
            elif opt.clusters:
                _stage_buffers(ops, opt, ws, "nd", n, h, w)
                if opt.n_regions > 0:
                    _stage_buffers(ops, opt, ws, "rt", n, h, w)
                if private == np.uint8:
                    ws["out32"] = _torch().empty((n, h, w), dtype=_torch().int32, device=ops.device)
            ws["scratch"] = ops.gabor_scratch(n, h, w)
        return ws

    def _workspace(self, g, h, w, mode):
        """``_tail_workspace`` behind a cache of the most recent shapes, with the slab placed (``_place_slab``)."""
        key = (g, h, w, mode)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._tail_workspace(g, h, w, mode)
            self._place_slab(ws, g, h, w, g if mode == "per_image" else 1)
            # keep the eight most recent (batch, shape, mode) triples resident (a data set alternating landscape and
            # portrait batches, each with a remainder batch at its end, beside a global-codebook run, would otherwise
            # rebuild - and re-place - its workspace on every switch; 0.95 GB per 64-image entry)
            if len(self._ws) >= 8:
                self._ws.pop(next(iter(self._ws)))
            self._ws[key] = ws
        return ws

    def _place_slab(self, ws, g, h, w, n_sets):
        """Optionally pick, among ``slab_candidates`` allocations, the feature slab the Lloyd pass streams fastest.

        Measured on MI355X (tools/slab_placement.py, profiles/r2_notes.md): the SAME pass kernel on the SAME bytes runs up
        to 6-7 % faster or slower depending on which 0.9 GB allocation holds them (0.169 vs 0.180 ms, stable per allocation
        for the life of the process; the first large allocation of a process is usually a fast one, which points at how
        contiguously the driver could back it - translation reach - rather than at the addresses, which show no pattern).
        With ``slab_candidates`` > 1 that many allocations are timed once with the pass kernel itself and the fastest is
        kept; the others go back to the allocator. Off by default (1): it costs transient memory, synchronises the host
        at first use of a shape and puts extra launches into a profile. bench.py asks for 2 and reports their times."""
        n_cand = self.slab_candidates
        if not self.native or ws["feats"].numel() < (256 << 20) or n_cand <= 1:
            return
        torch = _torch()
        n_cand = min(n_cand, (24 << 30) // max(1, ws["feats"].numel()))      # at most 24 GB of candidates
        cands = [ws["feats"]]
        for _ in range(n_cand - 1):
            try:
                cands.append(self.ops.feature_slab(g, h, w))
            except torch.OutOfMemoryError:       # a job that fits with one slab must not fail here
                break
        if len(cands) < 2:
            return
        best = [float("inf")] * len(cands)
        with torch.cuda.device(self.ops.device):
            for s in cands:
                s.zero_()                                  # defined bytes: the timing must not depend on stale data
            for rnd in range(3):
                for i, s in enumerate(cands):
                    for rev in (False, True):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        self.ops.assign_accumulate(s, ws["cent"], g, h, w, self.k, n_sets, ws["labels"], ws["partials"],
                                                   reverse=rev)
                        e1.record()
                        e1.synchronize()
                        if rnd and rev:
                            best[i] = min(best[i], e0.elapsed_time(e1))
        keep = min(range(len(cands)), key=lambda i: best[i])
        ws["feats"] = cands[keep]
        del cands                                          # the rejected slabs return to torch's caching allocator
        self.slab_placement_ms = best                      # diagnostics (bench.py prints it)

    def group_size(self, b, h, w, mode):
        if mode == "global":
            return b
        per_image = self.ops.lib.gcs_feature_slab_bytes(1, h, w, self.bank.n_scales, self.bank.n_orient) \
            if self.native else 2 * self.bank.n_features * h * w
        return max(1, min(b, _SLAB_BUDGET // max(1, per_image)))

    # ---- device-resident API (used by bench.py: inputs already in HBM)
    def segment_device(self, imgs, mode="per_image", out=None, dist_group=None, group=None, codebook=None, refine=0):
        """imgs: (B,H,W,3) uint8 device tensor -> (B,H,W) int32 device tensor. ``codebook``: a ``KMeansModel`` (SPEC.md §28) in
        place of the centroids the Lloyd stage would make for itself - ``refine = 0``: frozen, the stage is one assign pass;
        ``refine = m``: m update passes from it first. See ``predict_device``."""
        torch = _torch()
        self._check_args(imgs, mode, dist_group=dist_group, kind="tensor")
        imgs = imgs.contiguous()
        b, h, w, _ = imgs.shape
        opt = self._opt
        if codebook is not None:
            codebook, refine = self._codebook_check(codebook, b, mode, refine, dist_group)
            opt = opt._replace(n_iter=refine + 1)
        if self.native and imgs.device != self.ops.device:
            raise ValueError(f"imgs live on {imgs.device}, this Segmenter on {self.ops.device}")
        if out is None:
            out = torch.empty((b, h, w), dtype=torch.int32, device=imgs.device)
        elif out.dtype != torch.int32 or tuple(out.shape) != (b, h, w) or out.device != imgs.device \
                or not out.is_contiguous():
            raise ValueError("out must be a contiguous (B,H,W) int32 tensor on the device of imgs")
        g = group or self.group_size(b, h, w, mode)
        with self._device():
            for g0 in range(0, b, g):
                n = min(g, b - g0)
                ws = self._workspace(n, h, w, mode) if n == g else self._tail_workspace(n, h, w, mode)
                _step_features(self.ops, self._opt, ws, imgs[g0:g0 + n], n, h, w)
                _step_cluster(self.ops, opt, ws, out[g0:g0 + n], n, h, w, mode, self.debug, dist_group,
                              **({} if codebook is None else {"init": self._codebook_init(codebook, g0, n)}))
                self._note_plane(ws)
            if not self._post_passes:                      # (SPEC.md §18: the step's map is connected and numbered as §7 numbers)
                return out
            if self.min_region_size > 0:
                regions = torch.empty_like(out)
                self.ops.merge_small_regions(out, self.min_region_size, regions)
                out.copy_(regions)
            elif self.connectivity:
                regions = torch.empty_like(out)
                self.ops.connected_regions(out, regions)
                out.copy_(regions)
        return out

    # ---- the k-means model (SPEC.md §28)
    def _codebook_check(self, model, b, mode, refine=0, dist_group=None):
        """The argument rules of a call that takes a codebook, before anything is launched -> (the model on the plan's device,
        ``refine`` as an int)."""
        if not isinstance(model, KMeansModel):
            raise ValueError(f"codebook must be a KMeansModel, got {type(model).__name__}")
        if self.n_superpixels > 0:
            raise ValueError("a codebook takes the place of the Lloyd stage's centroids: it needs n_superpixels = 0")
        if dist_group is not None:
            raise ValueError("a codebook does not run over a dist_group")
        m = _as_int(refine)
        if m is None or m < 0:
            raise ValueError(f"refine must be an integer >= 0, got {refine!r}")
        if model.signature != self.model_signature:
            diff = sorted(n for n in set(model.signature) | set(self.model_signature)
                          if model.signature.get(n) != self.model_signature.get(n))
            raise ValueError(f"the model was fitted in another feature space than this plan's: {', '.join(diff)} differ")
        if model.n_features != self.bank.n_features:
            raise ValueError(f"the model has {model.n_features} features, this plan's bank {self.bank.n_features}")
        if model.n_sets != 1 and (model.n_sets != b or mode != "per_image"):
            raise ValueError(f"a model of {model.n_sets} codebooks labels a batch of {model.n_sets} images in mode 'per_image', "
                             f"got {b} images in mode {mode!r}")
        return model.to(self.ops.device), m

    @staticmethod
    def _codebook_init(model, g0, n):
        """``lloyd``'s ``init`` for images [g0, g0 + n) of a batch: the model's centroids copied into the step's own (one codebook
        is broadcast over the sets), which the update passes of a warm start then change - the model never is."""
        i16 = _torch().int16
        src = model.centroids.view(i16)

        def init(cent):
            cent.copy_(src if model.n_sets == 1 else src[g0:g0 + n])
        return init

    def _model_steps(self, imgs, mode, codebook, opt, out):
        """The step on every group of a (B,H,W,3) uint8 device tensor, checked by the caller: yields (g0, n, workspace) with the
        group's slab filled and, where ``opt`` is given, its Lloyd stage run at ``opt`` into ``out`` (from ``codebook``, or from
        the init of SPEC.md §4), the final centroids in the workspace's ``cent``."""
        b, h, w, _ = imgs.shape
        g = self.group_size(b, h, w, mode)
        for g0 in range(0, b, g):
            n = min(g, b - g0)
            ws = self._workspace(n, h, w, mode) if n == g else self._tail_workspace(n, h, w, mode)
            _step_features(self.ops, self._opt, ws, imgs[g0:g0 + n], n, h, w)
            if opt is not None:
                _step_cluster(self.ops, opt, ws, out[g0:g0 + n], n, h, w, mode, self.debug,
                              **({} if codebook is None else {"init": self._codebook_init(codebook, g0, n)}))
            yield g0, n, ws

    def _model_args(self, imgs, mode, model, refine=0):
        """What the entry points of the model share in front of their first launch -> (imgs, model, refine)."""
        self._check_args(imgs, mode, kind="tensor")
        if self.n_superpixels > 0:
            raise ValueError("the k-means model is the Lloyd stage's: it needs n_superpixels = 0")
        if not hasattr(self.ops, "kmeans_evaluate"):
            raise ValueError("the k-means model needs ops that have kmeans_evaluate")
        if self.native and imgs.device != self.ops.device:
            raise ValueError(f"imgs live on {imgs.device}, this Segmenter on {self.ops.device}")
        if model is not None:
            model, refine = self._codebook_check(model, imgs.shape[0], mode, refine)
        return imgs.contiguous(), model, refine

    def fit_device(self, imgs, mode="global", init=None, n_init=1):
        """(B,H,W,3) uint8 device tensor -> the ``KMeansModel`` of the plan's own step on it (SPEC.md §28): the centroids the Lloyd
        loop ends on - one codebook in mode "global", B in "per_image" - with the count and the inertia of every cluster under
        them, from one evaluate launch on the slab the step left in its workspace. ``init``: a model to start the loop from in
        place of the plan's own start (the plan's ``n_iter`` passes either way). ``n_init = n > 1`` (SPEC.md §29; a plan with
        ``init = "kmeans++"``, no ``init`` model): n loops on the same slab from the seeds of ``seed``, ``seed + 1``, ...; every set
        keeps the loop whose inertias sum to the least (ties: the lowest restart), chosen on the device, and
        ``predict_device(imgs, model)`` delivers that loop's labels."""
        torch = _torch()
        n_init = _as_int(n_init)
        if n_init is None or n_init < 1:
            raise ValueError("n_init must be an integer >= 1")
        if n_init > 1 and (init is not None or not self._seeding):
            raise ValueError('n_init > 1 restarts the seeding: it needs a plan with init = "kmeans++" and no init model')
        imgs, init, _ = self._model_args(imgs, mode, init)
        b, h, w, _ = imgs.shape
        n_sets = b if mode == "per_image" else 1
        with self._device():
            labels = torch.empty((b, h, w), dtype=torch.int32, device=imgs.device)
            cent = torch.empty((n_sets, self.k, self.bank.n_features), dtype=torch.int16, device=imgs.device)
            stats = torch.empty((n_sets, self.k, 2), dtype=torch.int64, device=imgs.device)
            for g0, n, ws in self._model_steps(imgs, mode, init, self._model_opt, labels):
                ns = n if mode == "per_image" else 1
                cent[g0:g0 + ns].copy_(ws["cent"])
                self.ops.kmeans_evaluate(ws["feats"], ws["cent"], n, h, w, self.k, ns, stats=stats[g0:g0 + ns])
                for i in range(1, n_init):                 # the restarts, on the slab the first loop filled
                    again = torch.empty((ns, self.k, 2), dtype=torch.int64, device=imgs.device)
                    opt = self._model_opt._replace(seed=((self.seed + i) & _U64, self.seed_trials))
                    _step_cluster(self.ops, opt, ws, labels[g0:g0 + n], n, h, w, mode, self.debug)
                    self.ops.kmeans_evaluate(ws["feats"], ws["cent"], n, h, w, self.k, ns, stats=again)
                    better = again[:, :, 1].sum(dim=1) < stats[g0:g0 + ns, :, 1].sum(dim=1)      # strictly: ties keep the earlier
                    cent[g0:g0 + ns] = torch.where(better[:, None, None], ws["cent"], cent[g0:g0 + ns])
                    stats[g0:g0 + ns] = torch.where(better[:, None, None], again, stats[g0:g0 + ns])
        return KMeansModel(cent, stats[..., 0].contiguous(), stats[..., 1].contiguous(), self.model_signature)

    def seed_device(self, imgs, mode="per_image", seed=None, trials=None, stride=None):
        """(B,H,W,3) uint8 device tensor -> the ``KMeansModel`` of the k-means++ seeds of SPEC.md §29 themselves, before any Lloyd
        pass: one codebook per image, or one for the batch in mode "global", with the counts and inertias of one evaluate launch.
        ``seed``, ``trials``: the plan's ``seed`` and ``seed_trials`` unless given; ``stride``: ``seed_stride`` of each group unless
        given. Works on any plan with ``n_superpixels = 0``, whatever its ``init``."""
        torch = _torch()
        seed, trials = _check_seeding("kmeans++", self.seed if seed is None else seed, self.seed_trials if trials is None else trials)
        if stride is not None and (_as_int(stride) is None or not 1 <= stride <= 4096 or stride & (stride - 1)):
            raise ValueError(f"stride must be a power of two in 1..4096, got {stride!r}")
        imgs, _, _ = self._model_args(imgs, mode, None)
        if not hasattr(self.ops, "kmeans_seed"):
            raise ValueError("seed_device needs ops that have kmeans_seed")
        b, h, w, _ = imgs.shape
        n_sets = b if mode == "per_image" else 1
        if stride is None:
            seed_stride(b if mode == "global" else 1, h, w)            # (ValueError before any launch)
        with self._device():
            cent = torch.empty((n_sets, self.k, self.bank.n_features), dtype=torch.int16, device=imgs.device)
            stats = torch.empty((n_sets, self.k, 2), dtype=torch.int64, device=imgs.device)
            for g0, n, ws in self._model_steps(imgs, mode, None, None, None):
                ns = n if mode == "per_image" else 1
                _seed_init(self.ops, ws["feats"], n, h, w, self.k, ns, seed, trials, stride)(ws["cent"])
                cent[g0:g0 + ns].copy_(ws["cent"])
                self.ops.kmeans_evaluate(ws["feats"], ws["cent"], n, h, w, self.k, ns, stats=stats[g0:g0 + ns])
        return KMeansModel(cent, stats[..., 0].contiguous(), stats[..., 1].contiguous(), self.model_signature)

    def predict_device(self, imgs, model, refine=0, mode="per_image", out=None):
        """(B,H,W,3) uint8 device tensor -> (B,H,W) int32 labels under ``model`` (SPEC.md §28): the feature stages, then the Lloyd
        stage started from a copy of the model's centroids with ``n_iter = refine + 1`` - ``refine = 0`` is ONE assign pass with
        the codebook as it is, so cluster ids mean the same from call to call. A one-codebook model is shared by every image;
        ``refine = m > 0`` with ``mode = "per_image"`` lets every image refine its own copy, with "global" one copy is refined over
        the batch. A model of B codebooks labels image i of a batch of B with codebook i. The plan's post-passes and
        ``tree_nodes = "clusters"`` run as they do without a codebook. ValueError: ``n_superpixels > 0``, a model whose signature
        is not the plan's, a B-codebook model on a batch of another size or in mode "global"."""
        return self.segment_device(imgs, mode, out, codebook=model, refine=refine)

    def evaluate_device(self, imgs, model=None, mode="per_image", labels=True, best=False, second=False, stats=True):
        """(B,H,W,3) uint8 device tensor -> dict of the outputs of SPEC.md §28 that were asked for: ``labels`` (B,H,W) int32,
        ``best`` and ``second`` (B,H,W) int64, ``stats`` (n_sets, k, 2) int64 = (count, inertia), measured against ``model``'s
        codebooks as they are, or, without one, against the centroids the plan's own Lloyd loop ends on in ``mode``."""
        torch = _torch()
        if not (labels or best or second or stats):
            raise ValueError("evaluate_device needs at least one of labels, best, second and stats")
        imgs, model, _ = self._model_args(imgs, mode, model)
        b, h, w, _ = imgs.shape
        n_sets = model.n_sets if model is not None else (b if mode == "per_image" else 1)
        res = {}
        with self._device():
            new = lambda dt: torch.empty((b, h, w), dtype=dt, device=imgs.device)
            for name, on, dt in (("labels", labels, torch.int32), ("best", best, torch.int64), ("second", second, torch.int64)):
                if on:
                    res[name] = new(dt)
            if stats:
                res["stats"] = torch.zeros((n_sets, self.k, 2), dtype=torch.int64, device=imgs.device)
            own = new(torch.int32) if model is None else None
            for g0, n, ws in self._model_steps(imgs, mode, None, self._model_opt if model is None else None, own):
                if model is None:
                    cent, ns = ws["cent"], n if mode == "per_image" else 1
                else:
                    ns = 1 if n_sets == 1 else n
                    cent = model.centroids.view(torch.int16)[0 if n_sets == 1 else g0:][:ns]
                part = torch.empty((ns, self.k, 2), dtype=torch.int64, device=imgs.device) if stats else None
                self.ops.kmeans_evaluate(ws["feats"], cent, n, h, w, self.k, ns, stats=part,
                                         **{name: res[name][g0:g0 + n] for name in ("labels", "best", "second") if name in res})
                if stats:                                  # (one codebook over several groups: the groups' tables add up)
                    res["stats"][0 if n_sets == 1 else g0:][:ns] += part
        return res

    def confidence_device(self, imgs, model=None, mode="per_image"):
        """(B,H,W,3) uint8 device tensor -> (labels (B,H,W) int32, confidence (B,H,W) float32 in [0, 1]) of SPEC.md §28:
        (second - best) / second in float64, 0 where second = 0 - 0 for a pixel as close to another centroid as to its own, 1 for a
        pixel on its centroid. ``model``, ``mode``: as in ``evaluate_device``."""
        res = self.evaluate_device(imgs, model, mode, labels=True, best=True, second=True, stats=False)
        return res["labels"], confidence_of(res["best"], res["second"])

    # ---- the regulariser (SPEC.md §30)
    def kmeans_costs_device(self, imgs, model=None, mode="per_image"):
        """(B,H,W,3) uint8 device tensor -> (costs (B,k,H,W) int64, labels (B,H,W) int32, stats (n_sets,k,2) int64): the cost
        volume of SPEC.md §30 - the squared distance of every pixel to every centroid - under ``model``'s codebooks as they are or,
        without one, under the centroids the plan's own Lloyd loop ends on in ``mode``, with the labels and the table of SPEC.md
        §28 (``labels`` is the argmin of ``costs`` over j, ties to the lowest j). Ignores the plan's ``regularize``."""
        torch = _torch()
        imgs, model, _ = self._model_args(imgs, mode, model)
        if not hasattr(self.ops, "kmeans_costs"):
            raise ValueError("the cost volume needs ops that have kmeans_costs")
        b, h, w, _ = imgs.shape
        n_sets = model.n_sets if model is not None else (b if mode == "per_image" else 1)
        plain = self._model_opt._replace(clusters=False, n_regions=0)    # (the loop alone: no node map, no tree)
        with self._device():
            costs = torch.empty((b, self.k, h, w), dtype=torch.int64, device=imgs.device)
            labels = torch.empty((b, h, w), dtype=torch.int32, device=imgs.device)
            stats = torch.zeros((n_sets, self.k, 2), dtype=torch.int64, device=imgs.device)
            own = torch.empty_like(labels) if model is None else None
            for g0, n, ws in self._model_steps(imgs, mode, None, plain if model is None else None, own):
                if model is None:
                    cent, ns = ws["cent"], n if mode == "per_image" else 1
                else:
                    ns = 1 if n_sets == 1 else n
                    cent = model.centroids.view(torch.int16)[0 if n_sets == 1 else g0:][:ns]
                part = torch.empty((ns, self.k, 2), dtype=torch.int64, device=imgs.device)
                self.ops.kmeans_evaluate(ws["feats"], cent, n, h, w, self.k, ns, labels=labels[g0:g0 + n], stats=part)
                self.ops.kmeans_costs(ws["feats"], cent, n, h, w, self.k, ns, costs[g0:g0 + n])
                stats[0 if n_sets == 1 else g0:][:ns] += part    # (one codebook over several groups: the groups' tables add up)
        return costs, labels, stats

    def relax_labels_device(self, costs, labels, beta, sweeps=4, neighbours=8):
        """SPEC.md §30 on any cost volume: ``costs`` (B,k,H,W) int64 in 0 .. 2^62 - 1, ``labels`` (B,H,W) int32 (a value outside
        0..k-1 is "no label"), ``beta`` an integer or a (B,) int64 tensor -> (labels (B,H,W) int32 after ``sweeps`` (0..64) sweeps
        over ``neighbours`` (4 or 8), changed (B, sweeps) int32, energy (B, 2) int64 = (unary, pairs) of the delivered map). The
        inputs are not changed. Ignores the plan's options: k is the volume's."""
        torch = _torch()
        if not hasattr(self.ops, "label_relax"):
            raise ValueError("relax_labels_device needs ops that have label_relax")
        s, n = _as_int(sweeps), _as_int(neighbours)
        if s is None or not 0 <= s <= 64:
            raise ValueError(f"sweeps must be an integer in 0..64, got {sweeps!r}")
        if n not in (4, 8):
            raise ValueError(f"neighbours must be 4 or 8, got {neighbours!r}")
        if costs.dtype != torch.int64 or costs.ndim != 4 or not 1 <= costs.shape[1] <= _lib.K_MAX:
            raise ValueError("costs must be a (B,k,H,W) int64 tensor with k in 1..16")
        b, k, h, w = costs.shape
        if labels.dtype != torch.int32 or tuple(labels.shape) != (b, h, w) or labels.device != costs.device:
            raise ValueError("labels must be a (B,H,W) int32 tensor on the device of costs")
        if not (1 <= b <= 65535 and 1 <= h <= 4096 and 1 <= w <= 4096):
            raise ValueError("relax_labels_device takes 1..65535 images of 1..4096 rows and columns")
        if not isinstance(beta, torch.Tensor):
            if _as_int(beta) is None:
                raise ValueError(f"beta must be an integer or a (B,) int64 tensor, got {beta!r}")
            beta = torch.full((b,), _as_int(beta), dtype=torch.int64, device=costs.device)
        elif beta.dtype != torch.int64 or tuple(beta.shape) != (b,) or beta.device != costs.device:
            raise ValueError("beta must be an integer or a (B,) int64 tensor on the device of costs")
        with self._device():
            out = torch.empty((b, h, w), dtype=torch.int32, device=costs.device)
            changed = torch.empty((b, s), dtype=torch.int32, device=costs.device)
            energy = torch.empty((b, 2), dtype=torch.int64, device=costs.device)
            work = torch.empty((b, h, w), dtype=torch.int32, device=costs.device)
            self.ops.label_relax(costs.contiguous(), beta.contiguous(), b, h, w, k, n, s, labels.contiguous(), out, workspace=work,
                                 changed=changed, energy=energy)
        return out, changed, energy

    def _superpixel_check(self, h, w, mode="per_image", out_dtype=None, dist_group=None):
        """The argument rules of SPEC.md §13 for one image shape (``h`` None: only those that need no shape), before anything is
        launched; returns (ny, nx)."""
        if mode != "per_image":
            raise ValueError("n_superpixels > 0: centres are per image, mode must be 'per_image'")
        if dist_group is not None:
            raise ValueError("n_superpixels > 0 does not run over a dist_group")
        if h is None:
            return None
        if h > _SP_SIDE_MAX or w > _SP_SIDE_MAX:
            raise ValueError(f"n_superpixels > 0 needs images of at most {_SP_SIDE_MAX} x {_SP_SIDE_MAX} pixels")
        _, ny, nx = superpixel_grid(h, w, self.n_superpixels)
        if ny * nx > SUPERPIXELS_MAX:
            raise ValueError(f"n_superpixels = {self.n_superpixels} on {h} x {w} pixels gives a grid of {ny} x {nx} centres, "
                             f"more than {SUPERPIXELS_MAX}")
        n_labels = min(ny * nx, self.n_regions) if self.n_regions > 0 else ny * nx      # SPEC.md §14: a cut has min(alive, R) labels
        if self._components:
            n_labels = self.n_regions                      # SPEC.md §18: min(nodes, R); uint8 without R was refused in _check_args
        if out_dtype is not None and np.dtype(out_dtype) == np.uint8 and n_labels > 256:
            raise ValueError(f"out_dtype uint8 cannot hold the {n_labels} labels of this superpixel grid")
        return ny, nx

    def _cluster_check(self, h, w, mode="per_image", dist_group=None):
        """The argument rules of SPEC.md §21 (``h`` None: only those that need no shape), before anything is launched: the tree is
        per image, so one rank's global codebook is fine and a group of ranks is not."""
        if dist_group is not None:
            raise ValueError('tree_nodes = "clusters" does not run over a dist_group')
        if mode == "global":
            import torch.distributed as td
            if td.is_available() and td.is_initialized() and td.get_world_size() > 1:
                raise ValueError('tree_nodes = "clusters" with mode "global" runs on one rank only')
        if h is not None and (h > _SP_SIDE_MAX or w > _SP_SIDE_MAX):
            raise ValueError(f'tree_nodes = "clusters" needs images of at most {_SP_SIDE_MAX} x {_SP_SIDE_MAX} pixels')

    def _note_plane(self, ws):
        """SPEC.md §23: the step that has just run left the edge map of its batch in its tree stage; ``segment_regions`` takes it
        from there instead of computing it again (it is valid until the next step on the same workspace). ``segment_regions``
        clears the note before its call and takes it once behind it, so a host path that leaves no note costs one ``edges_device``
        and never a plane of another image."""
        if self._boundary and ws.get("rt") is not None:
            self._last_plane = ws["rt"][0]["grad"]

    def _tree_buffers(self, b, h, w, K):
        return (self.ops.region_tree_edges_buffers if self._boundary else self.ops.region_tree_buffers)(b, h, w, K)

    def _cluster_maps(self, imgs, tree):
        """The step of SPEC.md §21 on a (B,H,W,3) uint8 device tensor without a cut: the fresh int32 node map and the workspace;
        ``tree``: the uncut tree is in its ``"rt"``, built behind one read of the batch's node counts at K = the largest of them
        rounded up to a multiple of 64 (as ``_superpixel_maps`` does for SPEC.md §18)."""
        torch = _torch()
        self._check_args(imgs, kind="tensor")
        imgs = imgs.contiguous()
        b, h, w, _ = imgs.shape
        with self._device():
            ws = self._tail_workspace(b, h, w, "per_image")
            _step_features(self.ops, self._opt, ws, imgs, b, h, w)
            out = torch.empty((b, h, w), dtype=torch.int32, device=imgs.device)
            _step_cluster(self.ops, self._opt, ws, out, b, h, w, "per_image", self.debug, tree=False)
            if tree:
                K = min(NODES_MAX, -(-int(ws["nd"][2].max()) // 64) * 64)
                ws["rt"] = self._tree_buffers(b, h, w, K)
                _step_tree(self.ops, self._opt, ws, ws["rt"], out, b, h, w, K)
        return out, ws

    def _superpixel_maps(self, imgs, tree, centres=False, nodes=None):
        """The step on a (B,H,W,3) uint8 device tensor with SPEC.md §13 as its second piece and no post-passes: the fresh int32 §13
        map (the node map of SPEC.md §18 in that mode, unless ``nodes=False``), the workspace (``tree``: the uncut tree of SPEC.md
        §14 is in its ``"rt"``) and, if asked for, the centres. In the mode of §18 the tree is built here, behind one read of the
        batch's node counts, at K = the largest of them rounded up to a multiple of 64 (the tree does not depend on K beyond
        capacity): merge list and the sweeps' tables stay as small as the batch allows."""
        torch = _torch()
        self._check_args(imgs, kind="tensor")
        imgs = imgs.contiguous()
        b, h, w, _ = imgs.shape
        _, ny, nx = superpixel_grid(h, w, self.n_superpixels)
        with self._device():
            ws = self._tail_workspace(b, h, w, "per_image")
            _step_features(self.ops, self._opt, ws, imgs, b, h, w)
            out = torch.empty((b, h, w), dtype=torch.int32, device=imgs.device)
            centres = torch.empty((b, ny * nx, self.bank.n_features + 2), dtype=torch.int32, device=imgs.device) if centres else None
            trim = tree and self._components and nodes is None
            _step_cluster(self.ops, self._opt, ws, out, b, h, w, "per_image", self.debug, centres=centres,
                          tree=False if trim else tree, nodes=nodes)
            if trim:
                K = min(NODES_MAX, -(-int(ws["nd"][2].max()) // 64) * 64)
                ws["rt"] = self._tree_buffers(b, h, w, K)
                _step_tree(self.ops, self._opt, ws, ws["rt"], out, b, h, w, K, ws["sp"][0])
        return out, ws, centres

    def region_tree_device(self, imgs):
        """(B,H,W,3) uint8 device tensor -> (labels (B,H,W) int32: the §13 map; merges (B, K-1, 2) int32; costs (B, K-1) int64: the
        unsigned 64-bit costs, all below 2^62; alive (B,) int32) of SPEC.md §14, K = ny * nx: no cut, no post-passes. Any
        ``n_regions`` of the plan is ignored; ``cut_regions_device`` cuts the tree at any R for the cost of a relabel. With
        ``tree_nodes = "components"`` (SPEC.md §18) ``labels`` is the node map N and K the batch's largest node count rounded up to
        a multiple of 64 (one read of B integers from the device): the first rows of the tree at K_cap. With ``tree_nodes =
        "clusters"`` (SPEC.md §21) the same, on the node map of the k-means map."""
        if self._clusters:                                 # SPEC.md §21: the node map of the k-means map, the tree from the slab
            if not hasattr(self.ops, "region_tree_edges" if self._boundary else "region_tree_slab"):
                raise ValueError("region_tree_device needs ops that have the region tree")
            out, ws = self._cluster_maps(imgs, tree=True)
            return (out,) + ws["rt"][1:]
        if self.n_superpixels == 0:
            raise ValueError("region_tree_device needs Segmenter(n_superpixels=n) with n > 0")
        if not hasattr(self.ops, "region_tree_edges" if self._boundary else "region_tree"):
            raise ValueError("region_tree_device needs ops that have the region tree")
        out, ws, _ = self._superpixel_maps(imgs, tree=True)
        return (out,) + ws["rt"][1:]

    def cut_regions_device(self, labels, merges, alive, R):
        """The cut of SPEC.md §14 at ``R`` (1..4096) of a tree ``region_tree_device`` returned: a fresh (B,H,W) int32 label map with
        min(alive, R) labels per image, numbered in increasing order of each group's smallest superpixel index."""
        torch = _torch()
        R = _check_regions(R, 1)
        if R == 0:
            raise ValueError("R must be in 1..4096")
        b, h, w = labels.shape
        out = torch.empty_like(labels)
        with self._device():
            self.ops.region_tree_cut(labels, merges, alive, b, h, w, merges.shape[1] + 1, R, out)
        return out

    def contour_map_device(self, labels, merges, alive, out=None):
        """The contour map of SPEC.md §15 of a tree ``region_tree_device`` returned (or of any label map and merge list of that
        form): a (B,H,W) int32 tensor, 0 inside the regions of the finest cut and, on a boundary pixel, the level in 1 .. alive at
        which that boundary disappears: ``contours > max(0, alive - R)`` is the thick boundary map of the cut at R. It describes
        the raw cuts: ``connectivity`` and ``min_region_size`` are not reflected (with ``tree_nodes = "components"``, SPEC.md §18, the
        delivered maps are the raw cuts). ``out``: a tensor to fill (not ``labels``)."""
        torch = _torch()
        if not hasattr(self.ops, "region_tree_contours"):
            raise ValueError("contour_map_device needs ops that have the contour map")
        if labels.dim() != 3 or labels.dtype != torch.int32:
            raise ValueError("labels must be a (B,H,W) int32 tensor")
        b, h, w = labels.shape
        if merges.dim() != 3 or merges.shape[0] != b or merges.shape[2] != 2 or not 1 <= merges.shape[1] + 1 <= SUPERPIXELS_MAX:
            raise ValueError(f"merges must be a (B, K - 1, 2) int32 tensor with K in 1..{SUPERPIXELS_MAX}")
        if tuple(alive.shape) != (b,):
            raise ValueError("alive must be a (B,) int32 tensor")
        if h > _SP_SIDE_MAX or w > _SP_SIDE_MAX or b > 65535:
            raise ValueError(f"the contour map takes at most 65535 images of at most {_SP_SIDE_MAX} x {_SP_SIDE_MAX} pixels")
        K = merges.shape[1] + 1
        if out is None:
            out = torch.empty_like(labels)
        with self._device():
            # (the workspace comes from and goes back to the stream-ordered allocator: no state a second stream could share)
            self.ops.region_tree_contours(labels, merges, alive, b, h, w, K, self.ops.contour_buffers(b, K), out)
        return out

    def contours_device(self, imgs):
        """(B,H,W,3) uint8 device tensor -> (contours (B,H,W) int32, alive (B,) int32): features, superpixels (SPEC.md §13), tree
        (§14), contour map (§15). Needs ``Segmenter(n_superpixels=n)``; any ``n_regions`` of the plan is ignored."""
        if not hasattr(self.ops, "region_tree_contours"):
            raise ValueError("contours_device needs ops that have the contour map")
        labels, merges, _, alive = self.region_tree_device(imgs)
        return self.contour_map_device(labels, merges, alive), alive

    # ---- SPEC.md §19: descriptors and mean-colour pictures of the regions of a map and of the cuts of a tree
    def _need_props(self):
        if not hasattr(self.ops, "region_props"):
            raise ValueError("the region descriptors need ops that have them")

    def region_props_device(self, imgs, labels, K=None, features=False):
        """(B,H,W,3) uint8 and (B,H,W) int32 device tensors -> the leaf table of SPEC.md §19: ``(sums (B, K, 6 + D) int64, bbox
        (B, K, 4) int32)``: per label the bits of the uint64 columns n, sum y, sum x, sum R, sum G, sum B (and, with
        ``features=True``, the sums of the plan's D canonical features, made from ``imgs`` as ``features_device`` makes them; D = 0
        otherwise) and the inclusive box (y0, x0, y1, x1), (H, W, -1, -1) for a label that owns no pixel. ``K=None``: one read of
        ``labels.max()`` from the device. Any label map will do: a k-means map, its connected regions, a tree's leaves, a cut."""
        torch = _torch()
        self._need_props()
        if labels.dim() != 3 or labels.dtype != torch.int32 or imgs.dim() != 4 or tuple(imgs.shape) != tuple(labels.shape) + (3,):
            raise ValueError("labels must be a (B,H,W) int32 tensor and imgs the (B,H,W,3) uint8 tensor of the same images")
        imgs, labels = imgs.contiguous(), labels.contiguous()
        b, h, w = labels.shape
        with self._device():
            K = max(1, int(labels.max()) + 1) if K is None else int(K)
            canon = self.features_device(imgs) if features else None
            d = self.bank.n_features if features else 0
            if K < 1 or b * K * (6 + d) >= 2 ** 31:
                raise ValueError("K must be at least 1 and B * K * (6 + D) below 2^31")
            sums = torch.empty((b, K, 6 + d), dtype=torch.int64, device=labels.device)
            bbox = torch.empty((b, K, 4), dtype=torch.int32, device=labels.device)
            self.ops.region_props(labels, imgs, canon, b, h, w, K, sums, bbox)
        return sums, bbox

    def cut_props_device(self, sums, bbox, merges, alive, regions, shape=None):
        """The tables of every requested cut from the leaf table, without reading a pixel (SPEC.md §19). sums, bbox: what
        ``region_props_device`` returned for the map and the K of ``region_tree_device``; merges, alive: that tree; regions: 1 .. 64
        distinct integers in 1 .. 4096, in any order. Returns ``(group (n, B, K) int32, sums_out (B, Rsum, C) int64, bbox_out
        (B, Rsum, 4) int32, offsets)``, device tensors and a list of n integers, in the caller's order of ``regions``: ``group[j][b][q]``
        is the label ``cut_regions_device(..., regions[j])`` gives the leaf q (-1: q owns no pixel), and the rows ``offsets[j] ..
        offsets[j] + min(K, regions[j]) - 1`` of sums_out / bbox_out are that cut's table (rows behind its groups: zeros, the empty
        box). ``shape``: (H, W) of the images, for the empty box; default: the leaf table's own empty box, or (0, 0)."""
        torch = _torch()
        from .evaluate_gpu import _need_cuts
        self._need_props()
        regs, order = _need_cuts(regions)
        if sums.dim() != 3 or merges.dim() != 3 or merges.shape[1] + 1 != sums.shape[1]:
            raise ValueError("sums must be the (B, K, C) leaf table of the tree's label map: K = merges.shape[1] + 1")
        b, K, _ = sums.shape
        srt = [regs[j] for j in order]
        starts = np.concatenate([[0], np.cumsum([min(K, r) for r in srt])])
        with self._device():
            if shape is None:
                empty = bbox[:, :, 2] < 0
                shape = (int(bbox[:, :, 0][empty].max()), int(bbox[:, :, 1][empty].max())) if bool(empty.any()) else \
                    (int(bbox[:, :, 2].max()) + 1, int(bbox[:, :, 3].max()) + 1)
            h, w = (max(1, int(v)) for v in shape)
            regs_d = torch.tensor(srt, dtype=torch.int32).to(sums.device)
            group = torch.empty((len(srt), b, K), dtype=torch.int32, device=sums.device)
            sums_out = torch.empty((b, int(starts[-1]), sums.shape[2]), dtype=torch.int64, device=sums.device)
            bbox_out = torch.empty((b, int(starts[-1]), 4), dtype=torch.int32, device=sums.device)
            self.ops.region_props_cuts(sums.contiguous(), bbox.contiguous(), merges.contiguous(), alive.contiguous(), regs_d, b, h, w,
                                       K, group, sums_out, bbox_out)
            inverse = np.empty(len(order), np.int64)
            inverse[order] = np.arange(len(order))                 # the caller's j-th R is the inverse[j]-th cut of the call
            group = group[torch.from_numpy(inverse).to(sums.device)]
        return group, sums_out, bbox_out, [int(starts[i]) for i in inverse]

    def paint_device(self, labels, sums, group=None):
        """The mean-colour picture of SPEC.md §19: (B,H,W) int32 labels -> a fresh (B,H,W,3) uint8 device tensor. ``sums``: a table
        whose rows the labels name (``group`` None: the leaf table of this map) or the rows of one cut (``sums_out[:, o : o + rows]``,
        read in place) with ``group`` (B, K) int32, that cut's slice of ``cut_props_device``. Black where a label is out of range or its row is empty."""
        torch = _torch()
        self._need_props()
        if labels.dim() != 3 or labels.dtype != torch.int32 or sums.dim() != 3:
            raise ValueError("labels must be a (B,H,W) int32 tensor and sums a (B, G, C) int64 tensor")
        b, h, w = labels.shape
        K = int(sums.shape[1]) if group is None else int(group.shape[-1])
        out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=labels.device)
        with self._device():
            self.ops.region_paint(labels.contiguous(), None if group is None else group.contiguous(), sums, b, h, w, K, out)
        return out

    # ---- SPEC.md §20: which regions touch, and along how much boundary
    def _need_adjacency(self):
        if not hasattr(self.ops, "region_adjacency"):
            raise ValueError("the region adjacency graph needs ops that have it")

    def region_adjacency_device(self, labels, K=None, imgs=None, strength=None, capacity=None):
        """(B,H,W) int32 device tensor -> the edge table of SPEC.md §20, ``(edges (B, capacity, 2) int32, vals (B, capacity, 3) int64,
        count (B,) int32)``: per image ``count`` rows (a, b), a < b, sorted, with the bits of the uint64 columns length (pixel pairs
        across the boundary), contrast (their summed squared colour difference; 0 without ``imgs``, the (B,H,W,3) uint8 images) and
        strength (the summed values, negatives as 0, of ``strength``, a (B,H,W) int32 plane, on both sides; 0 without); rows behind
        them hold (-1, -1) and zeros, and an image with more than ``capacity`` edges has count -1. ``K=None``: one read of
        ``labels.max()`` from the device. ``capacity=None``: min(16384, max(64, 4 K), K (K - 1) / 2 or 1, 2HW - H - W or 1)."""
        torch = _torch()
        self._need_adjacency()
        if labels.dim() != 3 or labels.dtype != torch.int32:
            raise ValueError("labels must be a (B,H,W) int32 tensor")
        labels = labels.contiguous()
        b, h, w = labels.shape
        with self._device():
            K = max(1, int(labels.max()) + 1) if K is None else int(K)
            if K < 1:
                raise ValueError("K must be at least 1")
            if capacity is None:
                capacity = min(16384, max(64, 4 * K), K * (K - 1) // 2 or 1, 2 * h * w - h - w or 1)
            cap = int(capacity)
            if not 1 <= cap <= 16384:
                raise ValueError("capacity must be in 1 .. 16384")
            edges = torch.empty((b, cap, 2), dtype=torch.int32, device=labels.device)
            vals = torch.empty((b, cap, 3), dtype=torch.int64, device=labels.device)
            count = torch.empty((b,), dtype=torch.int32, device=labels.device)
            self.ops.region_adjacency(labels, None if imgs is None else imgs.contiguous(),
                                      None if strength is None else strength.contiguous(), b, h, w, K,
                                      self.ops.adjacency_buffers(b, cap), edges, vals, count)
        return edges, vals, count

    def cut_adjacency_device(self, edges, vals, count, group, G=None, capacity=None):
        """The edge tables of cuts from the leaf table, without reading a pixel (SPEC.md §20). edges, vals, count: what
        ``region_adjacency_device`` returned for the leaf map; ``group`` (n_cuts, B, K) int32 as ``cut_props_device`` returns it (or
        any relabelling of the K leaves; entries outside 0 .. G-1 drop their leaf). ``G``: the number of groups, default K.
        ``capacity``: default min(the leaf table's, G (G - 1) / 2 or 1). Returns ``(edges (n_cuts, B, capacity, 2), vals (n_cuts, B, capacity, 3), count
        (n_cuts, B))`` in the same format: the graph of the map ``cut_regions_device`` writes at that cut."""
        torch = _torch()
        self._need_adjacency()
        if group.dim() != 3 or edges.dim() != 3 or group.shape[1] != edges.shape[0]:
            raise ValueError("group must be an (n_cuts, B, K) int32 tensor and edges the (B, capacity, 2) leaf table of the same images")
        n, b, K = group.shape
        G = K if G is None else int(G)
        cap = min(int(edges.shape[1]), G * (G - 1) // 2 or 1) if capacity is None else int(capacity)
        if G < 1 or not 1 <= cap <= 16384:
            raise ValueError("G must be at least 1 and capacity in 1 .. 16384")
        with self._device():
            edges_out = torch.empty((n, b, cap, 2), dtype=torch.int32, device=edges.device)
            vals_out = torch.empty((n, b, cap, 3), dtype=torch.int64, device=edges.device)
            count_out = torch.empty((n, b), dtype=torch.int32, device=edges.device)
            self.ops.region_adjacency_cuts(edges.contiguous(), vals.contiguous(), count.contiguous(), group.contiguous(), b, K, G,
                                           self.ops.adjacency_buffers(n * b, cap), edges_out, vals_out, count_out)
        return edges_out, vals_out, count_out

    def superpixels_device(self, imgs):
        """(B,H,W,3) uint8 device tensor -> (labels (B,H,W) int32, centres (B, ny * nx, D + 2) int32: the D features, cy, cx the
        last assign used) of SPEC.md §13, without the post-passes (tests / debugging)."""
        if self.n_superpixels == 0:
            raise ValueError("superpixels_device needs Segmenter(n_superpixels=n) with n > 0")
        out, _, centres = self._superpixel_maps(imgs, tree=False, centres=True, nodes=False)
        return out, centres

    def _opponent(self, imgs, colour):
        return _opponent(self.ops, imgs, colour)

    def _check_strips(self):
        """The options the two row-strip entry points refuse."""
        if self._relax:
            raise ValueError("regularize > 0 is not supported on row strips (a strip would need a halo of 4 rows per sweep)")
        if self._seeding:
            raise ValueError('init = "kmeans++" is not supported on row strips (the candidates would be one strip\'s)')
        if self.n_superpixels > 0:
            raise ValueError("n_superpixels > 0 is not supported on row strips")
        if self._clusters:
            raise ValueError('tree_nodes = "clusters" is not supported on row strips (regions would cross strip boundaries)')
        if self.min_region_size > 0:
            raise ValueError("min_region_size is not supported on row strips (regions would cross strip boundaries)")
        if self.smoothing > 0:
            raise ValueError("smoothing is not supported on row strips (the halo would have to grow by the smoothing radius)")

    def shard_rows(self, height, world, rank):
        """``shard_rows`` for THIS plan's bank (its pyramid depth and kernel size decide alignment and halo)."""
        return shard_rows(height, world, rank, self.bank.n_levels, self.bank.ksize)

    def segment_rows_sharded_device(self, strip, r0, r1, s0, height, dist_group=None, out=None, codebook=None):
        """Row-sharded images with one global codebook (BASELINE config 5).

        ``strip``: (B, s1-s0, W, 3) uint8 device tensor = global rows [s0, s1) of B images of
        ``height`` rows, of which this rank owns [r0, r1) (see ``shard_rows``). The halo rows
        feed the Gabor stage with real neighbour data (outer image borders still reflect, as
        SPEC.md §3 says), are excluded from every k-means sum, and are dropped from the result.
        Returns the (B, r1-r0, W) int32 labels of the owned rows; identical to the same rows of
        the unsharded result. Needs torch.distributed initialised when the image is split.
        """
        torch = _torch()
        self._check_strips()
        if codebook is not None:
            raise ValueError("a codebook is not supported on row strips (the strips' init is the exchange of SPEC.md §4's pixels)")
        strip = strip.contiguous()
        b, hs, w, _ = strip.shape
        if hs < 8 or w < 8:
            raise ValueError("strips must be at least 8x8 (including halo)")
        if not (s0 <= r0 < r1 <= s0 + hs <= height):
            raise ValueError("inconsistent strip geometry")
        align = 1 << (self.bank.n_levels - 1)
        if s0 % align or r0 % align or (r1 % align and r1 != height) or ((s0 + hs) % align and s0 + hs != height):
            raise ValueError(f"strip boundaries must be multiples of {align} rows (pyramid alignment; use shard_rows)")
        halo = halo_rows(self.bank.n_levels, self.bank.ksize)
        if (r0 - s0 < halo and s0 > 0) or (s0 + hs - r1 < halo and s0 + hs < height):
            raise ValueError(f"interior strip edges need {halo} halo rows (use shard_rows)")
        check_position_range(self.position_weight, height, w)
        ws = self._tail_workspace(b, hs, w, "global")
        # (T_g is per pixel: a strip with its halo rows transforms on its own; global coordinates: row 0 of the strip is row s0)
        _step_features(self.ops, self._opt, ws, strip, b, hs, w, y0=s0)
        k, dfeat = self.k, self.bank.n_features
        import torch.distributed as td
        use_dist = td.is_available() and td.is_initialized() and td.get_world_size(dist_group) > 1

        def init(cent):
            # SPEC.md §4: p_j = floor((2j+1) P / (2k)) over image 0 of the global batch, global coordinates
            p = height * w
            byx = []
            for j in range(k):
                pj = ((2 * j + 1) * p) // (2 * k)
                y, x = pj // w, pj % w
                byx.append((0, y - s0, x) if r0 <= y < r1 else (-1, 0, 0))
            rows_ = self.ops.features_gather(ws["feats"], b, hs, w,
                                             torch.tensor(byx, dtype=torch.int32, device=strip.device))
            table = rows_.view(torch.int16).to(torch.int32) & 0xFFFF          # uint16 values, zero if not owned
            if use_dist:
                _collective(td.all_reduce, table, op=td.ReduceOp.SUM, group=dist_group)
            cent.copy_(table.to(torch.int16).view(1, k, dfeat))               # wraps back to the uint16 bits

        full = torch.empty((b, hs, w), dtype=torch.int32, device=strip.device)
        _step_cluster(self.ops, self._opt, ws, full, b, hs, w, "global", self.debug, dist_group, rows=(r0 - s0, r1 - s0), init=init)
        res = full[:, r0 - s0:r1 - s0]
        if out is not None:
            out.copy_(res)
            return out
        return res.contiguous()

    def segment_owned_rows_device(self, owned, height, dist_group=None, codebook=None):
        """Row-sharded images where every rank holds ONLY its own rows on its device (BASELINE config 5, option (ii) of
        SURVEY §8e): the halo rows the Gabor stage needs are fetched from the neighbouring ranks device to device
        (``torch.distributed`` point-to-point: RCCL send / recv over xGMI on a multi-GPU node; gloo in the tests), then
        the strip runs through ``segment_rows_sharded_device``.

        ``owned``: (B, r1-r0, W, 3) uint8 device tensor = rows [r0, r1) of B images of ``height`` rows, with
        (r0, r1) = ``shard_rows(height, world, rank, n_levels, ksize)[:2]``. Every rank must own at least the halo
        (``halo_rows(n_levels, ksize)`` rows), so that a halo comes from ONE neighbour. Returns the (B, r1-r0, W) int32 labels."""
        torch = _torch()
        self._check_strips()
        if codebook is not None:
            raise ValueError("a codebook is not supported on row strips (the strips' init is the exchange of SPEC.md §4's pixels)")
        import torch.distributed as td
        if not (td.is_available() and td.is_initialized()):
            raise RuntimeError("segment_owned_rows_device needs torch.distributed (one rank per row strip)")
        world, rank = td.get_world_size(dist_group), td.get_rank(dist_group)
        nl, ks = self.bank.n_levels, self.bank.ksize
        r0, r1, s0, s1 = shard_rows(height, world, rank, nl, ks)
        owned = owned.contiguous()
        b, ho, w, _ = owned.shape
        if ho != r1 - r0:
            raise ValueError(f"rank {rank} owns rows [{r0}, {r1}) of {height}: got {ho} rows")
        halo = halo_rows(nl, ks)
        bounds = [shard_rows(height, world, r, nl, ks) for r in range(world)]
        if world > 1 and min(x[1] - x[0] for x in bounds) < halo:
            raise ValueError(f"every rank must own at least {halo} rows for a single-hop halo exchange")
        up, down = rank - 1, rank + 1
        gloo_host = owned.is_cuda and td.get_backend(dist_group) == "gloo"      # gloo moves host memory only

        def wire(t):
            return t.cpu() if gloo_host else t
        ops, recv_top, recv_bot = [], None, None
        peer = (lambda r: td.get_global_rank(dist_group, r)) if dist_group is not None else (lambda r: r)
        if up >= 0:                                          # my first rows are the upper neighbour's bottom halo
            ops.append(td.P2POp(td.isend, wire(owned[:, :s1_of(bounds, up) - r0].contiguous()), peer(up), dist_group))
            recv_top = torch.empty((b, r0 - s0, w, 3), dtype=torch.uint8, device="cpu" if gloo_host else owned.device)
            ops.append(td.P2POp(td.irecv, recv_top, peer(up), dist_group))
        if down < world:                                     # my last rows are the lower neighbour's top halo
            ops.append(td.P2POp(td.isend, wire(owned[:, bounds[down][2] - r0:].contiguous()), peer(down), dist_group))
            recv_bot = torch.empty((b, s1 - r1, w, 3), dtype=torch.uint8, device="cpu" if gloo_host else owned.device)
            ops.append(td.P2POp(td.irecv, recv_bot, peer(down), dist_group))
        if ops:
            for req in td.batch_isend_irecv(ops):
                req.wait()
        parts = ([recv_top.to(owned.device)] if recv_top is not None else []) + [owned] + \
                ([recv_bot.to(owned.device)] if recv_bot is not None else [])
        strip = torch.cat(parts, dim=1) if len(parts) > 1 else owned
        return self.segment_rows_sharded_device(strip, r0, r1, s0, height, dist_group)

    def features_device(self, imgs):
        """Canonical (B,D,H,W) uint16 features as an int16 tensor (tests / debugging): what the Lloyd passes consume, smoothed
        when ``smoothing`` is on."""
        self._check_args(imgs, kind="tensor", cluster=False)
        imgs = imgs.contiguous()
        b, h, w, _ = imgs.shape
        ws = self._tail_workspace(b, h, w, "per_image", slab_only=True)
        _step_features(self.ops, self._opt, ws, imgs, b, h, w)
        return _unpack(self.ops, ws, b, h, w)

    def edges_device(self, imgs, y0=0):
        """(B,H,W,3) uint8 device tensor -> (B,H,W) int32 texture-gradient edge map of SPEC.md §22: how fast the plan's features
        (``smoothing``, the colour and the position options included) change from one pixel to the next, every pyramid level
        differenced at its own resolution, read from the feature slab (the canonical tensor is never made). ``k``, ``n_iter`` and
        the region options play no part. ``y0``: only 0 - a row strip of a taller image is refused (its differences at the strip's
        edges are not the image's, and its halo rows are not the caller's)."""
        if int(y0) != 0:
            raise ValueError("edges_device is not supported on row strips (differences would be clamped at the strip's edges)")
        if not hasattr(self.ops, "feature_gradient"):
            raise ValueError("the edge map needs ops that have it")
        self._check_args(imgs, kind="tensor", cluster=False)
        imgs = imgs.contiguous()
        b, h, w, _ = imgs.shape
        with self._device():
            ws = self._tail_workspace(b, h, w, "per_image", slab_only=True)
            _step_features(self.ops, self._opt, ws, imgs, b, h, w)
            out = _torch().empty((b, h, w), dtype=_torch().int32, device=imgs.device)
            self.ops.feature_gradient(ws["feats"], b, h, w, out)
        return out

    def texton_gradient_device(self, labels, K=None, radius=8, n_directions=8, gradient=None, directions=False, thin=False):
        """(B,H,W) int32 device label map -> (B,H,W) int32 texton gradient of SPEC.md §24: the largest chi-square distance, over
        ``n_directions`` directions, between the label histograms of the two halves of a disc of ``radius`` pixels (mirrored at
        the border). ``K``: the number of labels (None: one read of ``labels.max()`` from the device; at most 64; values outside
        0 .. K-1 count in no bin). ``gradient``: a (B,H,W) int32 edge map G >= 0 (``edges_device``): the result is then
        floor(sqrt(TG * G)). ``directions=True``: returns ``(map, dir)``, dir (B,H,W) uint8 = the lowest direction of the
        maximum, 0 where TG = 0. ``thin=True``: the map is thinned along ``dir`` (SPEC.md §26, ``thin_edges_device``) by one more
        launch on the same stream, and the thinned map is what is returned."""
        if not hasattr(self.ops, "texton_gradient"):
            raise ValueError("the texton gradient needs ops that have it")
        self._need_thin_ops(thin)
        torch = _torch()
        if getattr(labels, "ndim", 0) != 3 or labels.dtype != torch.int32:
            raise ValueError("labels must be a (B,H,W) int32 device tensor")
        r, n = _check_texton(radius, n_directions)
        labels = labels.contiguous()
        b, h, w = labels.shape
        return self._half_disc_map("texton", labels, labels, K, gradient, directions,
                                   lambda K, g, out, dirs: self.ops.texton_gradient(labels, b, h, w, K, r, n, g, out, dirs),
                                   thin=n if thin else 0)

    def _need_thin_ops(self, thin):
        if thin and not hasattr(self.ops, "edge_thin"):
            raise ValueError("thin edges need ops that have them")

    def _half_disc_map(self, what, labels, like, K, gradient, directions, launch, thin=0):
        """What ``texton_gradient_device`` and ``cue_gradient_device`` share: K (one read of ``labels.max()`` when None; 1 without
        labels) and its limits, ``out`` and ``dirs`` on the (B,H,W) pixels and the device of ``like``, and
        ``launch(K, gradient, out, dirs)``. ``thin`` = n > 0: ``dirs`` is made either way and the map is thinned behind the launch
        (SPEC.md §26)."""
        torch = _torch()
        shape = tuple(like.shape[:3])
        with self._device():
            if labels is None:
                K = 1
            else:
                K = int(labels.max()) + 1 if K is None else _as_int(K)
            if K is None or not 1 <= K <= 64:
                raise ValueError(f"the {what} gradient takes 1 <= K <= 64 labels, got {K}")
            out = torch.empty(shape, dtype=torch.int32, device=like.device)
            dirs = torch.empty(shape, dtype=torch.uint8, device=like.device) if directions or thin else None
            launch(K, None if gradient is None else gradient.contiguous(), out, dirs)
            if thin:
                thick, out = out, torch.empty_like(out)
                self.ops.edge_thin(thick, dirs, *shape, thin, out)
        return (out, dirs) if directions else out

    def texton_edges_device(self, imgs, radius=8, n_directions=8, mode="per_image", joined=True, thin=False):
        """(B,H,W,3) uint8 device tensor -> (B,H,W) int32 edge map E = floor(sqrt(TG * G)) of SPEC.md §24, the whole chain on one
        feature slab: the features, G = the texture gradient of §22 (``edges_device``), the plan's Lloyd loop (``mode`` as in
        ``segment_device``), its int32 label map, and the texton gradient TG of that map at ``radius`` and ``n_directions``.
        ``joined=False``: TG alone (G is not computed). The labels are the plain k-means map: a plan with ``n_superpixels > 0``,
        ``tree_nodes = "clusters"`` or a post-pass (``connectivity``, ``min_region_size``) is refused, and so are row strips, a
        ``dist_group`` (there is no such argument) and a global codebook over more than one rank. ``thin=True``: the kernel also
        writes its direction map and the thin launch of SPEC.md §26 runs behind it on the same stream; the thinned map is returned.
        ``thin=False`` enqueues exactly the launches it always did."""
        self._need_edge_ops("texton")
        self._need_thin_ops(thin)
        self._need_plain_map("texton_edges_device")
        r, n = _check_texton(radius, n_directions)
        return self._edges_chain("texton", imgs, mode, joined, cluster=True, thin=n if thin else 0,
                                 launch=lambda ws, imgs, labels, grad, out, dirs: self.ops.texton_gradient(
                                     labels, *out.shape, self._opt.k, r, n, grad, out, dirs))

    def _need_edge_ops(self, what):
        for name in (what + "_gradient", "feature_gradient"):
            if not hasattr(self.ops, name):
                raise ValueError(f"the {what} edge map needs ops that have it")

    def _need_plain_map(self, who):
        if self.n_superpixels > 0 or self._clusters or self._post_passes or self._relax:
            raise ValueError(f"{who} needs the plain k-means map (no n_superpixels, tree_nodes, post-pass or regularize)")

    def _edges_chain(self, what, imgs, mode, joined, cluster, launch, thin=0):
        """The chain behind ``texton_edges_device`` and ``cue_edges_device`` on one feature slab, once the caller has checked its
        ops, its plan and its parameters: the argument checks, the features, G when ``joined``, the plan's Lloyd loop and its int32
        label map when ``cluster`` (then ``mode="global"`` runs on one rank), and ``launch(ws, imgs, labels or None, G or None,
        out, dirs or None)``, the ``what`` gradient. ``thin`` = n > 0: the gradient writes ``dirs`` too and the map is thinned behind
        it (SPEC.md §26); 0: ``dirs`` is None and nothing is added."""
        self._check_args(imgs, mode, kind="tensor", cluster=cluster)
        if cluster and mode == "global":
            import torch.distributed as td
            if td.is_available() and td.is_initialized() and td.get_world_size() > 1:
                raise ValueError(f"{what}_edges_device runs on one rank only")
        torch = _torch()
        imgs = imgs.contiguous()
        b, h, w, _ = imgs.shape
        new = lambda: torch.empty((b, h, w), dtype=torch.int32, device=imgs.device)
        with self._device():
            ws = self._tail_workspace(b, h, w, mode if cluster else "per_image", slab_only=not cluster)
            _step_features(self.ops, self._opt, ws, imgs, b, h, w)
            grad = labels = None
            if joined:
                grad = new()
                self.ops.feature_gradient(ws["feats"], b, h, w, grad)
            if cluster:
                labels = new()
                _step_cluster(self.ops, self._opt, ws, labels, b, h, w, mode, self.debug)
            out = new()
            dirs = torch.empty((b, h, w), dtype=torch.uint8, device=imgs.device) if thin else None
            launch(ws, imgs, labels, grad, out, dirs)
            if thin:
                thick, out = out, new()
                self.ops.edge_thin(thick, dirs, b, h, w, thin, out)
        return out

    def cue_gradient_device(self, labels, imgs, K=None, radius=8, n_directions=8, bins=16, weights=(2, 2, 1, 1), gradient=None,
                            directions=False, thin=False):
        """The boundary map PB of SPEC.md §25 of any (B,H,W) int32 device label map and any (B,H,W,3) uint8 device image: the
        chi-square distances of the label histograms (weight ``weights[0]``) and of the histograms of the three channels quantised
        to ``bins`` bins (``weights[1:]``), added per direction before the maximum over ``n_directions`` is taken. ``labels`` /
        ``imgs`` may be None when their weights are 0. ``K``, ``radius``, ``gradient``, ``directions``: as in
        ``texton_gradient_device`` (``K`` plays no part when ``weights[0]`` is 0). ``thin``: as in ``texton_gradient_device``."""
        if not hasattr(self.ops, "cue_gradient"):
            raise ValueError("the cue gradient needs ops that have it")
        self._need_thin_ops(thin)
        torch = _torch()
        r, n = _check_texton(radius, n_directions)
        nb, wts = _check_cues(bins, weights)
        if wts[0] and (getattr(labels, "ndim", 0) != 3 or labels.dtype != torch.int32):
            raise ValueError("labels must be a (B,H,W) int32 device tensor")
        if any(wts[1:]) and (getattr(imgs, "ndim", 0) != 4 or imgs.shape[3] != 3 or imgs.dtype != torch.uint8):
            raise ValueError("imgs must be a (B,H,W,3) uint8 device tensor")
        labels = labels.contiguous() if wts[0] else None
        imgs = imgs.contiguous() if any(wts[1:]) else None
        b, h, w = (labels.shape if labels is not None else imgs.shape[:3])
        if labels is not None and imgs is not None and tuple(imgs.shape[:3]) != (b, h, w):
            raise ValueError("labels and imgs must cover the same (B,H,W) pixels")
        return self._half_disc_map("cue", labels, labels if labels is not None else imgs, K, gradient, directions,
                                   lambda K, g, out, dirs: self.ops.cue_gradient(labels, imgs, b, h, w, K, nb, wts, r, n, g, out, dirs),
                                   thin=n if thin else 0)

    def cue_edges_device(self, imgs, radius=8, n_directions=8, bins=16, weights=(2, 2, 1, 1), mode="per_image", joined=True,
                         thin=False):
        """(B,H,W,3) uint8 device tensor -> (B,H,W) int32 boundary map E' = floor(sqrt(PB * G)) of SPEC.md §25, the whole chain on
        one feature slab: the features, G = the texture gradient of §22, the plan's Lloyd loop and its int32 label map (``mode`` as
        in ``segment_device``), then ONE launch that adds, per direction, the chi-square distances of the label histograms and of
        the three channels of the image the Gabor stage saw (Y, Co, Cg of §11 when the plan has ``chroma_gain``, else R, G, B),
        quantised to ``bins`` bins, with the integer ``weights`` (textons, channel 0, 1, 2). ``joined=False``: PB alone (G is not
        computed). With ``weights[0] == 0`` NO Lloyd pass is enqueued, and the plan's clustering options play no part; otherwise
        the labels are the plain k-means map and ``texton_edges_device``'s refusals hold. Row strips are refused either way (there
        is no such argument). ``thin``: as in ``texton_edges_device``."""
        self._need_edge_ops("cue")
        self._need_thin_ops(thin)
        r, n = _check_texton(radius, n_directions)
        nb, wts = _check_cues(bins, weights)
        if wts[0] > 0:
            self._need_plain_map("cue_edges_device with weights[0] > 0")

        def launch(ws, imgs, labels, grad, out, dirs):
            self.ops.cue_gradient(labels, ws["colour"] if self._opt.colour else imgs, *out.shape, self._opt.k, nb, wts, r, n, grad,
                                  out, dirs)
        return self._edges_chain("cue", imgs, mode, joined, cluster=wts[0] > 0, launch=launch, thin=n if thin else 0)

    def thin_edges_device(self, edges, dirs, n_directions=8):
        """(B,H,W) int32 device edge map and its (B,H,W) uint8 direction map -> (B,H,W) int32 thin map T of SPEC.md §26: a pixel
        keeps max(E, 0) when no larger value lies along the normal of its direction (of ``n_directions``, SPEC.md §24's) among its
        eight neighbours, linearly interpolated, and is 0 otherwise; strict on one side and weak on the other, so one pixel of a
        two-pixel plateau survives. A direction >= ``n_directions`` gives 0. One launch; the maps are those of
        ``texton_gradient_device`` / ``cue_gradient_device`` with ``directions=True``, or any others."""
        self._need_thin_ops(True)
        torch = _torch()
        if getattr(edges, "ndim", 0) != 3 or edges.dtype != torch.int32:
            raise ValueError("edges must be a (B,H,W) int32 device tensor")
        if getattr(dirs, "ndim", 0) != 3 or dirs.dtype != torch.uint8 or tuple(dirs.shape) != tuple(edges.shape):
            raise ValueError("dirs must be a (B,H,W) uint8 device tensor covering the same pixels as edges")
        n = _as_int(n_directions)
        if n is None or not 1 <= n <= 16:
            raise ValueError(f"n_directions must be in 1..16, got {n_directions!r}")
        edges, dirs = edges.contiguous(), dirs.contiguous()
        with self._device():
            out = torch.empty_like(edges)
            self.ops.edge_thin(edges, dirs, *edges.shape, n, out)
        return out

    # ---- host API: the slot
    def segment_batch(self, imgs: np.ndarray, mode="per_image", out_dtype=np.int32, codebook=None, refine=0) -> np.ndarray:
        """(B,H,W,3) uint8 host array -> fresh (B,H,W) host label array (the calling convention of script.py:25,30).

        ``out_dtype``: np.int32 (default, SPEC.md §1) or np.uint8 (a quarter of the bytes; metrics.py:43 casts the map
        with ``.astype('int')`` anyway; not with ``connectivity=True`` or ``min_region_size > 0``, whose region ids exceed 255).
        The image upload goes through a cached pinned staging buffer, cut into chunks so that the copy of chunk n+1
        (its own stream) overlaps the Gabor stage of chunk n; the labels are copied straight into a fresh pinned
        buffer that the returned array owns. ``codebook``, ``refine``: a ``KMeansModel`` in place of the stage's own centroids
        (``predict_device``), on the plain path: upload, step, download."""
        torch = _torch()
        if isinstance(imgs, (list, tuple)):                        # B equally shaped (H,W,3) images: staged one by one
            imgs = _ImageList(imgs)
        else:
            imgs = np.ascontiguousarray(imgs)
        out_dtype = self._check_args(imgs, mode, out_dtype)
        b, h, w, _ = imgs.shape
        if codebook is not None:                                   # (SPEC.md §28: the plain path)
            dev = torch.from_numpy(np.asarray(imgs)).to(self.ops.device)
            return self.segment_device(dev, mode, codebook=codebook, refine=refine).cpu().numpy().astype(out_dtype, copy=False)
        path = self._host_path(b, h, w, mode)
        if path == "plain":                                        # (test stand-ins, post-passes, collectives, large §13 calls)
            dev = torch.from_numpy(np.asarray(imgs)).to(self.ops.device)
            return self.segment_device(dev, mode).cpu().numpy().astype(out_dtype, copy=False)
        if path == "graph":
            return self._segment_small(imgs, mode, out_dtype)
        ops, opt, dev = self.ops, self._opt, self.ops.device
        st = self._host_state(b, h, w)
        ws = self._workspace(b, h, w, mode)
        cur = torch.cuda.current_stream(dev)
        n_chunks = min(b, 4)
        bounds = [(b * i) // n_chunks for i in range(n_chunks + 1)]
        pin_np = st["pin_in"].numpy()
        with torch.cuda.device(dev):
            st["copy"].wait_stream(cur)                            # the device input buffer is free again
            # Host memcpy into the pinned buffer, chunk by chunk on two worker threads (numpy releases the GIL): one thread
            # stages a 16-image chunk in 0.2 ms, which alone would pace the uploads and the Gabor launches behind them
            # (4 x 0.26 ms before the last chunk's kernels can start, against 0.44 ms of Gabor work).
            if self._stagers is None:
                from concurrent.futures import ThreadPoolExecutor
                self._stagers = ThreadPoolExecutor(2, thread_name_prefix="gcs-stage")
            staged = [self._stagers.submit(_copy_images, pin_np, imgs, bounds[i], bounds[i + 1]) for i in range(n_chunks)]
            for i in range(n_chunks):
                g0, g1 = bounds[i], bounds[i + 1]
                staged[i].result()
                with torch.cuda.stream(st["copy"]):
                    st["dev_in"][g0:g1].copy_(st["pin_in"][g0:g1], non_blocking=True)
                    st["ev"][i].record(st["copy"])
                cur.wait_event(st["ev"][i])
                _step_features(ops, opt, ws, st["dev_in"][g0:g1], b, h, w, chunk=(g0, g1))
            _step_features(ops, opt, ws, None, b, h, w)            # once for the batch, behind every chunk's Gabor stage on `cur`
            dev_out = st["dev_out"] if out_dtype == np.uint8 else st["dev_out32"]
            _step_cluster(ops, opt, ws, dev_out, b, h, w, mode, self.debug)
            self._note_plane(ws)
            # The result is a FRESH pinned host buffer per call, handed to the caller as the base of the returned
            # array (torch's caching host allocator recycles it once the caller drops the array): the device-to-host
            # copy lands directly in caller-owned memory, with no pageable copy and no first-touch page faults.
            res = torch.empty((b, h, w), dtype=dev_out.dtype, pin_memory=True)
            ops.download(res, dev_out)                             # copy engines, as in segment_stream (not the blit kernel)
            cur.synchronize()
        return res.numpy()

    def segment_stream(self, batches, mode="per_image", out_dtype=np.int32, depth=2, codebook=None, refine=0):
        """Pipelined host API: a generator over the label arrays of an iterable of equally shaped (B,H,W,3) uint8 host
        batches, in order - ``for labels in seg.segment_stream(loader): ...`` instead of calling ``segment_batch`` per batch
        (the loop of script.py:22-38 over a data set). Results equal ``segment_batch(batch, mode, out_dtype)``.

        Three streams work on ``depth + 1`` buffer slots: while batch n runs through the Gabor stage and the Lloyd passes,
        batch n+1 is copied into pinned memory and uploaded and the labels of batch n-1 are downloaded into a fresh pinned
        array that the caller owns, both by the copy engines (gcs_download: see there). A result is handed out ``depth``
        batches after its input was taken (sooner when the input ends). With a ``codebook`` every batch takes
        ``segment_batch``'s plain path."""
        out_dtype = self._check_args(None, mode, out_dtype)
        if codebook is not None:
            for imgs in batches:
                yield self.segment_batch(imgs, mode, out_dtype, codebook=codebook, refine=refine)
            return
        if not self._may_pipeline(mode):
            for imgs in batches:                                   # no pipeline for post-passes / collectives / stand-ins / §13
                yield self.segment_batch(imgs, mode, out_dtype)
            return
        pipe = _StreamPipe(self, mode, out_dtype, depth)
        try:
            for imgs in batches:
                yield from pipe.push(imgs)
            yield from pipe.drain()
        finally:
            pipe.close()

    def _segment_small(self, imgs, mode, out_dtype):
        """One image (or a small batch): the slot as script.py:22-30 calls it, once per image. A step is ~25 launches of
        kernels that take microseconds each, so the host's launch calls, not the device, set the latency: the whole step
        (Gabor stage, n_iter Lloyd passes, label raster) is captured ONCE per shape as a HIP graph on static buffers and
        replayed per call - upload, one graph launch, download."""
        torch = _torch()
        b, h, w, _ = imgs.shape
        dev = self.ops.device
        key = (b, h, w, mode, out_dtype.str)
        ent = self._graphs.get(key)
        with torch.cuda.device(dev):
            if ent is None:
                # every buffer the graph touches belongs to the entry (all allocated here, outside the capture)
                ws = self._tail_workspace(b, h, w, mode, private=out_dtype)
                dev_in = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
                dev_out = torch.empty((b, h, w), dtype=torch.uint8 if out_dtype == np.uint8 else torch.int32, device=dev)
                pin_in = torch.empty((b, h, w, 3), dtype=torch.uint8, pin_memory=True)

                # (the closure must not capture `self`: the entry lives in self._graphs, and a Segmenter inside a reference
                # cycle is freed - with its graphs, streams, pinned and device buffers - only when the cyclic collector
                # happens to run, not when the last user drops it)
                ops, opt, debug = self.ops, self._opt, self.debug

                def step():
                    _step_features(ops, opt, ws, dev_in, b, h, w)
                    _step_cluster(ops, opt, ws, dev_out, b, h, w, mode, debug)
                dev_in.zero_()
                step()                                     # eager once: first-use work (side-stream creation) outside the capture
                # (a STREAM wait - the step joins its side stream back into this one: a device-wide synchronize is refused while
                # any thread of the process captures, and invalidates that thread's capture: _CaptureGuard)
                torch.cuda.current_stream(dev).synchronize()
                graph = torch.cuda.CUDAGraph()
                # capture under the module's guard (_CaptureGuard: serialised, collector off for exactly that long, retired
                # graphs parked meanwhile); a refused capture (e.g. the caller's own capture is open on this thread) is reported
                # once and the shape then runs as eager launches
                if not _CAPTURES.capture(torch, graph, step, dev):
                    _CAPTURES.fell_back(key, "torch.cuda.graph raised RuntimeError")
                    graph = None
                    torch.cuda.current_stream(dev).synchronize()
                ent = dict(graph=graph, step=step, ws=ws, dev_in=dev_in, dev_out=dev_out, pin_in=pin_in, scratch=ws["scratch"],
                           rt=ws.get("rt"))          # (the tree buffers of SPEC.md §14, None when that stage is off)
                if len(self._graphs) >= 4:                 # evicted plans leave through the guard: never inside an open capture
                    _CAPTURES.retire([self._graphs.pop(next(iter(self._graphs)))])
                self._graphs[key] = ent
            cur = torch.cuda.current_stream(dev)
            _stage(ent["pin_in"], imgs)
            ent["dev_in"].copy_(ent["pin_in"], non_blocking=True)
            if ent["graph"] is not None:
                ent["graph"].replay()
            else:
                ent["step"]()
            self._note_plane(ent["ws"])
            res = torch.empty((b, h, w), dtype=ent["dev_out"].dtype, pin_memory=True)   # caller-owned pinned result
            res.copy_(ent["dev_out"], non_blocking=True)
            cur.synchronize()
        return res.numpy()

    def _copy_streams(self):
        """The upload and the download stream of this Segmenter, created once and shared by every host path and shape. HIP maps
        a process's streams onto a few hardware queues (four by default): with a pair of streams per shape and path, a
        download stream ended up on the compute stream's queue and every label download then held back the next batch's
        kernels (the pipelined rate fell from 4 360 to 3 300 Mpix/s as soon as segment_batch had created its own copy stream;
        profiles/r3_notes.md). Default stream + the Gabor side stream + these two = four."""
        if self._copy_pair is None:
            torch = _torch()
            dev = self.ops.device
            self._copy_pair = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        return self._copy_pair

    def _host_state(self, b, h, w):
        """Pinned staging buffers, device input / uint8 output buffers, copy stream and events for one batch shape."""
        torch = _torch()
        key = (b, h, w)
        st = self._host.get(key)
        if st is None:
            dev = self.ops.device
            st = dict(pin_in=torch.empty((b, h, w, 3), dtype=torch.uint8, pin_memory=True),
                      dev_in=torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev),
                      dev_out=torch.empty((b, h, w), dtype=torch.uint8, device=dev),
                      dev_out32=torch.empty((b, h, w), dtype=torch.int32, device=dev),
                      copy=self._copy_streams()[0], ev=[torch.cuda.Event() for _ in range(4)])
            if len(self._host) >= 4:                               # keep the four most recent shapes (see _workspace)
                self._host.pop(next(iter(self._host)))
            self._host[key] = st
        return st

    def __call__(self, img: np.ndarray, codebook=None, refine=0) -> np.ndarray:
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("img must be an (H,W,3) uint8 array (skimage.io.imread of an RGB file)")
        if codebook is not None:
            return self.segment_batch(img[None], codebook=codebook, refine=refine)[0]
        return self.segment_batch(img[None])[0]

    def segment_images(self, images, batch=64, out_dtype=np.int32, codebook=None, refine=0):
        """The loop of script.py:22-38 as a generator: ``for labels in seg.segment_images(loader): ...`` yields, in input
        order, exactly what ``segment(img)`` returns for every (H,W,3) uint8 image of an iterable - any mix of shapes (BSD500
        holds 481x321 and 321x481 images). Images wait in per-shape groups of up to ``batch`` and go through the device
        together (per-image codebooks, so grouping does not change any label): the data-set loop at the batch rate instead of
        one 0.28 ms call per image. Held back at any time: up to two batches per shape in flight (one computing, one
        downloading), the partial group of every shape, and at most ``2 * batch`` finished label maps that wait for an
        EARLIER image of another shape - when that many have piled up, the group (or the pipeline) that holds the oldest
        outstanding image is flushed early as a partial batch, so a rare shape at the start of a long or endless loader
        neither stalls the output nor grows the pinned result memory without bound. ``codebook``: a one-codebook ``KMeansModel``
        for every image (``predict_device``; every group then takes ``segment_batch``'s plain path)."""
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        out_dtype = self._check_args(None, "per_image", out_dtype)
        if codebook is not None and getattr(codebook, "n_sets", 1) != 1:
            raise ValueError("segment_images groups the images itself: it takes a model of one codebook")
        with_model = {} if codebook is None else dict(codebook=codebook, refine=refine)
        groups, ready, nxt = {}, {}, 0
        pipes, tags = {}, {}                   # per shape: the pipeline of its FULL batches and the image indices in flight
        piped = self._may_pipeline("per_image") and codebook is None

        def emit(idx, labels):
            for i, lab in zip(idx, labels):
                ready[i] = lab

        def flush(shape, final):
            idx, imgs = zip(*groups.pop(shape))
            h, w = shape[:2]
            if piped and not final and len(idx) * h * w > _GRAPH_MAX_PIXELS \
                    and self.group_size(len(idx), h, w, "per_image") >= len(idx):
                # full batches of one shape follow each other through the three-stream pipeline (upload, compute and
                # download of consecutive batches overlap); their label maps fall due one push later
                if shape not in pipes:
                    pipes[shape], tags[shape] = _StreamPipe(self, "per_image", out_dtype, 1), []
                tags[shape].append(idx)
                for labels in pipes[shape].push(_ImageList(imgs)):
                    emit(tags[shape].pop(0), labels)
            else:
                emit(idx, self.segment_batch(list(imgs), "per_image", out_dtype, **with_model))

        try:
            for n, img in enumerate(images):
                img = np.asarray(img)
                if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                    raise ValueError("every image must be an (H,W,3) uint8 array (skimage.io.imread of an RGB file)")
                groups.setdefault(img.shape, []).append((n, img))
                if len(groups[img.shape]) >= batch:
                    flush(img.shape, False)
                if len(ready) >= 2 * batch and nxt not in ready:
                    # bound the wait: the oldest outstanding image sits in a partial group or in a pipeline
                    held = [sh for sh, g in groups.items() if g and g[0][0] == nxt]
                    if held:
                        flush(held[0], True)
                    else:
                        for shape, pipe in pipes.items():
                            if tags[shape] and tags[shape][0][0] == nxt:
                                for labels in pipe.drain():
                                    emit(tags[shape].pop(0), labels)
                while nxt in ready:
                    yield ready.pop(nxt)
                    nxt += 1
            for shape, pipe in pipes.items():                      # the input has ended
                for labels in pipe.drain():
                    emit(tags[shape].pop(0), labels)
            while groups:                                          # remainders: oldest waiting image first
                flush(min(groups, key=lambda sh: groups[sh][0][0]), True)
            while nxt in ready:
                yield ready.pop(nxt)
                nxt += 1
        finally:
            for pipe in pipes.values():
                pipe.close()


class _StreamPipe:
    """The three-stream pipeline behind Segmenter.segment_stream / segment_images for ONE batch shape: ``push(batch)`` stages
    and uploads the batch, queues its Gabor stage, Lloyd passes and label download, and returns the label arrays that have
    become due (``depth`` pushes later, in order); ``drain()`` returns the rest.

    ``depth + 1`` buffer slots: while batch n computes, batch n+1 is copied into pinned memory and uploaded and the labels of
    batch n-1 are downloaded into a fresh pinned array that the caller owns, both by the copy engines. The download is not a
    ``tensor.copy_`` / hipMemcpyAsync: on this stack that device-to-host copy runs as a blit KERNEL (`__amd_rocclr_copyBuffer`
    in the kernel trace) and, for as long as PCIe takes - 0.75 ms for the 39.5 MB of a 64-image int32 batch - the kernels of
    every other stream crawl (profiles/r3_notes.md); gcs_download hands the same bytes to SDMA, like the uploads."""

    def __init__(self, seg, mode, out_dtype, depth):
        self.seg, self.mode, self.depth = seg, mode, int(depth)
        self.n_slots = max(2, self.depth + 1)
        torch = _torch()
        self.t_dtype = torch.uint8 if np.dtype(out_dtype) == np.uint8 else torch.int32
        self.st = self.ws = self.shape = None
        self.n = 0
        self.pending = []                                          # (download event, result array) in input order

    def _open(self, imgs):
        torch = _torch()
        seg, dev, n_slots = self.seg, self.seg.ops.device, self.n_slots
        b, h, w, _ = imgs.shape
        seg._check_args(imgs, self.mode)                           # (once per stream; out_dtype: the entry point has checked it)
        if seg.group_size(b, h, w, self.mode) < b:
            raise ValueError("batch too large for one feature slab: use smaller batches")
        self.shape = (b, h, w)
        self.ws = seg._workspace(b, h, w, self.mode)
        key = (b, h, w, n_slots, self.t_dtype)
        st = seg._stream.get(key)
        if st is None or st["busy"]:           # pinning 3 x 30 MB costs ms: the state is kept for the next stream of this shape
            st = dict(pin_in=[torch.empty((b, h, w, 3), dtype=torch.uint8, pin_memory=True) for _ in range(n_slots)],
                      dev_in=[torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev) for _ in range(n_slots)],
                      dev_out=[torch.empty((b, h, w), dtype=self.t_dtype, device=dev) for _ in range(n_slots)],
                      up=seg._copy_streams()[0], down=seg._copy_streams()[1],
                      ev_up=[torch.cuda.Event() for _ in range(n_slots)],
                      ev_done=[torch.cuda.Event() for _ in range(n_slots)],
                      ev_down=[torch.cuda.Event() for _ in range(n_slots)], busy=False)
            if key not in seg._stream:                             # (a second live stream of the same shape stays private)
                if len(seg._stream) >= 4:
                    idle = [k for k, v in seg._stream.items() if not v["busy"]]
                    if idle:
                        seg._stream.pop(idle[0])
                if len(seg._stream) < 4:
                    seg._stream[key] = st
        else:                                                      # a stream abandoned half way may still own the slots
            st["up"].synchronize()
            st["down"].synchronize()
            torch.cuda.current_stream(dev).synchronize()
        st["busy"] = True
        self.st = st

    def push(self, imgs):
        torch = _torch()
        seg, ops, dev = self.seg, self.seg.ops, self.seg.ops.device
        if not isinstance(imgs, _ImageList):
            imgs = np.ascontiguousarray(imgs)
        if imgs.dtype != np.uint8 or imgs.ndim != 4 or imgs.shape[3] != 3:
            raise ValueError("every batch must be a (B,H,W,3) uint8 array")
        b, h, w, _ = imgs.shape
        with torch.cuda.device(dev):
            if self.st is None:
                self._open(imgs)
            elif (b, h, w) != self.shape:
                raise ValueError(f"batch {self.n} has shape {(b, h, w)}, the stream was opened with {self.shape}")
            st, ws, n, n_slots = self.st, self.ws, self.n, self.n_slots
            cur = torch.cuda.current_stream(dev)
            i = n % n_slots
            if n >= n_slots:
                st["ev_up"][i].synchronize()                       # the slot's previous upload has left the pinned buffer
            _stage(st["pin_in"][i], imgs)                          # host memcpy, while the device works on earlier batches
            with torch.cuda.stream(st["up"]):
                if n >= n_slots:
                    st["up"].wait_event(st["ev_done"][i])          # dev_in[i] is no longer being read
                st["dev_in"][i].copy_(st["pin_in"][i], non_blocking=True)
                st["ev_up"][i].record(st["up"])
            cur.wait_event(st["ev_up"][i])
            if n >= n_slots:
                cur.wait_event(st["ev_down"][i])                   # dev_out[i] has been downloaded
            _step_features(ops, seg._opt, ws, st["dev_in"][i], b, h, w)
            _step_cluster(ops, seg._opt, ws, st["dev_out"][i], b, h, w, self.mode, seg.debug)
            st["ev_done"][i].record(cur)
            land = torch.empty((b, h, w), dtype=self.t_dtype, pin_memory=True)   # caller-owned; torch recycles it once dropped
            with torch.cuda.stream(st["down"]):
                st["down"].wait_event(st["ev_done"][i])
                ops.download(land, st["dev_out"][i])
                st["ev_down"][i].record(st["down"])
            ev = torch.cuda.Event()
            ev.record(st["down"])
            self.pending.append((ev, land.numpy()))
            self.n += 1
            out = []
            while len(self.pending) > self.depth:
                ev0, res0 = self.pending.pop(0)
                ev0.synchronize()
                out.append(res0)
            return out

    def drain(self):
        out = []
        for ev0, res0 in self.pending:
            ev0.synchronize()
            out.append(res0)
        self.pending = []
        return out

    def close(self):
        """Leave the compute stream ordered behind the copy streams and hand the slot buffers back for reuse."""
        if self.st is not None:
            torch = _torch()
            cur = torch.cuda.current_stream(self.seg.ops.device)
            cur.wait_stream(self.st["up"])
            cur.wait_stream(self.st["down"])
            # Results nobody took (an abandoned or failed generator): their pinned landing buffers come from torch's host
            # allocator, which knows nothing about the raw gcs_download still writing them - wait for those copies before
            # the arrays are dropped, or the next pinned allocation could be handed a block with a transfer in flight.
            for ev0, _ in self.pending:
                ev0.synchronize()
            self.pending = []
            self.st["busy"] = False
            self.st = None


class _ImageList:
    """A list of equally shaped (H,W,3) uint8 images seen as a (B,H,W,3) batch without stacking them first."""
    ndim, dtype = 4, np.dtype(np.uint8)

    def __init__(self, items):
        self.items = [np.ascontiguousarray(x) for x in items]
        if not self.items:
            raise ValueError("empty batch")
        first = self.items[0]
        if any(x.dtype != np.uint8 or x.shape != first.shape for x in self.items) or first.ndim != 3:
            raise ValueError("a list batch must hold equally shaped (H,W,3) uint8 images")
        self.shape = (len(self.items),) + first.shape

    def __array__(self, dtype=None, copy=None):
        return np.stack(self.items)


def _copy_images(dst, imgs, g0, g1):
    """dst[g0:g1] = imgs[g0:g1] for an array batch or an _ImageList."""
    if isinstance(imgs, _ImageList):
        for i in range(g0, g1):
            np.copyto(dst[i], imgs.items[i])
    else:
        np.copyto(dst[g0:g1], imgs[g0:g1])


def _stage(pinned, imgs):
    """Host array -> pinned staging tensor with ONE plain memcpy (numpy, GIL released). Not `tensor.copy_`: that runs on
    torch's intra-op pool, which sizes itself by the machine's core count and not by the process's CPU quota - on a
    256-core host inside a 16-core cgroup the pool's threads get throttled and a 30 MB copy takes 10+ ms instead of 0.5."""
    _copy_images(pinned.numpy(), imgs, 0, imgs.shape[0])


_default: dict = {}


def _need_cut(kw):
    """A one-shot call that delivers a label map builds a tree only to cut it: SPEC.md §23 without ``n_regions`` has nothing to weigh."""
    if kw.get("merge_cost", "features") == "boundary" and not kw.get("n_regions"):
        raise ValueError('merge_cost = "boundary" needs n_regions = R with R > 0 here: without a cut no tree is built')


def _plan(kw) -> Segmenter:
    key = tuple(sorted(kw.items()))
    if key not in _default:
        _default.clear()
        _default[key] = Segmenter(**kw)
    return _default[key]


def _with_model(kw):
    """``codebook`` and ``refine`` taken out of a one-shot call's keywords (plans are cached by what is left) -> the keywords of the
    host paths: none without a codebook."""
    codebook, refine = kw.pop("codebook", None), kw.pop("refine", 0)
    return {} if codebook is None else dict(codebook=codebook, refine=refine)


def segment(img, **kw) -> np.ndarray:
    """Drop-in for ``slic(img, ...)`` at script.py:30: (H,W,3) uint8 -> (H,W) int32 labels 0..k-1. ``codebook=model, refine=m``:
    under a ``KMeansModel`` of ``fit_codebook`` (``Segmenter.predict_device``) instead of the image's own centroids."""
    model = _with_model(kw)
    _need_cut(kw)
    return _plan(kw)(img, **model)


def fit_codebook(imgs, mode="global", n_init=1, **kw) -> KMeansModel:
    """(B,H,W,3) uint8 host array (or B equally shaped images) -> the ``KMeansModel`` of ``Segmenter.fit_device`` on them, on
    the host: one codebook for the batch in mode "global". ``n_init``: restarts (with ``init="kmeans++"``; SPEC.md §29).
    ``kw``: the plan's options, cached like ``segment``'s."""
    seg = _plan(kw)
    dev = _torch().from_numpy(np.ascontiguousarray(np.asarray(imgs)))
    return seg.fit_device(dev.to(seg.ops.device) if seg.native else dev, mode, n_init=n_init).cpu()


def segment_confidence(img, codebook=None, **kw):
    """(H,W,3) uint8 -> ((H,W) int32 labels, (H,W) float32 confidence in [0, 1]) of SPEC.md §28
    (``Segmenter.confidence_device``): how much nearer a pixel is to its centroid than to the next one. ``codebook``: a
    ``KMeansModel``; without one, the image's own centroids. ``kw``: the plan's options, cached like ``segment``'s."""
    img = _one_image(img)
    seg = _plan(kw)
    labels, conf = seg.confidence_device(_batch_of_one(seg, img), codebook)
    return labels[0].cpu().numpy(), conf[0].cpu().numpy()


def segment_contours(img, **kw) -> np.ndarray:
    """(H,W,3) uint8 -> (H,W) float32 boundary strengths in [0, 1]: the contour map of SPEC.md §15 divided by max(1, alive), so
    that thresholding it at (alive - R) / alive gives the boundaries of the cut at R regions. ``kw``: the plan's options
    (``n_superpixels`` is needed); the plan is cached like ``segment``'s."""
    img = _one_image(img)
    if not kw.get("n_superpixels") and kw.get("tree_nodes") != "clusters":
        raise ValueError('segment_contours needs n_superpixels=n with n > 0, or tree_nodes="clusters"')
    seg = _plan(kw)
    contours, alive = seg.contours_device(_batch_of_one(seg, img))
    return (contours[0].cpu().numpy().astype(np.float32) / np.float32(max(1, int(alive[0])))).astype(np.float32)


def segment_edges(img, **kw) -> np.ndarray:
    """(H,W,3) uint8 -> (H,W) float32 edge strengths in [0, 1]: the texture-gradient map of SPEC.md §22
    (``Segmenter.edges_device``) divided by its largest value, all zeros for a map that is zero everywhere. ``kw``: the plan's
    options (the bank, ``smoothing``, colour and position options shape the map; clustering options play no part); the plan is
    cached like ``segment``'s."""
    img = _one_image(img)
    seg = _plan(kw)
    return _over_largest(seg.edges_device(_batch_of_one(seg, img)))


def segment_texton_edges(img, radius=8, n_directions=8, thin=False, **kw) -> np.ndarray:
    """(H,W,3) uint8 -> (H,W) float32 edge strengths in [0, 1]: the map E of SPEC.md §24 (``Segmenter.texton_edges_device``: the
    texton gradient of the plan's k-means map joined with the texture gradient of §22) divided by its largest value, all zeros
    for a map that is zero everywhere, as ``segment_edges`` normalises. ``thin=True``: the thin map T of SPEC.md §26, normalised
    the same way. ``kw``: the plan's options, cached like ``segment``'s."""
    img = _one_image(img)
    seg = _plan(kw)
    return _over_largest(seg.texton_edges_device(_batch_of_one(seg, img), radius=radius, n_directions=n_directions, thin=bool(thin)))


def segment_cue_edges(img, radius=8, n_directions=8, bins=16, weights=(2, 2, 1, 1), thin=False, **kw) -> np.ndarray:
    """(H,W,3) uint8 -> (H,W) float32 edge strengths in [0, 1]: the map E' of SPEC.md §25 (``Segmenter.cue_edges_device``: the
    brightness, colour and texton cues joined per direction, then with the texture gradient of §22) divided by its largest value,
    all zeros for a map that is zero everywhere, as ``segment_edges`` normalises. ``thin=True``: the thin map T of SPEC.md §26,
    normalised the same way. ``kw``: the plan's options, cached like ``segment``'s."""
    img = _one_image(img)
    r, n = _check_texton(radius, n_directions)
    nb, wts = _check_cues(bins, weights)
    seg = _plan(kw)
    return _over_largest(seg.cue_edges_device(_batch_of_one(seg, img), radius=r, n_directions=n, bins=nb, weights=wts,
                                              thin=bool(thin)))


def segment_images(images, batch=64, **kw):
    """Generator form of the loop at script.py:22-38: yields ``segment(img)`` for every image of an iterable, in order, with
    the images batched per shape behind the scenes (``Segmenter.segment_images``)."""
    out_dtype = kw.pop("out_dtype", np.int32)
    model = _with_model(kw)
    _need_cut(kw)
    return _plan(kw).segment_images(images, batch=batch, out_dtype=out_dtype, **model)


def segment_batch(imgs, mode="per_image", **kw) -> np.ndarray:
    """(B,H,W,3) uint8 -> (B,H,W) int32; equals stack([segment(i) for i in imgs]) in per_image mode."""
    out_dtype = kw.pop("out_dtype", np.int32)
    model = _with_model(kw)
    _need_cut(kw)
    return _plan(kw).segment_batch(imgs, mode, out_dtype=out_dtype, **model)


def _one_image(img):
    img = np.ascontiguousarray(img)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError("img must be an (H,W,3) uint8 array")
    return img


def _batch_of_one(seg, img):
    """The (H,W,3) image as a (1,H,W,3) tensor where the plan's ops run."""
    dev = _torch().from_numpy(img[None])
    return dev.to(seg.ops.device) if seg.native else dev


def _over_largest(maps):
    """The first map of a (B,H,W) int32 tensor as float32, divided by its largest value; zeros for a map that is zero everywhere."""
    g = maps[0].cpu().numpy()
    top = int(g.max())
    if top == 0:
        return np.zeros(g.shape, np.float32)
    return (g.astype(np.float32) / np.float32(top)).astype(np.float32)


def segment_regions(img, adjacency=False, gradient=False, **kw):
    """(H,W,3) uint8 -> ``(labels (H,W) int32, table)``: ``segment(img, **kw)`` and the descriptors of its regions (SPEC.md §19,
    ``regions.region_table``: area, centroid, bbox, mean_rgb, mean_features, used; one entry per label 0 .. labels.max()). The table
    is made from the delivered map, behind every post-pass of the plan, so it describes what the caller gets. ``adjacency=True``: the
    table gains the key ``"adjacency"``, the region adjacency graph of the delivered map (SPEC.md §20, ``regions.adjacency_table``
    with ``n_regions`` = the number of labels: pairs, length, mean_contrast from ``img``, mean_strength 0, degree, neighbours).
    A delivered map with more than 16 384 edges (no map of connected regions of fewer than 5 463 labels has) raises ``ValueError``.
    ``gradient=True`` (with ``adjacency=True``): the texture-gradient edge map of SPEC.md §22 (``Segmenter.edges_device`` of the
    same plan) is the graph's strength plane, so ``mean_strength`` is the mean gradient along each shared boundary; without it the
    output is what it was, bit for bit."""
    if gradient and not adjacency:
        raise ValueError("gradient=True needs adjacency=True (the gradient is the strength plane of the adjacency graph)")
    from .regions import region_table, adjacency_table
    _need_cut(kw)
    torch = _torch()
    img = _one_image(img)
    seg = _plan(kw)
    seg._last_plane = None                                         # only a plane this very call's step leaves is taken below
    labels = seg(img)
    dev = seg.ops.device
    imgs_d = torch.from_numpy(img[None]).to(dev)
    lab_d = torch.from_numpy(np.ascontiguousarray(labels[None], np.int32)).to(dev)
    sums, bbox = seg.region_props_device(imgs_d, lab_d)
    table = region_table(sums[0].cpu().numpy(), bbox[0].cpu().numpy())
    if adjacency:
        k = int(sums.shape[1])
        strength = None
        if gradient:                                               # SPEC.md §23: the tree's step has left the plane of this image
            strength, seg._last_plane = seg._last_plane, None
            if strength is None or tuple(strength.shape) != tuple(lab_d.shape):    # (no such step ran: the map on its own)
                strength = seg.edges_device(imgs_d)
        edges, vals, count = seg.region_adjacency_device(lab_d, K=k, imgs=imgs_d, strength=strength)
        if int(count[0]) < 0:                                      # more edges than the default capacity: once more at the largest
            edges, vals, count = seg.region_adjacency_device(lab_d, K=k, imgs=imgs_d, strength=strength, capacity=16384)
        table["adjacency"] = adjacency_table(edges[0].cpu().numpy(), vals[0].cpu().numpy(), int(count[0]), n_regions=k)
    return labels, table


def render_regions(img, labels) -> np.ndarray:
    """(H,W,3) uint8 image and an (H,W) label map of it -> (H,W,3) uint8: every region in its mean colour (SPEC.md §19), black
    where a label is negative. Runs on the plan the module-level calls hold (the default plan if there is none yet)."""
    torch = _torch()
    img = _one_image(img)
    labels = np.ascontiguousarray(labels, np.int32)
    if labels.shape != img.shape[:2]:
        raise ValueError("labels must be the (H,W) map of img")
    seg = next(iter(_default.values())) if _default else _plan({})
    dev = seg.ops.device
    lab = torch.from_numpy(labels[None]).to(dev)
    sums, _ = seg.region_props_device(torch.from_numpy(img[None]).to(dev), lab)
    return seg.paint_device(lab, sums)[0].cpu().numpy()
