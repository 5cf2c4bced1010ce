"""Scoring on the GPU: the kernels give integer counts and tables, the float arithmetic of the reference
(BSD_metrics/metrics.py:58-201; region agreement: SPEC.md §8) runs here in the reference's order, so the floats are its floats.
Four layers, each with the C entry points it calls:

1. One image, truth uploaded per call: ``boundary_counts_device`` / ``boundary_scores_device`` (gcs_boundary_counts),
   ``region_counts_device`` (gcs_region_counts), ``region_agreement_device`` (gcs_region_counts, gcs_region_agreement),
   ``all_scores_device`` (gcs_boundary_counts, gcs_region_counts).
2. A batch, truth uploaded per call: ``all_scores_batch_device`` (gcs_boundary_counts_batch, gcs_region_counts_batch,
   gcs_region_agreement with agreement=True).
3. A batch on resident truth: ``DeviceTruth`` (gcs_truth_prepare), ``submit_scores_batch_resident`` /
   ``all_scores_batch_resident`` (gcs_score_batch_resident, gcs_region_agreement with agreement=True).
4. Every cut of a region tree on resident truth: ``boundary_sweep_resident`` (gcs_boundary_sweep_resident) with
   ``sweep_counts`` / ``sweep_scores``; ``region_sweep_resident`` (gcs_region_counts_batch[_u8], gcs_region_sweep) with
   ``sweep_agreement``; ``under_sweep_resident`` (gcs_region_counts_batch[_u8], gcs_region_sweep_under) and ``cut_shapes_device``
   (gcs_cut_shapes) with ``sweep_reference_scores``; ``metrics_sweep_resident`` chains them all (SPEC.md §15 - §17).
   ``edge_match_counts_resident`` / ``edge_match_resident`` (gcs_truth_thin, gcs_match_offsets, gcs_edge_match): the one-to-one
   matching score of an edge map at every threshold at once (SPEC.md §27).

The host arithmetic exists once: ``_boundary_scores``, ``_region_scores_batch`` and ``evaluate.agreement_from_sums``.
"""
from __future__ import annotations

import weakref
from collections import namedtuple
from math import pi

import numpy as np

from . import _lib
from .evaluate import agreement_from_sums

SWEEP_LEVELS = 4096                                              # the most labels a region tree has (SPEC.md §14)
SWEEP_CUTS = 64                                                  # the most cuts one gcs_region_sweep call takes
MATCH_LEVELS = 256                                               # the most levels gcs_edge_match takes (SPEC.md §27)
MATCH_DIST2_MAX = 160                                            # the largest D2 gcs_match_offsets makes a table for


# ------------------------------------------------------------------------------------------------------------------------
# Argument checks

def _need_labels(labels, ndim, what="labels"):
    import torch
    if labels.dtype != torch.int32 or labels.dim() != ndim:
        raise ValueError(f"{what} must be {'an (H,W)' if ndim == 2 else 'a (B,H,W)'} int32 tensor")


def _need_truths(truths, labels):
    if truths.dim() != 3 or truths.shape[1:] != labels.shape or truths.element_size() != 2:
        raise ValueError("truths must be an (A,H,W) 16-bit tensor matching labels")


def _need_match(shape, device, truth, what):
    if tuple(shape) != (truth.b, truth.h, truth.w) or device != truth.device:
        raise ValueError(f"{what} batch does not match the resident truth (images, shape or device)")


def _need_two_pixels(h, w):
    if h * w < 2:
        raise ValueError(f"region agreement needs at least 2 pixels, got {h * w}")


def _need_cuts(regions):
    """The checked list of R and the positions that put it into strictly decreasing order (what the sweep calls want)."""
    try:
        regs = [int(r) for r in regions]
        same = all(r == q for r, q in zip(regs, regions))
    except (TypeError, ValueError):
        raise ValueError("regions must be a list of integers") from None
    if not same or not 1 <= len(regs) <= SWEEP_CUTS or len(set(regs)) != len(regs) or min(regs) < 1 or max(regs) > SWEEP_LEVELS:
        raise ValueError(f"regions must be 1..{SWEEP_CUTS} distinct integers in 1..{SWEEP_LEVELS}")
    return regs, sorted(range(len(regs)), key=lambda j: -regs[j])


def _need_tree(labels, merges, alive, device, whose, truth=None):
    """The checks of a region tree's three tensors (``Segmenter.region_tree_device``), the labels against ``truth`` when given;
    -> them, contiguous."""
    import torch
    _need_labels(labels, 3)
    if truth is not None:
        _need_match(labels.shape, labels.device, truth, "label")
    b = labels.shape[0]
    if merges.dtype != torch.int32 or merges.dim() != 3 or merges.shape[0] != b or merges.shape[2] != 2 or \
            not 1 <= merges.shape[1] + 1 <= SWEEP_LEVELS:
        raise ValueError(f"merges must be a (B, K - 1, 2) int32 tensor with K in 1..{SWEEP_LEVELS}")
    if alive.dtype != torch.int32 or tuple(alive.shape) != (b,):
        raise ValueError("alive must be a (B,) int32 tensor")
    if merges.device != device or alive.device != device:
        raise ValueError(f"merges / alive are not on the device of {whose}")
    return labels.contiguous(), merges.contiguous(), alive.contiguous()


def _need_contours(contours, labels):
    _need_labels(contours, 3, "contours")
    if contours.shape != labels.shape or contours.device != labels.device:
        raise ValueError("contours must match labels (shape and device)")


def _need_tree_and_cuts(labels, merges, alive, regions, truth):
    """Every check of a sweep over a tree's contingency tables, before anything runs -> (labels, merges, alive, regs, order)."""
    labels, merges, alive = _need_tree(labels, merges, alive, truth.device, "the resident truth", truth)
    regs, order = _need_cuts(regions)
    _need_two_pixels(*labels.shape[1:])
    k = merges.shape[1] + 1
    if truth.t * k * truth.stride > 1 << 30:
        raise ValueError(f"the leaf tables [{truth.t}][{k}][{truth.stride}] exceed 2^30 counters")
    return labels, merges, alive, regs, order


# ------------------------------------------------------------------------------------------------------------------------
# Host arithmetic

def _boundary_scores(g, ann) -> dict:
    """metrics.py:69-74 and :88-96 on Python floats (the same IEEE doubles, no NumPy scalar boxing per operation): g = sum bd(L),
    ann = per annotator [recall numerator, recall denominator, precision numerator], flat."""
    a = len(ann) // 3
    recall = 0
    precision = 0
    for i in range(0, 3 * a, 3):                                 # in annotator order
        recall += ann[i] / ann[i + 1]                            # ZeroDivisionError as metrics.py:72
        precision += ann[i + 2] / g                              # ZeroDivisionError as metrics.py:94
    recall /= a
    precision /= a
    s = recall + precision
    return {"recall": recall, "precision": precision, "fmeasure": 0.0 if s == 0 else 2.0 * precision * recall / s}


def scores_from_counts(counts) -> dict:
    """metrics.py:69-74 and :88-96 arithmetic on the integer counts [1 + 3A] (plain Python floats)."""
    c = np.asarray(counts).astype(np.float64).tolist()           # rounds as float(np.uint64) does
    return _boundary_scores(c[0], c[1:])


def _region_scores_batch(under, under_np, area, perim, first, nx, ny):
    """metrics.py:128-146 and :188-201 for a batch: under / under_np [T] = the integer sums of metrics.py:129-130, :137-139
    (exact in any order), area / perim [B][n_seg]. The sums of fractions keep the reference's order, term by term
    (metrics.py:131, :140, :194-201)."""
    b = len(first) - 1
    u_t = under.astype(np.float64) / (nx * ny)
    unp_t = under_np.astype(np.float64) / (nx * ny)
    max_area = float(nx * ny)
    a64 = area.astype(np.int64)
    per = perim.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = 4 * pi * (a64 / max_area) * a64 / (per * per)                    # metrics.py:199, element by element
    out = []
    u_t, unp_t, first = u_t.tolist(), unp_t.tolist(), np.asarray(first).tolist()  # Python floats, as in _boundary_scores
    terms, has = terms.tolist(), (per > 0).tolist()
    for i in range(b):
        t0, t1 = first[i], first[i + 1]
        under_i = 0.
        under_np_i = 0.
        for t in range(t0, t1):                                                  # metrics.py:131,140: += in annotator order
            under_i += u_t[t]
            under_np_i += unp_t[t]
        compactness = 0
        for term, ok in zip(terms[i], has[i]):                                   # metrics.py:194-201: index order
            if ok:
                compactness += term
        out.append({"underseg": under_i / (t1 - t0), "undersegNP": under_np_i / (t1 - t0), "compactness": float(compactness)})
    return out


def region_scores_from_counts(hist, area, perim, n_truth, nx, ny) -> dict:
    """metrics.py:128-146 and :188-201 arithmetic on the integer tables of one image, giving the reference's floats.
    ``n_truth[a]`` = max(truth_a) + 1 (metrics.py:116): only those columns of annotator a exist there."""
    area64 = np.asarray(area).astype(np.int64)
    under, under_np = [], []
    for a in range(hist.shape[0]):
        h = hist[a][:, :int(n_truth[a])].astype(np.int64)
        under.append(int(np.sum(area64 - h.max(axis=1))))                        # metrics.py:129-130
        under_np.append(int(np.sum(np.minimum(h, h.sum(axis=1)[:, None] - h))))  # metrics.py:137-139
    return _region_scores_batch(np.array(under, np.int64), np.array(under_np, np.int64), area64[None], np.asarray(perim)[None],
                                [0, hist.shape[0]], nx, ny)[0]


def _agreement_arrays(raw, n):
    """A downloaded agreement block of n maps, ``sums uint64 [n][4] | terms float64 [n][4]`` -> the two arrays."""
    return raw[:n * 4].view(np.uint64).reshape(n, 4), raw[n * 4:n * 8].view(np.float64).reshape(n, 4)


def _batch_scores(counts, seg_max, reg, first, n_pixels, agree=None) -> list:
    """The dicts of a batch from its counts [B + 3T] (gcs.h layout), label maxima, region scores and agreement scores."""
    b = len(first) - 1
    cf = np.asarray(counts).astype(np.float64).tolist()
    first = np.asarray(first).tolist()
    out = []
    for i in range(b):
        out.append({"regions": int(seg_max[i]) + 1,                              # metrics.py:51
                    **_boundary_scores(cf[i], cf[b + 3 * first[i]:b + 3 * first[i + 1]]), **reg[i],
                    "density": cf[i] / float(n_pixels),                          # metrics.py:157
                    **(agree[i] if agree is not None else {})})
    return out


# ------------------------------------------------------------------------------------------------------------------------
# 1. One image, truth uploaded per call

def _truth_stack(segments_truth, device):
    import torch
    t = np.stack([np.asarray(s).astype(np.uint16) for s in segments_truth])
    return t, torch.from_numpy(np.ascontiguousarray(t.view(np.int16))).to(device)


def boundary_counts_device(labels, truths):
    """labels: (H,W) int32 device tensor; truths: (A,H,W) int16/uint16-bits device tensor.
    Returns the uint64 counts [1 + 3A] as a host numpy array."""
    import torch
    lib = _lib.load()
    _need_labels(labels, 2)
    _need_truths(truths, labels)
    a, h, w = truths.shape
    labels, truths = labels.contiguous(), truths.contiguous()
    scratch = torch.empty(lib.gcs_boundary_scratch_bytes(a, h, w), dtype=torch.uint8, device=labels.device)
    counts = torch.empty(1 + 3 * a, dtype=torch.int64, device=labels.device)
    _lib.check(lib.gcs_boundary_counts(labels.data_ptr(), truths.data_ptr(), a, h, w, scratch.data_ptr(),
                                       counts.data_ptr(), torch.cuda.current_stream(labels.device).cuda_stream),
               "gcs_boundary_counts")
    return counts.cpu().numpy().astype(np.uint64)


def boundary_scores_device(labels, segments_truth) -> dict:
    """labels: (H,W) int32 device tensor (e.g. a row of Segmenter.segment_device);
    segments_truth: list of (H,W) integer arrays (groundtruth.get_segment_from_filename)."""
    if len(segments_truth) == 0:
        raise ZeroDivisionError("no annotator maps (metrics.py:74 divides by len(img_truth))")
    return scores_from_counts(boundary_counts_device(labels, _truth_stack(segments_truth, labels.device)[1]))


def _region_tables(labels, truths, n_segments, n_truth_labels):
    """gcs_region_counts on checked tensors: the device tables (hist [A,n_segments,n_truth_labels], area, perimeters)."""
    import torch
    a, h, w = truths.shape
    labels, truths = labels.contiguous(), truths.contiguous()
    hist = torch.empty((a, n_segments, n_truth_labels), dtype=torch.int32, device=labels.device)
    area = torch.empty(n_segments, dtype=torch.int32, device=labels.device)
    perim = torch.empty(n_segments, dtype=torch.int32, device=labels.device)
    _lib.check(_lib.load().gcs_region_counts(labels.data_ptr(), truths.data_ptr(), a, h, w, int(n_segments),
                                             int(n_truth_labels), hist.data_ptr(), area.data_ptr(), perim.data_ptr(),
                                             torch.cuda.current_stream(labels.device).cuda_stream), "gcs_region_counts")
    return hist, area, perim


def region_counts_device(labels, truths, n_segments, n_truth_labels):
    """labels: (H,W) int32 device tensor with values < n_segments; truths: (A,H,W) 16-bit device tensor with
    values < n_truth_labels. Returns host arrays (hist [A,n_segments,n_truth_labels], area, perimeters)."""
    _need_labels(labels, 2)
    _need_truths(truths, labels)
    return tuple(x.cpu().numpy() for x in _region_tables(labels, truths, n_segments, n_truth_labels))


def _agreement_launch(hist, img_of_d, seg_max_d, t, n_seg, stride, out):
    """gcs_region_agreement on device tables hist [t][n_seg][stride] into the block ``out`` (int64 [8 t]: sums | terms); its
    scratch goes back to the stream-ordered allocator."""
    import torch
    lib = _lib.load()
    scratch = torch.empty(lib.gcs_region_agreement_scratch_bytes(t, n_seg, stride), dtype=torch.uint8, device=hist.device)
    _lib.check(lib.gcs_region_agreement(hist.data_ptr(), img_of_d.data_ptr() if img_of_d is not None else None,
                                        seg_max_d.data_ptr() if seg_max_d is not None else None, t, n_seg, stride,
                                        scratch.data_ptr(), out.data_ptr(), out.data_ptr() + t * 32,
                                        torch.cuda.current_stream(hist.device).cuda_stream), "gcs_region_agreement")


def region_agreement_device(labels, segments_truth) -> dict:
    """``evaluate.region_agreement`` (PRI, VoI, covering; SPEC.md §8) of one (H,W) int32 device label map: the contingency
    tables by gcs_region_counts, their reduction by gcs_region_agreement, 64 bytes per annotator map downloaded."""
    import torch
    if len(segments_truth) == 0:
        raise ZeroDivisionError("no annotator maps")
    _need_labels(labels, 2)
    t, truths = _truth_stack(segments_truth, labels.device)
    h, w = labels.shape
    _need_two_pixels(h, w)
    a = len(t)
    n_seg = int(labels.max().item()) + 1
    hist, area, perim = _region_tables(labels, truths, n_seg, int(t.max()) + 1)
    out = torch.empty(a * 8, dtype=torch.int64, device=labels.device)
    _agreement_launch(hist, None, None, a, n_seg, hist.shape[2], out)
    return agreement_from_sums(*_agreement_arrays(out.cpu().numpy(), a), [0, a], h * w)[0]


def all_scores_device(labels, segments_truth) -> dict:
    """Every number of ``evaluate.metrics.get_metrics()`` (= metrics.py:246-255 plus F) for a device label map:
    stencils, masked sums and histograms on the GPU, the reference's float arithmetic on the host."""
    if len(segments_truth) == 0:
        raise ZeroDivisionError("no annotator maps (metrics.py:74 divides by len(img_truth))")
    t, truths = _truth_stack(segments_truth, labels.device)
    nx, ny = labels.shape
    n_segments = int(labels.max().item()) + 1                    # metrics.py:51
    n_truth = [int(s.max()) + 1 for s in t]                      # metrics.py:116
    counts = boundary_counts_device(labels, truths)
    out = {"regions": n_segments}
    out.update(scores_from_counts(counts))
    hist, area, perim = region_counts_device(labels, truths, n_segments, max(n_truth))
    out.update(region_scores_from_counts(hist, area, perim, n_truth, nx, ny))
    out["density"] = float(counts[0]) / float(nx * ny)           # metrics.py:157
    return out


# ------------------------------------------------------------------------------------------------------------------------
# 2. A batch, truth uploaded per call

def all_scores_batch_device(labels, truth, first=None, img_of=None, n_truth=None, n_segments=None, agreement=False) -> list:
    """Every number of ``evaluate.metrics.get_metrics()`` for a whole batch of device label maps in THREE launches
    (boundary maps, boundary counts, region tables) and one device-to-host copy per table, instead of a scoring call
    and two host round trips per image (metrics.py:58-201 loops over images in script.py:22).

    labels: (B,H,W) int32 device tensor; truth / first / img_of / n_truth: ``PackedTruth.stack(ids)`` (or the same
    layout built by hand): all annotator maps of image 0, then of image 1, ...; n_segments: max label + 1 over the
    batch (default: read from the labels; metrics.py:51 per image is the image's own max + 1, applied below).
    agreement=True: each dict also gets "PRI", "VoI" and "covering" (SPEC.md §8) from one more launch on the same tables.
    A ``DeviceTruth`` as ``truth``: ``all_scores_batch_resident``."""
    import torch
    if isinstance(truth, DeviceTruth):
        return all_scores_batch_resident(labels, truth, n_segments, agreement=agreement)
    lib = _lib.load()
    _need_labels(labels, 3)
    b, h, w = labels.shape
    truth = np.ascontiguousarray(truth, np.uint16)
    t = truth.shape[0]
    if truth.shape[1:] != (h, w) or len(first) != b + 1 or int(first[-1]) != t or len(img_of) != t:
        raise ValueError("truth stack does not match the label batch")
    if any(int(first[i + 1]) == int(first[i]) for i in range(b)):
        raise ZeroDivisionError("an image has no annotator maps (metrics.py:74 divides by len(img_truth))")
    dev = labels.device
    labels = labels.contiguous()
    seg_max_dev = seg_max = labels.reshape(b, -1).max(dim=1).values     # per-image max label, one small copy below
    truth_d = torch.from_numpy(truth.view(np.int16)).to(dev)
    first_d = torch.from_numpy(np.ascontiguousarray(first, np.int32)).to(dev)
    img_of_d = torch.from_numpy(np.ascontiguousarray(img_of, np.int32)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scratch = torch.empty(lib.gcs_boundary_batch_scratch_bytes(b, t, h, w), dtype=torch.uint8, device=dev)
    counts = torch.empty(b + 3 * t, dtype=torch.int64, device=dev)
    _lib.check(lib.gcs_boundary_counts_batch(labels.data_ptr(), truth_d.data_ptr(), img_of_d.data_ptr(), b, t, h, w,
                                             scratch.data_ptr(), counts.data_ptr(), stream), "gcs_boundary_counts_batch")
    seg_max = seg_max.cpu().numpy()
    n_seg = int(n_segments) if n_segments is not None else int(seg_max.max()) + 1
    stride = int(max(n_truth))
    a_max = int(max(int(first[i + 1]) - int(first[i]) for i in range(b)))
    hist = torch.empty((t, n_seg, stride), dtype=torch.int32, device=dev)
    area = torch.empty((b, n_seg), dtype=torch.int32, device=dev)
    perim = torch.empty((b, n_seg), dtype=torch.int32, device=dev)
    _lib.check(lib.gcs_region_counts_batch(labels.data_ptr(), truth_d.data_ptr(), first_d.data_ptr(), b, t, a_max, h, w,
                                           n_seg, stride, hist.data_ptr(), area.data_ptr(), perim.data_ptr(), stream),
               "gcs_region_counts_batch")
    agree = None
    if agreement:
        _need_two_pixels(h, w)
        agr = torch.empty(t * 8, dtype=torch.int64, device=dev)
        _agreement_launch(hist, img_of_d, seg_max_dev.to(torch.int32).contiguous(), t, n_seg, stride, agr)
        agree = agreement_from_sums(*_agreement_arrays(agr.cpu().numpy(), t), first, h * w)
    counts = counts.cpu().numpy().astype(np.uint64)
    hist, area, perim = hist.cpu().numpy(), area.cpu().numpy(), perim.cpu().numpy()
    reg = []
    for i in range(b):
        t0, t1, n_i = int(first[i]), int(first[i + 1]), int(seg_max[i]) + 1      # metrics.py:51: the image's own max + 1
        reg.append(region_scores_from_counts(hist[t0:t1, :n_i], area[i, :n_i], perim[i, :n_i], n_truth[t0:t1], h, w))
    return _batch_scores(counts, seg_max, reg, first, h * w, agree)


# ------------------------------------------------------------------------------------------------------------------------
# 3. Resident ground truth. metrics.py:48-49 derives find_boundaries(truth) anew for every image it scores and groundtruth.py:44-48
# rescans the split directories per id; the batched scorer above still uploads the annotator maps (40 MB per 24 images) and
# re-derives their boundary / dilated planes on every call - 67 % of a segment + score loop. The maps are constants of the data
# set: a DeviceTruth holds them on the device once, as uint8 maps (region tables) and as bit planes of bd(T) and dil5(bd(T)) with
# the counts sum bd(T) (gcs_truth_prepare), and a scoring call touches nothing else of them.

def _block_layout(b, t, cap, agreement):
    """The result block of a resident scoring call: ({slot: (byte offset, bytes)}, total bytes), every slot on a 16-byte
    boundary. The agreement slot (sums uint64 [t][4] | terms float64 [t][4]) comes LAST: the offsets before it do not depend on
    it, and a call without agreement copies only the part before it."""
    sizes = [("counts", (b + 3 * t) * 8), ("under", t * 8), ("under_np", t * 8), ("seg_max", b * 4), ("area", b * cap * 4),
             ("perim", b * cap * 4)] + ([("agreement", t * 64)] if agreement else [])
    offs, o = {}, 0
    for name, nbytes in sizes:
        offs[name] = (o, nbytes)
        o += (nbytes + 15) // 16 * 16
    return offs, o


# cap: segments the tables are laid out for; dev / host: the device block and its pinned mirror, offs: their _block_layout, used:
# the bytes in front of the agreement slot; scratch: the label maps' bit planes; hist: the contingency tables [t][cap][stride],
# which never leave the device; agr_scratch: scratch of gcs_region_agreement, or None (a block without the agreement slot)
_ResultBlock = namedtuple("_ResultBlock", "cap dev host offs scratch hist agr_scratch used")


class DeviceTruth:
    """The annotator maps of a list of equally shaped images, resident on a device in the form the scorer consumes.

    Build with ``DeviceTruth(truth, first, img_of, n_truth, device)`` from a ``PackedTruth.stack(ids)`` tuple, or
    ``PackedTruth.to_device(ids, device)``. Pass it to ``all_scores_batch_device(labels, device_truth)``."""

    def __init__(self, truth, first, img_of, n_truth, device="cuda"):
        import torch
        lib = _lib.load()
        truth = np.ascontiguousarray(truth, np.uint16)
        self.t, self.h, self.w = (int(x) for x in truth.shape)
        self.first = np.ascontiguousarray(first, np.int32)
        self.img_of = np.ascontiguousarray(img_of, np.int32)
        self.b = len(self.first) - 1
        if int(self.first[-1]) != self.t or len(self.img_of) != self.t:
            raise ValueError("first / img_of do not describe the truth stack")
        if np.any(np.diff(self.first) <= 0):
            raise ZeroDivisionError("an image has no annotator maps (metrics.py:74 divides by len(img_truth))")
        self.n_truth = np.asarray(n_truth, np.int64)
        self.stride = int(self.n_truth.max())
        self.a_max = int(np.diff(self.first).max())
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:           # 'cuda' -> the current device, so that it compares equal to a tensor's
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        with torch.cuda.device(dev):
            t16 = torch.from_numpy(truth.view(np.int16)).to(dev)
            self.planes = torch.empty(lib.gcs_bit_planes_bytes(self.t, self.h, self.w), dtype=torch.uint8, device=dev)
            self.bd_counts = torch.empty(self.t, dtype=torch.int64, device=dev)
            self.u8 = self.stride <= 256                       # BSD500: the largest annotator label is 208
            self.maps = torch.empty((self.t, self.h, self.w), dtype=torch.uint8, device=dev) if self.u8 else t16
            _lib.check(lib.gcs_truth_prepare(t16.data_ptr(), self.t, self.h, self.w, self.planes.data_ptr(),
                                             self.bd_counts.data_ptr(), self.maps.data_ptr() if self.u8 else None,
                                             torch.cuda.current_stream(dev).cuda_stream), "gcs_truth_prepare")
            self.first_d = torch.from_numpy(self.first).to(dev)
            self.img_of_d = torch.from_numpy(self.img_of).to(dev)
            torch.cuda.current_stream(dev).synchronize()       # t16 may go (uint8 case): the kernels that read it are done
        self._out = None                                       # the _ResultBlock
        self._scratch = None
        self._pending = None                                   # weak reference to the submission that owns the result block
        self._thin = None                                      # SPEC.md §27: (thin planes, |Q_t| on the device, |Q_t| on the host)

    def thin_planes(self):
        """SPEC.md §27: ``(thin, counts, n_thin)`` - the contours Q_t = ``evaluate.thin_boundaries(s_t)`` as a (T,H,W) uint8
        device tensor, |Q_t| as a (T,) int32 device tensor and as a host int64 array. Made by gcs_truth_thin on first use and
        kept; nothing else of the truth changes."""
        import torch
        if self._thin is None:
            lib = _match_lib()
            if self.h > 4096 or self.w > 4096:
                raise ValueError("the matcher takes images of at most 4096 x 4096 pixels")
            with torch.cuda.device(self.device):
                thin = torch.empty((self.t, self.h, self.w), dtype=torch.uint8, device=self.device)
                counts = torch.empty(self.t, dtype=torch.int32, device=self.device)
                _lib.check(lib.gcs_truth_thin(self.maps.data_ptr(), self.t, self.h, self.w, int(self.u8), thin.data_ptr(),
                                              counts.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "gcs_truth_thin")
                self._thin = (thin, counts, counts.cpu().numpy().astype(np.int64))
        return self._thin

    def _uncollected(self):
        """The submission whose numbers still sit in this truth's ONE result block, or None (collected, or dropped)."""
        p = self._pending() if self._pending is not None else None
        return p if p is not None and not p._collected else None

    def _buffers(self, n_seg, agreement=False) -> _ResultBlock:
        """ONE device block for everything a call returns (_block_layout) and its pinned mirror: one device-to-host copy of a few
        KB and one synchronisation per call instead of five; the contingency tables stay on the device (gcs_region_reduce takes
        the two sums metrics.py:128-140 needs out of them).

        ONE entry per DeviceTruth (so one submission at a time: submit_scores_batch_resident refuses a second one while the
        first is uncollected), sized to a CAPACITY of segments (the next power of two, at least 8): a data-set loop over
        connected-region maps, whose label count differs from batch to batch, reuses it and reallocates - dropping the old
        blocks - only when a batch needs more, or needs the agreement slot and its scratch for the first time (the kernels take
        the capacity as their table stride; segments that do not occur have area 0 and perimeter 0 and add nothing to any
        score)."""
        import torch
        cap = 8                                                 # (k-means maps of the default k stay at their exact size)
        while cap < n_seg:
            cap *= 2
        if self._scratch is None:                               # the label maps' bit planes: does not depend on n_seg
            self._scratch = torch.empty(_lib.load().gcs_bit_planes_bytes(self.b, self.h, self.w), dtype=torch.uint8,
                                        device=self.device)
        ent = self._out
        if ent is None or ent.cap < cap or (agreement and ent.agr_scratch is None):
            self._out = ent = None                              # the old blocks go back to the allocator first
            offs, total = _block_layout(self.b, self.t, cap, agreement)
            dev_blk = torch.empty(total, dtype=torch.uint8, device=self.device)
            host_blk = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            hist = torch.empty(self.t * cap * self.stride, dtype=torch.int32, device=self.device)
            agr_scratch = None
            if agreement:
                agr_scratch = torch.empty(_lib.load().gcs_region_agreement_scratch_bytes(self.t, cap, self.stride),
                                          dtype=torch.uint8, device=self.device)
            ent = self._out = _ResultBlock(cap, dev_blk, host_blk, offs, self._scratch, hist, agr_scratch,
                                           offs["agreement"][0] if agreement else total)
        return ent


# host / offs / cap: the pinned result block, its layout and capacity; event: recorded behind the result copy
_Submission = namedtuple("_Submission", "truth b h w n_seg cap host offs event agreement")


class _PendingScores:
    """Scores of one batch on their way: kernels and the result copy are enqueued, ``result()`` waits for the copy and does the
    reference's float arithmetic (``all_scores_batch_resident`` = submit + result). The numbers wait in the pinned result block of
    their DeviceTruth, and there is ONE such block per DeviceTruth: collect this submission (or drop it) before submitting the
    next batch against the SAME DeviceTruth. Submitting a batch against ANOTHER DeviceTruth before collecting this one is the
    intended pipelining: its kernels run under this one's host arithmetic."""

    def __init__(self, submission):
        self._s = submission
        self._collected = False

    def result(self) -> list:
        """The scores, once: the result block belongs to the next submission from here on (also when this raises what the
        reference raises for a degenerate image)."""
        if self._collected:
            raise RuntimeError("this submission has been collected already: its result block may hold a later batch by now")
        self._s.event.synchronize()
        try:
            return self._finish()
        finally:
            self._collected = True

    def _finish(self) -> list:
        s, offs = self._s, self._s.offs
        raw = s.host.numpy()
        view = lambda k, dt: raw[offs[k][0]:offs[k][0] + offs[k][1]].view(dt)
        seg_max = view("seg_max", np.int32)
        if int(seg_max.max()) >= s.n_seg:
            raise ValueError(f"a label map holds label {int(seg_max.max())} but n_segments = {s.n_seg}")
        area = view("area", np.int32).reshape(s.b, s.cap)[:, :s.n_seg]     # laid out at the capacity; columns >= n_seg are zero
        perim = view("perim", np.int32).reshape(s.b, s.cap)[:, :s.n_seg]
        first = s.truth.first
        reg = _region_scores_batch(view("under", np.uint64), view("under_np", np.uint64), area, perim, first, s.h, s.w)
        agree = agreement_from_sums(*_agreement_arrays(view("agreement", np.int64), s.truth.t), first, s.h * s.w) if s.agreement else None
        return _batch_scores(view("counts", np.uint64), seg_max, reg, first, s.h * s.w, agree)   # counts < 2^53: exact floats


def submit_scores_batch_resident(labels, truth: DeviceTruth, n_segments=None, agreement=False) -> _PendingScores:
    """Enqueue the scoring of a (B,H,W) int32 device label batch against resident ground truth; ``.result()`` returns what
    ``all_scores_batch_device`` returns. One result block per DeviceTruth: collect a submission (``.result()``), or drop it,
    before submitting the next batch against the SAME DeviceTruth - a second submission while the first is uncollected raises
    RuntimeError instead of overwriting the first one's numbers. Submissions against different DeviceTruth objects pipeline
    freely. agreement=True: one more launch on the contingency tables the scorer leaves on the
    device (gcs_region_agreement, rows bounded by the labels' maxima) and "PRI", "VoI", "covering" in every dict, from the same
    single copy."""
    import torch
    lib = _lib.load()
    _need_labels(labels, 3)
    b, h, w = labels.shape
    _need_match((b, h, w), labels.device, truth, "label")
    labels = labels.contiguous()
    n_seg = int(n_segments) if n_segments is not None else int(labels.max().item()) + 1
    if agreement:
        _need_two_pixels(h, w)
    if truth._uncollected() is not None:
        raise RuntimeError("one result block per DeviceTruth: collect the earlier submission with .result() (or drop it) before "
                           "submitting the next batch against the same DeviceTruth")
    blk = truth._buffers(n_seg, agreement)
    base = blk.dev.data_ptr()
    ptr = {k: base + o for k, (o, _) in blk.offs.items()}
    with torch.cuda.device(truth.device):
        stream = torch.cuda.current_stream(truth.device)
        _lib.check(lib.gcs_score_batch_resident(labels.data_ptr(), truth.planes.data_ptr(), truth.bd_counts.data_ptr(),
                                                truth.maps.data_ptr(), 1 if truth.u8 else 0, truth.first_d.data_ptr(),
                                                truth.img_of_d.data_ptr(), b, truth.t, truth.a_max, h, w, blk.cap, truth.stride,
                                                blk.scratch.data_ptr(), blk.hist.data_ptr(), ptr["counts"], ptr["seg_max"],
                                                ptr["area"], ptr["perim"], ptr["under"], ptr["under_np"], stream.cuda_stream),
                   "gcs_score_batch_resident")
        if agreement:
            _lib.check(lib.gcs_region_agreement(blk.hist.data_ptr(), truth.img_of_d.data_ptr(), ptr["seg_max"], truth.t, blk.cap,
                                                truth.stride, blk.agr_scratch.data_ptr(), ptr["agreement"],
                                                ptr["agreement"] + truth.t * 32, stream.cuda_stream), "gcs_region_agreement")
        used = blk.dev.numel() if agreement else blk.used       # the block may carry the agreement slot of an earlier call
        if used == blk.dev.numel():
            blk.host.copy_(blk.dev, non_blocking=True)
        else:
            blk.host[:used].copy_(blk.dev[:used], non_blocking=True)
        event = torch.cuda.Event()
        event.record(stream)
    pending = _PendingScores(_Submission(truth, b, h, w, n_seg, blk.cap, blk.host, blk.offs, event, agreement))
    truth._pending = weakref.ref(pending)
    return pending


def all_scores_batch_resident(labels, truth: DeviceTruth, n_segments=None, agreement=False) -> list:
    """``all_scores_batch_device`` on resident ground truth: kernels on bit planes and uint8 maps, the tables reduced on the
    device, ONE device-to-host copy of a few KB. ``n_segments``: an upper bound of max label + 1 over the batch (the
    Segmenter's k); None reads it from the labels (one more synchronisation)."""
    return submit_scores_batch_resident(labels, truth, n_segments, agreement).result()


# ------------------------------------------------------------------------------------------------------------------------
# 4a. Boundary scores of every cut of a region tree at once (SPEC.md §15): three histograms of the contour map per image, one
# pass over the map.

def boundary_sweep_resident(contours, alive, truth: DeviceTruth):
    """contours: (B,H,W) int32 device tensor of ``Segmenter.contour_map_device``; alive: the (B,) int32 tensor beside it; truth: the resident ground truth of the same images. Returns host arrays
    ``(hist_map uint32 [B][K + 1], hist_rec uint32 [T][K + 1], hist_prec uint32 [T][K + 1])`` with K = max(alive) (every level
    the batch's trees have): #{U = s}, #{bd(T_t) : M5(U) = s}, #{dil5(bd(T_t)) : U = s}. Buffers of its own: ``truth``'s result block and
    its one-submission rule are not touched."""
    import torch
    lib = _lib.load()
    _need_labels(contours, 3, "contours")
    b, h, w = contours.shape
    _need_match((b, h, w), contours.device, truth, "contour")
    if tuple(alive.shape) != (b,):
        raise ValueError("alive must be a (B,) tensor")
    if h > 4096 or w > 4096:
        raise ValueError("the sweep takes images of at most 4096 x 4096 pixels")
    k = min(max(1, int(alive.max().item())), SWEEP_LEVELS)       # U lies in 0 .. alive: the bins of the largest tree of the batch
    contours = contours.contiguous()
    with torch.cuda.device(truth.device):
        hist = torch.empty((b + 2 * truth.t, k + 1), dtype=torch.int32, device=truth.device)
        _lib.check(lib.gcs_boundary_sweep_resident(contours.data_ptr(), truth.planes.data_ptr(), truth.img_of_d.data_ptr(), b, truth.t,
                                                   h, w, k, hist.data_ptr(), torch.cuda.current_stream(truth.device).cuda_stream),
                   "gcs_boundary_sweep_resident")
        raw = hist.cpu().numpy().view(np.uint32)
    ann = raw[b:].reshape(truth.t, 2, k + 1)
    return raw[:b].copy(), ann[:, 0].copy(), ann[:, 1].copy()


def sweep_counts(hists, alive, bd_counts, first, regions) -> np.ndarray:
    """The integer counts ``gcs_boundary_counts_resident`` returns for the cut at every R of ``regions``, from the histograms of
    ``boundary_sweep_resident``: uint64 [len(regions)][B + 3T] in that call's layout ([b], then per annotator [B + 3t] recall
    numerator, [B + 3t + 1] = bd_counts[t], [B + 3t + 2] precision numerator): suffix sums over the bins above
    max(0, alive_b - R)."""
    hist_map, hist_rec, hist_prec = (np.asarray(x).astype(np.uint64) for x in hists)
    alive = np.asarray(alive).astype(np.int64).ravel()
    first = np.asarray(first).astype(np.int64)
    bd_counts = np.asarray(bd_counts).astype(np.uint64).ravel()
    b, t, nb = hist_map.shape[0], hist_rec.shape[0], hist_map.shape[1]
    if len(alive) != b or len(first) != b + 1 or int(first[-1]) != t or len(bd_counts) != t:
        raise ValueError("alive / first / bd_counts do not describe the histograms")
    # above[s] = sum of the bins > s (s = 0 .. nb - 1)
    above = [np.concatenate([np.cumsum(x[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((x.shape[0], 1), np.uint64)], axis=1)
             for x in (hist_map, hist_rec, hist_prec)]
    img_of = np.repeat(np.arange(b), np.diff(first))
    out = np.zeros((len(regions), b + 3 * t), np.uint64)
    for j, r in enumerate(regions):
        if int(r) < 1:
            raise ValueError("R must be >= 1")
        tau = np.minimum(np.maximum(alive - int(r), 0), nb - 1)
        out[j, :b] = above[0][np.arange(b), tau]
        out[j, b::3] = above[1][np.arange(t), tau[img_of]]
        out[j, b + 1::3] = bd_counts
        out[j, b + 2::3] = above[2][np.arange(t), tau[img_of]]
    return out


def sweep_scores(hists, alive, bd_counts, first, regions) -> list:
    """Per image a list with one ``{"recall", "precision", "fmeasure"}`` per R of ``regions``: the floats
    ``all_scores_batch_resident`` gives for ``cut_regions_device(..., R)`` (the same integer counts through the same float
    operations in the same order, ``_boundary_scores``). ZeroDivisionError where the reference raises it: a cut without a
    boundary pixel (R = 1), an annotator map without one."""
    counts = sweep_counts(hists, alive, bd_counts, first, regions).astype(np.float64).tolist()
    first = np.asarray(first).astype(np.int64).tolist()
    b = len(first) - 1
    return [[_boundary_scores(c[i], c[b + 3 * first[i]:b + 3 * first[i + 1]]) for c in counts] for i in range(b)]


def edge_sweep_resident(edges, truth: DeviceTruth, levels=256, step=None):
    """Boundary scores of an edge-strength map at ``levels`` thresholds at once (SPEC.md §22). edges: (B,H,W) int32 device tensor of
    non-negative strengths (``Segmenter.edges_device``); truth: the resident ground truth of the same images. The map is quantised
    on the device, q = min(levels, edges // step) with ``step`` defaulting to ceil((batch max + 1) / levels) (one read from the
    device), and swept like a contour map (gcs_boundary_sweep_resident with K = levels): level tau = 0 .. levels - 1 is the
    boundary map q > tau, i.e. edges >= step (tau + 1). Returns ``(recall, precision, fmeasure, step)``, float64 host arrays
    [B][levels]: the floats of ``evaluate.edge_scores`` at the thresholds step (tau + 1) - 1 (the same integer counts through the
    same float operations), zeros where a level leaves an image without a boundary pixel. ``evaluate.ods_ois(fmeasure,
    [step * (tau + 1) - 1 for tau in range(levels)])`` serves the table: its "regions" axis is then the threshold (ties go to the
    lowest)."""
    import torch
    from .evaluate import edge_scores_from_counts
    lib = _lib.load()
    _need_labels(edges, 3, "edges")
    b, h, w = edges.shape
    _need_match((b, h, w), edges.device, truth, "edge map")
    levels = int(levels)
    if not 1 <= levels <= SWEEP_LEVELS:
        raise ValueError(f"levels must be in 1 .. {SWEEP_LEVELS}")
    if h > 4096 or w > 4096:
        raise ValueError("the sweep takes images of at most 4096 x 4096 pixels")
    with torch.cuda.device(truth.device):
        if step is None:
            step = -(-(int(edges.max().item()) + 1) // levels)
        step = int(step)
        if step < 1:
            raise ValueError("step must be at least 1")
        q = torch.clamp(torch.div(edges, step, rounding_mode="floor"), max=levels).to(torch.int32).contiguous()
        hist = torch.empty((b + 2 * truth.t, levels + 1), dtype=torch.int32, device=truth.device)
        _lib.check(lib.gcs_boundary_sweep_resident(q.data_ptr(), truth.planes.data_ptr(), truth.img_of_d.data_ptr(), b, truth.t,
                                                   h, w, levels, hist.data_ptr(), torch.cuda.current_stream(truth.device).cuda_stream),
                   "gcs_boundary_sweep_resident")
        raw = hist.cpu().numpy().view(np.uint32)
        bd_counts = truth.bd_counts.cpu().numpy()
    ann = raw[b:].reshape(truth.t, 2, levels + 1)
    # q > tau is the cut of a tree with `levels` leaves at R = levels - tau: sweep_counts' suffix sums as they are
    counts = sweep_counts((raw[:b], ann[:, 0], ann[:, 1]), np.full(b, levels), bd_counts, truth.first,
                          [levels - tau for tau in range(levels)]).astype(np.float64).tolist()
    first = truth.first.tolist()
    out = np.zeros((3, b, levels))
    for tau, c in enumerate(counts):
        for i in range(b):
            sc = edge_scores_from_counts(c[i], c[b + 3 * first[i]:b + 3 * first[i + 1]])
            out[0, i, tau], out[1, i, tau], out[2, i, tau] = sc["recall"], sc["precision"], sc["fmeasure"]
    return out[0], out[1], out[2], step


# ------------------------------------------------------------------------------------------------------------------------
# 4a'. One-to-one matching counts of a level map at every level at once (SPEC.md §27): the levels are nested, so one incremental
# maximum matching per annotator map serves them all; one 64-lane workgroup per map, all maps of the batch side by side.

def _match_lib():
    lib = _lib.load()
    for name in _lib.MATCH_EXTENSIONS:
        if not hasattr(lib, name):
            raise ValueError(f"the device matcher needs a library that has it (this libgcs.so does not export {name})")
    return lib


def _match_offsets(lib, d2):
    table, n = np.zeros((512, 2), np.int32), np.zeros(1, np.int32)
    _lib.check(lib.gcs_match_offsets(int(d2), table.ctypes.data, n.ctypes.data), "gcs_match_offsets")
    return table[:int(n[0])].copy()


def _match_arguments(shape, device, truth, levels, max_dist2):
    """Every check of the match calls, before anything runs -> (levels, D2)."""
    from .evaluate import match_distance2
    b, h, w = shape
    _need_match((b, h, w), device, truth, "level map")
    levels = int(levels)
    if not 1 <= levels <= MATCH_LEVELS:
        raise ValueError(f"levels must be in 1 .. {MATCH_LEVELS}")
    if h > 4096 or w > 4096:
        raise ValueError("the matcher takes images of at most 4096 x 4096 pixels")
    d2 = match_distance2(h, w) if max_dist2 is None else int(max_dist2)
    if not 0 <= d2 <= MATCH_DIST2_MAX:
        raise ValueError(f"max_dist2 must be in 0 .. {MATCH_DIST2_MAX}, got {d2}")
    return levels, d2


def edge_match_counts_resident(q, truth: DeviceTruth, levels, max_dist2=None, stats=False):
    """SPEC.md §27. q: (B,H,W) int32 device tensor of levels, read as clamp(q, 0, levels); truth: the resident ground truth of the
    same images. Returns host int64 arrays ``(matched [T][levels], above [B][levels], n_thin [T])``: matched[t][tau] = the
    cardinality of a maximum matching between {q_b > tau} (b = img_of[t]) and Q_t = ``evaluate.thin_boundaries(s_t)`` with a pair
    allowed iff dy^2 + dx^2 <= ``max_dist2`` (None: ``evaluate.match_distance2(H, W)``; at most 160), above[b][tau] = #{q_b > tau},
    n_thin[t] = |Q_t|: what ``evaluate.match_count`` gives level by level. ``stats=True`` appends the kernel's uint32 [T][4]
    counters per map: search steps, 64-lane probes, deepest stack, failed searches. Buffers of its own."""
    import torch
    _need_labels(q, 3, "q")
    levels, d2 = _match_arguments(q.shape, q.device, truth, levels, max_dist2)
    lib = _match_lib()
    b, h, w = q.shape
    q = q.contiguous()
    with torch.cuda.device(truth.device):
        thin, _, n_thin = truth.thin_planes()
        offsets = torch.from_numpy(_match_offsets(lib, d2)).to(truth.device)
        cap = int(n_thin.max()) + 1
        ws = torch.empty(lib.gcs_edge_match_bytes(b, truth.t, h, w, cap), dtype=torch.uint8, device=truth.device)
        out = torch.empty((truth.t + b, levels), dtype=torch.int32, device=truth.device)
        _lib.check(lib.gcs_edge_match(q.data_ptr(), thin.data_ptr(), truth.img_of_d.data_ptr(), b, truth.t, h, w, levels,
                                      offsets.data_ptr(), len(offsets), cap, ws.data_ptr(), out.data_ptr(),
                                      out[truth.t:].data_ptr(), torch.cuda.current_stream(truth.device).cuda_stream),
                   "gcs_edge_match")
        raw = out.cpu().numpy().astype(np.int64)
        counters = ws[:16 * truth.t].cpu().numpy().view(np.uint32).reshape(truth.t, 4) if stats else None
    if (raw[:truth.t] < 0).any():
        raise _lib.GcsError("gcs_edge_match: a map's search stack overflowed")       # cap = max |Q_t| + 1: cannot happen
    res = (raw[:truth.t].copy(), raw[truth.t:].copy(), n_thin.copy())
    return res + (counters,) if stats else res


def edge_match_resident(edges, truth: DeviceTruth, levels=256, step=None, max_dist2=None):
    """One-to-one matching scores of an edge-strength map at ``levels`` thresholds at once (SPEC.md §27, the metric of §26).
    edges: (B,H,W) int32 device tensor of non-negative strengths; truth: the resident ground truth of the same images. The map is
    quantised exactly as in ``edge_sweep_resident`` (q = min(levels, edges // step), ``step`` defaulting to
    ceil((batch max + 1) / levels)); level tau is the boundary map edges >= step (tau + 1). Returns ``(recall, precision,
    fmeasure, step)``, float64 host arrays [B][levels]: row i holds, float for float, ``evaluate.match_scores(edges[i], truths_i,
    [step * (tau + 1) - 1 for tau in range(levels)], max_dist2)`` - the same integers through ``evaluate.edge_scores_from_counts``
    - zeros where a level leaves an image without a boundary pixel, ZeroDivisionError for an annotator map without a contour."""
    import torch
    from .evaluate import edge_scores_from_counts
    _need_labels(edges, 3, "edges")
    levels, d2 = _match_arguments(edges.shape, edges.device, truth, levels, max_dist2)
    _match_lib()
    b = edges.shape[0]
    with torch.cuda.device(truth.device):
        if step is None:
            step = -(-(int(edges.max().item()) + 1) // levels)
        step = int(step)
        if step < 1:
            raise ValueError("step must be at least 1")
        q = torch.clamp(torch.div(edges, step, rounding_mode="floor"), max=levels).to(torch.int32).contiguous()
    matched, above, n_thin = edge_match_counts_resident(q, truth, levels, d2)
    m, g, n = matched.astype(np.float64).tolist(), above.astype(np.float64).tolist(), n_thin.astype(np.float64).tolist()
    first = truth.first.tolist()
    out = np.zeros((3, b, levels))
    for i in range(b):
        for tau in range(levels):
            ann = []
            for t in range(first[i], first[i + 1]):
                ann += [m[t][tau], n[t], m[t][tau]]
            sc = edge_scores_from_counts(g[i][tau], ann)
            out[0, i, tau], out[1, i, tau], out[2, i, tau] = sc["recall"], sc["precision"], sc["fmeasure"]
    return out[0], out[1], out[2], step


# ------------------------------------------------------------------------------------------------------------------------
# 4b. The region metrics of every cut of a region tree at once (SPEC.md §16): the leaf tables from one pass over the pixels,
# every coarser table from the merge list by adding rows.

def _leaf_tables(labels, merges, truth, stream):
    """The contingency tables of the superpixels, uint32 [T][K][stride] on the device (one launch on ``stream``)."""
    import torch
    lib = _lib.load()
    (b, h, w), k = labels.shape, merges.shape[1] + 1
    hist = torch.empty(truth.t * k * truth.stride, dtype=torch.int32, device=truth.device)
    side = torch.empty(2 * b * k, dtype=torch.int32, device=truth.device)        # area | perimeter of the leaves: not used
    counts = lib.gcs_region_counts_batch_u8 if truth.u8 else lib.gcs_region_counts_batch
    _lib.check(counts(labels.data_ptr(), truth.maps.data_ptr(), truth.first_d.data_ptr(), b, truth.t, truth.a_max, h, w, k,
                      truth.stride, hist.data_ptr(), side.data_ptr(), side.data_ptr() + 4 * b * k, stream), "gcs_region_counts_batch")
    return hist


def _cuts_in_callers_order(arrays, n, t, order):
    """Arrays [n * t][m] as a sweep wrote them (cut-major, R decreasing) -> new arrays [n][t][m] in the caller's order of R."""
    out = []
    for src in arrays:
        dst = np.empty((n, t, src.shape[-1]), src.dtype)
        dst[order] = src.reshape(n, t, -1)
        out.append(dst)
    return tuple(out)


def region_sweep_resident(labels, merges, alive, truth: DeviceTruth, regions):
    """labels (B,H,W) int32, merges (B, K-1, 2) int32, alive (B,) int32: the device tensors ``Segmenter.region_tree_device`` returned;
    truth: the resident ground truth of the same images; regions: 1 .. 64 distinct integers in 1 .. 4096, in any order. Returns host
    arrays ``(sums uint64 [len(regions)][T][4], terms float64 [len(regions)][T][4])`` in the caller's order of ``regions``: per cut and
    annotator map what gcs_region_agreement writes for the contingency table of ``cut_regions_device(labels, merges, alive, R)``
    (the raw cuts: ``connectivity`` and ``min_region_size`` are not reflected; with ``tree_nodes="components"``, SPEC.md §18, the
    delivered maps are the raw cuts). Two launches (the leaf tables with K rows; the
    sweep) and one download. Buffers of its own: ``truth``'s result block and its one-submission rule are not touched."""
    import torch
    labels, merges, alive, regs, order = _need_tree_and_cuts(labels, merges, alive, regions, truth)
    b, h, w = labels.shape
    k, t, stride, n = merges.shape[1] + 1, truth.t, truth.stride, len(regs)
    lib = _lib.load()
    with torch.cuda.device(truth.device):
        dev = truth.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        hist = _leaf_tables(labels, merges, truth, stream)
        regs_d = torch.tensor([regs[j] for j in order], dtype=torch.int32).to(dev)
        ws = torch.empty(lib.gcs_region_sweep_workspace_bytes(t, k, stride, n), dtype=torch.uint8, device=dev)
        out = torch.empty(2 * n * t * 4, dtype=torch.int64, device=dev)          # an agreement block of n t maps, cut-major
        _lib.check(lib.gcs_region_sweep(hist.data_ptr(), merges.data_ptr() if k > 1 else None, alive.data_ptr(),
                                        truth.img_of_d.data_ptr(), regs_d.data_ptr(), b, t, k, stride, n, ws.data_ptr(),
                                        out.data_ptr(), out.data_ptr() + n * t * 32, stream), "gcs_region_sweep")
        raw = out.cpu().numpy()
    return _cuts_in_callers_order(_agreement_arrays(raw, n * t), n, t, order)


def sweep_agreement(sums, terms, first, n_pixels, regions) -> list:
    """Per image a list with one ``{"PRI", "VoI", "covering"}`` per R of ``regions``, from the arrays of ``region_sweep_resident``:
    ``agreement_from_sums`` per cut, so the floats are those of every other path of SPEC.md §8 on the same sums. Raises, per cut,
    if a table did not count every pixel (N_t != n_pixels: a label outside 0 .. K-1)."""
    sums, terms = np.asarray(sums), np.asarray(terms)
    n = len(regions)
    if sums.ndim != 3 or sums.shape != terms.shape or sums.shape[0] != n or sums.shape[2] != 4:
        raise ValueError("sums / terms must be [len(regions)][T][4] arrays")
    if int(np.asarray(first)[-1]) != sums.shape[1]:
        raise ValueError("first does not describe the annotator maps of sums / terms")
    per_cut = [agreement_from_sums(sums[j], terms[j], first, n_pixels) for j in range(n)]
    return [[per_cut[j][i] for j in range(n)] for i in range(len(first) - 1)]


# ------------------------------------------------------------------------------------------------------------------------
# 4c. The reference's region and shape metrics of every cut of a region tree at once (SPEC.md §17): the undersegmentation sums from
# the walk of 4b, area / perimeter / boundary count from one pass over (labels, contour map).

def under_sweep_resident(labels, merges, alive, truth: DeviceTruth, regions, agreement=False):
    """The arguments of ``region_sweep_resident``, checked, ordered and buffered in the same way. Returns the host array ``counts uint64
    [len(regions)][T][3] = {N_t, under, under_np}`` in the caller's order of ``regions``: per cut and annotator map the pixels its
    contingency table counts and the two integer sums of metrics.py:129-131 and :137-140 for ``cut_regions_device(labels, merges,
    alive, R)`` (the raw cuts). agreement=True: ``(counts, sums, terms)``, the last two what ``region_sweep_resident`` returns, bit
    for bit, from the same walk. Two launches (the leaf tables; gcs_region_sweep_under) and one download."""
    import torch
    labels, merges, alive, regs, order = _need_tree_and_cuts(labels, merges, alive, regions, truth)
    b, k, t, stride, n = labels.shape[0], merges.shape[1] + 1, truth.t, truth.stride, len(regs)
    lib = _lib.load()
    with torch.cuda.device(truth.device):
        dev = truth.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        hist = _leaf_tables(labels, merges, truth, stream)
        regs_d = torch.tensor([regs[j] for j in order], dtype=torch.int32).to(dev)
        ws = torch.empty(lib.gcs_region_sweep_under_workspace_bytes(t, k, stride, n), dtype=torch.uint8, device=dev)
        out = torch.empty(n * t * (11 if agreement else 3), dtype=torch.int64, device=dev)   # under [n t][3] | sums | terms [n t][4]
        agr = out.data_ptr() + n * t * 24
        _lib.check(lib.gcs_region_sweep_under(hist.data_ptr(), merges.data_ptr() if k > 1 else None, alive.data_ptr(),
                                              truth.img_of_d.data_ptr(), regs_d.data_ptr(), b, t, k, stride, n, ws.data_ptr(),
                                              out.data_ptr(), agr if agreement else None, agr + n * t * 32 if agreement else None,
                                              stream), "gcs_region_sweep_under")
        raw = out.cpu().numpy()
    arrays = [raw[:n * t * 3].view(np.uint64).reshape(n * t, 3)]
    if agreement:
        arrays += _agreement_arrays(raw[n * t * 3:], n * t)
    got = _cuts_in_callers_order(arrays, n, t, order)
    return got if agreement else got[0]


def cut_shapes_device(labels, contours, merges, alive, regions):
    """labels, merges, alive: the device tensors of ``Segmenter.region_tree_device``; contours: the (B,H,W) int32 tensor
    ``Segmenter.contour_map_device`` made of them; regions: as in ``region_sweep_resident``. Returns host arrays ``(area uint32
    [len(regions)][B][K], perim uint32 [len(regions)][B][K], boundary uint32 [len(regions)][B])`` in the caller's order of ``regions``:
    per cut the pixel count and the perimeter (metrics.py:160-180) of every group, held at the group's smallest label (0 for every
    other label), and the number of thick-boundary pixels (metrics.py:157), for the raw cuts. Three launches, one download."""
    import torch
    labels, merges, alive = _need_tree(labels, merges, alive, labels.device, "the labels")
    _need_contours(contours, labels)
    regs, order = _need_cuts(regions)
    (b, h, w), k, n = labels.shape, merges.shape[1] + 1, len(regs)
    if h > 4096 or w > 4096:
        raise ValueError("the sweep takes images of at most 4096 x 4096 pixels")
    contours = contours.contiguous()
    lib = _lib.load()
    with torch.cuda.device(labels.device):
        dev = labels.device
        regs_d = torch.tensor([regs[j] for j in order], dtype=torch.int32).to(dev)
        ws = torch.empty(lib.gcs_cut_shapes_workspace_bytes(b, k, n), dtype=torch.uint8, device=dev)
        out = torch.empty(n * b * (2 * k + 1), dtype=torch.int32, device=dev)    # area [n][b][k] | perim [n][b][k] | boundary [n][b]
        _lib.check(lib.gcs_cut_shapes(labels.data_ptr(), contours.data_ptr(), merges.data_ptr() if k > 1 else None, alive.data_ptr(),
                                      regs_d.data_ptr(), b, h, w, k, n, ws.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * n * b * k,
                                      out.data_ptr() + 8 * n * b * k, torch.cuda.current_stream(dev).cuda_stream), "gcs_cut_shapes")
        raw = out.cpu().numpy().view(np.uint32)
    area, perim = _cuts_in_callers_order((raw[:n * b * k].reshape(n * b, k), raw[n * b * k:2 * n * b * k].reshape(n * b, k)), n, b, order)
    boundary = np.empty((n, b), np.uint32)
    boundary[order] = raw[2 * n * b * k:].reshape(n, b)
    return area, perim, boundary


def sweep_reference_scores(counts, area, perim, boundary, alive, first, nx, ny, regions) -> list:
    """Per image a list with one ``{"regions", "underseg", "undersegNP", "compactness", "density"}`` per R of ``regions``, from the
    arrays of ``under_sweep_resident`` and ``cut_shapes_device``: the floats ``all_scores_batch_resident`` gives for
    ``cut_regions_device(..., R)`` (the same integers through ``_region_scores_batch``, whose sums run in the reference's order: a cut
    numbers its groups by increasing smallest label, the order of the rows here). ``regions`` = min(alive, R). Raises ValueError if a
    table did not count every pixel (N_t != nx * ny: a label outside 0 .. K-1), as the scorer does for such a map."""
    counts, area, perim, boundary = (np.asarray(x) for x in (counts, area, perim, boundary))
    alive = np.asarray(alive).astype(np.int64).ravel().tolist()
    first = np.asarray(first).astype(np.int64)
    n, b = len(regions), len(first) - 1
    if counts.ndim != 3 or counts.shape[0] != n or counts.shape[1] != int(first[-1]) or counts.shape[2] != 3:
        raise ValueError("counts must be a [len(regions)][T][3] array with T = first[-1]")
    if area.ndim != 3 or area.shape[:2] != (n, b) or perim.shape != area.shape or boundary.shape != (n, b) or len(alive) != b:
        raise ValueError("area / perim [len(regions)][B][K], boundary [len(regions)][B] and alive [B] do not describe the same cuts")
    if (counts[:, :, 0] != nx * ny).any():
        j, t = (int(v[0]) for v in np.nonzero(counts[:, :, 0] != nx * ny))
        raise ValueError(f"the table of annotator map {t} at R = {regions[j]} counts {int(counts[j, t, 0])} of {nx * ny} pixels: "
                         "a label outside 0 .. K-1")
    out = [[] for _ in range(b)]
    for j, r in enumerate(regions):
        reg = _region_scores_batch(counts[j, :, 1], counts[j, :, 2], area[j], perim[j], first, nx, ny)
        bd = boundary[j].astype(np.float64).tolist()
        for i in range(b):
            out[i].append({"regions": min(alive[i], int(r)), **reg[i], "density": bd[i] / float(nx * ny)})   # metrics.py:51, :157
    return out


def metrics_sweep_resident(labels, merges, alive, contours, truth: DeviceTruth, regions, agreement=False) -> list:
    """Per image a list with one dict per R of ``regions`` holding the seven keys of the reference's ``metrics.get_metrics()``
    (regions, recall, precision, underseg, undersegNP, compactness, density) and ``fmeasure``; agreement=True adds PRI, VoI and
    covering. The numbers ``all_scores_batch_resident(cut_regions_device(labels, merges, alive, R), truth, agreement=...)`` gives
    for every R, from one tree and one contour map: ``boundary_sweep_resident`` + ``sweep_scores``, ``under_sweep_resident`` and
    ``cut_shapes_device`` + ``sweep_reference_scores``, ``sweep_agreement``. Raises the reference's ZeroDivisionError where
    ``sweep_scores`` does (a cut without a boundary pixel: R = 1), once the sweeps have run: only their counts show it. Every
    argument is checked before the first launch."""
    _need_tree_and_cuts(labels, merges, alive, regions, truth)
    _need_contours(contours, labels)
    if max(labels.shape[1:]) > 4096:
        raise ValueError("the sweep takes images of at most 4096 x 4096 pixels")
    got = under_sweep_resident(labels, merges, alive, truth, regions, agreement)
    counts = got[0] if agreement else got
    shapes = cut_shapes_device(labels, contours, merges, alive, regions)
    hists = boundary_sweep_resident(contours, alive, truth)
    alive_h = alive.cpu().numpy()
    h, w = labels.shape[1:]
    rows = sweep_scores(hists, alive_h, truth.bd_counts.cpu().numpy(), truth.first, regions)
    ref = sweep_reference_scores(counts, *shapes, alive_h, truth.first, h, w, regions)
    out = [[{**s, **r} for s, r in zip(srow, rrow)] for srow, rrow in zip(rows, ref)]
    if agreement:
        agree = sweep_agreement(got[1], got[2], truth.first, h * w, regions)
        out = [[{**s, **a} for s, a in zip(row, arow)] for row, arow in zip(out, agree)]
    return out
