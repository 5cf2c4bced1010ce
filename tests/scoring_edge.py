"""The edge-shape scoring fixture (tests/golden/make_scoring_edge_golden.py), for the host and the GPU tests: label maps and
annotator stacks at shapes around the scorer's 16 x 64 tiles and 64-bit plane words, with the reference class's own numbers."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EXACT = ("recall", "precision", "density")                       # tests/test_evaluate.py: same integer counts, same divisions
CLOSE = ("underseg", "undersegNP", "compactness")                # rel 1e-12 there
ERRORS = {"ZeroDivisionError": ZeroDivisionError, "ValueError": ValueError}


def load():
    """[(key, label map int32 (H,W), annotator maps uint16 [A][H][W] (A may be 0), golden dict)] in key order."""
    maps = np.load(os.path.join(GOLD, "scoring_edge_maps.npz"))
    gold = json.load(open(os.path.join(GOLD, "scoring_edge_golden.json")))
    out = []
    for key in sorted(gold):
        shape, kind, stack = key.split("/")
        lab = maps["lab_%s_%s" % (shape, kind)].astype(np.int32)
        truth = np.zeros((0,) + lab.shape, np.uint16) if stack == "a0" else maps["truth_%s_%s" % (shape, stack)]
        out.append((key, lab, truth, gold[key]))
    return out


def _assemble(items):
    """[(label map, annotator maps [A][H][W])] -> labs [B][H][W] int32, truth [T][H][W] uint16, first [B+1], img_of [T]."""
    labs = np.stack([l for l, _ in items]).astype(np.int32)
    truth = np.concatenate([t for _, t in items]).astype(np.uint16)
    first = np.concatenate([[0], np.cumsum([len(t) for _, t in items])]).astype(np.int32)
    img_of = np.repeat(np.arange(len(items)), [len(t) for _, t in items]).astype(np.int32)
    return labs, truth, first, img_of


# ------------------------------------------------------------------------------------------------ restatements (host)
def _np_counts(labs, truth, img_of):
    """counts [B + 3T] of gcs.h from scipy: sum bd(L_b); per map t of image b: sum dil5(bd(L_b)) & bd(T_t), sum bd(T_t),
    sum bd(L_b) & dil5(bd(T_t))."""
    from gabor_color_image_segmentation_amd import evaluate as ev
    bd = [ev.find_boundaries(l) for l in labs]
    dil = [ev._dilate(b, 5) for b in bd]
    out = [int(b.sum()) for b in bd]
    for t, b in zip(truth, img_of):
        tb = ev.find_boundaries(t)
        out += [int((dil[b] & tb).sum()), int(tb.sum()), int((bd[b] & ev._dilate(tb, 5)).sum())]
    return np.array(out, np.int64)


def _np_tables(lab, truths, n_seg, stride):
    """hist [A][n_seg][stride], area, perim [n_seg] of one image: np.bincount and evaluate.metrics.perimeter. Pixels whose
    label is >= n_seg are in no table; pixels whose annotator label is >= stride are missing from hist alone."""
    from gabor_color_image_segmentation_amd.evaluate import metrics
    lab = np.asarray(lab).astype(np.int64)
    ok = lab < n_seg
    area = np.bincount(lab[ok], minlength=n_seg)
    m = metrics(None, lab, [])
    m.perimeter()                                                    # per label 0 .. max(lab), neighbours compared on the full map
    perim = np.zeros(n_seg, np.int64)
    k = min(n_seg, len(m.perimeters))
    perim[:k] = m.perimeters[:k].astype(np.int64)
    hist = np.zeros((len(truths), n_seg, stride), np.int64)
    for a, t in enumerate(truths):
        t = np.asarray(t).astype(np.int64)
        both = ok & (t < stride)
        hist[a] = np.bincount(lab[both] * stride + t[both], minlength=n_seg * stride).reshape(n_seg, stride)
    return hist, area, perim


def _np_tables_batch(labs, truth, first, n_seg, stride):
    parts = [_np_tables(labs[b], truth[first[b]:first[b + 1]], n_seg, stride) for b in range(len(labs))]
    return (np.concatenate([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]))


def _np_reduce(hist, area, img_of):
    """under [T], under_np [T] of gcs_region_reduce from the tables (metrics.py:129-130, :137-139)."""
    hist = hist.astype(np.int64)
    under = (area.astype(np.int64)[img_of] - hist.max(axis=2)).sum(axis=1)
    under_np = np.minimum(hist, hist.sum(axis=2, keepdims=True) - hist).sum(axis=(1, 2))
    return under, under_np


def _np_planes(maps):
    """bd and dil5 planes [2][M][H][W] (bool) from scipy."""
    from gabor_color_image_segmentation_amd import evaluate as ev
    bd = np.stack([ev.find_boundaries(m) for m in maps])
    return np.stack([bd, np.stack([ev._dilate(b, 5) for b in bd])])
