"""Scoring mirror of the reference's ``metrics`` class, on scipy.ndimage (host side).

Same constructor, method names, result keys and error behaviour as
/root/reference/BSD_metrics/metrics.py:18-255 so that ``script.py:36-38`` reads the same:

    m = metrics(img, labels, segments); m.set_metrics(); m.display_metrics()

Differences, all additive: ``fmeasure`` (the reference computes no F)
and vectorised implementations of the two per-pixel Python loops (metrics.py:120-126,
168-180). scikit-image is not available beside torch, so ``find_boundaries`` /
``dilation(rectangle(5,5))`` are restated on scipy.ndimage (verified bit-identical, and
pinned by tests/golden/scoring_golden.json which the reference class itself produced).
This module is product code: it never imports ``oracle``.
"""
from __future__ import annotations

from math import pi

import numpy as np
from scipy import ndimage as ndi

_CROSS = ndi.generate_binary_structure(2, 1)


def find_boundaries(lab: np.ndarray) -> np.ndarray:
    """skimage.segmentation.find_boundaries(lab) defaults (mode='thick', connectivity=1),
    as called at metrics.py:49,69,88,157: 3x3-cross max != min, reflect border."""
    lab = np.asarray(lab)
    return ndi.grey_dilation(lab, footprint=_CROSS) != ndi.grey_erosion(lab, footprint=_CROSS)


def _dilate(mask: np.ndarray, size: int) -> np.ndarray:
    """skimage.morphology.dilation(mask, rectangle(size, size)) for boolean masks."""
    return ndi.grey_dilation(mask.astype(np.uint8), footprint=np.ones((size, size), bool)).astype(bool)


class metrics:
    """Compute the metrics of a segmentation against the BSD manual segmentations."""

    def __init__(self, img, lb, segments_truth):
        # metrics.py:25-51
        self.img = img
        self.lb = np.asarray(lb).astype('int')
        self.nx, self.ny = self.lb.shape
        self.segments_truth = segments_truth
        self.img_truth = [find_boundaries(s) for s in self.segments_truth]
        self.n_segments = np.max(self.lb) + 1

    # ---- boundary recall / precision (metrics.py:58-96)
    def set_boundary_recall(self, size=5):
        bd = _dilate(find_boundaries(self.lb), size)
        self.recall = 0
        for truth in self.img_truth:
            self.recall += float(np.sum(bd & truth)) / float(np.sum(truth))
        self.recall /= len(self.img_truth)

    def set_boundary_precision(self, size=5):
        # the reference ignores ``size`` here and hard-codes 5 (metrics.py:93)
        bd = find_boundaries(self.lb)
        self.precision = 0
        global_score = float(np.sum(bd))
        for truth in self.img_truth:
            self.precision += float(np.sum(bd & _dilate(truth, 5))) / global_score
        self.precision /= len(self.img_truth)

    def set_fmeasure(self):
        """F = 2PR/(P+R), 0 when P+R = 0. Not in the reference."""
        s = self.recall + self.precision
        self.fmeasure = 0.0 if s == 0 else 2.0 * self.precision * self.recall / s

    # ---- undersegmentation (metrics.py:102-146), contingency table by bincount
    def set_undersegmentation(self):
        self.undersegmentation = 0.
        self.undersegmentationNP = 0.
        n = self.nx * self.ny
        for truth in self.segments_truth:
            truth = np.asarray(truth).astype(np.int64)
            n_labels = int(np.max(truth) + 1)
            hist = np.bincount((self.lb.astype(np.int64) * n_labels + truth).ravel(),
                               minlength=int(self.n_segments) * n_labels)
            hist = hist.reshape(int(self.n_segments), n_labels).astype(np.float64)
            area = hist.sum(axis=1)
            self.undersegmentation += float(np.sum(area - hist.max(axis=1))) / n
            self.undersegmentationNP += float(np.sum(np.minimum(hist, area[:, None] - hist))) / n
        self.undersegmentation /= len(self.segments_truth)
        self.undersegmentationNP /= len(self.segments_truth)

    # ---- geometry (metrics.py:152-201)
    def set_density(self):
        self.density = np.sum(find_boundaries(self.lb)) / float(self.nx * self.ny)

    def perimeter(self):
        lb = self.lb
        edge = np.zeros(lb.shape, bool)
        edge[0, :] = edge[-1, :] = True
        edge[:, 0] = edge[:, -1] = True
        inner = np.zeros(lb.shape, bool)
        c = lb[1:-1, 1:-1]
        inner[1:-1, 1:-1] = (lb[:-2, 1:-1] != c) | (lb[2:, 1:-1] != c) | (lb[1:-1, :-2] != c) | (lb[1:-1, 2:] != c)
        self.perimeters = np.bincount(lb[edge | inner].ravel(), minlength=int(self.n_segments)).astype(np.float64)

    def set_compactness(self):
        self.perimeter()
        self.compactness = 0
        max_area = float(self.nx * self.ny)
        areas = np.bincount(self.lb.ravel(), minlength=int(self.n_segments))
        for i in range(int(self.n_segments)):
            area = areas[i]
            perimeter = self.perimeters[i]
            ratio = area / max_area
            if perimeter > 0:
                self.compactness += 4 * pi * ratio * area / pow(perimeter, 2)

    # ---- orchestration (metrics.py:208-255)
    def set_metrics(self):
        self.set_boundary_recall()
        self.set_boundary_precision()
        self.set_fmeasure()
        self.set_density()
        self.set_undersegmentation()
        self.set_compactness()

    def display_metrics(self):
        print("Regions: " + str(self.n_segments) +
              " Recall: " + str(self.recall) +
              " Precision: " + str(self.precision) +
              " F-measure: " + str(self.fmeasure) +
              " Undersegmentation: " + str(self.undersegmentation) +
              " Undersegmentation (NP) " + str(self.undersegmentationNP) +
              " Compactness " + str(self.compactness) +
              " Density " + str(self.density))

    def get_metrics(self):
        return {"regions": self.n_segments, "recall": self.recall, "precision": self.precision,
                "fmeasure": self.fmeasure, "underseg": self.undersegmentation,
                "undersegNP": self.undersegmentationNP, "compactness": self.compactness,
                "density": self.density}


def boundary_scores(labels, segments_truth) -> dict:
    """Recall / precision / F of one label map (the part of the metric BASELINE.json names)."""
    m = metrics(None, labels, segments_truth)
    m.set_boundary_recall()
    m.set_boundary_precision()
    m.set_fmeasure()
    return {"recall": m.recall, "precision": m.precision, "fmeasure": m.fmeasure}


# ---- boundary scores of an edge-strength map at every threshold (SPEC.md §22)

def edge_scores_from_counts(g, ann) -> dict:
    """metrics.py:69-74 and :88-96 with the map ``edges > theta`` in place of ``find_boundaries(lb)``, on the integer counts of one
    threshold as Python floats: g = #{edges > theta}, ann = per annotator [recall numerator, #bd(T), precision numerator], flat.
    The zero rule: g = 0 (no boundary pixel) gives recall = precision = F = 0 instead of the reference's ZeroDivisionError."""
    if g == 0:
        return {"recall": 0.0, "precision": 0.0, "fmeasure": 0.0}
    a = len(ann) // 3
    recall = 0
    precision = 0
    for i in range(0, 3 * a, 3):                                 # in annotator order
        recall += ann[i] / ann[i + 1]                            # ZeroDivisionError as metrics.py:72: an annotator map without a boundary
        precision += ann[i + 2] / g
    recall /= a
    precision /= a
    s = recall + precision
    return {"recall": recall, "precision": precision, "fmeasure": 0.0 if s == 0 else 2.0 * precision * recall / s}


def edge_scores(edges, segments_truth, thresholds) -> dict:
    """Boundary recall / precision / F of an (H,W) integer edge-strength map against its annotator maps at every threshold of
    ``thresholds`` (integers, any order): the boundary map of threshold theta is ``edges > theta``, the arithmetic is the
    reference's (``metrics.set_boundary_recall`` / ``set_boundary_precision`` / ``set_fmeasure``) in its order. Returns
    ``{"recall", "precision", "fmeasure"}``, float64 arrays with one entry per threshold. The counts are taken from sorted values
    (dil5(edges > theta) = (the 5 x 5 maximum of edges) > theta), not from one dilation per threshold."""
    edges = np.asarray(edges)
    if edges.ndim != 2 or edges.dtype.kind not in "iu":
        raise ValueError("edges must be an (H,W) integer array")
    if len(segments_truth) == 0:
        raise ZeroDivisionError("no annotator maps")
    edges = edges.astype(np.int64)
    th = np.asarray(thresholds).astype(np.int64).ravel()
    above = lambda vals: vals.size - np.searchsorted(np.sort(vals, axis=None), th, side="right")    # #{vals > theta}
    m5 = ndi.maximum_filter(edges, size=5, mode="nearest")       # the window clipped to the image: what _dilate's reflection sees
    g = above(edges)
    per = []
    for s in segments_truth:
        truth = find_boundaries(s)
        per.append((above(m5[truth]), int(np.sum(truth)), above(edges[_dilate(truth, 5)])))
    out = {"recall": np.zeros(len(th)), "precision": np.zeros(len(th)), "fmeasure": np.zeros(len(th))}
    for j in range(len(th)):
        ann = []
        for rec, n_truth, prec in per:
            ann += [float(rec[j]), float(n_truth), float(prec[j])]
        sc = edge_scores_from_counts(float(g[j]), ann)
        for key in out:
            out[key][j] = sc[key]
    return out


# ---- one-to-one matching scores of an edge-strength map (SPEC.md §26): the metric that charges a thick map for its width

def thin_boundaries(s) -> np.ndarray:
    """One-pixel contours of a label map: pixel (y, x) is a boundary pixel iff its right or its lower neighbour (where the image
    has one) carries another label - the pair ownership of ``gcs_region_adjacency`` (SPEC.md §20). (H,W) bool."""
    s = np.asarray(s)
    if s.ndim != 2:
        raise ValueError("a label map must be an (H,W) array")
    out = np.zeros(s.shape, bool)
    out[:, :-1] |= s[:, :-1] != s[:, 1:]
    out[:-1, :] |= s[:-1, :] != s[1:, :]
    return out


def match_distance2(height, width) -> int:
    """SPEC.md §26: the largest squared distance of an allowed pair, (0.0075 x the diagonal)^2 in integers; 18 for 481 x 321."""
    return (9 * (int(height) ** 2 + int(width) ** 2)) // 160000


def match_count(p_mask, q_mask, d2) -> int:
    """The cardinality of a maximum matching between the pixels of two (H,W) bool masks, a pair being allowed iff its squared
    distance is at most ``d2``. The pairs are built offset by offset; the matching is scipy's Hopcroft-Karp."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    p_mask, q_mask = np.asarray(p_mask, bool), np.asarray(q_mask, bool)
    h, w = p_mask.shape
    n_p, n_q = int(p_mask.sum()), int(q_mask.sum())
    if n_p == 0 or n_q == 0:
        return 0
    p_id = np.full((h, w), -1, np.int64)
    q_id = np.full((h, w), -1, np.int64)
    p_id[p_mask] = np.arange(n_p)
    q_id[q_mask] = np.arange(n_q)
    reach = int(np.sqrt(d2))
    while (reach + 1) ** 2 <= d2:
        reach += 1
    while reach ** 2 > d2:
        reach -= 1
    rows, cols = [], []
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            if dy * dy + dx * dx > d2 or abs(dy) >= h or abs(dx) >= w:
                continue
            # q = p + (dy, dx): the two windows of the image that the offset maps onto each other
            ps = p_id[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)]
            qs = q_id[max(0, dy):h - max(0, -dy), max(0, dx):w - max(0, -dx)]
            both = (ps >= 0) & (qs >= 0)
            rows.append(ps[both])
            cols.append(qs[both])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    if rows.size == 0:
        return 0
    graph = csr_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(n_p, n_q))
    return int(np.sum(maximum_bipartite_matching(graph, perm_type="column") >= 0))


def match_scores(edges, segments_truth, thresholds, max_dist2=None) -> dict:
    """One-to-one matching recall / precision / F of an (H,W) integer edge-strength map at every threshold (SPEC.md §26). For a
    threshold theta, P = {edges > theta}; per annotator t, Q_t = ``thin_boundaries(s_t)`` and M_t = the cardinality of a maximum
    matching between P and Q_t with a pair allowed iff dy^2 + dx^2 <= D2 = ``match_distance2(H, W)`` (``max_dist2`` overrides
    it). recall = mean_t M_t / |Q_t| (ZeroDivisionError for an annotator without a boundary), precision = mean_t M_t / |P|, F and
    the zero rule (|P| = 0) as in ``edge_scores``, whose dict shape is returned. A map pixel is used at most once per annotator,
    so a ribbon k pixels wide has precision 1 / k where ``edge_scores`` gives it 1."""
    edges = np.asarray(edges)
    if edges.ndim != 2 or edges.dtype.kind not in "iu":
        raise ValueError("edges must be an (H,W) integer array")
    if len(segments_truth) == 0:
        raise ZeroDivisionError("no annotator maps")
    d2 = match_distance2(*edges.shape) if max_dist2 is None else int(max_dist2)
    if d2 < 0:
        raise ValueError("max_dist2 must be >= 0")
    truths = [thin_boundaries(s) for s in segments_truth]
    for t in truths:
        if t.shape != edges.shape:
            raise ValueError("every annotator map must have the shape of edges")
    th = np.asarray(thresholds).astype(np.int64).ravel()
    out = {"recall": np.zeros(len(th)), "precision": np.zeros(len(th)), "fmeasure": np.zeros(len(th))}
    for j, theta in enumerate(th):
        p_mask = edges > theta
        ann = []
        for t in truths:
            m = float(match_count(p_mask, t, d2)) if p_mask.any() else 0.0
            ann += [m, float(t.sum()), m]
        sc = edge_scores_from_counts(float(p_mask.sum()), ann)
        for key in out:
            out[key][j] = sc[key]
    return out


# ---- region agreement: PRI, VoI, segmentation covering (SPEC.md §8; not part of the reference's ``metrics``)

def agreement_sums(labels, truth):
    """The integer sums and float terms of SPEC.md §8 for ONE annotator map, from its contingency table (bincount):
    sums = [N, sum a^2, sum b^2, sum n^2] (Python ints), terms = [sum a log2 a, sum b log2 b, sum n log2 n,
    sum_j b_j n*_j / u*_j] (floats) - what gcs_region_agreement writes per map."""
    s = np.asarray(labels).astype(np.int64).ravel()
    g = np.asarray(truth).astype(np.int64).ravel()
    if s.shape != g.shape:
        raise ValueError("annotator map and label map differ in shape")
    if s.size and (s.min() < 0 or g.min() < 0):
        raise ValueError("labels must be non-negative")
    n_g = int(g.max()) + 1 if g.size else 1
    n_s = int(s.max()) + 1 if s.size else 1
    hist = np.bincount(s * n_g + g, minlength=n_s * n_g).reshape(n_s, n_g).astype(np.int64)
    a, b = hist.sum(axis=1), hist.sum(axis=0)
    nz = lambda v: v[v > 0].astype(np.float64)
    xlog = lambda v: float(np.sum(nz(v) * np.log2(nz(v))))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(hist > 0, hist / (a[:, None] + b[None, :] - hist), 0.0)
    best = ratio.max(axis=0)
    sums = [int(b.sum()), int(np.sum(a * a)), int(np.sum(b * b)), int(np.sum(hist * hist))]
    terms = [xlog(a), xlog(b), xlog(hist), float(np.sum(b.astype(np.float64) * best))]
    return sums, terms


def agreement_from_sums(sums, terms, first, n_pixels) -> list:
    """SPEC.md §8 from the per-map sums / terms ([T][4] each; maps first[i] .. first[i+1]-1 belong to image i): one dict
    {"PRI", "VoI", "covering"} per image, annotator means in annotator order. The ONE finishing step of the host definition
    and every device path, so the integer-derived PRI is the same float everywhere. Raises if a table did not count every
    pixel (N_t != n_pixels: a label outside the table)."""
    n = int(n_pixels)
    if n < 2:
        raise ValueError(f"region agreement needs at least 2 pixels, got {n}")
    pairs = n * (n - 1)
    out = []
    first = [int(f) for f in first]
    for i in range(len(first) - 1):
        t0, t1 = first[i], first[i + 1]
        if t1 <= t0:
            raise ZeroDivisionError("an image has no annotator maps")
        pri = voi = cov = 0.0
        for t in range(t0, t1):
            n_t, sa2, sb2, sn2 = (int(x) for x in sums[t])
            if n_t != n:
                raise ValueError(f"contingency table of map {t} counts {n_t} pixels, the image has {n} "
                                 "(a label outside the table)")
            hal, hbl, hnl, cv = (float(x) for x in terms[t])
            pri += 1.0 - (sa2 + sb2 - 2 * sn2) / pairs             # exact integers, one rounding
            voi += (hal + hbl - 2.0 * hnl) / n
            cov += cv / n
        k = t1 - t0
        out.append({"PRI": pri / k, "VoI": voi / k, "covering": cov / k})
    return out


def region_agreement(labels, segments_truth) -> dict:
    """PRI, VoI (bits) and segmentation covering of one label map against its annotator maps (SPEC.md §8).
    {"PRI", "VoI", "covering"}; labels / maps: (H,W) non-negative integer arrays."""
    labels = np.asarray(labels)
    if len(segments_truth) == 0:
        raise ZeroDivisionError("no annotator maps")
    if labels.size < 2:
        raise ValueError(f"region agreement needs at least 2 pixels, got {labels.size}")
    st = [agreement_sums(labels, g) for g in segments_truth]
    return agreement_from_sums([s for s, _ in st], [t for _, t in st], [0, len(st)], labels.size)[0]


# ---- the whole hierarchy at once (SPEC.md §15)

def ods_ois(f_table, regions, best="max") -> dict:
    """``f_table[b][j]`` = F of image b at ``regions[j]`` -> ``{"OIS", "ODS", "ODS_regions", "OIS_regions"}``: OIS = the mean over the
    images of each image's best F, ODS = the best mean F of one R for the whole set (on ties the smallest R), ``OIS_regions`` = each
    image's best R (smallest on ties). Plain Python floats, summed in image order. ``best="min"``: the best score is the lowest one
    (VoI, SPEC.md §16); ties still go to the smallest R."""
    if best not in ("max", "min"):
        raise ValueError('best must be "max" or "min"')
    pick = max if best == "max" else min                                   # both keep the first of equals
    regions = [int(r) for r in regions]
    rows = [[float(v) for v in row] for row in f_table]
    if not rows or not regions or any(len(row) != len(regions) for row in rows):
        raise ValueError("f_table must be a non-empty list of rows with one F per entry of regions")
    order = sorted(range(len(regions)), key=lambda j: regions[j])           # ties go to the smallest R: visit R in increasing order
    best_r, ois = [], 0.0
    for row in rows:
        j = pick(order, key=lambda q: row[q])                              # max / min keep the first of equals
        best_r.append(regions[j])
        ois += row[j]
    means = []
    for j in range(len(regions)):
        m = 0.0
        for row in rows:
            m += row[j]
        means.append(m / len(rows))
    jd = pick(order, key=lambda q: means[q])
    return {"OIS": ois / len(rows), "ODS": means[jd], "ODS_regions": regions[jd], "OIS_regions": best_r}
