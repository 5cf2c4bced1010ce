"""Host side of SPEC.md §19 and §20: the table of region descriptors from the integer sums and boxes the device made, and the region
adjacency graph from its edge rows. NumPy only."""
from __future__ import annotations

import numpy as np


def _mean(s, n):
    """SPEC.md §4's rounding rule, floor((2 S + n) / (2 n)), on Python integers (a uint64 sum does not fit int64 arithmetic in
    general); 0 where n = 0."""
    s, n = np.asarray(s, dtype=object), np.asarray(n, dtype=object)
    safe = np.where(n == 0, 1, n)
    return np.where(n == 0, 0, (2 * s + safe) // (2 * safe))


def region_table(sums, bbox) -> dict:
    """sums [..., K, 6 + D] (uint64, or the int64 that carries its bits), bbox [..., K, 4] int32: a leaf table or the rows of one cut
    (``Segmenter.region_props_device`` / ``cut_props_device``, downloaded) -> a dict of arrays over the same leading axes:

    ``area`` int64 [K]; ``centroid`` float64 [K][2] = (sum y / n, sum x / n), NaN for an unused row; ``bbox`` int32 [K][4] =
    (y0, x0, y1, x1) inclusive, (H, W, -1, -1) for an unused row; ``mean_rgb`` uint8 [K][3] and ``mean_features`` uint16 [K][D]
    by floor((2 S + n) / (2 n)), 0 for an unused row; ``used`` bool [K] = n > 0."""
    sums = np.ascontiguousarray(sums)
    if sums.dtype == np.int64:
        sums = sums.view(np.uint64)
    bbox = np.asarray(bbox)
    if sums.dtype != np.uint64 or sums.ndim < 2 or sums.shape[-1] < 6 or bbox.shape != sums.shape[:-1] + (4,):
        raise ValueError("sums must be a [..., K, 6 + D] uint64 array and bbox the [..., K, 4] array beside it")
    n = sums[..., 0]
    used = n > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        centroid = sums[..., 1:3].astype(np.float64) / n[..., None].astype(np.float64)
    mean = _mean(sums[..., 3:], n[..., None])
    return dict(area=n.astype(np.int64), centroid=centroid, bbox=bbox.astype(np.int32),
                mean_rgb=mean[..., :3].astype(np.uint8), mean_features=mean[..., 3:].astype(np.uint16), used=used)


def adjacency_table(edges, vals, count, n_regions=None) -> dict:
    """One image's edge table of SPEC.md §20 (``Segmenter.region_adjacency_device`` / ``cut_adjacency_device``, downloaded): edges
    [capacity, 2] int32, vals [capacity, 3] (uint64, or the int64 that carries its bits), count -> a dict over the n = count edges:

    ``pairs`` int32 [n][2], a < b, sorted; ``length`` int64 [n]; ``mean_contrast`` float64 [n] = contrast / length;
    ``mean_strength`` float64 [n] = strength / (2 length) (with the contour map as the plane: the mean tree level along the common
    boundary). With ``n_regions``: ``degree`` int64 [n_regions] and ``neighbours`` = (indptr int64 [n_regions + 1], indices int32
    [2 n]), the graph in CSR form, both directions, every region's neighbours ascending.
    ValueError when count is -1: the image has more edges than the table's capacity."""
    count = int(count)
    if count < 0:
        raise ValueError("the edge table overflowed (count = -1): call again with a larger capacity= (at most 16384)")
    edges, vals = np.asarray(edges), np.ascontiguousarray(vals)
    if vals.dtype == np.int64:
        vals = vals.view(np.uint64)
    if edges.ndim != 2 or edges.shape[1] != 2 or vals.dtype != np.uint64 or vals.shape != (edges.shape[0], 3) or count > edges.shape[0]:
        raise ValueError("edges must be a [capacity, 2] int32 array, vals the [capacity, 3] uint64 array beside it, count <= capacity")
    pairs = edges[:count].astype(np.int32)
    length = vals[:count, 0].astype(np.int64)
    flen = vals[:count, 0].astype(np.float64)
    out = dict(pairs=pairs, length=length, mean_contrast=vals[:count, 1].astype(np.float64) / flen,
               mean_strength=vals[:count, 2].astype(np.float64) / (2.0 * flen))
    if n_regions is not None:
        n_regions = int(n_regions)
        if count and (pairs.min() < 0 or pairs.max() >= n_regions):
            raise ValueError("an edge names a region outside 0 .. n_regions - 1")
        src = np.concatenate([pairs[:, 0], pairs[:, 1]]).astype(np.int64)
        dst = np.concatenate([pairs[:, 1], pairs[:, 0]]).astype(np.int64)
        order = np.lexsort((dst, src))
        degree = np.bincount(src, minlength=n_regions).astype(np.int64)
        out["degree"] = degree
        out["neighbours"] = (np.concatenate([[0], np.cumsum(degree)]).astype(np.int64), dst[order].astype(np.int32))
    return out
