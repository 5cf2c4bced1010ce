"""Host side of SPEC.md §19: the table of region descriptors from the integer sums and boxes the device made. NumPy only."""
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
