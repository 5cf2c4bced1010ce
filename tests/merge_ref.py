"""NumPy / scipy restatement of SPEC.md §9 (small-region merging), for the tests only. The package never imports it.

Regions are tracked by the raster id of their first component (SPEC §7 numbers components in raster order of their first
pixel, so the smallest component id of a group is its first pixel's rank, and comparing ids compares first pixels)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from oracle import spec_oracle as so


def round_bound(h, w):
    """floor(log2(H*W)) + 1: the most rounds §9 can take on an H x W image."""
    return int(h * w).bit_length()


def merge_small_regions(lab, m, return_rounds=False):
    """SPEC.md §9 on one (H,W) integer map: int64 region ids 0, 1, 2, ... in raster order of first pixel.
    With return_rounds=True also the number of rounds that merged something."""
    cc = so.connected_regions(np.asarray(lab))
    if m <= 1:
        return (cc, 0) if return_rounds else cc
    n = int(cc.max()) + 1
    base_size = np.bincount(cc.ravel(), minlength=n).astype(np.int64)
    a = np.concatenate([cc[:, :-1].ravel(), cc[:-1, :].ravel()])
    b = np.concatenate([cc[:, 1:].ravel(), cc[1:, :].ravel()])
    d = a != b
    edges = np.unique(np.stack([a[d], b[d]], axis=1), axis=0) if d.any() else np.zeros((0, 2), np.int64)
    group = np.arange(n, dtype=np.int64)               # group of each component = its smallest member component
    rounds = 0
    while True:
        size = np.bincount(group, weights=base_size, minlength=n).astype(np.int64)
        ea, eb = group[edges[:, 0]], group[edges[:, 1]]
        keep = ea != eb
        ea, eb = ea[keep], eb[keep]
        src = np.concatenate([ea, eb])                  # every adjacency in both directions
        dst = np.concatenate([eb, ea])
        absorb = size[src] < m
        src, dst = src[absorb], dst[absorb]
        if src.size == 0:
            break
        best = np.full(n, -1, np.int64)                 # key (|B|, -first(B)): size first, then the smaller id
        np.maximum.at(best, src, size[dst] * (n + 1) + (n - dst))
        picks = np.flatnonzero(best >= 0)
        target = n - best[picks] % (n + 1)
        g = coo_matrix((np.ones(picks.size), (picks, target)), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        low = np.full(comp.max() + 1, n, np.int64)      # new group id = smallest old group id of the component
        np.minimum.at(low, comp, np.arange(n))
        group = low[comp[group]]
        rounds += 1
    _, out = np.unique(group[cc], return_inverse=True)
    out = out.reshape(cc.shape).astype(np.int64)
    return (out, rounds) if return_rounds else out
