"""NumPy / Python restatement of SPEC.md §21 (the region tree on the connected regions of the k-means map), for the tests and the
quality tool only. The package never imports it and it uses none of the package's code: the features of tests/position_ref.py (§2,
§10 - §12), the k-means of the C oracle (§4), the node map of tests/component_tree_ref.py (§18) and the tree and its cut of
tests/region_tree_ref.py (§14)."""
import numpy as np

import component_tree_ref as ct
import position_ref as pr
import region_tree_ref as rt
from oracle import c_oracle as co

K_CAP = ct.K_CAP


def kmeans_maps(xs, k=8, n_iter=10, mode="per_image"):
    """Canonical features (B, D, H, W) -> the k-means maps L of SPEC.md §4, (B, H, W) int32."""
    xs = np.asarray(xs)
    b, d, h, w = xs.shape
    flat = np.ascontiguousarray(xs.reshape(b, d, h * w))
    if mode == "global":
        return co.kmeans(flat, k, n_iter)[0].reshape(b, h, w).astype(np.int32)
    return np.stack([co.kmeans(flat[i:i + 1], k, n_iter)[0].reshape(h, w) for i in range(b)]).astype(np.int32)


def tree(x, lab, m=0, k_cap=K_CAP, k=None, info=None):
    """Canonical features x (D, H, W) and the k-means map L -> (N, merges, costs, alive): §14 on (x, N), N = §18's node map of L."""
    return ct.tree(x, lab, m, k_cap, k, info)


def regions(x, lab, r, m=0, k_cap=K_CAP, info=None):
    """The delivered map: the cut at r (a list: one map per value, from one tree), or N itself for r = 0."""
    n_map, merges, _, alive = tree(x, lab, m, k_cap, info=info)
    if isinstance(r, (list, tuple)):
        return [rt.cut(n_map, merges, alive, q) if q else n_map for q in r]
    return rt.cut(n_map, merges, alive, r) if r else n_map


def segment_batch(imgs, r, k=8, n_iter=10, m=0, mode="per_image", w=0.0, g=0, mu=0, n_scales=4, n_orient=6, smoothing=0.0,
                  k_cap=K_CAP, **bank_kw):
    """(B, H, W, 3) uint8 images -> what Segmenter(tree_nodes="clusters", n_regions=r, k=k, min_region_size=m) delivers."""
    xs = np.stack([pr.features(np.asarray(im), w, g, mu, n_scales, n_orient, smoothing, **bank_kw) for im in imgs])
    labs = kmeans_maps(xs, k, n_iter, mode)
    return np.stack([regions(x, lab, r, m, k_cap) for x, lab in zip(xs, labs)])


def segment(img, r, **kw):
    return segment_batch(np.asarray(img)[None], r, **kw)[0]
