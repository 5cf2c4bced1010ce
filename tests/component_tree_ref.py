"""NumPy / Python restatement of SPEC.md §18 (the region tree on connected regions), for the tests and the quality tool only. The
package never imports it and it uses none of the package's code: the node map from tests/merge_ref.py (§7, §9), the tree and its cut
from tests/region_tree_ref.py (§14)."""
import numpy as np

import merge_ref as mr
import region_tree_ref as rt
from oracle import spec_oracle as so

K_CAP = 4096


def nodes(lab, m, k_cap=K_CAP, info=None):
    """(H, W) label map -> the node map of SPEC.md §18, int32: C = the connected regions of §7, m_guard = ceil(H W / k_cap),
    m_b = max(m, m_guard) if C > k_cap else m, N = §9 at m_b. ``info``: a dict that receives ``components`` (C), ``min_size`` (m_b)
    and ``nodes`` (the labels of N)."""
    lab = np.asarray(lab)
    if not 1 <= k_cap <= K_CAP or m < 0:
        raise ValueError("outside the domain of SPEC.md §18")
    c = int(so.connected_regions(lab).max()) + 1
    m_guard = -(-lab.shape[0] * lab.shape[1] // k_cap)
    m_b = max(int(m), m_guard) if c > k_cap else int(m)
    out = mr.merge_small_regions(lab, m_b).astype(np.int32)
    if info is not None:
        info.update(components=c, min_size=m_b, nodes=int(out.max()) + 1)
    return out


def tree(x, lab, m=0, k_cap=K_CAP, k=None, info=None):
    """Canonical features x (D, H, W) and a §13 map -> (N, merges, costs, alive): the tree of §14 on the node map, at capacity ``k``
    (None: the node count, the smallest that holds it; the rows of a larger one are these followed by (-1, -1) / 0 rows)."""
    n_map = nodes(lab, m, k_cap, info)
    count = int(n_map.max()) + 1
    merges, costs, alive = rt.build_tree(x, n_map, count if k is None else k, info)
    assert alive == count
    return n_map, merges, costs, alive


def segment(img, n, r, m=0, lam=576, n_iter=10, w=0.0, g=0, mu=0, n_scales=4, n_orient=6, smoothing=0.0, k_cap=K_CAP, **bank_kw):
    """(H, W, 3) uint8 image -> §13 superpixels, their node map (``m`` = min_region_size), the tree on it cut at r; with a list ``r``:
    one map per value, from one tree."""
    import position_ref as pr
    import superpixel_ref as sr
    x = pr.features(np.asarray(img), w, g, mu, n_scales, n_orient, smoothing, **bank_kw)
    n_map, merges, _, alive = tree(x, sr.superpixels(x, n, lam, n_iter), m, k_cap)
    if isinstance(r, (list, tuple)):
        return [rt.cut(n_map, merges, alive, q) for q in r]
    return rt.cut(n_map, merges, alive, r)
