"""NumPy / Python restatement of SPEC.md §20 (region adjacency graph), for the tests and the timing tool only. The package never
imports it and it uses none of the package's code. ``leaf_graph`` takes shifted comparisons, ``np.unique`` on a K + b and ``np.add.at``;
``leaf_graph_loops`` is the plain double loop the CPU tests hold it against; ``cut_graph`` restates the cuts on the leaf rows alone."""
import numpy as np


def _pairs(lab, img, plane):
    """Every pixel pair of the map as flat arrays: labels on both sides, squared colour difference, clamped plane sum."""
    lab = np.asarray(lab).astype(np.int64)
    img = None if img is None else np.asarray(img).astype(np.int64)
    pl = None if plane is None else np.maximum(np.asarray(plane).astype(np.int64), 0)
    la, lb, con, st = [], [], [], []
    for p, q in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
        la.append(lab[p].ravel())
        lb.append(lab[q].ravel())
        con.append(np.zeros(la[-1].size, np.int64) if img is None else ((img[p] - img[q]) ** 2).sum(-1).ravel())
        st.append(np.zeros(la[-1].size, np.int64) if pl is None else (pl[p] + pl[q]).ravel())
    return tuple(np.concatenate(v) for v in (la, lb, con, st))


def leaf_graph(lab, k, img=None, plane=None):
    """(H, W) labels, (H, W, 3) uint8 image or None, (H, W) int32 plane or None -> (edges int32 [n][2], vals uint64 [n][3]), the
    edges sorted by (a, b); a pair with a label outside 0 .. k-1 is a crossing of nothing."""
    la, lb, con, st = _pairs(lab, img, plane)
    ok = (la >= 0) & (la < k) & (lb >= 0) & (lb < k) & (la != lb)
    a, b = np.minimum(la, lb)[ok], np.maximum(la, lb)[ok]
    keys, inv = np.unique(a * k + b, return_inverse=True)
    vals = np.zeros((len(keys), 3), np.int64)
    np.add.at(vals[:, 0], inv, 1)
    np.add.at(vals[:, 1], inv, con[ok])
    np.add.at(vals[:, 2], inv, st[ok])
    return np.stack([keys // k, keys % k], 1).astype(np.int32).reshape(-1, 2), vals.astype(np.uint64)


def leaf_graph_loops(lab, k, img=None, plane=None):
    """The same by the definition: a loop over the pixels, Python integers."""
    lab = np.asarray(lab)
    h, w = lab.shape
    acc = {}
    for y in range(h):
        for x in range(w):
            for yy, xx in ((y, x + 1), (y + 1, x)):
                if yy >= h or xx >= w:
                    continue
                a, b = int(lab[y, x]), int(lab[yy, xx])
                if not (0 <= a < k and 0 <= b < k) or a == b:
                    continue
                row = acc.setdefault((min(a, b), max(a, b)), [0, 0, 0])
                row[0] += 1
                if img is not None:
                    row[1] += sum((int(img[y, x, c]) - int(img[yy, xx, c])) ** 2 for c in range(3))
                if plane is not None:
                    row[2] += max(int(plane[y, x]), 0) + max(int(plane[yy, xx]), 0)
    keys = sorted(acc)
    return np.array(keys, np.int32).reshape(-1, 2), np.array([acc[e] for e in keys], np.uint64).reshape(-1, 3)


def cut_graph(edges, vals, group, g):
    """Leaf rows (edges [n][2], vals [n][3]) under a group table (any integers) and G -> the rows of the cut, sorted."""
    group = np.asarray(group).astype(np.int64)
    edges = np.asarray(edges).astype(np.int64).reshape(-1, 2)
    vals = np.asarray(vals).astype(np.uint64).reshape(-1, 3)
    inside = ((edges >= 0) & (edges < len(group))).all(1)
    edges, vals = edges[inside], vals[inside]
    ga, gb = group[edges[:, 0]], group[edges[:, 1]]
    ok = (ga >= 0) & (ga < g) & (gb >= 0) & (gb < g) & (ga != gb)
    a, b = np.minimum(ga, gb)[ok], np.maximum(ga, gb)[ok]
    keys, inv = np.unique(a * g + b, return_inverse=True)
    out = np.zeros((len(keys), 3), np.uint64)
    for e in range(3):
        np.add.at(out[:, e], inv, vals[ok][:, e])
    return np.stack([keys // g, keys % g], 1).astype(np.int32).reshape(-1, 2), out


def table(edges, vals, cap):
    """The output format of one image at capacity ``cap``: (edges int32 [cap][2], vals uint64 [cap][3], count); more than ``cap``
    edges: count = -1 and sentinel rows only."""
    eo, vo = np.full((cap, 2), -1, np.int32), np.zeros((cap, 3), np.uint64)
    n = len(edges)
    if n > cap:
        return eo, vo, -1
    eo[:n], vo[:n] = edges, vals
    return eo, vo, n
