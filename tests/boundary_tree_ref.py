"""NumPy / Python restatement of SPEC.md §23 (region tree merged by boundary strength), for the tests and the tools only. The package
never imports it and it uses none of the package's code. Sequential and plain: a dict of edges, Python integers for every cost, every
node picks again in every round. The leaf table is §20's (tests/region_adjacency_ref.py), the plane §22's
(tests/feature_gradient_ref.py)."""
import numpy as np

import feature_gradient_ref as fg
import region_adjacency_ref as ra

K_MAX = 4096
E_MAX = 16384


def cost(length, strength):
    """floor(128 sigma / l): 256 times the mean of the plane over the pixels on both sides of the common boundary."""
    return (128 * int(strength)) // int(length)


def tree_of_table(edges, vals, count, used, k, info=None):
    """One image's table of §20 (edges [cap][2], vals [cap][3] = length, contrast, strength, count) and ``used`` [k] (not 0: the label
    owns a pixel) -> (merges int32 [k-1][2], costs uint64 [k-1], alive). count outside 0 .. cap (-1: overflow): alive as defined, no
    row. A row with a label outside 0 .. k-1, with a = b or with a label not in use is ignored; rows of one pair add up. ``info``
    receives ``rounds`` and ``edges`` (the live edges in front of every round)."""
    if not 1 <= k <= K_MAX:
        raise ValueError("outside the domain of SPEC.md §23")
    used = np.asarray(used).reshape(-1)[:k] != 0
    alive = int(used.sum())
    merges = np.full((k - 1, 2), -1, np.int32)
    costs = np.zeros(k - 1, np.uint64)
    edges = np.asarray(edges).reshape(-1, 2)
    vals = np.asarray(vals).astype(np.uint64).reshape(-1, 3)
    n_rounds, live_edges = 0, []
    if info is not None:
        info["rounds"], info["edges"] = 0, live_edges
    if not 0 <= int(count) <= len(edges):
        return merges, costs, alive
    g = {}
    for (a, b), v in zip(edges[:int(count)].tolist(), vals[:int(count)].tolist()):
        if not (0 <= a < k and 0 <= b < k) or a == b or not (used[a] and used[b]):
            continue
        row = g.setdefault((min(a, b), max(a, b)), [0, 0])
        row[0] += int(v[0])
        row[1] += int(v[2])
    t, left = 0, alive
    while left > 1 and g:
        live_edges.append(len(g))
        pick = {}
        for (a, b), (l, s) in g.items():
            c = cost(max(l, 1), s)
            for p, q in ((a, b), (b, a)):
                if p not in pick or (c, q) < pick[p]:
                    pick[p] = (c, q)
        pairs = sorted((c, a, b) for a, (c, b) in pick.items() if a < b and pick[b][1] == a)
        assert pairs, "a live edge and no mutual pair"
        n_rounds += 1
        for c, a, b in pairs:
            assert c < 2 ** 52 and pick[b][0] == c
            merges[t] = (a, b)
            costs[t] = c
            t += 1
        gone = {b: a for _, a, b in pairs}
        g2 = {}
        for (a, b), (l, s) in g.items():
            a2, b2 = gone.get(a, a), gone.get(b, b)
            if a2 == b2:
                continue
            row = g2.setdefault((min(a2, b2), max(a2, b2)), [0, 0])
            row[0] += l
            row[1] += s
        g = g2
        left -= len(pairs)
    if info is not None:
        info["rounds"] = n_rounds
    return merges, costs, alive


def used_labels(lab, k):
    lab = np.asarray(lab).astype(np.int64)
    ok = (lab >= 0) & (lab < k)
    return (np.bincount(lab[ok], minlength=k)[:k] > 0).astype(np.int32)


def build_tree(lab, k, plane, cap=E_MAX, info=None):
    """(H, W) labels, k, (H, W) int32 plane G -> (merges, costs, alive) of SPEC.md §23: the leaf table of §20 at capacity ``cap`` with
    G as its strength plane, then ``tree_of_table``."""
    e, v = ra.leaf_graph(lab, k, None, plane)
    eo, vo, n = ra.table(e, v, cap)
    return tree_of_table(eo, vo, n, used_labels(lab, k), k, info)


def gradient(x, n_scales, slots):
    """§22's plane of canonical features (D, H, W)."""
    return fg.gradient(x, n_scales, slots)
