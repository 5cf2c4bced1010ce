"""NumPy / Python restatement of SPEC.md §14 (region tree: agglomerative merging on the region adjacency graph), for the tests and
the quality tool only. The package never imports it and it uses none of the package's code. Sequential and plain: sets for the
adjacency, Python integers for the costs, every node picks again in every round."""
import numpy as np

K_MAX = 4096
D_MAX = 207
SIDE_MAX = 4096


def node_stats(x, lab, k):
    """x (D, H, W) integer features, lab (H, W) labels -> (n [k] int64, S [k][D] int64): pixel counts and exact feature sums of the
    labels 0 .. k-1; a pixel whose label is outside that range is counted nowhere."""
    x = np.asarray(x).astype(np.int64)
    lab = np.asarray(lab).astype(np.int64)
    ok = (lab >= 0) & (lab < k)
    flat = lab[ok]
    n = np.bincount(flat, minlength=k).astype(np.int64)
    s = np.zeros((k, x.shape[0]), np.int64)
    for p in range(x.shape[0]):
        np.add.at(s[:, p], flat, x[p][ok])
    return n, s


def adjacency(lab, k):
    """{label: set of labels}: two labels are adjacent when a pixel of one is a 4-neighbour of a pixel of the other; labels outside
    0 .. k-1 are adjacent to nothing."""
    lab = np.asarray(lab).astype(np.int64)
    adj = {}
    for a, b in ((lab[:, :-1], lab[:, 1:]), (lab[:-1, :], lab[1:, :])):
        m = (a != b) & (a >= 0) & (a < k) & (b >= 0) & (b < k)
        for p, q in set(zip(a[m].tolist(), b[m].tolist())):
            adj.setdefault(p, set()).add(q)
            adj.setdefault(q, set()).add(p)
    return adj


def _mean(s, n):
    return (2 * s + n) // (2 * n)                        # SPEC.md §4's rounding rule


def build_tree(x, lab, k, info=None):
    """-> (merges int32 [k-1][2], costs uint64 [k-1], alive int). Row t = the reps (a < b) of the two groups merged at step t; rows
    that were never written are (-1, -1) with cost 0 (rows >= alive - 1, and more when out-of-range labels cut the graph apart).
    ``info``: a dict that receives ``rounds``, the number of rounds taken."""
    x = np.asarray(x)
    if not (1 <= k <= K_MAX and 1 <= x.shape[0] <= D_MAX and max(x.shape[1:]) <= SIDE_MAX):
        raise ValueError("outside the domain of SPEC.md §14")
    n, s = node_stats(x, lab, k)
    adj = adjacency(lab, k)
    nodes = {int(q): dict(n=int(n[q]), S=s[q].copy(), m=_mean(s[q], int(n[q])), adj=set(adj.get(int(q), ())))
             for q in np.flatnonzero(n > 0)}
    alive = len(nodes)
    merges = np.full((k - 1, 2), -1, np.int32)
    costs = np.zeros(k - 1, np.uint64)
    t = n_rounds = 0

    def cost(a, b):
        d = nodes[a]["m"] - nodes[b]["m"]
        return int((d * d).sum()) * min(nodes[a]["n"], nodes[b]["n"])

    while len(nodes) > 1:
        pick = {}
        for a, na in nodes.items():
            if na["adj"]:
                pick[a] = min((cost(a, b), b) for b in na["adj"])
        pairs = sorted((c, a, b) for a, (c, b) in pick.items() if a < b and b in pick and pick[b][1] == a)
        if not pairs:                                    # only when out-of-range labels have cut the graph apart
            break
        n_rounds += 1
        for c, a, b in pairs:
            assert c < 2 ** 62 and pick[b][0] == c
            merges[t] = (a, b)
            costs[t] = c
            t += 1
        for c, a, b in pairs:
            na, nb = nodes[a], nodes.pop(b)
            na["n"] += nb["n"]
            na["S"] = na["S"] + nb["S"]
            na["m"] = _mean(na["S"], na["n"])
            na["adj"] |= nb["adj"]
        gone = {b: a for _, a, b in pairs}
        for a, na in nodes.items():
            na["adj"] = {gone.get(q, q) for q in na["adj"]} - {a}
    if info is not None:
        info["rounds"] = n_rounds
    return merges, costs, alive


def cut(lab, merges, alive, r):
    """The cut at R = r: the first max(0, alive - r) rows of ``merges`` applied ((-1, -1) rows skipped), the groups numbered 0, 1, ... in
    increasing order of their rep; a pixel whose label is outside 0 .. K-1 (K = rows + 1) comes out as -1."""
    lab = np.asarray(lab).astype(np.int64)
    merges = np.asarray(merges)
    k = merges.shape[0] + 1
    if r < 1:
        raise ValueError("R must be >= 1")
    parent = np.arange(k, dtype=np.int64)
    for a, b in merges[:max(0, int(alive) - int(r))]:
        if a >= 0:
            parent[b] = a                                # reps: a is the smallest label of the merged group
    root = parent.copy()
    for q in range(k):                                   # parent[q] <= q: one increasing sweep resolves every chain
        root[q] = root[parent[q]]
    ok = (lab >= 0) & (lab < k)
    used = np.zeros(k, bool)
    used[lab[ok]] = True
    reps = np.unique(root[used])
    new = np.full(k, -1, np.int64)
    new[reps] = np.arange(len(reps))
    out = np.full(lab.shape, -1, np.int64)
    out[ok] = new[root[lab[ok]]]
    return out.astype(np.int32)


def regions(x, lab, k, r):
    """Tree and cut in one call: canonical features x (D, H, W), labels (H, W) in 0 .. k-1 -> labels (H, W) int32 of the cut at r."""
    merges, _, alive = build_tree(x, lab, k)
    return cut(lab, merges, alive, r)


def segment(img, n, r, lam=576, n_iter=10, w=0.0, g=0, mu=0, n_scales=4, n_orient=6, smoothing=0.0, **bank_kw):
    """(H, W, 3) uint8 image -> §13 superpixels (tests/superpixel_ref.py) merged to r regions; with a list ``r``: one map per value,
    from one tree."""
    import position_ref as pr
    import superpixel_ref as sr
    x = pr.features(np.asarray(img), w, g, mu, n_scales, n_orient, smoothing, **bank_kw)
    lab = sr.superpixels(x, n, lam, n_iter)
    _, ny, nx = sr.grid(x.shape[1], x.shape[2], n)
    merges, _, alive = build_tree(x, lab, ny * nx)
    if isinstance(r, (list, tuple)):
        return [cut(lab, merges, alive, q) for q in r]
    return cut(lab, merges, alive, r)
