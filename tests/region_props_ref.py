"""NumPy / Python restatement of SPEC.md §19 (region descriptors and mean-colour pictures), for the tests and the timing tool only.
The package never imports it and it uses none of the package's code. The tables of the cuts are made by ANOTHER route than the
kernel's: the map is relabelled through ``region_tree_ref.cut`` and tabulated again; ``cut_tables_by_rows`` restates the kernel's own
route (rows added along the merge list) so that the CPU tests can hold the two against each other."""
import numpy as np

import region_tree_ref as rt

FIXED = 6                                                # n, sum y, sum x, sum R, sum G, sum B


def leaf_table(lab, k, img=None, feats=None, d=None):
    """(H, W) labels, (H, W, 3) uint8 image or None, (D, H, W) integer features or None -> (sums uint64 [k][6 + D], bbox int32
    [k][4]); a pixel whose label is outside 0 .. k-1 is counted nowhere; a label without pixels has the box (H, W, -1, -1)."""
    lab = np.asarray(lab).astype(np.int64)
    h, w = lab.shape
    d = (0 if feats is None else len(feats)) if d is None else d
    ok = (lab >= 0) & (lab < k)
    yy, xx = np.nonzero(ok)
    flat = lab[ok]
    cols = [np.ones(len(flat), np.int64), yy, xx]
    for ch in range(3):
        cols.append(np.zeros(len(flat), np.int64) if img is None else np.asarray(img)[..., ch][ok].astype(np.int64))
    for p in range(d):
        cols.append(np.asarray(feats[p]).astype(np.int64)[ok])
    sums = np.zeros((k, FIXED + d), np.int64)
    for e, v in enumerate(cols):
        np.add.at(sums[:, e], flat, v)
    bbox = np.empty((k, 4), np.int64)
    bbox[:] = (h, w, -1, -1)
    np.minimum.at(bbox[:, 0], flat, yy)
    np.minimum.at(bbox[:, 1], flat, xx)
    np.maximum.at(bbox[:, 2], flat, yy)
    np.maximum.at(bbox[:, 3], flat, xx)
    return sums.astype(np.uint64), bbox.astype(np.int32)


def counted(merges, k):
    """The merge list with every row that does not count (not 0 <= a < b < k with both still reps at that step) replaced by
    (-1, -1): what ``region_tree_ref.cut`` can apply."""
    merges = np.array(merges, np.int64).reshape(-1, 2)
    rep = [True] * k
    for t, (a, b) in enumerate(merges.tolist()):
        if 0 <= a < b < k and rep[a] and rep[b]:
            rep[b] = False
        else:
            merges[t] = (-1, -1)
    return merges.astype(np.int32)


def taus(alive, regions, k):
    """tau of every entry of ``regions``: max(0, alive - R), never past the list, and never below the entry before (an entry that is
    not below its predecessor repeats its predecessor's cut)."""
    out = []
    for r in regions:
        t = min(max(int(alive) - int(r), 0), k - 1)
        out.append(max(t, out[-1]) if out else t)
    return out


def cut_map(lab, merges, k, tau):
    """The map with the first ``tau`` rows applied, numbered as ``region_tree_ref.cut`` numbers (groups by increasing rep)."""
    rows = counted(merges, k).reshape(k - 1, 2).copy()
    rows[tau:] = -1
    return rt.cut(lab, rows, k, 1)                      # alive = k, R = 1: every row of the list, the cleared ones skipped


def cut_tables(lab, merges, alive, regions, k, img=None, feats=None):
    """One image: relabel, then tabulate. -> (group int32 [n][k], sums uint64 [Rsum][C], bbox int32 [Rsum][4], offsets [n + 1]):
    cut c owns the rows offsets[c] .. offsets[c + 1] - 1 (min(k, R_c) of them); a group whose number is not below that has no row."""
    lab = np.asarray(lab).astype(np.int64)
    n_leaf = leaf_table(lab, k)[0][:, 0]
    offsets = np.concatenate([[0], np.cumsum([min(k, max(int(r), 0)) for r in regions])]).astype(np.int64)
    group, sums, bbox = [], [], []
    for c, tau in enumerate(taus(alive, regions, k)):
        cm = cut_map(lab, merges, k, tau)
        ok = (lab >= 0) & (lab < k)
        g = np.full(k, -1, np.int32)
        g[lab[ok]] = cm[ok]                              # every pixel of a leaf carries the same new label:
        assert np.array_equal(g[lab[ok]], cm[ok]) and np.array_equal(g >= 0, n_leaf > 0)
        group.append(g)
        rows = int(offsets[c + 1] - offsets[c])
        s, bx = leaf_table(cm, max(rows, int(cm.max()) + 1, 1), img, feats)
        sums.append(s[:rows])
        bbox.append(bx[:rows])
    return np.stack(group), np.concatenate(sums), np.concatenate(bbox), offsets


def cut_tables_by_rows(sums, bbox, merges, alive, regions, shape):
    """The kernel's route on the leaf table alone: the counted rows below tau add row b into row a (boxes: min / max), the groups
    are numbered by increasing rep among the used leaves, the rows leave densely. ``shape``: (H, W), for the empty box. Same return as
    ``cut_tables``."""
    sums = np.asarray(sums).astype(np.uint64)
    k = sums.shape[0]
    rows_list = counted(merges, k).reshape(k - 1, 2)
    offsets = np.concatenate([[0], np.cumsum([min(k, max(int(r), 0)) for r in regions])]).astype(np.int64)
    group, out_s, out_b = [], [], []
    for c, tau in enumerate(taus(alive, regions, k)):
        s, bx = sums.copy(), np.array(bbox, np.int32)
        root = np.arange(k)
        for a, b in rows_list[:tau].tolist():
            if a < 0:
                continue
            s[a] += s[b]
            s[b] = 0
            bx[a, :2] = np.minimum(bx[a, :2], bx[b, :2])
            bx[a, 2:] = np.maximum(bx[a, 2:], bx[b, 2:])
            root[root == b] = a
        used = sums[:, 0] > 0
        reps = np.unique(root[used])
        number = np.full(k, -1, np.int32)
        number[reps] = np.arange(len(reps))
        group.append(np.where(used, number[root], -1).astype(np.int32))
        rows = int(offsets[c + 1] - offsets[c])
        ts = np.zeros((rows, sums.shape[1]), np.uint64)
        tb = np.empty((rows, 4), np.int32)
        tb[:] = (shape[0], shape[1], -1, -1)
        m = min(rows, len(reps))
        ts[:m], tb[:m] = s[reps[:m]], bx[reps[:m]]
        out_s.append(ts)
        out_b.append(tb)
    return np.stack(group), np.concatenate(out_s), np.concatenate(out_b), offsets


def mean(s, n):
    """SPEC.md §4's rounding rule on Python integers; 0 where n = 0."""
    s, n = int(s), int(n)
    return (2 * s + n) // (2 * n) if n else 0


def paint(lab, sums, group=None, k=None):
    """(H, W) labels -> (H, W, 3) uint8: the mean colour of row ``group[l]`` (or of row l) of ``sums``; black where the label is
    outside 0 .. k-1, the group entry negative (or past the table) or the row empty."""
    lab = np.asarray(lab).astype(np.int64)
    sums = np.asarray(sums)
    k = (len(sums) if group is None else len(group)) if k is None else k
    colour = np.zeros((len(sums) + 1, 3), np.uint8)      # the last row: black
    for g in range(len(sums)):
        colour[g] = [min(255, mean(sums[g][3 + ch], sums[g][0])) for ch in range(3)]
    ok = (lab >= 0) & (lab < k)
    g = np.where(ok, lab, 0)
    if group is not None:
        g = np.asarray(group).astype(np.int64)[g]
    g = np.where(ok & (g >= 0) & (g < len(sums)), g, len(sums))
    return colour[g]
