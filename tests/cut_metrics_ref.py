"""NumPy / Python restatement of SPEC.md §17 (the reference's region and shape metrics of every cut of the region tree), for the tests
only, by another method than the kernels': per cut the table of ``region_sweep_ref.cut_table`` reduced by whole-array expressions, and
every pixel relabelled to its group's rep before it is counted. The package never imports it. Below the restatement: the cases the
CPU and the GPU tests share."""
import numpy as np

import contour_map_ref as cm
import region_sweep_ref as rs


def contour_map(lab, merges, alive, k=None):
    """U of SPEC.md §15 for ANY merge list: rows that do not count (not 0 <= a < b < k with both reps at that step) are skipped, as
    §16 skips them; ``contour_map_ref.contour_map`` on the lists it accepts."""
    lab = np.asarray(lab).astype(np.int64)
    rows = np.asarray(merges).reshape(-1, 2)
    k = rows.shape[0] + 1 if k is None else int(k)
    s = np.full((k + 1, k + 1), int(alive), np.int32)
    np.fill_diagonal(s, 0)
    members = {q: [q] for q in range(k)}
    for t, (a, b) in enumerate(rows.tolist()):
        if 0 <= a < b < k and a in members and b in members:
            ma, mb = members[a], members.pop(b)
            s[np.ix_(ma, mb)] = t + 1
            s[np.ix_(mb, ma)] = t + 1
            members[a] = ma + mb
    l = np.where((lab >= 0) & (lab < k), lab, k)
    u = np.zeros(l.shape, np.int64)
    u[:, 1:] = np.maximum(u[:, 1:], s[l[:, 1:], l[:, :-1]])
    u[:, :-1] = np.maximum(u[:, :-1], s[l[:, :-1], l[:, 1:]])
    u[1:, :] = np.maximum(u[1:, :], s[l[1:, :], l[:-1, :]])
    u[:-1, :] = np.maximum(u[:-1, :], s[l[:-1, :], l[1:, :]])
    return u.astype(np.int32)


def tau_of(alive, r, k):
    if int(r) < 1:
        raise ValueError("R must be >= 1")
    return min(max(0, int(alive) - int(r)), k - 1)


def under_counts(lab, merges, alive, truths, regions, k=None, stride=None):
    """One image -> uint64 [len(regions)][A][3] = {N_t, under, under_np} in the order of ``regions``."""
    rows = np.asarray(merges).reshape(-1, 2)
    k = rows.shape[0] + 1 if k is None else int(k)
    out = np.zeros((len(regions), len(truths), 3), np.uint64)
    for t, g in enumerate(truths):
        leaf = rs.leaf_table(lab, g, k, stride)
        for j, r in enumerate(regions):
            n = rs.cut_table(leaf, rows, tau_of(alive, r, k))
            a = n.sum(axis=1)
            out[j, t] = [int(a.sum()), int(np.sum(a - n.max(axis=1))), int(np.sum(np.minimum(n, a[:, None] - n)))]
    return out


def shapes(lab, u, merges, alive, regions, k=None):
    """One image and its contour map -> (area uint32 [len(regions)][k], perim uint32 [len(regions)][k], boundary uint32
    [len(regions)]): every in-range pixel relabelled to its group's rep, then counted."""
    lab = np.asarray(lab).astype(np.int64)
    u = np.asarray(u).astype(np.int64)
    rows = np.asarray(merges).reshape(-1, 2)
    k = rows.shape[0] + 1 if k is None else int(k)
    ok = (lab >= 0) & (lab < k)
    border = np.zeros(lab.shape, bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    area = np.zeros((len(regions), k), np.uint32)
    perim = np.zeros((len(regions), k), np.uint32)
    boundary = np.zeros(len(regions), np.uint32)
    for j, r in enumerate(regions):
        tau = tau_of(alive, r, k)
        root = np.arange(k)
        for a, b in rs.written_rows(rows, k, tau):
            root[root == b] = a
        rep = root[np.where(ok, lab, 0)]
        thick = u > tau
        area[j] = np.bincount(rep[ok], minlength=k)
        perim[j] = np.bincount(rep[ok & (border | thick)], minlength=k)
        boundary[j] = int(thick.sum())
    return area, perim, boundary


def batch(labs, merges, alives, truths_per_image, regions, k=None, stride=None, us=None):
    """A batch -> what the two entry points write: (counts uint64 [n][T][3], area uint32 [n][B][k], perim uint32 [n][B][k], boundary
    uint32 [n][B], contour maps int32 [B][H][W]). ``us``: contour maps to use instead of ``contour_map`` of each image."""
    cs, ars, pes, bds, maps = [], [], [], [], []
    for i, lab in enumerate(labs):
        kk = np.asarray(merges[i]).reshape(-1, 2).shape[0] + 1 if k is None else k
        u = contour_map(lab, merges[i], alives[i], kk) if us is None else us[i]
        cs.append(under_counts(lab, merges[i], alives[i], truths_per_image[i], regions, kk, stride))
        a, p, b = shapes(lab, u, merges[i], alives[i], regions, kk)
        ars.append(a), pes.append(p), bds.append(b), maps.append(u)
    return np.concatenate(cs, axis=1), np.stack(ars, axis=1), np.stack(pes, axis=1), np.stack(bds, axis=1), np.stack(maps)


# ---- shared cases: name -> (labels (H, W), merges [k - 1][2], alive, annotator maps, regions)

TREES = {"chain": cm.chain, "star": cm.star, "balanced": cm.balanced}
R_4096 = [5000, 4096, 4095, 1000, 64, 8, 3, 2, 1]


def small_cases():
    """Everything but K = 4096, every R in 1 .. alive + 2 (the wall and the malformed lists: not comparable with a relabelled cut)."""
    out = {}
    lab, truths = rs.noise_case()
    for name, tree in TREES.items():
        out["k40_" + name] = (lab, tree(40), 40, truths, list(range(1, 43)))
    rng = np.random.default_rng(23)
    a = rng.integers(0, 40, (19, 23)).astype(np.int32)
    a[a == 17] = 3
    a[a == 30] = 31                                          # 38 of 40 labels own a pixel: the tree of the 38 as a chain, holes behind
    used = np.unique(a)
    m = np.full((39, 2), -1, np.int32)
    m[:37] = [(used[q - 1], used[q]) for q in range(37, 0, -1)]
    out["unused_labels"] = (a, m, 38, rs.noise_case(seed=5)[1], list(range(1, 41)))
    b = np.full((19, 23), 7, np.int32)
    b[:, :3] = 3
    b[:, 20:] = 3                                            # label 3 in two pieces
    b[5:9, 8:14] = 12
    b[12:15, 5:18] = np.arange(20, 33)[None, :] % 3 + 20
    m = np.full((39, 2), -1, np.int32)
    m[:5] = [(20, 21), (7, 12), (20, 22), (3, 7), (3, 20)]
    out["two_pieces"] = (b, m, 6, rs.noise_case(seed=5)[1], list(range(1, 9)))
    for shape in ((1, 7), (7, 1), (2, 2)):                   # every pixel on the image border
        n = shape[0] * shape[1]
        lab = np.random.default_rng(n).permutation(n).reshape(shape).astype(np.int32)
        out["shape_%dx%d" % shape] = (lab, cm.balanced(n), n, rs.noise_case(seed=n, shape=shape, n_maps=2)[1], list(range(1, n + 3)))
    out["k1"] = (np.zeros((5, 7), np.int32), np.zeros((0, 2), np.int32), 1, rs.noise_case(seed=2, shape=(5, 7))[1], [1, 2, 9])
    lab2 = (np.arange(35).reshape(5, 7) % 3 == 0).astype(np.int32)
    out["k2_joined"] = (lab2, np.array([[0, 1]], np.int32), 2, rs.noise_case(seed=3, shape=(5, 7))[1], [1, 2, 3, 4])
    out["k2_never_joined"] = (lab2, np.array([[-1, -1]], np.int32), 2, rs.noise_case(seed=3, shape=(5, 7))[1], [1, 2, 3, 4])
    return out


def odd_cases():
    """Lists and maps a relabelled cut does not describe: compared against the restatement alone."""
    out = {}
    lab, truths = rs.noise_case(seed=8, k=6, shape=(9, 11))
    out["holes"] = (lab, np.array([[1, 2], [-1, -1], [0, 1], [-1, -1], [3, 4]], np.int32), 6, truths, [7, 6, 5, 4, 3, 2, 1])
    bad = np.array([[1, 2], [0, 2], [2, 3], [4, 3], [3, 3], [0, 6], [0, 1]], np.int32)       # K = 8: rows 1 .. 4 do not count
    lab8, truths8 = rs.noise_case(seed=9, k=8, shape=(9, 11))
    out["malformed"] = (lab8, bad, 8, truths8, [9, 8, 7, 6, 5, 4, 3, 2, 1])
    wall, truthsw = rs.noise_case(seed=10, k=12, shape=(9, 11))
    wall = wall.copy()
    wall[:, 5] = -1                                          # a wall of out-of-range labels cuts the image in two
    wall[4, 2] = 12
    out["wall"] = (wall, cm.balanced(12), 12, truthsw, [14, 12, 11, 6, 3, 2, 1])
    return out


def one_pixel_cases():
    lab, truths = rs.one_pixel_case()
    return {"k4096_" + name: (lab, tree(4096), 4096, truths, R_4096) for name, tree in TREES.items()}
