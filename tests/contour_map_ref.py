"""NumPy / Python restatement of SPEC.md §15 (contour map of the region tree, sweep histograms), for the tests only, by another
method than the kernels': a K x K matrix of join levels filled row by row from the members of the two groups a row merges, then
four shifted comparisons of the label map; the histograms from ``evaluate.find_boundaries`` / ``_dilate`` and
``scipy.ndimage.grey_dilation``. The package never imports it."""
import numpy as np
from scipy import ndimage as ndi


def strengths(merges, k, alive):
    """-> s int64 [k + 1][k + 1]: s[p][q] of SPEC.md §15 for labels p, q in 0 .. k-1; index k stands for the label -1. Rows of
    ``merges`` that are (-1, -1) are skipped; a pair no row joins keeps ``alive``."""
    merges = np.asarray(merges).reshape(-1, 2)
    s = np.full((k + 1, k + 1), int(alive), np.int64)
    np.fill_diagonal(s, 0)
    members = {q: [q] for q in range(k)}
    for t, (a, b) in enumerate(merges.tolist()):
        if a < 0:
            continue
        assert 0 <= a < b < k and a in members and b in members, (t, a, b)
        ma, mb = members[a], members.pop(b)
        s[np.ix_(ma, mb)] = t + 1
        s[np.ix_(mb, ma)] = t + 1
        members[a] = ma + mb
    return s


def contour_map(lab, merges, alive):
    """(H, W) labels, merges [k - 1][2], alive -> U int32 (H, W)."""
    lab = np.asarray(lab).astype(np.int64)
    k = np.asarray(merges).reshape(-1, 2).shape[0] + 1
    s = strengths(merges, k, alive)
    l = np.where((lab >= 0) & (lab < k), lab, k)
    u = np.zeros(l.shape, np.int64)
    u[:, 1:] = np.maximum(u[:, 1:], s[l[:, 1:], l[:, :-1]])
    u[:, :-1] = np.maximum(u[:, :-1], s[l[:, :-1], l[:, 1:]])
    u[1:, :] = np.maximum(u[1:, :], s[l[1:, :], l[:-1, :]])
    u[:-1, :] = np.maximum(u[:-1, :], s[l[:-1, :], l[1:, :]])
    return u.astype(np.int32)


def window_max(u):
    """M5(U): the maximum over the 5 x 5 window clipped to the image (scipy's reflect border only repeats in-window pixels)."""
    return ndi.grey_dilation(np.asarray(u), footprint=np.ones((5, 5), bool))


def histograms(u, truths, k):
    """U (H, W) and the annotator maps of its image -> (hist_map [k + 1], hist_rec [A][k + 1], hist_prec [A][k + 1]) uint32."""
    from gabor_color_image_segmentation_amd.evaluate import _dilate, find_boundaries
    u = np.asarray(u).astype(np.int64)
    m5 = window_max(u)

    def hist(values):
        values = values[(values >= 1) & (values <= k)]
        return np.bincount(values, minlength=k + 1).astype(np.uint32)
    rec, prec = [], []
    for t in truths:
        bd = find_boundaries(np.asarray(t))
        rec.append(hist(m5[bd]))
        prec.append(hist(u[_dilate(bd, 5)]))
    return hist(u.ravel()), np.array(rec).reshape(len(truths), k + 1), np.array(prec).reshape(len(truths), k + 1)


def chain(k):
    return np.array([(q - 1, q) for q in range(k - 1, 0, -1)], np.int32).reshape(k - 1, 2)


def star(k):
    return np.array([(0, q) for q in range(1, k)], np.int32).reshape(k - 1, 2)


def balanced(k):
    """Pairs at distance 1, then 2, 4, ...: (0,1), (2,3), ..., then (0,2), (4,6), ...; any k."""
    rows, d = [], 1
    while d < k:
        rows += [(q, q + d) for q in range(0, k - d, 2 * d)]
        d *= 2
    return np.array(rows, np.int32).reshape(k - 1, 2)
