"""NumPy / Python restatement of SPEC.md §16 (region metrics of every cut of the region tree), for the tests only: a leaf table by
``bincount``, the merge rows applied one after the other as row additions, §8's sums and terms of the table in hand by whole-array
expressions. The package never imports it. Below the restatement: the cases the CPU and the GPU tests share."""
import numpy as np


def leaf_table(lab, truth, k, stride=None):
    """(H, W) labels and one annotator map -> int64 [k][stride] with n_ij = #{label i, annotator label j}; a pixel whose label is outside
    0 .. k-1 (or whose annotator label is >= stride) is counted nowhere."""
    lab = np.asarray(lab).astype(np.int64).ravel()
    g = np.asarray(truth).astype(np.int64).ravel()
    stride = int(g.max()) + 1 if stride is None else int(stride)
    ok = (lab >= 0) & (lab < k) & (g < stride)
    return np.bincount(lab[ok] * stride + g[ok], minlength=k * stride).reshape(k, stride).astype(np.int64)


def written_rows(merges, k, tau):
    """The rows among the first ``tau`` that count: 0 <= a < b < k and both still reps at that step. -> list of (a, b)."""
    rep = [True] * k
    out = []
    for a, b in np.asarray(merges).reshape(-1, 2)[:max(0, int(tau))].tolist():
        if 0 <= a < b < k and rep[a] and rep[b]:
            rep[b] = False
            out.append((a, b))
    return out


def cut_table(table, merges, tau):
    """The leaf table with the first ``tau`` rows applied: row b added into row a, row b emptied. A new array."""
    t = np.array(table, np.int64)
    for a, b in written_rows(merges, t.shape[0], tau):
        t[a] += t[b]
        t[b] = 0
    return t


def sums_terms(table):
    """§8's sums [N, sum a^2, sum b^2, sum n^2] (Python ints) and terms [sum a log2 a, sum b log2 b, sum n log2 n, sum_j b_j n*_j / u*_j]
    (floats) of one table, the row and column sums taken from the table itself."""
    n = np.asarray(table).astype(np.int64)
    a, b = n.sum(axis=1), n.sum(axis=0)

    def xlog(v):
        v = v[v > 0].astype(np.float64)
        return float(np.sum(v * np.log2(v)))
    u = a[:, None] + b[None, :] - n
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(n > 0, n / np.maximum(u, 1), 0.0)
    cov = float(np.sum(b.astype(np.float64) * ratio.max(axis=0))) if n.size else 0.0
    sums = [int(b.sum()), int(np.sum(a * a)), int(np.sum(b * b)), int(np.sum(n * n))]
    return sums, [xlog(a), xlog(b), xlog(n.ravel()), cov]


def sweep(lab, merges, alive, truths, regions, k=None, stride=None):
    """One image: -> (sums uint64 [len(regions)][A][4], terms float64 [len(regions)][A][4]) in the order of ``regions``."""
    merges = np.asarray(merges).reshape(-1, 2)
    k = merges.shape[0] + 1 if k is None else int(k)
    sums = np.zeros((len(regions), len(truths), 4), np.uint64)
    terms = np.zeros((len(regions), len(truths), 4), np.float64)
    for t, g in enumerate(truths):
        leaf = leaf_table(lab, g, k, stride)
        for j, r in enumerate(regions):
            if int(r) < 1:
                raise ValueError("R must be >= 1")
            s, f = sums_terms(cut_table(leaf, merges, max(0, int(alive) - int(r))))
            sums[j, t] = s
            terms[j, t] = f
    return sums, terms


# ---- shared cases

def noise_case(seed=40, k=40, shape=(19, 23), n_maps=3, top=None):
    """Noise labels in 0 .. k-1 and ``n_maps`` annotator maps of 7 labels (0 .. 6); ``top``: one pixel of every map gets that label."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, shape).astype(np.int32)
    truths = []
    for _ in range(n_maps):
        g = rng.integers(0, 7, shape).astype(np.uint16)
        g[:, :shape[1] // 3] = 2                                   # some structure: a large annotator region
        if top is not None:
            g[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = top
        truths.append(g)
    return lab, truths


def one_pixel_case(seed=64, side=64, n_maps=3):
    """side x side one-pixel labels (K = side^2) and annotator maps of 7 labels in vertical bands with noise."""
    rng = np.random.default_rng(seed)
    lab = np.arange(side * side, dtype=np.int32).reshape(side, side)
    truths = []
    for _ in range(n_maps):
        g = (np.arange(side)[None, :] * 7 // side + np.zeros((side, 1), np.int64)).astype(np.uint16)
        m = rng.random((side, side)) < 0.2
        g[m] = rng.integers(0, 7, int(m.sum()))
        truths.append(g)
    return lab, truths


def block_case():
    """321 x 481 in 23-pixel blocks (K = 14 * 21 = 294) and five block-shaped annotator maps with labels up to 207."""
    h, w = 321, 481
    yy, xx = np.mgrid[0:h, 0:w]
    lab = ((yy // 23) * 21 + xx // 23).astype(np.int32)
    truths = []
    for by, bx in ((20, 25), (17, 31), (40, 13), (11, 58), (29, 23)):
        nbx = (w + bx - 1) // bx
        truths.append((((yy // by) * nbx + xx // bx) % 208).astype(np.uint16))
    assert lab.max() == 293 and all(int(g.max()) == 207 for g in truths)
    return lab, truths
