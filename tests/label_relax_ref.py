"""SPEC.md §30 restated in NumPy int64: the four class sub-passes of an ICM sweep on a Potts energy, the tie rule, "no label", beta
from the stats table of SPEC.md §28, the changed counts and the energy. What gcs_label_relax and the host arithmetic are held to.
Test helper only; the product never imports it."""
import numpy as np

BETA_MAX = (1 << 58) - 1
NONE, ABSENT = -1, -2                      # "no label"; a neighbour outside the image
OFFSETS4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
OFFSETS8 = OFFSETS4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def q_of(lam):
    """round(256 lambda), halves up."""
    return int(np.floor(256.0 * float(lam) + 0.5))


def beta_of(stats, q):
    """stats (n_sets, k, 2) int64 = (count, inertia) -> (n_sets,) int64: (q * floor(sum inertia / sum count)) >> 8."""
    stats = np.asarray(stats, np.int64)
    m = stats[:, :, 1].sum(axis=1) // stats[:, :, 0].sum(axis=1)
    return (m * int(q)) >> 8


def clamp_beta(beta):
    return min(max(int(beta), 0), BETA_MAX)


def normalise(labels, k):
    """Labels outside 0..k-1 -> NONE."""
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab >= 0) & (lab < k), lab, NONE)


def _offsets(neighbours):
    assert neighbours in (4, 8)
    return OFFSETS4 if neighbours == 4 else OFFSETS8


def sub_pass(costs, lab, beta, cls, neighbours):
    """One sub-pass in place on ``lab`` (H, W) int64, raw values: class ``cls`` = 2 (y & 1) + (x & 1). Returns the changed count."""
    k, h, w = costs.shape
    cy, cx = cls >> 1, cls & 1
    if cy >= h or cx >= w:
        return 0
    pad = np.full((h + 2, w + 2), ABSENT, np.int64)
    pad[1:-1, 1:-1] = normalise(lab, k)
    ys, xs = np.mgrid[cy:h:2, cx:w:2]
    q = np.stack([pad[ys + 1 + dy, xs + 1 + dx] for dy, dx in _offsets(neighbours)])        # (n_off, hc, wc)
    n = (q != ABSENT).sum(axis=0)
    same = np.stack([(q == j).sum(axis=0) for j in range(k)])                               # (k, hc, wc)
    e = costs[:, ys, xs] + beta * (n[None] - same)
    best, arg = e.min(axis=0), e.argmin(axis=0)                                             # the first minimum: the lowest j
    raw = lab[ys, xs]
    own = pad[ys + 1, xs + 1]
    e_own = np.where(own == NONE, beta * (n - (q == NONE).sum(axis=0)),
                     np.take_along_axis(e, np.maximum(own, 0)[None], axis=0)[0])
    stay = np.where(own == NONE, e_own < best, e_own == best)     # the current label wins ties, "no label" never does
    lab[ys, xs] = np.where(stay, raw, arg)
    return int((~stay).sum())


def energy(costs, labels, neighbours):
    """(unary, pairs) of a map: unary = sum_p C[L(p)](p) (0 for "no label"), pairs = unordered neighbour pairs that differ."""
    k, h, w = costs.shape
    lab = normalise(labels, k)
    unary = int(np.where(lab == NONE, 0, np.take_along_axis(costs, np.maximum(lab, 0)[None], axis=0)[0]).sum())
    pairs = int((lab[:, 1:] != lab[:, :-1]).sum()) + int((lab[1:] != lab[:-1]).sum())
    if neighbours == 8:
        pairs += int((lab[1:, 1:] != lab[:-1, :-1]).sum()) + int((lab[1:, :-1] != lab[:-1, 1:]).sum())
    return unary, pairs


def relax(costs, labels, beta, sweeps, neighbours=8):
    """One image: costs (k, H, W), labels (H, W), beta int -> (labels (H, W) int32, changed [sweeps], (unary, pairs))."""
    costs = np.asarray(costs, np.int64)
    lab = np.asarray(labels).astype(np.int64).copy()
    beta = clamp_beta(beta)
    changed = [sum(sub_pass(costs, lab, beta, c, neighbours) for c in range(4)) for _ in range(sweeps)]
    return lab.astype(np.int32), changed, energy(costs, lab, neighbours)


def total_energy(costs, labels, beta, neighbours=8):
    unary, pairs = energy(np.asarray(costs, np.int64), labels, neighbours)
    return unary + clamp_beta(beta) * pairs


def relax_batch(costs, labels, beta, sweeps, neighbours=8):
    """costs (B, k, H, W), labels (B, H, W), beta (B,) -> (labels (B, H, W) int32, changed (B, sweeps) int32, energy (B, 2) int64)."""
    out = [relax(c, l, int(bt), sweeps, neighbours) for c, l, bt in zip(costs, labels, beta)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32).reshape(len(out), sweeps),
            np.array([o[2] for o in out], np.int64))


def cost_volume(x, cent, h, w):
    """x (B, P, D) canonical features, cent (n_sets, k, D) -> (B, k, H, W) int64: the distances of SPEC.md §28."""
    import kmeans_model_ref as km
    x, cent = np.asarray(x), np.asarray(cent)
    b, n_sets = x.shape[0], cent.shape[0]
    return np.stack([km.distances(x[i], cent[i if n_sets == b and b > 1 else 0]).T.reshape(-1, h, w) for i in range(b)])
