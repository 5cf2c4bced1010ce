"""SPEC.md §28 restated in NumPy int64 on canonical features: what gcs_kmeans_evaluate is held to, and the float64 finish of the
host. Test helper only; the product never imports it. Labels are also held to ``oracle.spec_oracle.kmeans_assign`` in the CPU
tests, so the restatement and the oracle of SPEC.md §4 check each other."""
import numpy as np

INT64_MAX = np.iinfo(np.int64).max


def distances(x, c, chunk=1 << 14):
    """x (P, D), c (k, D), any integer dtype -> (P, k) int64: d_j(p) = sum_d (x_pd - c_jd)^2, exact."""
    x, c = np.asarray(x).astype(np.int64), np.asarray(c).astype(np.int64)
    out = np.empty((x.shape[0], c.shape[0]), np.int64)
    for p0 in range(0, x.shape[0], chunk):
        diff = x[p0:p0 + chunk, None, :] - c[None, :, :]
        out[p0:p0 + chunk] = (diff * diff).sum(axis=2)
    return out


def evaluate(x, c):
    """One set: x (P, D), c (k, D) -> (label (P,) int32, best (P,) int64, second (P,) int64, stats (k, 2) int64)."""
    d = distances(x, c)
    p, k = d.shape
    label = d.argmin(axis=1)                          # the first minimum: ties go to the lowest j
    rows = np.arange(p)
    best = d[rows, label]
    if k == 1:
        second = best.copy()
    else:
        rest = d.copy()
        rest[rows, label] = INT64_MAX
        second = rest.min(axis=1)
    stats = np.zeros((k, 2), np.int64)
    np.add.at(stats[:, 0], label, 1)
    np.add.at(stats[:, 1], label, best)
    return label.astype(np.int32), best, second, stats


def evaluate_batch(x, cent):
    """x (B, P, D), cent (n_sets, k, D) with n_sets in {1, B} -> (labels (B, P) int32, best (B, P), second (B, P),
    stats (n_sets, k, 2)): image b against set b, or every image against set 0 with the tables added up."""
    x, cent = np.asarray(x), np.asarray(cent)
    b, n_sets = x.shape[0], cent.shape[0]
    assert n_sets in (1, b)
    stats = np.zeros((n_sets, cent.shape[1], 2), np.int64)
    labels, best, second = [], [], []
    for i in range(b):
        s = i if n_sets == b and b > 1 else 0
        lab, bs, sc, st = evaluate(x[i], cent[s])
        stats[s] += st
        labels.append(lab), best.append(bs), second.append(sc)
    return np.stack(labels), np.stack(best), np.stack(second), stats


def confidence(best, second):
    """(second - best) / second in float64, 0 where second = 0, as float32."""
    best, second = np.asarray(best, np.int64), np.asarray(second, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        conf = (second - best).astype(np.float64) / second.astype(np.float64)
    return np.where(second == 0, 0.0, conf).astype(np.float32)


def mse(stats, n_features):
    """stats (n_sets, k, 2) -> (n_sets,) float64: sum_j inertia_j / (P_set * D), P_set = sum_j count_j."""
    stats = np.asarray(stats, np.int64)
    return stats[:, :, 1].sum(axis=1).astype(np.float64) / (stats[:, :, 0].sum(axis=1) * int(n_features)).astype(np.float64)


def schedule(xs, c0, n_iter, mode):
    """SPEC.md §4's schedule from given centroids: xs (B, P, D), c0 (k, D) or (B, k, D) -> (labels (B, P) int32, centroids
    (n_sets, k, D) int64) after n_iter assign passes with an update between them; "per_image": every image refines its own copy,
    "global": one copy over the batch."""
    from oracle import spec_oracle as so
    xs = np.asarray(xs).astype(np.int64)
    c0 = np.asarray(c0).astype(np.int64)
    b = xs.shape[0]
    sets = [xs[i] for i in range(b)] if mode == "per_image" else [xs.reshape(-1, xs.shape[2])]
    labels, cents = [], []
    for s, x in enumerate(sets):
        c = (c0[s] if c0.ndim == 3 and c0.shape[0] > 1 else c0.reshape(-1, *c0.shape[-2:])[0]).copy()
        lab = None
        for t in range(n_iter):
            lab = so.kmeans_assign(x, c)
            if t < n_iter - 1:
                c = so.kmeans_update(x, lab, c)[0]
        labels.append(lab.reshape(-1, xs.shape[1]))
        cents.append(c)
    return np.concatenate(labels).astype(np.int32), np.stack(cents)
