"""SPEC.md §29 restated in NumPy int64 on canonical features, with Python integers for the draws (arithmetic mod 2^64 and the
128-bit product): what gcs_kmeans_seed is held to, the host's stride rule, and the selection among restarts. Test helper only;
the product never imports it."""
import numpy as np

import kmeans_model_ref as km

M64 = (1 << 64) - 1
N_MAX = 4096


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u(seed, r, t):
    return mix(mix(int(seed) & M64) ^ (16 * r + t))


def pick(v, total):
    """floor(v * total / 2^64): the high word of the 128-bit product."""
    return (int(v) * int(total)) >> 64


def grid(h, w, stride):
    """The candidate pixels of an (h, w) image -> (ys, xs): rows and columns of the grid."""
    axis = lambda n: np.minimum(stride * np.arange(-(-n // stride)) + stride // 2, n - 1)
    return axis(h), axis(w)


def candidates(h, w, stride):
    """Raster indices y * w + x of the candidates of one image, in raster order of the grid."""
    ys, xs = grid(h, w, stride)
    return (ys[:, None] * w + xs[None, :]).ravel()


def seed_stride(b_set, h, w):
    """The smallest power of two >= 8 at which a set of b_set images has at most 4096 candidates."""
    s = 8
    while s <= 4096:
        if b_set * -(-h // s) * -(-w // s) <= N_MAX:
            return s
        s *= 2
    raise ValueError("more than 4096 images in one set")


def seed_set(x, k, seed=0, trials=4):
    """One set: x (n, D) candidate features (any integer dtype), 1 <= n <= 4096 -> (centroids (k, D) int64, picks (k,) int32,
    potential int). ``rounds`` of the draws are in ``seed_trace``."""
    return seed_trace(x, k, seed, trials)[:3]


def seed_trace(x, k, seed=0, trials=4):
    """As ``seed_set``, plus the list of rounds: (T, [(rho_t, q_t, pot_t)]) for every round with T > 0, (T, None) otherwise."""
    x = np.asarray(x).astype(np.int64)
    n = x.shape[0]
    assert 1 <= n <= N_MAX and 1 <= k <= 16 and 1 <= trials <= 8
    dist = lambda q: km.distances(x, x[q:q + 1])[:, 0]
    picks = [pick(u(seed, 0, 0), n)]
    m = dist(picks[0])
    rounds = [(None, None)]
    for r in range(1, k):
        total = int(m.sum())
        if total == 0:
            q = pick(u(seed, r, 0), n)
            rounds.append((0, None))
        else:
            prefix = np.cumsum(m)
            tried = []
            for t in range(trials):
                rho = pick(u(seed, r, t), total)
                qt = int(np.searchsorted(prefix, rho, side="right"))     # the smallest q with prefix[q] > rho
                tried.append((rho, qt, int(np.minimum(m, dist(qt)).sum())))
            best = min(range(trials), key=lambda t: (tried[t][2], t))
            q = tried[best][1]
            rounds.append((total, tried))
        picks.append(q)
        m = np.minimum(m, dist(q))
    picks = np.asarray(picks, np.int32)
    return x[picks].copy(), picks, int(m.sum()), rounds


def seed_batch(xs, h, w, k, n_sets, stride, seed=0, trials=4):
    """xs (B, H*W, D) canonical features -> (centroids (n_sets, k, D) int64, picks (n_sets, k) int32, potential (n_sets,) int64):
    one set per image (n_sets = B) or one over the batch (n_sets = 1)."""
    xs = np.asarray(xs)
    b = xs.shape[0]
    assert n_sets in (1, b)
    cand = xs[:, candidates(h, w, stride)]                            # (B, per, D)
    sets = [cand[i] for i in range(b)] if n_sets == b else [cand.reshape(-1, xs.shape[2])]
    out = [seed_set(s, k, seed, trials) for s in sets]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.asarray([o[2] for o in out], np.int64))


def best_restart(inertias):
    """inertias (n_init, n_sets): the sum of a set's inertias after every restart -> (n_sets,) the restart each set keeps: the
    smallest, ties to the lowest restart."""
    return np.asarray(inertias).argmin(axis=0)
