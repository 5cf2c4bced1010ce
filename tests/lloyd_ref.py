"""Plain references of one Lloyd pass and of the SPEC.md §4 update, shared by the stage tests of the launch sequence
(tests/test_gpu_value_range.py) and of the self-updating pass (tests/fused_workspace.py, tests/test_gpu_self_updating_stages.py):
a caller-made codebook with a tie and extreme rows, exact int64 sums and counts of an assignment, and written sums that hit the
edges of floor((2 S + n) / (2 n))."""
import numpy as np

import hot_banks as hb
from oracle import spec_oracle as so


def _caller_codebook(x, k):
    """(k, D) int64 rows a caller might hand in, from the features x (P, D): pixels that hold values >= 32768, TWO IDENTICAL rows
    (the lowest index wins the tie, the other cluster stays empty), the features' rounded mean, an all-zero and an all-46339 row."""
    hot = np.argsort(-x.max(axis=1), kind="stable")
    mean = (2 * x.sum(axis=0) + len(x)) // (2 * len(x))
    rows = [x[hot[0]], x[hot[0]], mean, np.zeros_like(mean), np.full_like(mean, hb.G_MAX)]
    rows += [x[hot[(len(hot) * i) // 40]] for i in range(1, 12)]
    return np.stack(rows[:k]).astype(np.int64)


def _pass_reference(x, cent, vote):
    """x (B, P, D) int64, cent (n_sets, k, D), vote (B, P) bool -> labels (B, P), sums (n_sets, k, D), counts (n_sets, k)."""
    b, n_sets, k = x.shape[0], cent.shape[0], cent.shape[1]
    lab = np.stack([so.kmeans_assign(x[i], cent[i if n_sets > 1 else 0]) for i in range(b)])
    sums = np.zeros((n_sets, k, x.shape[2]), np.int64)
    cnt = np.zeros((n_sets, k), np.int64)
    for i in range(b):
        s = i if n_sets > 1 else 0
        for j in range(k):
            m = (lab[i] == j) & vote[i]
            sums[s, j] += x[i][m].sum(axis=0)
            cnt[s, j] += m.sum()
    return lab, sums, cnt


def _update_cases(d, k):
    """sums (k, d + 1) as Python-int lists and the expected centroids from a previous codebook `old`: S/n at 0, 0.5-ties (round
    half up), 32767.5, 46339, n = 1 and n = 64 * 481 * 321, and empty clusters between full ones."""
    n_big = 64 * 481 * 321
    rng = np.random.default_rng(3)
    old = rng.integers(0, hb.G_MAX + 1, (k, d)).tolist()
    sums, want = [], []
    for j in range(k):
        n = [1, 0, 2, n_big, 0, n_big - 1, 3, 1 << 20][j % 8]
        row = []
        for e in range(d):
            kind = (e + j) % 8
            v = [0, n // 2, (32767 * 2 + 1) * n // 2, hb.G_MAX * n, n - 1 if n else 0, 32768 * n, (hb.G_MAX * 2 - 1) * n // 2,
                 int(rng.integers(0, hb.G_MAX + 1)) * n + int(rng.integers(0, n + 1))][kind]
            row.append(min(v, hb.G_MAX * n))
        sums.append(row + [n])
        want.append([(2 * s + n) // (2 * n) for s in row] if n else old[j])
    return old, sums, want
