"""Plain references of one Lloyd pass and of the SPEC.md §4 update, shared by the stage tests of the launch sequence
(tests/test_gpu_value_range.py) and of the self-updating pass (tests/fused_workspace.py, tests/test_gpu_self_updating_stages.py):
a caller-made codebook with a tie and extreme rows, exact int64 sums and counts of an assignment, and written sums that hit the
edges of floor((2 S + n) / (2 n)). For batches of millions of pixels (tests/test_gpu_nt_arm.py): exact_pass, the same pass as float64
matrix products in torch, on whatever device holds the canonical features."""
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


# ------------------------------------------------------------------------------------------ millions of pixels
EXACT_MAX_PIXELS = 1 << 24         # what exact_pass admits in one batch (the bound below)


def exact_assign_sums(x, cent, votes):
    """One image, or any set of pixels. x (D, P) torch float64 holding integers 0 .. 46339, cent (k, D) float64 likewise, votes a
    list of (P,) bool masks -> labels (P,) int64 (ties: the lowest index) and, per mask, (sums (k, D), counts (k,)) as float64
    tensors holding exact integers.

    Exact because every number met is an integer below 2^53, whatever the order a matrix product adds in: a distance
    |x|^2 - 2 x.c + |c|^2 has terms of at most 2 D 46 339^2 <= 8.9e11 (D <= 207), a sum is at most P 46 339 <= 7.8e11 for
    P <= EXACT_MAX_PIXELS - asserted here."""
    import torch
    d, p = x.shape
    k = cent.shape[0]
    assert x.dtype == torch.float64 and cent.dtype == torch.float64 and cent.shape[1] == d
    assert p <= EXACT_MAX_PIXELS and 4 * d * hb.G_MAX ** 2 < 1 << 53 and EXACT_MAX_PIXELS * hb.G_MAX < 1 << 53
    assert 0 <= float(x.min()) and float(x.max()) <= hb.G_MAX and 0 <= float(cent.min()) and float(cent.max()) <= hb.G_MAX
    dist = (cent * cent).sum(1)[:, None] - 2.0 * (cent @ x) + (x * x).sum(0)[None]                      # (k, P)
    index = torch.arange(k, device=x.device)[:, None]
    lab = torch.where(dist == dist.min(0).values[None], index, k).min(0).values                          # lowest index wins a tie
    onehot = lab[None] == index
    out = []
    for v in votes:
        m = (onehot & v[None]).to(torch.float64)
        out.append((m @ x.T, m.sum(1)))
    return lab, out


def as_float64(feats16):
    """int16 tensor holding the bits of uint16 features -> float64 of their values."""
    import torch
    return (feats16.to(torch.int32) & 0xffff).to(torch.float64)


def exact_pass(feats, cent, windows):
    """The reference of one Lloyd pass over a whole batch, image by image on the device that holds ``feats``: (B, D, H, W) torch int16
    (the bits of the uint16 features gcs_features_unpack wrote), cent (n_sets, k, D) NumPy integers, windows a list of (row_lo,
    row_hi) -> labels (B, H, W) uint8 tensor on that device and, per window, (sums (n_sets, k, D), counts (n_sets, k)) NumPy int64
    of the pixels whose row is inside it."""
    import torch
    b, d, h, w = feats.shape
    n_sets, k = cent.shape[:2]
    assert n_sets in (1, b) and b * h * w <= EXACT_MAX_PIXELS
    c = torch.from_numpy(np.asarray(cent, np.float64)).to(feats.device)
    row = torch.arange(h, device=feats.device)[:, None].expand(h, w).reshape(-1)
    votes = [(row >= lo) & (row < hi) for lo, hi in windows]
    labels = torch.empty((b, h, w), dtype=torch.uint8, device=feats.device)
    acc = [(torch.zeros((n_sets, k, d), dtype=torch.float64, device=feats.device),
            torch.zeros((n_sets, k), dtype=torch.float64, device=feats.device)) for _ in windows]
    for i in range(b):
        s = i if n_sets > 1 else 0
        lab, res = exact_assign_sums(as_float64(feats[i].reshape(d, -1)), c[s], votes)
        labels[i] = lab.reshape(h, w).to(torch.uint8)
        for (sums, cnt), (s_i, n_i) in zip(acc, res):
            sums[s] += s_i
            cnt[s] += n_i
    out = []
    for sums, cnt in acc:
        assert float(sums.max()) < 1 << 53
        out.append((sums.cpu().numpy().astype(np.int64), cnt.cpu().numpy().astype(np.int64)))
    return labels, out


def updated(sums, cnt, old):
    """SPEC.md §4 on exact sums (n_sets, k, D), counts (n_sets, k) and the previous centroids: floor((2 S + n) / (2 n)) in int64
    (2 S + n < 2^41 here), an empty cluster keeps its centroid."""
    new = np.array(old, np.int64)
    nz = cnt > 0
    new[nz] = (2 * sums[nz] + cnt[nz][:, None]) // (2 * cnt[nz][:, None])
    return new
