"""NumPy restatement of SPEC.md §13 (superpixels: grid-local k-means), for the tests and the quality tool only. The package never
imports it and it uses none of the package's code: the features come from ``position_ref.features`` (C oracle + the restated
§10 - §12), the grid, init, assign, update and schedule are restated here in int64."""
import math

import numpy as np

import position_ref as pr

N_MAX = K_MAX = 4096
LAMBDA_MAX = 65535
SIDE_MAX = 4096
D_MAX = 207


def grid(h, w, n):
    """(S, ny, nx): S = max(1, rint(sqrt(H W / n))), ny = max(1, rint(H / S)), nx = max(1, rint(W / S)), rint = round-half-even on the
    float64 value (``np.rint``). Raises ValueError outside the domain or when ny * nx > 4096."""
    if not (isinstance(n, (int, np.integer)) and 2 <= n <= N_MAX):
        raise ValueError("n must be an integer in 2..4096")
    if not (1 <= h <= SIDE_MAX and 1 <= w <= SIDE_MAX):
        raise ValueError("H, W must be in 1..4096")
    s = max(1, int(np.rint(math.sqrt(np.float64(h * w) / np.float64(n)))))
    ny, nx = max(1, int(np.rint(np.float64(h) / np.float64(s)))), max(1, int(np.rint(np.float64(w) / np.float64(s))))
    if ny * nx > K_MAX:
        raise ValueError(f"grid {ny} x {nx} has more than {K_MAX} centres")
    return s, ny, nx


def init_positions(h, w, ny, nx):
    """(cy, cx) int64 [K]: cy_q = floor((2i+1) H / (2 ny)), cx_q = floor((2j+1) W / (2 nx)) for q = i nx + j."""
    i, j = np.divmod(np.arange(ny * nx, dtype=np.int64), nx)
    return ((2 * i + 1) * h) // (2 * ny), ((2 * j + 1) * w) // (2 * nx)


def candidates(h, w, ny, nx):
    """(9, H, W) int64: the centre index of cell (gi + di, gj + dj) for every pixel, di-major, -1 where the cell does not exist."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    gi, gj = (y * ny) // h, (x * nx) // w
    out = []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ci, cj = gi + di, gj + dj
            ok = (ci >= 0) & (ci < ny) & (cj >= 0) & (cj < nx)
            out.append(np.where(ok, ci * nx + cj, -1))
    return np.stack(out)


def assign(x, cent, cy, cx, ny, nx, lam, cand=None, info=None):
    """x (D, H, W), cent (K, D), cy / cx (K,), all int64 -> labels (H, W) int64: the argmin over the existing 3 x 3 candidates of
    sum_d (x_d - c_d)^2 + lam ((y - cy)^2 + (x - cx)^2), ties to the lowest centre index. ``info``, a dict, receives what the tests'
    witnesses need and the labels do not: ``tied`` = the pixels whose least distance two or more distinct centres attain, ``dmax`` =
    the largest distance of a pixel and an existing candidate, ``smax`` = the largest spatial term of one."""
    d, h, w = x.shape
    if cand is None:
        cand = candidates(h, w, ny, nx)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    best = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    lab = np.full((h, w), -1, np.int64)
    at_best = np.zeros((h, w), np.int64)             # candidates at the least distance so far (they are distinct centres)
    dmax = smax = 0
    for q in cand:                                   # di-major, dj-minor: increasing centre index
        ok = q >= 0
        qq = np.where(ok, q, 0)
        dist = lam * ((yy - cy[qq]) ** 2 + (xx - cx[qq]) ** 2)
        if info is not None and ok.any():
            smax = max(smax, int(dist[ok].max()))
        for p in range(d):                           # plane by plane: no (H, W, D) temporary
            dist = dist + (x[p] - cent[qq, p]) ** 2
        if info is not None and ok.any():
            dmax = max(dmax, int(dist[ok].max()))
            at_best = np.where(ok & (dist < best), 1, np.where(ok & (dist == best), at_best + 1, at_best))
        better = ok & ((dist < best) | ((dist == best) & (q < lab)))
        best = np.where(better, dist, best)
        lab = np.where(better, q, lab)
    if info is not None:
        info.update(tied=int((at_best >= 2).sum()), dmax=dmax, smax=smax)
    return lab


def update(x, lab, cent, cy, cx):
    """SPEC.md §4's rule floor((2 S + n) / (2 n)) on every feature and on cy, cx; an empty centre keeps its values."""
    d, h, w = x.shape
    k = cent.shape[0]
    flat = lab.ravel()
    cnt = np.bincount(flat, minlength=k).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    full = cnt > 0
    den = np.maximum(2 * cnt, 1)
    new = cent.copy()
    for p in range(d):
        s = _isum(flat, x[p].ravel(), k)
        new[:, p] = np.where(full, (2 * s + cnt) // den, cent[:, p])
    sy, sx = _isum(flat, yy.ravel(), k), _isum(flat, xx.ravel(), k)
    return new, np.where(full, (2 * sy + cnt) // den, cy), np.where(full, (2 * sx + cnt) // den, cx)


def _isum(idx, vals, k):
    """Exact int64 sums of vals per index (np.bincount's weights are float64: not used)."""
    out = np.zeros(k, np.int64)
    np.add.at(out, idx, vals)
    return out


def superpixels_on_grid(x, ny, nx, lam=576, n_iter=10, return_centres=False, trace=None):
    """Canonical features x (D, H, W) (uint16 values) -> labels (H, W) int32 of SPEC.md §13 on the caller's ny x nx grid (any 1 <= ny
    <= H, 1 <= nx <= W with ny * nx <= 4096, as gcs_superpixel_segment takes it): init, then n_iter assigns with an update behind all
    but the last. With ``return_centres``: also (K, D + 2) int64 = the D features, cy, cx the last assign used.
    ``trace``, a list, receives one dict per pass: ``empty`` = the centres the pass gave no pixel, ``empty_ids`` = which, ``tied`` =
    the pixels whose least distance two or more distinct centres attain, ``dmax`` / ``smax`` = the largest distance / spatial term of
    a pixel and a candidate. The labels and centres do not depend on it."""
    x = np.asarray(x).astype(np.int64)
    d, h, w = x.shape
    if not (isinstance(lam, (int, np.integer)) and 1 <= lam <= LAMBDA_MAX):
        raise ValueError("lambda must be an integer in 1..65535")
    if n_iter < 1:
        raise ValueError("n_iter must be >= 1")
    if d > D_MAX:
        raise ValueError("D must be at most 207")
    if not (1 <= h <= SIDE_MAX and 1 <= w <= SIDE_MAX):
        raise ValueError("H, W must be in 1..4096")
    if not (1 <= ny <= h and 1 <= nx <= w and ny * nx <= K_MAX):
        raise ValueError("the grid needs 1 <= ny <= H, 1 <= nx <= W, ny * nx <= 4096")
    cy, cx = init_positions(h, w, ny, nx)
    cent = x[:, cy, cx].T.copy()
    cand = candidates(h, w, ny, nx)
    for t in range(n_iter):
        info = None if trace is None else {}
        lab = assign(x, cent, cy, cx, ny, nx, int(lam), cand, info)
        if trace is not None:
            none = np.flatnonzero(np.bincount(lab.ravel(), minlength=ny * nx) == 0)
            trace.append(dict(info, empty=len(none), empty_ids=none.tolist()))
        if t < n_iter - 1:
            cent, cy, cx = update(x, lab, cent, cy, cx)
    lab = lab.astype(np.int32)
    if return_centres:
        return lab, np.concatenate([cent, cy[:, None], cx[:, None]], axis=1)
    return lab


def superpixels(x, n, lam=576, n_iter=10, return_centres=False):
    """``superpixels_on_grid`` on the grid of (H, W, n)."""
    x = np.asarray(x)
    _, ny, nx = grid(x.shape[1], x.shape[2], n)
    return superpixels_on_grid(x, ny, nx, lam, n_iter, return_centres)


def segment(img, n, lam=576, n_iter=10, w=0.0, g=0, mu=0, n_scales=4, n_orient=6, smoothing=0.0, return_centres=False, **bank_kw):
    """(H, W, 3) uint8 image -> §13 labels on the features of ``position_ref.features`` (the package's features, restated)."""
    x = pr.features(np.asarray(img), w, g, mu, n_scales, n_orient, smoothing, **bank_kw)
    return superpixels(x, n, lam, n_iter, return_centres)


def segment_batch(imgs, n, **kw):
    return np.stack([segment(im, n, **kw) for im in imgs])
