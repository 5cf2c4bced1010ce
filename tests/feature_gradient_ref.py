"""NumPy restatement of SPEC.md §22 (texture-gradient edge map), for the tests and the CPU quality tool only. The package never
imports it and it uses none of the package's code. Input: canonical features (D, H, W) as §3 lays them out (logical feature
d = c * F + f, f = s * slots + slot, scale s on pyramid level s // 2, a level-L plane replicated over 2^L x 2^L blocks), so level L of
plane d is ``x[d][::2^L, ::2^L]``. Python integers take the square root (``math.isqrt``): no float is involved."""
import math

import numpy as np


def level_of_plane(d, n_scales, slots):
    """Pyramid level of logical feature d of a bank of ``n_scales`` scales with ``slots`` slots each."""
    return ((d % (n_scales * slots)) // slots) // 2


def level_terms(x, n_scales, slots):
    """Canonical features (D, H, W) -> per level L a pair (DX_L, DY_L) of int64 arrays at the level's own resolution."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        x = x.view(np.uint16)
    x = x.astype(np.int64)
    d_n, h, w = x.shape
    assert d_n == 3 * n_scales * slots
    out = []
    for lv in range((n_scales + 1) // 2):
        planes = [d for d in range(d_n) if level_of_plane(d, n_scales, slots) == lv]
        g = x[planes][:, ::1 << lv, ::1 << lv]
        hl, wl = g.shape[1:]
        assert (hl, wl) == (-(-h // (1 << lv)), -(-w // (1 << lv)))
        xp, xm = np.minimum(np.arange(wl) + 1, wl - 1), np.maximum(np.arange(wl) - 1, 0)
        yp, ym = np.minimum(np.arange(hl) + 1, hl - 1), np.maximum(np.arange(hl) - 1, 0)
        out.append((((g[:, :, xp] - g[:, :, xm]) ** 2).sum(0), ((g[:, yp, :] - g[:, ym, :]) ** 2).sum(0)))
    return out


def energy(x, n_scales, slots):
    """E of SPEC.md §22: (H, W) int64."""
    _, h, w = np.asarray(x).shape
    y, xx = np.mgrid[0:h, 0:w]
    e = np.zeros((h, w), np.int64)
    for lv, (dx, dy) in enumerate(level_terms(x, n_scales, slots)):
        e += (dx >> (2 * lv))[y >> lv, xx >> lv] + (dy >> (2 * lv))[y >> lv, xx >> lv]
    return e


def gradient(x, n_scales, slots):
    """G = floor(sqrt(E)) of SPEC.md §22: (H, W) int32."""
    e = energy(x, n_scales, slots)
    vals, inv = np.unique(e, return_inverse=True)
    return np.array([math.isqrt(int(v)) for v in vals], np.int32)[inv.ravel()].reshape(e.shape)


def normalised(g):
    """``segment_edges``' map: G / max(G) as float32, zeros for a zero map."""
    g = np.asarray(g)
    top = int(g.max())
    return np.zeros(g.shape, np.float32) if top == 0 else (g.astype(np.float32) / np.float32(top)).astype(np.float32)
