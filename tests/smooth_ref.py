"""NumPy / scipy restatement of SPEC.md §10 (smoothing of the feature levels), for the tests only. The package never imports it,
and it does not use the package's bank code: the taps are computed again here with math.exp."""
import math

import numpy as np
from scipy import ndimage as ndi

from oracle import c_oracle as co
from oracle import spec_oracle as so

R_MAX = 24


def taps(K, n_scales=4, f_max=0.4, ratio=math.sqrt(2.0)):
    """SPEC.md §10: per scale s, (R_s, int64 taps w_{-R..R}). ValueError for a radius outside 1..24."""
    out = []
    for s in range(n_scales):
        f_base = f_max / ratio ** s * 2.0 ** (s // 2)
        sigma = K / (2.0 * f_base)
        r = math.ceil(3.0 * sigma)
        if not 1 <= r <= R_MAX:
            raise ValueError(f"radius {r} on scale {s}")
        g = [math.exp(-i * i / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
        tot = sum(g)
        w = [round(4096.0 * gi / tot) for gi in g]
        w[r] = 4096 - (sum(w) - w[r])
        out.append((r, np.array(w, np.int64)))
    return out


def taps_array(K, n_scales=4, f_max=0.4, ratio=math.sqrt(2.0)):
    """The same taps in the ABI's layout: int32 [n_scales][49] centred, int32 [n_scales] radii."""
    t = np.zeros((n_scales, 2 * R_MAX + 1), np.int32)
    rad = np.zeros(n_scales, np.int32)
    for s, (r, w) in enumerate(taps(K, n_scales, f_max, ratio)):
        t[s, R_MAX - r:R_MAX + r + 1] = w
        rad[s] = r
    return t, rad


def smooth_plane(g, w):
    """One level plane (H_L, W_L) uint16 -> h: int64 separable sums with the reflect border, (acc + 2^23) >> 24."""
    acc = ndi.correlate1d(np.asarray(g).astype(np.int64), w, axis=0, mode="reflect")
    acc = ndi.correlate1d(acc, w, axis=1, mode="reflect")
    return ((acc + (1 << 23)) >> 24).astype(np.uint16)


def smooth_plane_direct(g, w):
    """The same sum with explicit reflected indices (SPEC.md §3 rule r(i)), for cross-checking ``smooth_plane``."""
    g = np.asarray(g).astype(np.int64)
    r = (len(w) - 1) // 2

    def refl(i, n):
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    hh, ww = g.shape
    pad = g[refl(np.arange(-r, hh + r), hh)][:, refl(np.arange(-r, ww + r), ww)]
    acc = np.zeros((hh, ww), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            acc += w[dy] * w[dx] * pad[dy:dy + hh, dx:dx + ww]
    return ((acc + (1 << 23)) >> 24).astype(np.uint16)


def smooth_features(feats, K, n_scales, n_orient, f_max=0.4, ratio=math.sqrt(2.0)):
    """Canonical features (D, H, W) uint16 (SPEC.md §3) -> the features of §10: level L of plane d is feats[d, ::2^L, ::2^L],
    smoothed with the taps of d's scale and replicated back up over 2^L x 2^L blocks. K = 0: unchanged."""
    feats = np.asarray(feats)
    if K == 0:
        return feats.copy()
    t = taps(K, n_scales, f_max, ratio)
    nf = n_scales * n_orient
    h, w = feats.shape[1:]
    out = np.empty_like(feats)
    for d in range(feats.shape[0]):
        s = (d % nf) // n_orient
        L = s // 2
        sm = smooth_plane(feats[d, ::1 << L, ::1 << L], t[s][1])
        out[d] = sm.repeat(1 << L, axis=0).repeat(1 << L, axis=1)[:h, :w]
    return out


def features(img, K, n_scales=4, n_orient=6, ksize=13, f_max=0.4, ratio=math.sqrt(2.0), bandwidth=1.0):
    """Smoothed canonical features (D, H, W) uint16 of one (H, W, 3) uint8 image, from the C oracle's Gabor stage."""
    tapq, shift = so.bank(n_scales, n_orient, ksize, f_max, ratio, bandwidth)
    return smooth_features(co.gabor_features(img, tapq, shift, n_orient), K, n_scales, n_orient, f_max, ratio)


def segment_batch(imgs, K, k=8, n_iter=10, mode="per_image", **bank_kw):
    """Labels (B, H, W) int32 of SPEC.md §4 k-means on the smoothed features (C oracle k-means)."""
    imgs = np.asarray(imgs)
    b, h, w = imgs.shape[:3]
    x = np.stack([features(im, K, **bank_kw) for im in imgs]).reshape(b, -1, h * w)
    if mode == "global":
        return co.kmeans(x, k, n_iter)[0].reshape(b, h, w)
    return np.stack([co.kmeans(x[i:i + 1], k, n_iter)[0].reshape(h, w) for i in range(b)])


def segment(img, K, **kw):
    return segment_batch(np.asarray(img)[None], K, **kw)[0]
