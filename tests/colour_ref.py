"""NumPy restatement of SPEC.md §11 (opponent-colour front end and low-pass bank slots), for the tests only. The package never
imports it, and it does not use the package's bank code: the Gabor taps come from the oracle's own bank (oracle/spec_oracle.py),
the envelopes are computed again here, and features and labels go through the oracles with that ``tapq``."""
import math

import numpy as np

from oracle import c_oracle as co
from oracle import spec_oracle as so


def opponent(img, g):
    """T_g of SPEC.md §11 on an (..., 3) uint8 array of RGB pixels -> (..., 3) uint8 (Y, Co, Cg). g = 0: the image itself."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    if g == 0:
        return img.copy()
    assert 1 <= g <= 16
    r, gr, b = (img[..., c].astype(np.int64) for c in range(3))
    y = (r + 2 * gr + b + 2) >> 2
    co_ = np.clip(128 + ((g * (r - b)) >> 1), 0, 255)                     # numpy's >> on int64 is arithmetic (floor)
    cg = np.clip(128 + ((g * (2 * gr - r - b)) >> 2), 0, 255)
    return np.stack([y, co_, cg], axis=-1).astype(np.uint8)


def opponent_pixel(r, g_, b, gain):
    """The same rule on three Python integers (// is floor division)."""
    clamp = lambda v: max(0, min(255, v))
    return (r + 2 * g_ + b + 2) // 4, clamp(128 + (gain * (r - b)) // 2), clamp(128 + (gain * (2 * g_ - r - b)) // 4)


def envelopes(n_scales=4, ksize=13, f_max=0.4, ratio=math.sqrt(2.0), bandwidth=1.0):
    """The normalised Gaussian envelope of every scale (SPEC.md §2), float64 [n_scales, ksize, ksize]."""
    r = (ksize - 1) // 2
    kappa = math.sqrt(math.log(2.0) / 2.0) / math.pi * (2.0 ** bandwidth + 1.0) / (2.0 ** bandwidth - 1.0)
    out = np.empty((n_scales, ksize, ksize), np.float64)
    for s in range(n_scales):
        sigma = kappa / (f_max / ratio ** s * 2.0 ** (s // 2))
        for iy in range(ksize):
            for ix in range(ksize):
                out[s, iy, ix] = math.exp(-((ix - r) ** 2 + (iy - r) ** 2) / (2.0 * sigma * sigma))
        out[s] = out[s] / out[s].sum()
    return out


def bank(n_scales=4, n_orient=6, w=0.0, ksize=13, f_max=0.4, ratio=math.sqrt(2.0), bandwidth=1.0):
    """SPEC.md §11 bank: (tapq int64 [n_scales * n_slots, 2, ks, ks], shift, n_slots). w = 0: the plain bank of §2."""
    tapq, shift = so.bank(n_scales, n_orient, ksize, f_max, ratio, bandwidth)
    if w == 0:
        return tapq, shift, n_orient
    e = shift + 7                                                          # E, from the Gabor taps alone
    env = envelopes(n_scales, ksize, f_max, ratio, bandwidth)
    slot = np.zeros((n_scales, 1, 2, ksize, ksize), np.int64)
    slot[:, 0, 0] = np.rint(w * env * 2.0 ** e).astype(np.int64)
    full = np.concatenate([tapq.reshape(n_scales, n_orient, 2, ksize, ksize), slot], axis=1)
    return full.reshape(n_scales * (n_orient + 1), 2, ksize, ksize), shift, n_orient + 1


def slot_bound(tapq, shift, n_slots):
    """Largest value a low-pass slot can take, per scale: the all-255 image's, (255 * sum of the slot's taps) >> shift (the taps
    are non-negative, so no image gives more)."""
    slots = tapq.reshape(-1, n_slots, *tapq.shape[1:])[:, n_slots - 1, 0]
    assert slots.min() >= 0
    return [int((255 * int(t.sum())) >> shift) for t in slots]


def features(img, w=0.0, g=0, n_scales=4, n_orient=6, oracle=co, **bank_kw):
    """Canonical features (D, H, W) uint16 of one (H, W, 3) uint8 image under SPEC.md §11 (C oracle by default)."""
    tapq, shift, n_slots = bank(n_scales, n_orient, w, **bank_kw)
    return oracle.gabor_features(opponent(img, g), tapq, shift, n_slots)


def segment_batch(imgs, w=0.0, g=0, k=8, n_iter=10, mode="per_image", smoothing=0.0, n_scales=4, n_orient=6, **bank_kw):
    """Labels (B, H, W) int32 of SPEC.md §4 k-means on the features of §11 (smoothed as §10 says when ``smoothing`` > 0)."""
    imgs = np.asarray(imgs)
    b, h, wd = imgs.shape[:3]
    x = [features(im, w, g, n_scales, n_orient, **bank_kw) for im in imgs]
    if smoothing > 0:
        import smooth_ref as sr
        n_slots = n_orient + (1 if w else 0)
        x = [sr.smooth_features(f, smoothing, n_scales, n_slots, bank_kw.get("f_max", 0.4), bank_kw.get("ratio", math.sqrt(2.0)))
             for f in x]
    x = np.stack(x).reshape(b, -1, h * wd)
    if mode == "global":
        return co.kmeans(x, k, n_iter)[0].reshape(b, h, wd)
    return np.stack([co.kmeans(x[i:i + 1], k, n_iter)[0].reshape(h, wd) for i in range(b)])


def segment(img, w=0.0, g=0, **kw):
    return segment_batch(np.asarray(img)[None], w, g, **kw)[0]
