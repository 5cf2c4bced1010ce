"""NumPy restatement of SPEC.md §12 (position features: a coordinate slot per scale), for the tests only. The package never
imports it, and it does not use the package's bank code: the taps are those of ``colour_ref.bank`` (oracle Gabor taps, the
envelopes restated there) plus one zero slot per scale, the Gabor planes come from the C oracle with that ``tapq``, the slot's
planes are filled here as §12 defines them (level planes, then §3's block replication), and k-means runs through
``oracle.c_oracle.kmeans``."""
import math

import numpy as np

import colour_ref as cr
from oracle import c_oracle as co

VALUE_MAX = 46340


def n_slots(n_orient, w=0.0, mu=0):
    return n_orient + (1 if w > 0 else 0) + (1 if mu > 0 else 0)


def bank(n_scales=4, n_orient=6, w=0.0, mu=0, **bank_kw):
    """SPEC.md §12 bank: (tapq int64 [n_scales * n_slots, 2, ks, ks], shift, n_slots); the coordinate slot, all taps zero, is the
    last slot of every scale. mu = 0: the bank of §11 (w > 0) or §2."""
    tapq, shift, ns = cr.bank(n_scales, n_orient, w, **bank_kw)
    if mu == 0:
        return tapq, shift, ns
    ks = tapq.shape[-1]
    full = np.concatenate([tapq.reshape(n_scales, ns, 2, ks, ks), np.zeros((n_scales, 1, 2, ks, ks), np.int64)], axis=1)
    return full.reshape(n_scales * (ns + 1), 2, ks, ks), shift, ns + 1


def in_domain(mu, height, width):
    return mu * (max(height, width) - 1) <= VALUE_MAX


def slot_planes(h, w, s, mu, y0=0):
    """The two non-zero planes of scale s's coordinate slot as (h, w) int64 arrays at FULL resolution: the level planes of level
    L = s // 2, channel 0 = mu (y0 + (yl << L)), channel 1 = mu (xl << L), replicated over 2^L x 2^L blocks (SPEC.md §3)."""
    lv = s // 2
    hl, wl = -(-h // (1 << lv)), -(-w // (1 << lv))
    yl, xl = np.mgrid[0:hl, 0:wl].astype(np.int64)
    level = [mu * (y0 + (yl << lv)), mu * (xl << lv)]
    y, x = np.mgrid[0:h, 0:w]
    return [p[y >> lv, x >> lv] for p in level]


def fill_slot(feats, n_scales, slots, mu, y0=0):
    """Write the coordinate slot (slot ``slots - 1`` of every scale) of canonical features (D, H, W), in place; channel 2 := 0."""
    d, h, w = feats.shape
    f_n = n_scales * slots
    assert d == 3 * f_n
    for s in range(n_scales):
        f = s * slots + slots - 1
        rows, cols = slot_planes(h, w, s, mu, y0)
        assert rows.max() <= VALUE_MAX and cols.max() <= VALUE_MAX
        feats[0 * f_n + f] = rows
        feats[1 * f_n + f] = cols
        feats[2 * f_n + f] = 0
    return feats


def features(img, w=0.0, g=0, mu=0, n_scales=4, n_orient=6, smoothing=0.0, y0=0, **bank_kw):
    """Canonical features (D, H, W) uint16 of one (H, W, 3) uint8 image under SPEC.md §11 + §10 + §12: the Gabor and colour planes of
    the bank with the zero slot (C oracle), smoothed when ``smoothing`` > 0, then the coordinate planes written over the slot."""
    tapq, shift, slots = bank(n_scales, n_orient, w, mu, **bank_kw)
    f = co.gabor_features(cr.opponent(img, g), tapq, shift, slots)
    if mu > 0:
        f_n = n_scales * slots
        assert not f.reshape(3, n_scales, slots, -1)[:, :, slots - 1].any()       # zero taps: the Gabor stage leaves zeros
    if smoothing > 0:
        import smooth_ref as sr
        f = sr.smooth_features(f, smoothing, n_scales, slots, bank_kw.get("f_max", 0.4), bank_kw.get("ratio", math.sqrt(2.0)))
    if mu > 0:
        f = fill_slot(np.array(f, dtype=np.uint16), n_scales, slots, mu, y0)
    return f


def segment_batch(imgs, w=0.0, g=0, mu=0, k=8, n_iter=10, mode="per_image", smoothing=0.0, n_scales=4, n_orient=6, **bank_kw):
    """Labels (B, H, W) int32 of SPEC.md §4 k-means on the features of §12."""
    imgs = np.asarray(imgs)
    b, h, wd = imgs.shape[:3]
    x = np.stack([features(im, w, g, mu, n_scales, n_orient, smoothing, **bank_kw) for im in imgs]).reshape(b, -1, h * wd)
    if mode == "global":
        return co.kmeans(x, k, n_iter)[0].reshape(b, h, wd)
    return np.stack([co.kmeans(x[i:i + 1], k, n_iter)[0].reshape(h, wd) for i in range(b)])


def segment(img, w=0.0, g=0, mu=0, **kw):
    return segment_batch(np.asarray(img)[None], w, g, mu, **kw)[0]
