"""Legal, artificial "hot" banks and images that drive the uint16 features over their whole range (SPEC.md §3: up to
46339), for the tests only. The default banks cannot pass about 12 000 on any image; these box-shaped taps sit at the bounds
gcs_bank_pack accepts (sum|tapq_re|, sum|tapq_im| <= 32 896, imaginary taps summing to zero, |tap| <= 32 639) and keep
|a_re|, |a_im| <= 32767 on every image, so every value is inside the domain SPEC.md and include/gcs.h define.

For filter f = s * n_orient + o: theta = o pi / n_orient, proj = dx cos(theta) + dy sin(theta) over the ksize x ksize frame,
restricted to |dx|, |dy| <= rad (rad = r on even scales, r - min(2, r - 1) on odd ones, r = (ksize - 1) / 2); pos = proj > 0.5,
neg = proj < -0.5 (the same count n). tapq_im = +vi on pos and -vi on neg with vi = 16447 // n; tapq_re = +vr on pos with
vr = cap // n, cap = 32 896 for shift 8 (the short epilogue) and 16 448 for shift 7 (the general epilogue). (16447, not 16448:
`>> shift` is a floor, so an imaginary part of -255 * 16448 would come out as -32768 at shift 7 where n divides 16448; the real
parts are never negative here. |a_re|, |a_im| <= 32767 then holds on every image.)

odd="turned" (hot_taps, hot_bank) is the same recipe with another way of telling the two scales of a level apart: rad = r on EVERY
scale, and the odd scales are turned by half a step, theta = (o + 1/2) pi / n_orient. Every filter then has taps in the first and
the last row and column of the ksize x ksize frame (tapq_im in all of them), so that no K-step of the bank kernel multiplies
zeros on any filter; with the default, odd="inset", the outer two rows and columns of the odd scales are empty."""
import dataclasses
import math

import numpy as np

G_MAX = 46339                      # floor(sqrt(2 * 32767^2)): the largest feature SPEC.md §3 admits
IMAGE_KINDS = ("stripes0", "black_region", "stripes45", "white", "stripes90", "smooth", "stripes135", "noise")
STRIPE_KINDS = tuple(i for i, kind in enumerate(IMAGE_KINDS) if kind.startswith("stripes"))
BLACK_REGION = IMAGE_KINDS.index("black_region")


def hot_taps(n_scales, n_orient, ksize, shift, odd="inset"):
    """int16 [F, 2, ksize, ksize] taps of the recipe above (shift 7 or 8)."""
    if shift not in (7, 8):
        raise ValueError("the recipe is stated for shift 7 and 8")
    if odd not in ("inset", "turned"):
        raise ValueError("odd scales are 'inset' or 'turned'")
    cap = 32896 if shift == 8 else 16448
    r = (ksize - 1) // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    tapq = np.zeros((n_scales * n_orient, 2, ksize, ksize), np.int64)
    for s in range(n_scales):
        rad = r if s % 2 == 0 or odd == "turned" else r - min(2, r - 1)
        inside = (np.abs(dx) <= rad) & (np.abs(dy) <= rad)
        for o in range(n_orient):
            theta = (o + (0.5 if odd == "turned" and s % 2 else 0.0)) * math.pi / n_orient
            proj = dx * math.cos(theta) + dy * math.sin(theta)
            pos, neg = inside & (proj > 0.5), inside & (proj < -0.5)
            n = int(pos.sum())
            assert n > 0 and n == int(neg.sum())
            f = s * n_orient + o
            tapq[f, 1][pos] = 16447 // n
            tapq[f, 1][neg] = -(16447 // n)
            tapq[f, 0][pos] = cap // n
    assert np.abs(tapq).max() <= 32639
    return tapq.astype(np.int16)


def hot_bank(n_scales, n_orient, ksize, shift, odd="inset"):
    """A GaborBank of the package with the hot taps in place of the Gabor ones: the shape fields are those of make_bank."""
    from gabor_color_image_segmentation_amd.bank import make_bank
    return dataclasses.replace(make_bank(n_scales, n_orient, ksize), tapq=hot_taps(n_scales, n_orient, ksize, shift, odd),
                               shift=shift, exponent=shift + 7)


def _stripes(h, w, angle, phase, period=18):
    y, x = np.mgrid[0:h, 0:w]
    t = x * math.cos(angle) + y * math.sin(angle) + phase
    return np.where(np.mod(t, period) < period / 2, 255, 0).astype(np.uint8)


def hot_images(b, h, w, seed):
    """(b, h, w, 3) uint8, image i of kind IMAGE_KINDS[i % 8]: square-wave stripes of period 18 at four angles, a white image,
    a smooth 128 + 127 sin cos surface, uniform noise - channels = the pattern, it flipped vertically, it flipped horizontally -
    and "black_region": stripes on the left, black IN ALL THREE CHANNELS from 3/8 of the width on, so that a split slab holds
    tiles with and tiles without values >= 4096 side by side."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((b, h, w, 3), np.uint8)
    for i in range(b):
        kind = IMAGE_KINDS[i % len(IMAGE_KINDS)]
        phase = 0.0 if i < len(IMAGE_KINDS) else float(rng.integers(1, 18))   # (the first eight: the measured recipe)
        if kind == "black_region":
            p = _stripes(h, w, 0.0, phase)
            p[:, (3 * w) // 8:] = 0
            out[i] = p[..., None]
            continue
        if kind.startswith("stripes"):
            p = _stripes(h, w, math.radians(int(kind[7:])), phase)
        elif kind == "white":
            p = np.full((h, w), 255, np.uint8)
        elif kind == "smooth":
            p = np.rint(128 + 127 * np.sin((x + phase) / 9.0) * np.cos(y / 7.0)).astype(np.uint8)
        else:
            p = rng.integers(0, 256, (h, w), dtype=np.uint8)
        out[i] = np.stack([p, p[::-1], p[:, ::-1]], -1)
    return out


def hot_segmenter(bank, smoothing=0.0, **kw):
    """Segmenter whose device bank is ``bank``: Segmenter reads only shape fields of ``self.bank``; taps and shift reach the
    device through HipOps."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.segmenter import HipOps
    seg = Segmenter(bank.n_scales, bank.n_orient, ksize=bank.ksize, ops=HipOps(bank, "cuda:0", smoothing),
                    smoothing=smoothing, **kw)
    seg.bank = bank
    return seg
