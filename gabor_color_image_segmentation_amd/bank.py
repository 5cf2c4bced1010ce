"""Gabor filter bank in fixed point on an octave pyramid (SPEC.md §2).

The reference ships no Gabor code; this is the build-authored
bank that fills the segmenter slot at /root/reference/BSD_metrics/script.py:30.
Host-side only (numpy, float64 -> int16); the device receives the packed
int8 MFMA digits produced by ``gcs_bank_pack`` (include/gcs.h).
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

KSIZE_MAX = 15          # the HIP kernel's tap frame is 15 rows x 16 columns
N_SCALES_MAX = 8        # octave pyramid of at most 4 levels (scales 2L, 2L+1 run on level L)
TAPQ_MAX = 32639        # 127*256 + 127: largest value two signed byte digits hold
FEATURE_Q = 7           # features are Q7 grey levels
TAP_Q = 15              # taps are Q15 (less only for kernels so peaked that a tap would not fit two byte digits)


@dataclasses.dataclass(frozen=True)
class GaborBank:
    """Quantised bank. ``tapq`` is ``[F, 2, ksize, ksize]`` int16 (re, im)."""
    n_scales: int
    n_orient: int
    ksize: int
    f_max: float
    ratio: float
    bandwidth: float
    exponent: int            # E: tapq = rint(tap * 2**E)
    shift: int               # E - FEATURE_Q
    tapq: np.ndarray
    color_weight: float = 0.0     # w of SPEC.md §11 (0: a plain Gabor bank)
    n_gabor_orient: int = 0       # Gabor orientations per scale; 0 = n_orient (make_bank: n_orient minus the colour and the coordinate slot)
    position_weight: int = 0      # mu of SPEC.md §12 (0: no coordinate slot; else the LAST slot of every scale, zero taps)

    def __post_init__(self):
        if self.n_gabor_orient == 0:
            object.__setattr__(self, "n_gabor_orient", self.n_orient)

    @property
    def n_filters(self) -> int:
        return self.n_scales * self.n_orient

    @property
    def n_features(self) -> int:
        return 3 * self.n_filters

    @property
    def n_levels(self) -> int:
        """Pyramid levels the bank spans (SPEC.md §2): scales 2L and 2L+1 run on level L."""
        return (self.n_scales + 1) // 2


def gabor_taps(n_scales=4, n_orient=6, ksize=13, f_max=0.4, ratio=math.sqrt(2.0),
               bandwidth=1.0) -> np.ndarray:
    """Float64 taps ``[F, 2, ksize, ksize]`` (SPEC.md §2, before quantisation)."""
    return _taps_and_envelopes(n_scales, n_orient, ksize, f_max, ratio, bandwidth)[0]


def _taps_and_envelopes(n_scales, n_orient, ksize, f_max, ratio, bandwidth):
    """``gabor_taps`` and the normalised envelope of every scale, float64 ``[n_scales, ksize, ksize]``."""
    if ksize % 2 != 1 or not (1 <= ksize <= KSIZE_MAX):
        raise ValueError(f"ksize must be odd and <= {KSIZE_MAX}, got {ksize}")
    if n_scales < 1 or n_orient < 1:
        raise ValueError("n_scales and n_orient must be >= 1")
    if n_scales > N_SCALES_MAX:
        raise ValueError(f"n_scales must be <= {N_SCALES_MAX} (4 pyramid levels)")
    r = (ksize - 1) // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1].astype(np.float64)
    kappa = math.sqrt(math.log(2.0) / 2.0) / math.pi * \
        (2.0 ** bandwidth + 1.0) / (2.0 ** bandwidth - 1.0)
    taps = np.empty((n_scales * n_orient, 2, ksize, ksize), np.float64)
    envs = np.empty((n_scales, ksize, ksize), np.float64)
    for s in range(n_scales):
        freq = f_max / ratio ** s * 2.0 ** (s // 2)      # f_base: cycles per pixel of pyramid level s // 2
        sigma = kappa / freq
        env = np.exp(-(dx * dx + dy * dy) / (2.0 * sigma * sigma))
        env /= env.sum()
        envs[s] = env
        for o in range(n_orient):
            theta = o * math.pi / n_orient
            phase = 2.0 * math.pi * freq * (dx * math.cos(theta) + dy * math.sin(theta))
            taps[s * n_orient + o, 0] = env * np.cos(phase)
            taps[s * n_orient + o, 1] = env * np.sin(phase)
    return taps, envs


def check_color_weight(color_weight) -> float:
    """SPEC.md §11 parameter: 0 (off) or a finite 0 < w <= 1."""
    try:
        w = float(color_weight)
    except (TypeError, ValueError):
        raise ValueError(f"color_weight must be a number, got {color_weight!r}") from None
    if not (math.isfinite(w) and 0.0 <= w <= 1.0):
        raise ValueError(f"color_weight must be 0 (off) or in (0, 1], got {color_weight!r}")
    return w


POSITION_WEIGHT_MAX = 255
FEATURE_MAX = 46340     # SPEC.md §3 value range: the squared distance of two features stays below 2^31


def check_position_weight(position_weight) -> int:
    """SPEC.md §12 parameter: the integer 0 (off) or 1..255. Bools and floats (6.0 included) are refused: mu is an exact integer."""
    import numbers
    if isinstance(position_weight, bool) or not isinstance(position_weight, numbers.Integral) \
            or not (0 <= int(position_weight) <= POSITION_WEIGHT_MAX):
        raise ValueError(f"position_weight must be the integer 0 (off) or 1..{POSITION_WEIGHT_MAX}, got {position_weight!r}")
    return int(position_weight)


def check_position_range(position_weight, height, width) -> None:
    """SPEC.md §12 domain: mu * (max(height, width) - 1) <= 46 340, with the FULL image's row count for a row strip."""
    if position_weight > 0 and position_weight * (max(int(height), int(width)) - 1) > FEATURE_MAX:
        raise ValueError(f"position_weight = {position_weight} on a {height} x {width} image exceeds the feature range: "
                         f"mu * (max(height, width) - 1) must be <= {FEATURE_MAX} (SPEC.md §12)")


def make_bank(n_scales=4, n_orient=6, ksize=13, f_max=0.4, ratio=math.sqrt(2.0),
              bandwidth=1.0, color_weight=0.0, position_weight=0) -> GaborBank:
    """Quantise the bank to Q15 taps (SPEC.md §2): shift = 8, i.e. the response's Q7 value is bytes 1..2 of v.

    ``color_weight`` = w > 0 (SPEC.md §11): every scale gets one more filter behind its ``n_orient`` Gabor filters, the scale's
    envelope times w with zero imaginary taps. The bank returned then has ``n_orient + 1`` slots per scale and says so in its
    ``n_orient`` field - that is the shape the C ABI, the slab layout and every kernel see -, with the Gabor orientation count
    in ``n_gabor_orient``. The exponent comes from the Gabor taps alone: the Gabor slots equal the plain bank's bit for bit.

    ``position_weight`` = mu > 0 (SPEC.md §12): one more slot per scale, behind the Gabor filters and the colour slot, with all
    taps zero - the planes the coordinate kernel fills (``HipOps.position_features``). Counted in ``n_orient`` like the colour
    slot; every other filter equals the bank's without it bit for bit."""
    w = check_color_weight(color_weight)
    mu = check_position_weight(position_weight)
    taps, envs = _taps_and_envelopes(n_scales, n_orient, ksize, f_max, ratio, bandwidth)
    exponent = min(TAP_Q, int(math.floor(math.log2(TAPQ_MAX / np.abs(taps).max()))))
    tapq = np.rint(taps * 2.0 ** exponent).astype(np.int64)
    n_slots = n_orient
    if w > 0.0:
        n_slots = n_orient + 1
        full = np.zeros((n_scales, n_slots, 2, ksize, ksize), np.int64)
        full[:, :n_orient] = tapq.reshape(n_scales, n_orient, 2, ksize, ksize)
        full[:, n_orient, 0] = np.rint(w * envs * 2.0 ** exponent).astype(np.int64)
        tapq = full.reshape(n_scales * n_slots, 2, ksize, ksize)
    if mu > 0:
        full = np.zeros((n_scales, n_slots + 1, 2, ksize, ksize), np.int64)
        full[:, :n_slots] = tapq.reshape(n_scales, n_slots, 2, ksize, ksize)
        n_slots += 1
        tapq = full.reshape(n_scales * n_slots, 2, ksize, ksize)
    if np.abs(tapq).max() > TAPQ_MAX:
        raise AssertionError("tap quantisation overflowed the two-digit range")
    if exponent < FEATURE_Q:
        raise ValueError("bank too peaked for Q7 features")
    if np.any(tapq[:, 1].sum(axis=(1, 2)) != 0):
        raise AssertionError("imaginary taps must sum to zero (odd symmetry)")
    return GaborBank(n_scales, n_slots, ksize, float(f_max), float(ratio),
                     float(bandwidth), exponent, exponent - FEATURE_Q,
                     tapq.astype(np.int16), w, n_orient, mu)


def split_digits(tapq: np.ndarray):
    """tapq = 256*hi + lo with both digits in [-128, 127] (SPEC.md §2)."""
    q = tapq.astype(np.int32)
    lo = ((q + 128) & 255) - 128
    hi = (q - lo) >> 8
    if hi.min() < -128 or hi.max() > 127:
        raise AssertionError("high digit out of int8 range")
    return lo.astype(np.int8), hi.astype(np.int8)


SMOOTH_RADIUS_MAX = 24  # largest smoothing radius (SPEC.md §10): the HIP kernel's apron
SMOOTH_TAPS = 2 * SMOOTH_RADIUS_MAX + 1
SMOOTH_ONE = 4096       # the taps of a scale sum to this


def smoothing_taps(K, n_scales=4, n_orient=6, f_max=0.4, ratio=math.sqrt(2.0)):
    """SPEC.md §10 taps of smoothing ``K`` (> 0): ``(taps, radius)``, int32 ``[n_scales][49]`` centred (tap i of scale s at
    ``[s][24 + i]``) and int32 ``[n_scales]``. sigma_s = K / (2 f_base(s)) level pixels, R_s = ceil(3 sigma_s) in 1..24, integer
    taps that sum to 4096 exactly. Raises ValueError for a K that is not finite and positive or gives a radius outside 1..24."""
    K = float(K)
    if not math.isfinite(K) or K <= 0.0:
        raise ValueError(f"smoothing K must be finite and > 0 to have taps, got {K}")
    if not (1 <= n_scales <= N_SCALES_MAX) or n_orient < 1:
        raise ValueError("bad bank shape")
    taps = np.zeros((n_scales, SMOOTH_TAPS), np.int32)
    radius = np.zeros(n_scales, np.int32)
    for s in range(n_scales):
        f_base = f_max / ratio ** s * 2.0 ** (s // 2)
        sigma = K / (2.0 * f_base)
        r = math.ceil(3.0 * sigma)
        if not (1 <= r <= SMOOTH_RADIUS_MAX):
            raise ValueError(f"smoothing K = {K} gives radius {r} on scale {s}; SPEC.md §10 allows 1..{SMOOTH_RADIUS_MAX}")
        i = np.arange(-r, r + 1, dtype=np.float64)
        g = np.exp(-i * i / (2.0 * sigma * sigma))
        w = np.rint(SMOOTH_ONE * g / g.sum()).astype(np.int64)
        w[r] = 0
        w[r] = SMOOTH_ONE - w.sum()
        taps[s, SMOOTH_RADIUS_MAX - r:SMOOTH_RADIUS_MAX + r + 1] = w
        radius[s] = r
    return taps, radius

