"""NumPy restatement of SPEC.md §25 (the boundary map of a label map and three quantised image channels, joined per direction),
for the tests and the CPU quality tool only. The package never imports it and it uses none of the package's code. Everything
that §25 shares with §24 - the offsets, the halves, the mask table, the mirror border, the per-bin floor, the exact root - is
tests/texton_gradient_ref.py's, imported and unchanged; what is added here is the quantiser, the weights, the sum per direction
and the maximum with its direction. Integers throughout."""
import numpy as np

from texton_gradient_ref import chi_squares, joined, masks  # noqa: F401  (``joined`` and ``masks``: for the callers)

BINS = (2, 4, 8, 16, 32, 64)


def shift_of(bins):
    """shift = 8 - log2(bins) for the six bin counts of §25."""
    assert bins in BINS, bins
    return 8 - (int(bins).bit_length() - 1)


def quantise(channel, bins):
    """bin = v >> shift of a uint8 plane, as int32."""
    channel = np.asarray(channel)
    assert channel.dtype == np.uint8
    return (channel >> shift_of(bins)).astype(np.int32)


def _chi(plane, K, r, n, table, cache):
    """``chi_squares`` of one plane of bins, remembered in the dict ``cache`` (None: not remembered) so that callers that walk
    several weight sets over the same planes pay for a plane once. The arrays handed out are shared: nobody writes to them."""
    if cache is None:
        return chi_squares(plane, K, r, n, table)
    plane = np.ascontiguousarray(plane, np.int32)
    key = (plane.shape, plane.tobytes(), K, r, n, None if table is None else np.ascontiguousarray(table).tobytes())
    if key not in cache:
        cache[key] = chi_squares(plane, K, r, n, table)
    return cache[key]


def cue_chi_squares(lab, img, K, bins, weights, r, n, table=None, cache=None):
    """chi_{c,i} of every cue with a non-zero weight: {c: int64 [n][H][W]}. A cue of weight 0 is not read (``lab`` / ``img`` may
    be None then)."""
    w = [int(v) for v in weights]
    assert len(w) == 4 and all(0 <= v <= 16 for v in w) and any(w)
    out = {}
    if w[0]:
        out[0] = _chi(np.asarray(lab), K, r, n, table, cache)
    for c in (1, 2, 3):
        if w[c]:
            out[c] = _chi(quantise(np.asarray(img)[..., c - 1], bins), bins, r, n, table, cache)
    return out


def direction_sums(lab, img, K, bins, weights, r, n, table=None, cache=None):
    """P_i = sum over the cues of w_c chi_{c,i}: int64 [n][H][W]."""
    chi = cue_chi_squares(lab, img, K, bins, weights, r, n, table, cache)
    return sum(int(weights[c]) * x for c, x in chi.items())


def cue_gradient(lab, img, K, bins, weights, r, n, table=None, cache=None):
    """(PB int32 (H,W), dir uint8 (H,W)): the maximum of P_i over the directions and the lowest direction that attains it."""
    p = direction_sums(lab, img, K, bins, weights, r, n, table, cache)
    return p.max(axis=0).astype(np.int32), p.argmax(axis=0).astype(np.uint8)                # argmax: the first maximum


def summed_maxima(lab, img, K, bins, weights, r, n, table=None, cache=None):
    """The ablation of the per-direction join: sum over the cues of w_c max_i chi_{c,i}, int32 (H,W). Not what §25 defines."""
    chi = cue_chi_squares(lab, img, K, bins, weights, r, n, table, cache)
    return sum(int(weights[c]) * x.max(axis=0) for c, x in chi.items()).astype(np.int32)


def cue_edges(lab, img, grad, K, bins, weights, r, n, table=None, cache=None):
    """E' = floor(sqrt(PB * max(G, 0))), or PB for ``grad`` None."""
    pb = cue_gradient(lab, img, K, bins, weights, r, n, table, cache)[0]
    return pb if grad is None else joined(pb, np.maximum(np.asarray(grad), 0))
