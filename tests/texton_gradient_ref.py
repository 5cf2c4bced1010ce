"""NumPy restatement of SPEC.md §24 (texton gradient of a label map, joined with an edge map), for the tests and the CPU quality
tool only. The package never imports it and it uses none of the package's code. The border is an explicit mirror-index gather
(``mirror``), so nothing rests on a library's border modes; the counts are differences of per-row running sums over the runs of set
bits of every mask row, so any mask table is taken, not only half discs. Integers throughout; ``math.isqrt`` takes the root."""
import math

import numpy as np


def direction(i, n):
    """(a_i, b_i): the normal of direction i of n, scaled by 1024 and rounded."""
    return (math.floor(1024 * math.cos(math.pi * i / n) + 0.5), math.floor(1024 * math.sin(math.pi * i / n) + 0.5))


def masks(r, n):
    """The half-disc table: uint32 [n][2][2r+1], side 0 = A (s > 0), 1 = B (s < 0); row dy + r, bit dx + r."""
    assert 1 <= r <= 15 and 1 <= n <= 16
    out = np.zeros((n, 2, 2 * r + 1), np.uint32)
    for i in range(n):
        a, b = direction(i, n)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy * dy + dx * dx > r * r:
                    continue
                s = dx * a + dy * b
                if s > 0:
                    out[i, 0, dy + r] |= np.uint32(1 << (dx + r))
                elif s < 0:
                    out[i, 1, dy + r] |= np.uint32(1 << (dx + r))
    return out


def mirror(t, size):
    """mir(t, N) for an integer array t: reflection that does not repeat the edge pixel, any t."""
    t = np.asarray(t, np.int64)
    if size == 1:
        return np.zeros_like(t)
    p = 2 * (size - 1)
    u = np.mod(t, p)                                          # non-negative
    return np.where(u < size, u, p - u)


def _runs(word, width):
    """The maximal runs [lo, hi) of set bits among bits 0 .. width-1 of a mask row."""
    out, lo = [], None
    for bit in range(width + 1):
        on = bit < width and (int(word) >> bit) & 1
        if on and lo is None:
            lo = bit
        elif not on and lo is not None:
            out.append((lo, bit))
            lo = None
    return out


def chi_squares(lab, K, r, n, table=None):
    """chi_i of SPEC.md §24 for every direction: int64 [n][H][W]. ``table``: any uint32 [n][2][2r+1] in place of ``masks(r, n)``
    (bits above 2r are ignored)."""
    lab = np.asarray(lab)
    assert lab.ndim == 2 and 1 <= K <= 64
    table = masks(r, n) if table is None else np.asarray(table)
    assert table.shape == (n, 2, 2 * r + 1)
    h, w = lab.shape
    width = 2 * r + 1
    pad = lab[mirror(np.arange(-r, h + r), h)][:, mirror(np.arange(-r, w + r), w)]       # pad[y + dy + r][x + dx + r]
    runs = [[[_runs(table[i, side, m], width) for m in range(width)] for side in range(2)] for i in range(n)]
    chi = np.zeros((n, h, w), np.int64)
    for j in range(K):
        plane = pad == j
        if not plane.any():
            continue                                          # g = h = 0 everywhere: the bin adds nothing
        csum = np.zeros((h + 2 * r, w + 2 * r + 1), np.int64)
        csum[:, 1:] = np.cumsum(plane, axis=1)
        for i in range(n):
            cnt = np.zeros((2, h, w), np.int64)
            for side in range(2):
                for m in range(width):
                    for lo, hi in runs[i][side][m]:
                        cnt[side] += csum[m:m + h, hi:hi + w] - csum[m:m + h, lo:lo + w]
            tot = cnt[0] + cnt[1]
            num = 64 * (cnt[0] - cnt[1]) ** 2
            chi[i] += np.where(tot > 0, num // np.maximum(tot, 1), 0)                      # the floor is per bin
    return chi


def texton_gradient(lab, K, r, n, masks=None):
    """(TG int32 (H,W), dir uint8 (H,W)): the maximum over the directions and the lowest direction that attains it."""
    chi = chi_squares(lab, K, r, n, masks)
    return chi.max(axis=0).astype(np.int32), chi.argmax(axis=0).astype(np.uint8)           # argmax: the first maximum


def joined(tg, g):
    """E = floor(sqrt(TG * G)) for G >= 0: int32, Python integers under the root."""
    prod = np.asarray(tg).astype(np.int64) * np.asarray(g).astype(np.int64)
    vals, inv = np.unique(prod, return_inverse=True)
    return np.array([math.isqrt(int(v)) for v in vals], np.int32)[inv.ravel()].reshape(prod.shape)


def normalised(e):
    """``segment_texton_edges``' map: E / max(E) as float32, zeros for a zero map."""
    e = np.asarray(e)
    top = int(e.max())
    return np.zeros(e.shape, np.float32) if top == 0 else (e.astype(np.float32) / np.float32(top)).astype(np.float32)
