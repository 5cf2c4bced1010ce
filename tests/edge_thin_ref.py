"""NumPy restatement of SPEC.md §26 (thin boundary maps), written from the section's text: the step table from §24's normals,
the clamped neighbours and the two comparisons in Python integers. Slow and plain; never used by the product."""
import math

import numpy as np


def normal(i, n):
    """SPEC.md §24: (a_i, b_i), a along x and b along y."""
    return math.floor(1024 * math.cos(math.pi * i / n) + 0.5), math.floor(1024 * math.sin(math.pi * i / n) + 0.5)


def _sign(v):
    return (v > 0) - (v < 0)


def steps(n):
    """The table of §26: int32 [n][8] = dy1, dx1, dy2, dx2, w1, w2, 0, 0."""
    assert 1 <= n <= 16
    table = np.zeros((n, 8), np.int32)
    for i in range(n):
        a, b = normal(i, n)
        A, B, sa, sb = abs(a), abs(b), _sign(a), _sign(b)
        if A >= B:
            q1, w2, w1 = (0, sa), B, A - B
        else:
            q1, w2, w1 = (sb, 0), A, B - A
        table[i] = [q1[0], q1[1], sb, sa, w1, w2, 0, 0]
    return table


def thin(edges, dirs, n, table=None):
    """T of §26 for one (H,W) map: ``edges`` any integers, ``dirs`` uint8, ``table`` any (n, 8) step table (None: ``steps(n)``).
    Offsets outside -1 .. 1 are clamped, as the section says the kernel does."""
    edges, dirs = np.asarray(edges), np.asarray(dirs)
    table = steps(n) if table is None else np.asarray(table)
    h, w = edges.shape
    v = np.maximum(edges.astype(np.int64), 0)
    c = lambda y, x: int(v[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])
    unit = lambda t: min(max(int(t), -1), 1)
    out = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            i = int(dirs[y, x])
            here = int(v[y, x])
            if i >= n or here <= 0:
                continue
            dy1, dx1, dy2, dx2 = (unit(t) for t in table[i, :4])
            w1, w2 = int(table[i, 4]), int(table[i, 5])
            plus = w1 * c(y + dy1, x + dx1) + w2 * c(y + dy2, x + dx2)
            minus = w1 * c(y - dy1, x - dx1) + w2 * c(y - dy2, x - dx2)
            m = w1 + w2
            if m * here > minus and m * here >= plus:
                out[y, x] = here
    return out


def thin_fast(edges, dirs, n, table=None):
    """``thin`` on whole arrays (edge padding = the clamp), for maps too large for the pixel loop. int64 products: exact for
    w1 + w2 <= 2048 and values below 2^31."""
    edges, dirs = np.asarray(edges), np.asarray(dirs)
    table = steps(n) if table is None else np.asarray(table)
    h, w = edges.shape
    v = np.maximum(edges.astype(np.int64), 0)
    pad = np.pad(v, 1, mode="edge")
    ys, xs = np.mgrid[0:h, 0:w]
    ok = dirs < n
    row = table[np.where(ok, dirs, 0).astype(np.int64)].astype(np.int64)
    off = np.clip(row[..., :4], -1, 1)
    w1, w2 = row[..., 4], row[..., 5]
    tap = lambda dy, dx: pad[ys + 1 + dy, xs + 1 + dx]
    plus = w1 * tap(off[..., 0], off[..., 1]) + w2 * tap(off[..., 2], off[..., 3])
    minus = w1 * tap(-off[..., 0], -off[..., 1]) + w2 * tap(-off[..., 2], -off[..., 3])
    mv = (w1 + w2) * v
    keep = ok & (v > 0) & (mv > minus) & (mv >= plus)
    return np.where(keep, v, 0).astype(np.int32)
