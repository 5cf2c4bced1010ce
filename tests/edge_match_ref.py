"""SPEC.md §27 restated in plain NumPy / Python: the incremental one-to-one matching of a level map against a thin contour, every
level at once. Test helper only; it calls nothing of the library. ``evaluate.match_count`` (scipy's Hopcroft-Karp, one matching
per level) is the independent reference the tests hold this - and the kernel - against."""
import numpy as np

FREE, NOT, DEAD = -1, -2, -3


def offsets(d2):
    """The disc's (dy, dx) pairs with dy^2 + dx^2 <= d2 in row-major order, int32 [n][2]."""
    reach = 0
    while (reach + 1) ** 2 <= d2:
        reach += 1
    return np.array([(dy, dx) for dy in range(-reach, reach + 1) for dx in range(-reach, reach + 1) if dy * dy + dx * dx <= d2],
                    np.int32).reshape(-1, 2)


def thin(s):
    """Q of a label map: a pixel whose right or lower neighbour (where the image has one) carries another label. (H,W) bool."""
    s = np.asarray(s)
    h, w = s.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            out[y, x] = (x + 1 < w and s[y, x + 1] != s[y, x]) or (y + 1 < h and s[y + 1, x] != s[y, x])
    return out


def sweep(q, truth, levels, offs, cap=None):
    """q: (H,W) integers, read as clamp(q, 0, levels); truth: (H,W) bool, Q; offs: [n][2] allowed (dy, dx). Returns
    (M int64 [levels], above int64 [levels], steps): M[tau] = the size of a maximum matching between {q > tau} and Q. The rule of
    §27: pixels enter in descending level (raster order inside a level), one alternating-path search per pixel, the contour pixels
    a failed search visited are dead from then on. ``cap``: a search that would push more than ``cap`` contour pixels makes the
    whole row -1."""
    q = np.clip(np.asarray(q).astype(np.int64), 0, levels)
    h, w = q.shape
    state = np.where(np.asarray(truth, bool), FREE, NOT).astype(np.int64).ravel()
    offs = [(int(dy), int(dx)) for dy, dx in np.asarray(offs).reshape(-1, 2)]
    matched, above = np.zeros(levels, np.int64), np.zeros(levels, np.int64)
    count = seen = steps = 0
    flat = q.ravel()
    for v in range(levels, 0, -1):
        for p in np.flatnonzero(flat == v):
            seen += 1
            stack, log, visited, cur = [], [], set(), int(p)
            while True:
                steps += 1
                y, x = divmod(cur, w)
                free = nxt = None
                for dy, dx in offs:
                    yy, xx = y + dy, x + dx
                    if not (0 <= yy < h and 0 <= xx < w):
                        continue
                    u = yy * w + xx
                    if state[u] == FREE:
                        free = u
                        break
                    if nxt is None and state[u] >= 0 and u not in visited:
                        nxt = u
                if free is not None:
                    state[free] = cur
                    for u, left in stack:
                        state[u] = left
                    count += 1
                    break
                if nxt is not None:
                    if cap is not None and len(log) >= cap:
                        return np.full(levels, -1, np.int64), None, steps
                    visited.add(nxt)
                    log.append(nxt)
                    stack.append((nxt, cur))
                    cur = int(state[nxt])
                    continue
                if not stack:
                    for u in log:
                        state[u] = DEAD
                    break
                cur = stack.pop()[1]
        matched[v - 1], above[v - 1] = count, seen
    return matched, above, steps
