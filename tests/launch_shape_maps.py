"""Label maps for the connected-regions and merge kernels at the shapes where their launches change: grids are
min(1024, ceil(P / 256)) workgroups of 256 threads, so the grid-stride loops take a second step only above P = 262 144, and
cc_rank_kernel splits P over 1 024 threads (P = 1 023, 1 024, 1 025; P = 1; single rows and columns)."""
import numpy as np

SMALL_SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 5), (31, 33), (32, 32), (25, 41)]
LARGE_SHAPE = (520, 510)                                # P = 265 200 > 1 024 * 256
assert LARGE_SHAPE[0] * LARGE_SHAPE[1] > 1024 * 256


def maps(h, w, seed=0):
    """{name: (H,W) int32 map}. "own" gives every pixel its own label; the combs are ONE long region with a tooth in every
    other column, joined by a spine in the first (comb_top) or the last row (comb_bottom: every tooth's smallest pixel lies in
    row 0, so the teeth are united from below and roots get re-parented from many sides), and a separate gap between the teeth.
    "patch" is 4-label noise inside one constant background that owns the first rows (and, at the large shape, the rows of the
    second grid-stride step of workgroup 0): its merges take several rounds, and no thread of workgroup 0 ever takes part."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    y, x = np.mgrid[:h, :w]
    top = ((x % 2 == 0) | (y == 0)).astype(np.int32)
    bottom = ((x % 2 == 0) | (y == h - 1)).astype(np.int32)
    inside = (y >= 3 * h // 10) & (y < 8 * h // 10) & (x >= w // 5) & (x < 4 * w // 5)
    patch = np.where(inside, rng.integers(1, 5, (h, w)), 0).astype(np.int32)
    return {"noise2": rng.integers(0, 2, (h, w)).astype(np.int32),
            "noise4": rng.integers(0, 4, (h, w)).astype(np.int32),
            "own": np.arange(h * w, dtype=np.int32).reshape(h, w)[::-1, ::-1].copy(),     # labels in reverse raster order
            "constant": np.full((h, w), 7, np.int32),
            "rows1": (y % 2).astype(np.int32),
            "cols1": (x % 2).astype(np.int32),
            "checker": ((y + x) % 2).astype(np.int32),
            "comb_top": top,
            "comb_bottom": bottom,
            "patch": patch}


def few_valued(h, w, seed=0):
    """The maps with a handful of label values (the scipy oracle loops over the distinct values: "own" is left to a direct
    comparison with np.arange)."""
    return {k: v for k, v in maps(h, w, seed).items() if k != "own"}
