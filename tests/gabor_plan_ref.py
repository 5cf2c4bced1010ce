"""The shape-dependent part of the Gabor launch plan (csrc/gabor_plan.h) restated in plain Python, and a parser of the text
gcs_selftest_gabor_plan writes. The restatement covers the tile counts, the persistent grid, the small-call rule and the fork
condition - not which instantiation a launch takes: that is held to the recorded table tests/golden/gabor_plan_table.json."""
import collections
import ctypes as C
import re

FORK_MIN_PIXELS = 1 << 21
Launch = collections.namedtuple("Launch", "kernel args l0 l1 f0 grid_x grid_y tiles side join")
_LINE = re.compile(r"(\w+)(?:<([^>]*)>)? levels=(\d+):(\d+) f0=(\d+) grid=(\d+)x(\d+) tiles=(\d+) stream=(main|side) join=([01])")


def plan(lib, b, h, w, ns, no, ks, shift, cu_count, forked=0):
    """The hook's answer as a list of Launch (args: the template arguments as written, e.g. "3,2,7,-2,true,false"), None if refused."""
    buf = C.create_string_buffer(1 << 15)
    n = lib.gcs_selftest_gabor_plan(b, h, w, ns, no, ks, shift, cu_count, forked, buf, len(buf))
    if n < 0:
        return None
    out = []
    for line in buf.value.decode().splitlines():
        m = _LINE.fullmatch(line)
        assert m, line
        out.append(Launch(m.group(1), m.group(2) or "", int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6)),
                          int(m.group(7)), int(m.group(8)), m.group(9) == "side", m.group(10) == "1"))
    assert len(out) == n, (n, len(out))
    return out


def bank_launches(launches):
    return [l for l in launches if l.kernel == "gabor_mfma_kernel"]


def form(l):
    """Launch form of a bank launch: the instantiation, "<MT,GQ,KS,LVL,FAST,SPLIT>", with "g" behind it for the grouped launch
    (grid.y row-tile groups of one-tile workgroups)."""
    return "<%s>%s" % (l.args, "g" if l.grid_y > 1 else "")


# ---------------------------------------------------------------------------------------------- restated geometry
def n_levels(ns):
    return (ns + 1) // 2


def level_filters(ns, no):
    return [(2 if ns - 2 * lv >= 2 else 1) * no for lv in range(n_levels(ns))]


def split_slab(ns, no):
    return n_levels(ns) <= 2 and 3 * ns * no < 80


def regions(h, w, ns):
    """[(rows, columns)] of the main region of every level: the level itself, or - banks of at most two levels whose right / bottom
    edge is 1 or 2 pixels beyond a multiple of 8 - the level without that packed strip."""
    may_pack = n_levels(ns) <= 2 and h >= 8 and w >= 8
    pack_r, pack_b = may_pack and w % 8 in (1, 2), may_pack and h % 8 in (1, 2)
    out = []
    hl, wl = h, w
    for lv in range(n_levels(ns)):
        out.append(((h // 8 * 8) >> lv if pack_b else hl, (w // 8 * 8) >> lv if pack_r else wl))
        hl, wl = (hl + 1) // 2, (wl + 1) // 2
    return out


def half_tiles(h, w, ns):
    """32 x 32 half tiles of every level's main region"""
    return [-(-rw // 32) * -(-rh // 32) for rh, rw in regions(h, w, ns)]


def tiles_per_image(h, w, ns):
    """a workgroup's 64 x 32 tile is any two consecutive half tiles of one image"""
    return [(n + 1) // 2 for n in half_tiles(h, w, ns)]


def fuse_small(b, h, w, ns, no, cu_count):
    """A two-level call whose tiles all fit the resident slots (two workgroups per compute unit) at once - except the split-slab
    banks with 9 to 11 filters per level."""
    fl = level_filters(ns, no)
    return (n_levels(ns) == 2 and b * sum(tiles_per_image(h, w, ns)) <= 2 * cu_count and
            not (split_slab(ns, no) and 9 <= fl[0] <= 11))


def forks(b, h, w, ns, forked):
    return bool(forked) and n_levels(ns) == 2 and b * h * w >= FORK_MIN_PIXELS


def level_lists(b, h, w, ns, no, cu_count):
    """[(L0, L1)] of the bank launches: runs of levels with equal filter counts share a tile list in banks of three or four levels
    and in small calls."""
    fl, out, l0 = level_filters(ns, no), [], 0
    fused = n_levels(ns) > 2 or fuse_small(b, h, w, ns, no, cu_count)
    while l0 < len(fl):
        l1 = l0 + 1
        while fused and l1 < len(fl) and fl[l1] == fl[l0]:
            l1 += 1
        out.append((l0, l1))
        l0 = l1
    return out


def list_geometry(b, h, w, ns, l0, l1, cu_count):
    """(total_tiles, grid.x, [end of every level's tiles in the list])"""
    tpi = tiles_per_image(h, w, ns)
    ends, total = [], 0
    for lv in range(l0, l1):
        total += b * tpi[lv]
        ends.append(total)
    return total, min(total, 2 * cu_count), ends


def walk_crosses_a_level(total, grid_x, ends):
    """Some persistent workgroup (tiles g, g + grid.x, ...) works on tiles of two levels."""
    level = lambda t: sum(t >= e for e in ends)
    return any(level(g) != level(t) for g in range(grid_x) for t in range(g + grid_x, total, grid_x))
