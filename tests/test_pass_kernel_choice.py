"""Which Lloyd-pass kernel a (bank, k) takes (csrc/lloyd_pass.h: gcs_pass_kernel, through the host-only hook
gcs_selftest_pass_kernel), and what the pass entry points answer to calls they refuse - both against
tests/golden/pass_kernel_table.json, recorded at the commit before the choice had a function of its own
(tests/golden/make_pass_kernel_table.py: a launch recorded the stringified kernel instead of launching). No GPU: nothing here
launches, and no pointer is dereferenced.

The `nt` limit of a launch (csrc/lloyd_pass.h: gcs_pass_nt_limit, through the hook gcs_selftest_pass_nt_limit) against kp_nt_limit
restated here, and the preconditions of the cases of tests/test_gpu_nt_arm.py."""
import ctypes as C
import json
import os

import pytest

from gabor_color_image_segmentation_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(8, 8), (321, 481), (2048, 2048)]
NO_SPLIT_ONLY = {"narrow<1,9>", "narrow<1,10>", "narrow<2,10>"}
SELF_UPDATING = {"split<1,3>", "split<1,3,2>"}


@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


@pytest.fixture(scope="module")
def table():
    return json.load(open(os.path.join(HERE, "golden", "pass_kernel_table.json")))


@pytest.fixture(scope="module")
def recorded(table):
    """{(n_scales, n_orient, k): display name, or None where the parent refused the call}"""
    want = {}
    for name, rows in table["choice"].items():
        for ns, no, mask in rows:
            for k in range(1, 17):
                if mask >> (k - 1) & 1:
                    assert (ns, no, k) not in want
                    want[ns, no, k] = None if name == "refused" else name
    assert len(want) == 8 * 70 * 16
    return want


def _name(lib, h, w, ns, no, k):
    s = lib.gcs_selftest_pass_kernel(h, w, ns, no, k)
    return None if s is None else s.decode()


def test_choice_equals_the_recorded_one_over_the_whole_domain(lib, recorded):
    """n_scales 1..8 x n_orient 1..70 x k 1..16, and the same answer for 8 x 8, 321 x 481 and 2048 x 2048."""
    bad = [(key, [_name(lib, h, w, *key) for h, w in SHAPES], want) for key, want in recorded.items()
           if [_name(lib, h, w, *key) for h, w in SHAPES] != [want] * len(SHAPES)]
    assert not bad, (len(bad), bad[:5])
    assert {n for n in recorded.values() if n} >= SELF_UPDATING | {"generic", "wide8w<1,5>", "native<4,3,6>", "native<4,2,0>"}


def test_default_library_never_takes_a_no_split_only_kernel(lib, recorded):
    got = {_name(lib, h, w, *key) for key in recorded for h, w in SHAPES}
    assert not got & NO_SPLIT_ONLY, got & NO_SPLIT_ONLY
    assert not set(recorded.values()) & NO_SPLIT_ONLY


def test_refused_shapes_banks_and_k_give_null(lib):
    for args in [(0, 8, 4, 6, 8), (8, 0, 4, 6, 8), (8, 8, 0, 6, 8), (8, 8, 9, 6, 8), (8, 8, 4, 0, 8), (8, 8, 4, 6, 0), (8, 8, 4, 6, 17),
                 (30000, 30000, 4, 6, 8), (8, 8, 8, 70, 16)]:
        assert lib.gcs_selftest_pass_kernel(*args) is None, args


def test_value_range_case_ids_name_the_kernel_their_bank_takes(lib):
    """The ids of PASS_CASES (tests/pass_cases.py) are claims: each starts with the hook's answer for its bank and k."""
    from pass_cases import PASS_CASES
    assert len(PASS_CASES) >= 28
    for (ns, no, _ks, _shift, k), case_id in PASS_CASES:
        name = _name(lib, 41, 74, ns, no, k)
        assert name and (case_id == name or case_id.startswith(name + "_")), (case_id, name)


def test_fused_workspace_follows_the_choice(lib, table):
    """gcs_kmeans_fused_workspace_bytes != 0 exactly where the classic choice is split<1,3> or split<1,3,2> (n_sets = 1 and B) -
    and exactly where the parent's was."""
    was = {(ns, no, k) for ns, no, mask in table["fused"] for k in range(1, 17) if mask >> (k - 1) & 1}
    for ns in range(1, 9):
        for no in range(1, 71):
            for k in range(1, 17):
                for h, w in SHAPES:
                    want = _name(lib, h, w, ns, no, k) in SELF_UPDATING
                    got = [lib.gcs_kmeans_fused_workspace_bytes(b, h, w, ns, no, k, n) != 0 for b, n in ((1, 1), (3, 1), (3, 3))]
                    assert got == [want] * 3 and want == ((ns, no, k) in was), (ns, no, k, h, w, got, want)
    assert lib.gcs_kmeans_fused_workspace_bytes(3, 40, 56, 4, 6, 8, 2) == 0


# The same table, continued past what the fixture recorded: the first batch kp_batch_fits refuses (2048 x 2048 has 16 384 tiles on
# every bank, 32 768 * 16 384 = 2^29 > 2^29 - 1; 32 767 images fit: tests/test_large_offset_geometry.py) and a split image of more
# than 2^32 - 1 bytes (30 001 x 1002 on a 2x13 bank: gcs_make_layout refuses it, so "image too large for the split slab's pass" is
# never reached), through the three entry points.
_BATCH = "batch too large for one launch"
LIMIT_ERRORS = [
    {"fn": "gcs_kmeans_assign_accumulate", "args": ["P", "P", 32768, 2048, 2048, ns, no, 8, n_sets, 0, 2048, 0, "P", "P", None], "rc": 1,
     "message": "gcs_kmeans_assign_accumulate: " + _BATCH} for ns, no in ((4, 6), (8, 8), (7, 10)) for n_sets in (1, 32768)] + [
    {"fn": "gcs_kmeans_assign_raster", "args": ["P", "P", 32768, 2048, 2048, 4, 6, 8, 1, 0, "P", 0, None, None], "rc": 1,
     "message": "gcs_kmeans_assign_accumulate: " + _BATCH},
    {"fn": "gcs_kmeans_pass_fused", "args": ["P", 32768, 2048, 2048, 4, 6, 8, 1, 0, 0, 0, "P", "P", None, 0, None], "rc": 1,
     "message": "gcs_kmeans_pass_fused: batch or image too large for one launch"},
    {"fn": "gcs_kmeans_assign_accumulate", "args": ["P", "P", 1, 30001, 1002, 2, 13, 8, 1, 0, 30001, 0, "P", "P", None], "rc": 1,
     "message": "gcs_kmeans_assign_accumulate: bad shape or bank"},
    {"fn": "gcs_kmeans_assign_raster", "args": ["P", "P", 1, 30001, 1002, 2, 13, 8, 1, 0, "P", 0, None, None], "rc": 1,
     "message": "gcs_kmeans_assign_accumulate: bad shape or bank"},
    {"fn": "gcs_kmeans_pass_fused", "args": ["P", 1, 30001, 1002, 2, 13, 8, 1, 0, 0, 0, "P", "P", None, 0, None], "rc": 1,
     "message": "gcs_kmeans_pass_fused: bad shape or bank"}]


def test_bad_arguments_keep_their_code_and_message(lib, table):
    """Every rule of lloyd_pass and of gcs_kmeans_pass_fused, through the three entry points: (rc, gcs_last_error()) as recorded. The
    calls return before any launch ("P": a pointer that is never dereferenced)."""
    fake = C.c_void_p(4096)
    errors = table["errors"]                         # (what the fixture must hold is asked of the fixture alone, below)
    for e in errors + LIMIT_ERRORS:
        args = [fake if a == "P" else C.c_void_p(None) if a is None else C.c_int(a) for a in e["args"]]
        rc = getattr(lib, e["fn"])(*args)
        assert (rc, lib.gcs_last_error().decode()) == (e["rc"], e["message"]), e
    # the fixture holds a case of every rule
    said = {(e["fn"], e["message"].split(": ", 1)[1][:24]) for e in errors}
    for fn, rule in [("gcs_kmeans_assign_accumulate", "NULL pointer"), ("gcs_kmeans_assign_accumulate", "bad shape or bank"),
                     ("gcs_kmeans_assign_accumulate", "need 0 <= row_lo"), ("gcs_kmeans_assign_accumulate", "B too large"),
                     ("gcs_kmeans_assign_accumulate", "batch too large"), ("gcs_kmeans_assign_accumulate", "k must be in 1..16"),
                     ("gcs_kmeans_assign_accumulate", "n_sets must be 1 or B"), ("gcs_kmeans_assign_accumulate", "k*D too large"),
                     ("gcs_kmeans_assign_raster", "NULL pointer"), ("gcs_kmeans_assign_raster", "feature vectors of 208"),
                     ("gcs_kmeans_assign_raster", "batch too large"), ("gcs_kmeans_assign_raster", "k must be in 1..16"),
                     ("gcs_kmeans_pass_fused", "NULL pointer"), ("gcs_kmeans_pass_fused", "bad shape or bank"),
                     ("gcs_kmeans_pass_fused", "pass must be >= 0"), ("gcs_kmeans_pass_fused", "no self-updating pass"),
                     ("gcs_kmeans_pass_fused", "batch or image too large")]:
        assert any(f == fn and m.startswith(rule[:24]) for f, m in said), (fn, rule)
    null_args = {(e["fn"], i) for e in errors for i, a in enumerate(e["args"][:-1]) if a is None}
    assert null_args >= {("gcs_kmeans_assign_accumulate", 0), ("gcs_kmeans_assign_accumulate", 1), ("gcs_kmeans_assign_accumulate", 12),
                         ("gcs_kmeans_assign_raster", 0), ("gcs_kmeans_assign_raster", 1), ("gcs_kmeans_assign_raster", 10),
                         ("gcs_kmeans_pass_fused", 0), ("gcs_kmeans_pass_fused", 11), ("gcs_kmeans_pass_fused", 12),
                         ("gcs_kmeans_pass_fused", 13)}


# ------------------------------------------------------------------------------------------ the `nt` limit of a launch
KEEP_BYTES = 256 << 20             # csrc/lloyd_pass.h: the end of every sweep list that is loaded plain (the Infinity Cache's size)
NT_B = [1, 3, 16, 28, 64, 400]
NT_SHAPES = [(41, 74), (321, 481), (2048, 2048)]


def _nt_limit(name, ntiles, tile_bytes, b, n_sets):
    """kp_nt_limit: list positions below the result are loaded `nt`. A sweep list is the whole batch, or one image with per-image
    codebooks (then the budget is shared by the B lists); a split-slab pass streams 3/4 of a tile, the deep-bank pass all of it, and
    every other kernel loads plain."""
    if name.startswith("split<"):
        stream = tile_bytes // 4 * 3
    elif name.startswith("native<"):
        stream = tile_bytes
    else:
        return 0
    lists, nlist = (b, ntiles) if n_sets == b else (1, ntiles * b)
    return max(nlist - KEEP_BYTES // stream // lists, 0)


def test_nt_limit_equals_the_restated_one(lib):
    """Every bank of PASS_CASES and the default 4x6 and 8x8 banks, n_sets 1 and B, B and shapes as listed; both arms and every
    family occur."""
    from slab_layout import tile_geometry
    from pass_cases import PASS_CASES
    banks = sorted({(ns, no, k) for (ns, no, _ks, _shift, k), _ in PASS_CASES} | {(4, 6, 8), (8, 8, 8)})
    seen = {}
    for ns, no, k in banks:
        for h, w in NT_SHAPES:
            name = _name(lib, h, w, ns, no, k)
            ntiles, tile_bytes, split = tile_geometry(lib, h, w, ns, no)
            assert split == name.startswith("split<"), (name, split)
            for b in NT_B:
                for n_sets in {1, b}:
                    want = _nt_limit(name, ntiles, tile_bytes, b, n_sets)
                    got = lib.gcs_selftest_pass_nt_limit(b, h, w, ns, no, k, n_sets)
                    assert got == want, (name, (ns, no, k), (b, h, w), n_sets, got, want)
                    fam = seen.setdefault(name.split("<")[0], set())
                    fam.add("nt" if want else "plain")
                    if n_sets == b and b > 1 and want:
                        fam.add("nt per image")
    assert seen["split"] == seen["native"] == {"nt", "plain", "nt per image"}, seen
    assert set(seen) == {"split", "native", "narrow", "wide", "wide8w", "generic"}, set(seen)
    assert lib.gcs_selftest_pass_nt_limit(64, 321, 481, 4, 6, 8, 1) == 64 * 607 - KEEP_BYTES // 17280       # the timed shape: 23 314 of 38 848


def test_nt_limit_is_zero_for_plain_kernels_and_minus_one_where_refused(lib, recorded):
    """Over the whole recorded domain: -1 exactly where the table says "refused", 0 for every narrow, wide and generic kernel whatever
    the size, never negative otherwise; and -1 for the calls lloyd_pass refuses for B, n_sets or the batch size."""
    for (ns, no, k), name in recorded.items():
        got = {lib.gcs_selftest_pass_nt_limit(b, h, w, ns, no, k, n) for h, w in ((321, 481), (2048, 2048)) for b in (1, 64, 400)
               for n in {1, b}}
        if name is None:
            assert got == {-1}, (ns, no, k, got)
        elif name.split("<")[0] in ("split", "native"):
            assert min(got) >= 0 and max(got) > 0, (ns, no, k, name, got)
        else:
            assert got == {0}, (ns, no, k, name, got)
    for args in [(0, 321, 481, 4, 6, 8, 1), (65536, 8, 8, 4, 6, 8, 1), (3, 321, 481, 4, 6, 8, 2), (3, 321, 481, 4, 6, 8, 0),
                 (3, 321, 481, 4, 6, 0, 1), (3, 321, 481, 4, 6, 17, 1), (3, 0, 481, 4, 6, 8, 1), (3, 321, 481, 9, 6, 8, 1),
                 (40000, 2048, 2048, 4, 6, 8, 1), (1, 30000, 30000, 4, 6, 8, 1)]:
        assert lib.gcs_selftest_pass_nt_limit(*args) == -1, args
    assert lib.gcs_selftest_pass_nt_limit(3, 321, 481, 4, 6, 8, 3) == 0 and lib.gcs_selftest_pass_nt_limit(1, 8, 8, 1, 1, 1, 1) == 0


def test_nt_arm_cases_satisfy_their_preconditions(lib):
    """tests/test_gpu_nt_arm.py: the twelve kernels that have an `nt` arm, each id names the kernel its bank takes, the G written
    beside a case is what the launcher computes, 0 < nt_limit < nlist with at least G + 1 positions on either side, nt_limit no
    multiple of G, nt_limit > 0 per image list where a case runs per-image codebooks, a self-updating pass where it runs one - and
    no batch is larger than it has to be: one image fewer breaks a condition."""
    import test_gpu_nt_arm as nt
    kernels = set()
    for case in nt.NT_CASES:
        case_id, bank, (b, h, w), g, what = case
        limit, nlist, _ = nt.preconditions(lib, case)
        assert limit == _nt_limit(nt.kernel_of(lib, case), *__import__("slab_layout").tile_geometry(lib, h, w, *bank[:2])[:2], b, 1)
        kernels.add(nt.kernel_of(lib, case) + ("_self_updating" if what == "fused" else ""))
        smaller = (case_id, bank, (b - 1, h, w), None, "pass")
        g1 = nt.launch_workgroups(lib, smaller)
        l1 = lib.gcs_selftest_pass_nt_limit(b - 1, h, w, bank[0], bank[1], bank[4], 1)
        n1 = nlist // b * (b - 1)
        assert not (l1 >= g1 + 1 and n1 - l1 >= g1 + 1 and l1 % g1), (case_id, "B - 1 would do")
        assert 2.3e6 <= b * h * w <= 6.2e6, (case_id, b * h * w)
    assert kernels == {"split<1,3,2>", "split<1,3>", "split<1,5>", "split<2,5>", "split<1,3,2>_self_updating", "split<1,3>_self_updating",
                       "native<2,3,0>", "native<2,3,6>", "native<3,3,0>", "native<3,3,6>", "native<4,3,6>", "native<4,2,0>"}, kernels
    assert sum(c[4] == "per_image" for c in nt.NT_CASES) == 2
