"""Which Lloyd-pass kernel a (bank, k) takes (csrc/lloyd_pass.h: gcs_pass_kernel, through the host-only hook
gcs_selftest_pass_kernel), and what the pass entry points answer to calls they refuse - both against
tests/golden/pass_kernel_table.json, recorded at the commit before the choice had a function of its own
(tests/golden/make_pass_kernel_table.py: a launch recorded the stringified kernel instead of launching). No GPU: nothing here
launches, and no pointer is dereferenced."""
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
    """The ids of PASS_CASES (tests/test_gpu_value_range.py) are claims: each starts with the hook's answer for its bank and k."""
    from test_gpu_value_range import PASS_CASES
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


def test_bad_arguments_keep_their_code_and_message(lib, table):
    """Every rule of lloyd_pass and of gcs_kmeans_pass_fused, through the three entry points: (rc, gcs_last_error()) as recorded. The
    calls return before any launch ("P": a pointer that is never dereferenced)."""
    fake = C.c_void_p(4096)
    errors = table["errors"]
    for e in errors:
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
