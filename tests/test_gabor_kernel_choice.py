"""Which kernels one gcs_gabor_features call launches (csrc/gabor_plan.h: gabor_plan, through the host-only hook
gcs_selftest_gabor_plan): the bank-kernel instantiations against tests/golden/gabor_plan_table.json, recorded at the commit before the
plan had a function of its own (tests/golden/make_gabor_plan_table.py: a launch recorded the stringified kernel instead of
launching); tile counts, grids, the small-call rule and the fork condition against the restatement tests/gabor_plan_ref.py; and the
statement of WHICH TEST REACHES WHICH INSTANTIATION: the launch forms reachable over the domain are exactly those the cases of
tests/test_gpu_gabor_instantiations.py name. No GPU: nothing here launches, and no pointer is dereferenced.

Compiled but unreachable (UNREACHABLE below; gabor_launch instantiates every arm of GCS_GABOR_ARMS for both slab formats): 7 of the 90
instantiations, all of them split-slab forms of a fused list. A split-slab bank has at most two levels and D < 80, so its fused list
is the small call of a four-scale bank with 2 n_orient <= 12 filters per level. Such a level of 8 or 12 filters runs grouped (MT = 1),
one of 10 is excluded from the small call, one of 6 ends in a tile with one filter pair (<2,1,..>), smaller ones are one tile: the
split forms of <2,2,7|8,-1,*> and of <3,*,7,-2,*> cannot be chosen."""
import ctypes as C
import json
import os

import pytest

import gabor_plan_ref as gp
from gabor_color_image_segmentation_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
CU = 256
BANKS = [(ns, no) for ns in range(1, 9) for no in range(1, 71) if ns * no <= 70]
KSIZES = {0: (1, 3, 5, 7, 9, 11, 13), 1: (15,)}
SHIFTS = {0: (8,), 1: (7,)}
# (H, W): (a batch that is not small for any bank at 256 compute units, one that is small for every bank; None: there is none)
SHAPES = {(8, 8): (300, 1), (321, 481): (16, 1), (2048, 2048): (1, None)}
COMPILED = {"<%d,%d,%d,%d,%s,%s>" % (mt, gq, ks, lv, fa, sp) for mt, ks in ((3, 7), (2, 7), (1, 7), (2, 8), (1, 8))
            for gq, fa in ((1, "false"), (2, "true"), (2, "false")) for lv in ((-2, 0, 1) if mt == 3 else (0, 1, -1))
            for sp in ("true", "false")}
UNREACHABLE = {"<2,2,7,-1,false,true>", "<2,2,7,-1,true,true>", "<2,2,8,-1,false,true>", "<2,2,8,-1,true,true>",
               "<3,1,7,-2,false,true>", "<3,2,7,-2,false,true>", "<3,2,7,-2,true,true>"}


@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    """{(n_scales, n_orient, ksize class, shift class, small): plan}"""
    table = json.load(open(os.path.join(HERE, "golden", "gabor_plan_table.json")))
    assert table["cu_count"] == CU
    want = {}
    for plan, rows in table["plans"].items():
        for ns, no, mask in rows:
            for bit in range(8):
                if mask >> bit & 1:
                    key = (ns, no, bit >> 2, bit >> 1 & 1, bit & 1)
                    assert key not in want
                    want[key] = plan
    assert len(want) == len(BANKS) * 8
    return want


def _plan_key(launches):
    return "; ".join("<%s> %d:%d +%d x%d" % (l.args, l.l0, l.l1, l.f0, l.grid_y) for l in gp.bank_launches(launches))


def test_bank_launches_equal_the_recorded_ones_over_the_whole_domain(lib, recorded):
    """Every bank with n_scales * n_orient <= 70, every odd ksize, shift 8 and 7, small and not-small calls, with and without a side
    stream: instantiation, levels, first filter and grid.y of every bank launch, the same at 8 x 8, 321 x 481 and 2048 x 2048."""
    bad = []
    for (ns, no, ksc, sh, small), want in recorded.items():
        for (h, w), batch in SHAPES.items():
            if batch[small] is None:
                continue
            for ks in KSIZES[ksc]:
                for shift in SHIFTS[sh]:
                    for forked in (0, 1):
                        got = _plan_key(gp.plan(lib, batch[small], h, w, ns, no, ks, shift, CU, forked))
                        if got != want:
                            bad.append(((ns, no, ks, shift, small, h, w, forked), got, want))
    assert not bad, (len(bad), bad[:3])


def test_refused_calls_give_minus_one_and_short_buffers_are_safe(lib):
    ok = (2, 40, 56, 4, 6, 13, 8, CU, 0)
    buf = C.create_string_buffer(4096)
    n = lib.gcs_selftest_gabor_plan(*ok, buf, len(buf))
    assert n == 2 and buf.value.decode().count("\n") == 2                 # a small call: gabor_pre01_kernel and one grouped launch
    for i, v in [(0, 0), (0, 65536), (1, 7), (2, 7), (3, 0), (3, 9), (4, 0), (5, 0), (5, 14), (5, 17), (6, -1), (6, 24), (7, -1)]:
        args = list(ok)
        args[i] = v
        assert lib.gcs_selftest_gabor_plan(*args, buf, len(buf)) == -1 and buf.value == b"", (i, v)
    assert lib.gcs_selftest_gabor_plan(1, 30000, 30000, 4, 6, 13, 8, CU, 0, buf, len(buf)) == -1
    assert lib.gcs_selftest_gabor_plan(1, 8, 20000, 4, 6, 13, 8, CU, 0, buf, len(buf)) == -1      # the pyramid row buffer
    assert lib.gcs_selftest_gabor_plan(*ok, None, 0) == 2
    small = C.create_string_buffer(b"\x7f" * 120, 120)
    assert lib.gcs_selftest_gabor_plan(*ok, small, 100) == 2
    assert small.raw[100:] == b"\x7f" * 20 and small.value.decode().count("\n") == 1             # whole lines only, nothing past the end


# ------------------------------------------------------------------------------------------ geometry against the restatement
GEO_SHAPES = [(8, 8), (9, 10), (33, 41), (34, 42), (35, 36), (40, 40), (64, 64), (65, 130), (72, 88), (81, 121), (321, 481),
              (481, 321), (322, 482), (323, 480), (1024, 2048)]
GEO_BANKS = [(1, 3), (2, 6), (3, 5), (3, 8), (4, 4), (4, 5), (4, 6), (4, 9), (4, 11), (5, 4), (6, 8), (7, 5), (8, 8)]
GEO_B = [1, 2, 3, 4, 7, 16, 64, 300]
GEO_CU = [256, 304, 80, 8]


def test_tiles_grids_streams_and_the_small_call_equal_the_restated_ones(lib):
    """Every launch of the plan at a spread of batches, shapes (packed strips: H or W = 8 k + 1, 8 k + 2) and compute-unit counts."""
    seen = set()
    for h, w in GEO_SHAPES:
        for ns, no in GEO_BANKS:
            tpi, nl, fl = gp.tiles_per_image(h, w, ns), gp.n_levels(ns), gp.level_filters(ns, no)
            packed = nl <= 2 and (h % 8 in (1, 2) or w % 8 in (1, 2))
            for b in GEO_B:
                for cu in GEO_CU:
                    for forked in (0, 1):
                        launches = gp.plan(lib, b, h, w, ns, no, 13, 8, cu, forked)
                        ctx = (b, h, w, ns, no, cu, forked)
                        small, fork = gp.fuse_small(b, h, w, ns, no, cu), gp.forks(b, h, w, ns, forked)
                        pre = [l for l in launches if l.kernel in ("gabor_plane_kernel", "gabor_down_kernel", "gabor_pre01_kernel")]
                        if small and not fork:
                            assert [(l.kernel, l.l0, l.l1) for l in pre] == [("gabor_pre01_kernel", 0, 2)], ctx
                        else:
                            assert [(l.kernel, l.args, l.l0) for l in pre] == [("gabor_plane_kernel", "0", 0)] + [
                                ("gabor_down_kernel", "true" if lv == 1 else "false", lv) for lv in range(1, nl)], ctx
                        assert all(l.grid_y == b for l in pre) and launches[:len(pre)] == pre, ctx
                        lists = gp.level_lists(b, h, w, ns, no, cu)
                        bank = gp.bank_launches(launches)
                        assert sorted({(l.l0, l.l1) for l in bank}) == lists, ctx
                        for l in bank:
                            total, grid_x, _ = gp.list_geometry(b, h, w, ns, l.l0, l.l1, cu)
                            assert (l.tiles, l.grid_x) == (total, grid_x) == (b * sum(tpi[l.l0:l.l1]), min(total, 2 * cu)), (ctx, l)
                            grouped = small and fl[l.l0] % 4 == 0 and fl[l.l0] > 4
                            assert l.grid_y == (fl[l.l0] // 4 if grouped else 1), (ctx, l)
                            seen.add(("grouped" if grouped else "plain", "small" if small else "not small", "walk" if total > grid_x else ""))
                        # filters: the launches of a list cover [0, FL) in order, each at most 12 (8 in a fused list) filters
                        for l0, l1 in lists:
                            starts = [l.f0 for l in bank if (l.l0, l.l1) == (l0, l1)]
                            assert starts == sorted(starts) and starts[0] == 0 and starts[-1] < fl[l0], (ctx, starts)
                        strips = [l for l in launches if l.kernel == "gabor_strip_kernel"]
                        assert bool(strips) == packed and all(l.args == "7" and l.grid_x == (l.tiles + 3) // 4 for l in strips), ctx
                        # streams: level 1 of a forked call on the side stream, everything else on the caller's; a call of this
                        # spread is never small and forked at once, so nothing joins before the end
                        assert not (small and fork) and all(l.side == (fork and l.l0 >= 1) and not l.join for l in launches), (ctx, launches)
                        seen.add("fork" if fork else "one stream")
    assert seen >= {"fork", "one stream", ("grouped", "small", ""), ("plain", "small", ""), ("plain", "not small", "walk"),
                    ("plain", "not small", "")}, seen
    # small AND forked (a device of 2048 compute units): level 1's planes come from the side stream, the caller joins it in front of
    # the first launch that reads them, and the fused list runs on the caller's stream
    p = gp.plan(lib, 16, 321, 481, 4, 6, 13, 8, 2048, 1)
    assert [(l.kernel, l.l0, l.l1, l.side, l.join) for l in p] == [
        ("gabor_plane_kernel", 0, 1, False, False), ("gabor_down_kernel", 1, 2, True, False), ("gabor_strip_kernel", 0, 2, False, True),
        ("gabor_mfma_kernel", 0, 2, False, False)] and (p[3].args, p[3].grid_x, p[3].grid_y) == ("1,2,7,-1,true,true", 16 * 95, 3)
    # the measured configuration: 64 BSD images, default bank
    p = gp.bank_launches(gp.plan(lib, 64, 321, 481, 4, 6, 13, 8, CU, 1))
    assert [(l.args, l.tiles, l.grid_x, l.side) for l in p] == [("3,2,7,0,true,true", 64 * 75, 512, False),
                                                                 ("3,2,7,1,true,true", 64 * 20, 512, True)]


# ------------------------------------------------------------------------------------------ which test reaches which instantiation
def _reachable(lib):
    """{launch form: a (n_scales, n_orient, ksize, shift, small) that takes it} over the whole domain at 256 compute units"""
    out = {}
    for ns, no in BANKS:
        for ks in range(1, 16, 2):
            for shift in (7, 8):
                for small in (0, 1):
                    b, (h, w) = (1, (72, 88)) if small else (300, (8, 8))
                    for l in gp.bank_launches(gp.plan(lib, b, h, w, ns, no, ks, shift, CU, 0)):
                        out.setdefault(gp.form(l), (ns, no, ks, shift, small))
    return out


def test_reachable_launch_forms_are_exactly_those_the_gpu_cases_name(lib):
    """83 instantiations, 107 launch forms; the 7 compiled instantiations nothing can select are those listed above; every form has a
    case in tests/test_gpu_gabor_instantiations.py, every case id names what the hook answers for its call, and no case is
    redundant. Fails when a case leaves the table and when the launcher gains an arm without a case."""
    import test_gpu_gabor_instantiations as gi
    reach = _reachable(lib)
    inst = {f.rstrip("g") for f in reach}
    assert (len(inst), len(reach)) == (83, 107), (len(inst), len(reach))
    assert inst <= COMPILED and COMPILED - inst == UNREACHABLE, sorted(COMPILED - inst)
    named = {}
    for cfg, forms in gi.CASES:
        batch = gi.inputs_for(lib, cfg, CU)
        assert gi.plan_forms(lib, cfg, batch, CU) == forms.split(" "), (cfg, batch, gi.plan_forms(lib, cfg, batch, CU))
        for f in forms.split(" "):
            named.setdefault(f, []).append(cfg)
    missing, extra = set(reach) - set(named), set(named) - set(reach)
    assert not missing and not extra, ({f: reach[f] for f in missing}, extra)
    for cfg, forms in gi.CASES:
        assert any(named[f] == [cfg] for f in forms.split(" ")), ("redundant case", cfg)
    assert len(gi.CASES) == len({cfg for cfg, _ in gi.CASES}) <= 55
    assert len({gi.case_id(c) for c in gi.CASES}) == len(gi.CASES)


def test_gpu_cases_meet_their_preconditions_and_no_batch_is_larger_than_needed(lib):
    """At 256 compute units, through the helper the GPU test uses at the device's own count: every condition of the module docstring
    of tests/test_gpu_gabor_instantiations.py holds, one image fewer breaks one, and the batches stay a few hundred thousand pixels.
    The helper also finds a batch on devices of 8, 64, 80 and 304 compute units, with the same launch forms."""
    import test_gpu_gabor_instantiations as gi
    batches = set()
    for cfg, forms in gi.CASES:
        b, h, w = gi.inputs_for(lib, cfg, CU)
        assert gi.unmet(lib, cfg, (b, h, w), CU) == [] and gi.unmet(lib, cfg, (b - 1, h, w), CU) != [], cfg
        assert b * h * w <= 330000, (cfg, b, h, w)
        launches = gp.bank_launches(gp.plan(lib, b, h, w, *cfg[:4], CU, 1))
        assert not any(l.side for l in launches)
        if cfg[4]:
            assert (b, h, w) == (2, 72, 88) and gp.half_tiles(h, w, cfg[0]) == [9, 4] and all(l.tiles <= l.grid_x for l in launches)
        else:
            assert (h, w) == (35, 36) and gp.tiles_per_image(h, w, cfg[0]) == [2] + [1] * (gp.n_levels(cfg[0]) - 1)
            assert any(l.tiles > l.grid_x for l in launches)
            assert all(l.tiles > l.grid_x for l in launches if l.l1 - l.l0 > 1), cfg
        batches.add((gp.n_levels(cfg[0]), cfg[4], b))
        for cu in (8, 64, 80, 304):
            assert gi.plan_forms(lib, cfg, gi.inputs_for(lib, cfg, cu), cu) == forms.split(" "), (cfg, cu)
    assert batches == {(2, 1, 2), (2, 0, 257), (3, 0, 171), (4, 0, 129)}, batches


def test_every_launch_of_a_gpu_case_has_taps_in_every_k_step_of_every_filter(lib):
    """gcs_bank_pack centres the ksize x ksize kernel in the 15 x 15 frame (first row (15 - ksize) / 2); K-step kk of the bank kernel
    is frame rows 2 kk and 2 kk + 1, KS = 7 or 8 of them (csrc/gabor.hip). A launch whose filters have no tap in a K-step would
    compute the same features with that K-step dropped or wrong. So: every filter of every level of every bank launch of every
    case has a non-zero tap in every K-step of its instantiation (the cases' banks turn their odd scales instead of insetting them:
    tests/hot_banks.py), the two scales of a level still differ in every filter, and the inset default would NOT do."""
    import numpy as np
    import hot_banks as hb
    import test_gpu_gabor_instantiations as gi

    def k_step_taps(taps, ks):
        """[F, 8]: sum of |tap| (real and imaginary) of every filter in each of the frame's eight row pairs"""
        frame = np.zeros((taps.shape[0], 2, 16, ks), np.int64)
        off = (15 - ks) // 2
        frame[:, :, off:off + ks] = np.abs(taps.astype(np.int64))
        return frame.reshape(taps.shape[0], 2, 8, 2 * ks).sum((1, 3))

    inset_fails = 0
    for cfg, forms in gi.CASES:
        ns, no, ks, shift, _small = cfg
        taps = gi.case_bank(cfg).tapq
        assert np.array_equal(taps, hb.hot_taps(ns, no, ks, shift, odd="turned"))
        per, per_inset = k_step_taps(taps, ks), k_step_taps(hb.hot_taps(ns, no, ks, shift), ks)
        fl = gp.level_filters(ns, no)
        first = [sum(fl[:lv]) for lv in range(len(fl))]
        for lv, n in enumerate(fl):                         # the filters of a level are pairwise different
            assert len({taps[f].tobytes() for f in range(first[lv], first[lv] + n)}) == n, (cfg, lv)
        for l in gp.bank_launches(gp.plan(lib, *gi.inputs_for(lib, cfg, CU), ns, no, ks, shift, CU, 1)):
            mt, _gq, n_k = (int(v) for v in l.args.split(",")[:3])
            assert n_k == (7 if ks <= 13 else 8)
            for lv in range(l.l0, l.l1):
                fs = range(first[lv] + l.f0, first[lv] + min(fl[lv], l.f0 + 4 * mt * l.grid_y))
                assert len(fs) > 0 and (per[fs.start:fs.stop, :n_k] > 0).all(), (cfg, gp.form(l), lv)
                assert (per[fs.start:fs.stop, n_k:] == 0).all()
                inset_fails += not (per_inset[fs.start:fs.stop, :n_k] > 0).any(0).all()
    assert inset_fails > 0


def test_the_table_of_design_md_is_the_case_table(lib):
    """DESIGN.md 4.1 lists every launch form with the pytest ids of the cases that run it: one row per reachable form, the ids those
    of CASES, whole (so that `pytest -k` takes them), and the bank of the second column that of one of the row's cases."""
    import re
    import test_gpu_gabor_instantiations as gi
    want = {}
    for case in gi.CASES:
        for f in case[1].split(" "):
            want.setdefault(f, []).append(gi.case_id(case))
    rows = {}
    for line in open(os.path.join(os.path.dirname(HERE), "DESIGN.md"), encoding="utf-8"):
        m = re.fullmatch(r"\| `(<[^`]*>g?)` \| (\d+x\d+) [^|]* \| (`.*`) \|\n?", line)
        if m:
            assert m.group(1) not in rows, m.group(1)
            rows[m.group(1)] = re.findall(r"`([^`]+)`", m.group(3))
            assert any(i.startswith(m.group(2) + "_") for i in rows[m.group(1)]), line
    assert rows == want, (sorted(set(rows) ^ set(want)), [f for f in rows if f in want and rows[f] != want[f]])
    assert set(rows) == set(_reachable(lib))
