"""Every reachable gabor_mfma_kernel<MT, GQ, KS, LVL, FAST, SPLIT> instantiation and launch form against the C oracle, bit for bit.
gcs_gabor_features picks one of 90 compiled instantiations per launch (csrc/gabor_plan.h); over n_scales 1..8, n_scales * n_orient
<= 70, odd ksize 1..15, shift 7 / 8, small and not-small calls the plan reaches 83 of them, 107 launch forms when the grouped launch
(grid.y row-tile groups, "g" behind the instantiation) counts separately. CASES is a greedy cover of those 107 forms computed from the
hook gcs_selftest_gabor_plan; no case is redundant, and tests/test_gabor_kernel_choice.py asserts on the CPU that the union of the
forms named here IS the reachable set, that every case names exactly what the hook answers for it, and the preconditions below.

A case is (n_scales, n_orient, ksize, shift, small) with a hot bank and the hot images of tests/hot_banks.py (values across every
nibble of both slab formats; each case asserts its reference holds values >= 4096) and covers every launch of its plan. The banks
are hot_bank(..., odd="turned"): with the default bank the odd scale of a level has no taps in the outer two rows of its frame, and
a form whose only launch here holds odd-scale filters alone (a quarter of them: the trailing launches of wide levels) would
multiply zeros in its first and last K-step. Turned, every filter of every launch has taps in every K-step (asserted on the CPU).
  small      2 images of 72 x 88: every tile of both levels fits the resident slots (fused or grouped launch forms), level 0 has 9
             half tiles (an absent second half), rows and columns end inside a 32 x 32 half tile.
  not small  images of 35 x 36 (two level-0 tiles, one tile on every other level), the smallest batch with which every fused list
             of the plan has more tiles than workgroups - a persistent workgroup walks several tiles through the double-buffered
             LDS - and some workgroup's walk crosses a level boundary, and with which some launch of a plan without fused lists
             has more tiles than workgroups: at 256 compute units 257 images for a two-level bank, 171 for a five-scale bank (a
             list of levels 0 and 1, then level 2) and 129 for a seven-scale one (levels 0 to 2, then level 3).
             inputs_for derives the batch for the device's own compute-unit count; the test asserts the plan of the very call it
             makes holds the forms of its id.
Known limit: the walk condition is met at its minimum. In a two-level case only the LVL = 0 launches walk (514 tiles on 512
workgroups: two workgroups take a second tile); every LVL = 1 launch has 257 tiles for 512 workgroups, so no LVL = 1 instantiation
goes through the double-buffered second tile in this file (the batch-64 tests of tests/test_gpu_golden.py and
tests/test_gpu_value_range.py do: 1280 level-1 tiles on 512 workgroups, for the forms of their own banks only).
The features go into a slab filled with 0x5a, come back through gcs_features_unpack and are compared with == to
oracle.c_oracle.gabor_features, image by image.

Seconds per case on an MI355X box (the whole test; the C oracle runs on eight threads): the small cases up to 0.06, the others 0.14
(5x2, 7x2) - 1.1 (4x14: 257 images, 168 planes), most of it the oracle; the file: 19 s.

Mutants of the library, run once and not kept. Each changes values only - a bias register or an A fragment behind its load in
enter_level of gabor_mfma_kernel - never an address, a bound, a barrier or a wait. All four were built into ONE library, not one
library each: `if constexpr` confines them to pairwise disjoint sets of instantiations, so a failing case names its mutant.
(M1) LVL == -2: level 1's bias of the launch's first two filters + 256.
(M2) <3,1,7,1,*,false> (a wide level-1 launch of three tiles, one filter pair in the last): that pair's bias + 256.
(M3) <2,1,8,1,*,*>: the last K-step's A fragments (frame rows 14 and 15) zero.
(M4) <1,2,7,0,false,*>, second group of a grouped launch (blockIdx.y == 1): the bias of its second filter pair + 256.
That library against this file: 7 cases failed, 48 passed. M1: 4x9_ks13_shift8_small, 4x11_ks13_shift7_small. M2:
4x11_ks13_shift7_walk. M3: 4x3_ks15_shift7_walk and 4x7_ks15_shift8_walk (the latter runs the form on odd-scale filters alone and
passed the mutant while its bank was the inset one). M4: 3x8_ks13_shift7_small, 3x12_ks13_shift7_small.
The same library against the GPU suite as it was before this file (902 tests): 901 passed. No test that names its bank failed -
M2, M3 and M4 went unseen by all of them - and one test failed by the luck of its draw:
test_gpu_parity.py::test_randomised_shapes_banks_and_codebooks_against_the_c_oracle, 3 of its 60 random cases. The two of them that
its output keeps are 4x9 banks on one tiny image (31 x 11, 34 x 24), small calls that take LVL = -2, wrong in planes 18 and 19 of
every channel: M1. (The third lies in front of the 3000 characters the test prints.)"""
import concurrent.futures
import time

import numpy as np
import pytest

import gabor_plan_ref as gp
import hot_banks as hb

SMALL_SHAPE = (72, 88)
WALK_SHAPE = (35, 36)

# (n_scales, n_orient, ksize, shift, small), the launch forms of the case's plan (what gcs_selftest_gabor_plan answers, sorted)
CASES = [
    ((3, 1, 13, 7, 0), '<1,1,7,0,false,true> <1,1,7,1,false,true>'),
    ((3, 5, 13, 7, 0), '<2,1,7,1,false,true> <3,1,7,0,false,true>'),
    ((3, 7, 13, 7, 0), '<2,1,7,0,false,true> <2,2,7,0,false,true> <2,2,7,1,false,true>'),
    ((3, 8, 13, 7, 1), '<1,2,7,0,false,true>g <1,2,7,1,false,true>g'),
    ((3, 8, 13, 8, 1), '<1,2,7,0,true,true>g <1,2,7,1,true,true>g'),
    ((3, 8, 15, 7, 1), '<1,2,8,0,false,true>g <1,2,8,1,false,true>g'),
    ((3, 8, 15, 8, 1), '<1,2,8,0,true,true>g <1,2,8,1,true,true>g'),
    ((3, 9, 15, 7, 0), '<1,1,8,0,false,false> <1,1,8,1,false,false> <2,2,8,0,false,false> <2,2,8,1,false,false>'),
    ((3, 12, 13, 7, 1), '<1,2,7,0,false,false>g <1,2,7,1,false,false>g'),
    ((3, 12, 13, 8, 1), '<1,2,7,0,true,false>g <1,2,7,1,true,false>g'),
    ((3, 12, 15, 7, 1), '<1,2,8,0,false,false>g <1,2,8,1,false,false>g'),
    ((3, 12, 15, 8, 1), '<1,2,8,0,true,false>g <1,2,8,1,true,false>g'),
    ((4, 1, 13, 7, 1), '<1,1,7,-1,false,true>'),
    ((4, 1, 15, 7, 1), '<1,1,8,-1,false,true>'),
    ((4, 2, 13, 7, 0), '<1,2,7,0,false,true> <1,2,7,1,false,true>'),
    ((4, 2, 13, 7, 1), '<1,2,7,-1,false,true>'),
    ((4, 2, 13, 8, 0), '<1,2,7,0,true,true> <1,2,7,1,true,true>'),
    ((4, 2, 13, 8, 1), '<1,2,7,-1,true,true>'),
    ((4, 2, 15, 7, 0), '<1,2,8,0,false,true> <1,2,8,1,false,true>'),
    ((4, 2, 15, 7, 1), '<1,2,8,-1,false,true>'),
    ((4, 2, 15, 8, 1), '<1,2,8,-1,true,true>'),
    ((4, 3, 13, 7, 1), '<2,1,7,-1,false,true>'),
    ((4, 3, 15, 7, 0), '<2,1,8,0,false,true> <2,1,8,1,false,true>'),
    ((4, 3, 15, 7, 1), '<2,1,8,-1,false,true>'),
    ((4, 4, 13, 7, 1), '<1,2,7,-1,false,true>g'),
    ((4, 4, 13, 8, 0), '<2,2,7,0,true,true> <2,2,7,1,true,true>'),
    ((4, 4, 13, 8, 1), '<1,2,7,-1,true,true>g'),
    ((4, 4, 15, 7, 1), '<1,2,8,-1,false,true>g'),
    ((4, 4, 15, 8, 1), '<1,2,8,-1,true,true>g'),
    ((4, 5, 13, 7, 0), '<3,1,7,0,false,true> <3,1,7,1,false,true>'),
    ((4, 5, 15, 7, 0), '<1,1,8,0,false,true> <1,1,8,1,false,true> <2,2,8,0,false,true> <2,2,8,1,false,true>'),
    ((4, 6, 13, 7, 0), '<3,2,7,0,false,true> <3,2,7,1,false,true>'),
    ((4, 6, 13, 8, 0), '<3,2,7,0,true,true> <3,2,7,1,true,true>'),
    ((4, 6, 15, 8, 0), '<1,2,8,0,true,true> <1,2,8,1,true,true> <2,2,8,0,true,true> <2,2,8,1,true,true>'),
    ((4, 7, 13, 7, 0), '<2,1,7,0,false,false> <2,1,7,1,false,false> <2,2,7,0,false,false> <2,2,7,1,false,false>'),
    ((4, 7, 15, 8, 0), '<2,1,8,0,false,false> <2,1,8,1,false,false> <2,2,8,0,true,false> <2,2,8,1,true,false>'),
    ((4, 8, 13, 7, 1), '<1,2,7,-1,false,false>g'),
    ((4, 8, 13, 8, 1), '<1,2,7,-1,true,false>g'),
    ((4, 8, 15, 7, 1), '<1,2,8,-1,false,false>g'),
    ((4, 8, 15, 8, 1), '<1,2,8,-1,true,false>g'),
    ((4, 9, 13, 8, 1), '<2,1,7,-1,false,false> <3,2,7,-2,true,false>'),
    ((4, 10, 13, 8, 0), '<2,2,7,0,true,false> <2,2,7,1,true,false> <3,2,7,0,true,false> <3,2,7,1,true,false>'),
    ((4, 10, 15, 7, 0), '<1,2,8,0,false,false> <1,2,8,1,false,false> <2,2,8,0,false,false> <2,2,8,1,false,false>'),
    ((4, 10, 15, 8, 0), '<1,2,8,0,true,false> <1,2,8,1,true,false> <2,2,8,0,true,false> <2,2,8,1,true,false>'),
    ((4, 11, 13, 7, 0), '<3,1,7,0,false,false> <3,1,7,1,false,false> <3,2,7,0,false,false> <3,2,7,1,false,false>'),
    ((4, 11, 13, 7, 1), '<3,1,7,-2,false,false> <3,2,7,-2,false,false>'),
    ((4, 13, 13, 7, 0), '<1,1,7,0,false,false> <1,1,7,1,false,false> <3,2,7,0,false,false> <3,2,7,1,false,false>'),
    ((4, 14, 13, 7, 0), '<1,2,7,0,false,false> <1,2,7,1,false,false> <3,2,7,0,false,false> <3,2,7,1,false,false>'),
    ((4, 14, 13, 8, 0), '<1,2,7,0,true,false> <1,2,7,1,true,false> <3,2,7,0,true,false> <3,2,7,1,true,false>'),
    ((5, 2, 13, 7, 0), '<1,1,7,-1,false,false> <1,2,7,-1,false,false>'),
    ((7, 2, 15, 7, 0), '<1,1,8,-1,false,false> <1,2,8,-1,false,false>'),
    ((5, 4, 13, 8, 0), '<1,2,7,-1,true,false> <2,2,7,-1,true,false>'),
    ((7, 4, 15, 8, 0), '<1,2,8,-1,true,false> <2,2,8,-1,true,false>'),
    ((5, 5, 13, 7, 0), '<1,1,7,-1,false,false> <2,1,7,-1,false,false> <2,2,7,-1,false,false>'),
    ((7, 5, 15, 7, 0), '<1,1,8,-1,false,false> <2,1,8,-1,false,false> <2,2,8,-1,false,false>'),
]


def case_id(case):
    (ns, no, ks, shift, small), forms = case
    return "%dx%d_ks%d_shift%d_%s-%s" % (ns, no, ks, shift, "small" if small else "walk", forms.replace(" ", "+"))


def case_bank(cfg):
    """The case's bank: hot taps whose odd scales are turned, not inset, so that every filter has taps in every K-step of its frame
    (module docstring; tests/test_gabor_kernel_choice.py asserts it for every launch of every case)."""
    return hb.hot_bank(*cfg[:4], odd="turned")


def plan_forms(lib, cfg, batch, cu_count):
    ns, no, ks, shift, _small = cfg
    return sorted({gp.form(l) for l in gp.bank_launches(gp.plan(lib, *batch, ns, no, ks, shift, cu_count, 1))})


def unmet(lib, cfg, batch, cu_count):
    """The conditions (module docstring) the batch (B, H, W) does NOT meet for this case on `cu_count` compute units; [] = all met.
    Tile counts and the small-call rule come from the restatement (tests/gabor_plan_ref.py), the launches from the hook."""
    ns, no, ks, shift, small = cfg
    b, h, w = batch
    bad = []
    launches = gp.bank_launches(gp.plan(lib, b, h, w, ns, no, ks, shift, cu_count, 1))
    is_small = gp.fuse_small(b, h, w, ns, no, cu_count)
    if small:
        if not is_small:
            bad.append("every tile of both levels fits the resident slots")
        if b < 2:
            bad.append("at least two images")
        if not any(n % 2 for n in gp.half_tiles(h, w, ns)):
            bad.append("a level with an odd half-tile count")
        if h % 32 == 0 or w % 32 == 0:
            bad.append("rows and columns end inside a half tile")
        return bad
    if is_small:
        bad.append("not a small call")
    if not any(l.tiles > l.grid_x for l in launches):
        bad.append("a launch with more tiles than workgroups")
    for l in launches:
        if l.l1 - l.l0 > 1:
            total, grid_x, ends = gp.list_geometry(b, h, w, ns, l.l0, l.l1, cu_count)
            assert (total, grid_x) == (l.tiles, l.grid_x), (cfg, batch, l)
            if not gp.walk_crosses_a_level(total, grid_x, ends):
                bad.append("a walk across a level boundary in the list of levels %d:%d" % (l.l0, l.l1))
    return bad


def inputs_for(lib, cfg, cu_count):
    """(B, H, W) of the case on a device of `cu_count` compute units: the smallest batch that meets every condition."""
    if cfg[4]:
        batch = (2,) + SMALL_SHAPE
        assert not unmet(lib, cfg, batch, cu_count), (cfg, cu_count, unmet(lib, cfg, batch, cu_count))
        return batch
    for b in range(1, 4097):
        if not unmet(lib, cfg, (b,) + WALK_SHAPE, cu_count):
            return (b,) + WALK_SHAPE
    raise AssertionError(("no batch meets the conditions", cfg, cu_count))


pytestmark = pytest.mark.gpu
_REF = {}
_POOL = []


def _ref_features(cfg, imgs):
    """C-oracle features (B, D, H, W) uint16 of a hot bank, cached per (bank, images), never modified."""
    from oracle import c_oracle as co
    key = (cfg, imgs.shape, imgs.tobytes())
    if key not in _REF:
        if len(_REF) > 2:
            _REF.pop(next(iter(_REF)))
        if not _POOL:
            _POOL.append(concurrent.futures.ThreadPoolExecutor(8))
        bank = case_bank(cfg)
        ref = np.stack(list(_POOL[0].map(lambda im: co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient), imgs)))
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_launch_of_the_plan_equals_the_oracle(torch_cuda, case):
    torch = torch_cuda
    t0 = time.time()
    cfg, forms = case
    seg = hb.hot_segmenter(case_bank(cfg))
    ops, lib = seg.ops, seg.ops.lib
    cu = lib.gcs_device_cu_count()
    b, h, w = batch = inputs_for(lib, cfg, cu)
    # the plan of the very call below (cu_count = 0: the device's own) holds the forms this case is responsible for
    assert plan_forms(lib, cfg, batch, 0) == forms.split(" "), (case_id(case), batch, cu, plan_forms(lib, cfg, batch, 0))
    imgs = hb.hot_images(b, h, w, seed=h + w + cfg[1])
    ref = _ref_features(cfg[:4], imgs)
    assert ref.max() >= 4096 and (ref >= 4096).mean() > 0.25, (int(ref.max()), float((ref >= 4096).mean()))
    feats = ops.feature_slab(b, h, w)
    feats.fill_(0x5a)
    ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
    got = ops.features_unpack(feats, b, h, w).cpu().numpy().view(np.uint16)
    assert got.shape == ref.shape
    for i in range(b):
        if not np.array_equal(got[i], ref[i]):
            plane, y, x = (int(v) for v in np.argwhere(got[i] != ref[i])[0])
            n_bad = int((got != ref).sum())
            raise AssertionError("%s %s: %d values differ; first at image %d plane %d y %d x %d: got %d, want %d" %
                                 (case_id(case), batch, n_bad, i, plane, y, x, got[i, plane, y, x], ref[i, plane, y, x]))
    print("%s %s: %.2f s" % (case_id(case), batch, time.time() - t0))
