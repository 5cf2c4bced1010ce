"""The self-updating Lloyd pass (gcs_kmeans_pass_fused: the two FUSED instantiations of kmeans_pass_mfma_kernel) stage by stage.
One launch does what four kernels did - init, assign + sums, the fold of the shared rows, the SPEC.md §4 update - and keeps a
three-buffer rotation going; tests/test_gpu_self_updating_passes.py sees all of it only through the final labels. Here every launch
starts from a workspace the test has written (tests/fused_stages.py) and every piece of the workspace is compared afterwards, bit
for bit, with the model of tests/fused_workspace.py (so.kmeans_init, so.kmeans_assign, int64 sums, the update in Python integers;
the model itself is checked against the oracle without a GPU in tests/test_fused_workspace.py): the sums and counts in the shared
rows, the centroids in `cent` and in the array the pass writes, the array and the buffer it must keep, the buffer it must clear
(filled with non-zero bytes before), the ticket and the padding. The written sums are those of _update_cases (0.5-ties, 32767.5,
46339, n = 1, n = 64 * 481 * 321 so that 2 S + n passes 2^38, empty clusters between full ones); features are the C oracle's on the
banks and images of tests/hot_banks.py (values >= 32768, flagged beside unflagged tiles), and the tests assert that their inputs
hold all that.

Mutants of csrc/lloyd_mfma.hip, each built in a scratch copy, run once against this file and once against
tests/test_gpu_self_updating_passes.py as it was before this file (failed tests: here / there):
(1) the prologue's fold keeps the sum in 32 bits: 23 / 0; (2) `s / c` in place of `(2 s + c) / (2 c)`: 38 / 22; (3) an empty cluster
reads the centroid array the pass writes: 39 / 1; (4) the prologue's clear drops the gridDim.y factor (per-image: set 0 only):
39 / 8; (5) the last workgroup of the grid skips its atomic adds: 42 / 23; (6) workgroup 0 adds one pixel too many to every count:
42 / 22; (7) the fold reads row 0 only: 3 / 0 (the three child processes with more than one row); (8) the last workgroup's clear
stops one element short: 40 / 17; (9) `cent` is written for set 0 only: 39 / 1. Of 42 tests here and 29 there: the suite before
let (1) and (7) through and saw (3) and (9) in one test each."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_stages as fs
import hot_banks as hb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


# (n_scales, n_orient, ksize, shift): level 0 holds 32 planes or more (the L0T = 2 instantiation) ...
BANKS_L0T2 = [(4, 6, 13, 7), (4, 6, 13, 8), (2, 6, 13, 8), (2, 8, 13, 7), (1, 16, 11, 7), (3, 7, 13, 8)]
# ... or fewer (L0T = 0)
BANKS_L0T0 = [(4, 5, 13, 7), (2, 5, 11, 7), (3, 3, 9, 8), (1, 4, 9, 7), (1, 1, 15, 7)]
ALL_K = [(4, 6, 13, 7), (2, 5, 11, 7)]
CASES = [(cfg, k) for cfg in BANKS_L0T2 + BANKS_L0T0 for k in (range(1, 9) if cfg in ALL_K else (3, 8))]
# (B, H, W): three images; both packed strips; no strip; one tile; one image
SHAPES = [(3, 41, 74), (2, 81, 121), (1, 64, 96), (3, 9, 10), (1, 41, 74)]


def _images(b, h, w):
    """b hot images; a single image is the one with a black region (flagged beside unflagged tiles)."""
    imgs = hb.hot_images(max(b, 2), h, w, seed=h + w)
    return imgs[hb.BLACK_REGION:hb.BLACK_REGION + 1] if b == 1 else imgs[:b]


def _level0_planes(cfg):
    return 3 * cfg[1] * min(2, cfg[0])


@pytest.mark.parametrize("cfg,k", CASES, ids=["%dx%d_ks%d_shift%d_k%d" % (c + (k,)) for c, k in CASES])
def test_one_pass_from_a_written_workspace(torch_cuda, cfg, k):
    """(a) pass t = 1 .. 4 (every residue of the rotation, both centroid arrays) from the state 'as pass t - 1 left it', not last:
    `cent` and array t & 1 = floor((2 S + n) / (2 n)) in Python integers, an empty cluster keeps the centroid of array (t - 1) & 1;
    that array and buffer (t - 1) % 3 unchanged; buffer (t + 1) % 3 zero in every byte of every set; buffer t % 3 = the exact
    sums and counts of the oracle's features assigned to those centroids; ticket 0. (b) the same state as the LAST pass: labels as
    int32 and uint8 raster, buffer t % 3 still zero, buffer (t - 1) % 3 cleared, ticket 0. (c) pass 0: the init pixels of every
    set and the exact sums; as the only pass, nothing but the centroids and the labels. Both sweep directions give the same bits.
    Every shape of SHAPES, both codebook modes; all four t on the first shape, one on each of the others."""
    assert (_level0_planes(cfg) >= 32) == (cfg in BANKS_L0T2)
    hot = mixed = 0
    held = {}
    for si, (b, h, w) in enumerate(SHAPES):
        st = fs.stage(torch_cuda, cfg, _images(b, h, w))
        hot += st.x.max() >= 32768
        mixed += st.mixed_tiles()
        if h * w > 1000:
            assert st.x.max() >= 32768 and st.mixed_tiles(), (b, h, w, int(st.x.max()))
        for mode in ("global", "per_image") if b > 1 else ("global",):
            for t in (1, 2, 3, 4) if si == 0 else (1 + (si + k) % 4,):
                for last in (False, True):
                    hold = fs.check_written_pass(st, mode, k, t, last, (cfg, (b, h, w)))
                    held = {key: held.get(key, False) or v for key, v in hold.items()}
            for last in (False, True):
                fs.check_pass0(st, mode, k, last, (cfg, (b, h, w)))
    assert hot >= 4 and mixed >= 4, (hot, mixed)
    if k >= 6 and 3 * cfg[0] * cfg[1] >= 8:
        assert all(held.values()), held


def test_hundreds_of_workgroups_add_into_one_row(torch_cuda):
    """B = 64 at 72 x 104 with one global codebook: every workgroup of the grid adds into the same k * (D + 1) addresses, and one of
    them publishes the centroids. Passes 0 and 1, and pass 2 as the last one (the ticket over the whole grid)."""
    cfg, k, (b, h, w) = (4, 6, 13, 7), 8, (64, 72, 104)
    st = fs.stage(torch_cuda, cfg, hb.hot_images(b, h, w, seed=0))
    assert b * st.parts >= 512 and st.layout("global", k)[1] == 1, st.parts
    assert st.x.max() >= 32768 and st.mixed_tiles()
    fs.check_pass0(st, "global", k, False, "B=64")
    fs.check_written_pass(st, "global", k, 1, False, "B=64", need_inputs=True)
    fs.check_written_pass(st, "global", k, 2, True, "B=64", need_inputs=True)


def _loop_images(h, w):
    """Three hot images, a constant image and a two-colour image (fewer distinct pixels than k: empty clusters, pass after pass)."""
    flat = np.full((h, w, 3), 90, np.uint8)
    two = flat.copy()
    two[:, w // 2:] = (200, 30, 120)
    return np.concatenate([hb.hot_images(3, h, w, seed=3), flat[None], two[None]])


@pytest.mark.parametrize("mode", ["per_image", "global"])
@pytest.mark.parametrize("cfg,k", [((4, 6, 13, 7), 8), ((2, 5, 11, 7), 5)], ids=["4x6_k8", "2x5_k5"])
def test_a_loop_watched_from_inside(torch_cuda, cfg, k, mode):
    """(e) five direct calls on a zeroed workspace, the whole workspace read back after each: the buffer a pass added into holds the
    exact sums for the centroids it used, its centroids are so.kmeans_update of the pass before, and the loop ends on the C oracle's
    labels with the workspace as it was found."""
    st = fs.stage(torch_cuda, cfg, _loop_images(64, 96))
    want = fs.check_loop(st, mode, k, 5, cfg)
    assert st.x.max() >= 32768
    if mode == "per_image":
        assert len(np.unique(want[3])) == 1 and (k < 8 or len(np.unique(want[4])) < 8)       # the constant and the two-colour image


@pytest.mark.parametrize("value", [2, 7, 64])
def test_more_than_one_shared_row(torch_cuda, value):
    """(f) GCS_KP_FOLD_ROWS = 2, 7, 64 (read once per process, hence a child: tests/checkers/fold_rows_child.py, one at a time,
    never retried): the workspace grows with the rows, written shares spread over all rows fold to the exact centroids, the rows a
    pass adds into hold the exact total on more than one row, and whole loops equal the C oracle."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "checkers", "fold_rows_child.py")
    env = dict(os.environ, GCS_KP_FOLD_ROWS=str(value))
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, f"child ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith(f"OK fold rows {value}"), r.stdout[-2000:]
    print(last)
