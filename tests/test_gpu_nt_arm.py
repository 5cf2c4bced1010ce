"""The nontemporal-load arm of every Lloyd pass against exact sums. The split-slab forms of kmeans_pass_mfma_kernel and every form of
kmeans_pass_native_kernel compile their tile load twice, plain and `nt` (csrc/lloyd_pass.h), and the host sends the list positions
below gcs_pass_nt_limit down the `nt` arm - none at all unless a sweep list streams more than 256 MiB, which no other kernel-level
test does. Each case here is the smallest batch of BSD-size hot images (tests/hot_banks.py) that puts BOTH arms into one launch:
0 < nt_limit < nlist with at least G + 1 list positions on either side (G = the launch's workgroups: every workgroup takes each arm
at least once) and nt_limit no multiple of G; for the split banks the tiles below the limit hold flagged and unflagged ones in both
sweep directions (the TOP-run loads have an `nt` form of their own). tests/test_pass_kernel_choice.py proves the first three on the
CPU; the test asserts all of them again.

The reference (tests/lloyd_ref.py: exact_pass) never touches a pass kernel: the canonical features gcs_features_unpack gives (held to
the C oracle here on three images of the batch, and at these banks in tests/test_gpu_value_range.py), distances, sums and counts as
float64 matrix products of integers below 2^53, ties to the lowest index; it is itself held to so.kmeans_assign and
lloyd_ref._pass_reference on 100 000 random pixels of every case. Every comparison is ==.

Seconds per case on an MI355X box (the whole test, host reference included; the file: 28 s): split<1,3,2> 3.4 (with the batch's
set-up, which the next two cases share), its self-updating form 3.0, split<2,5> 1.7, split<1,3> 2.3, its self-updating form 4.1,
split<1,5> 1.2, native<2,3,0> 1.4, native<2,3,6> 1.4, native<3,3,0> 1.5, native<3,3,6> 1.6, native<4,3,6> 2.2, native<4,2,0> 1.7.

Mutants of the library, each built in a scratch copy and run once against this file and against the GPU suite as it was before it.
They copy one staging register over another behind the loads of the `nt` arm only - a load duplicated inside the tile, no address
changed (failed tests: here / before):
(A) stage_load_split, `nt` arm: `st[1] = st[0]` behind the LO / MID loads and `stt[1] = stt[0]` behind the TOP loads: the six split
cases here / 11 of 890 before, every one of them 64 images or 2048 x 2048 on a 4x6-style bank, i.e. split<1,3,2> and its self-updating
form (test_batch_64_global_codebook_every_label of test_gpu_value_range.py, test_gpu_colour_features.py and
test_gpu_feature_smoothing.py; the two batch-64 goldens of test_gpu_golden.py; test_the_timed_batch[global-10] and [per_image-4] of
test_gpu_self_updating_passes.py; four config-3 / config-5 tests of test_distributed.py): split<1,3>, split<1,5>, split<2,5> and the
self-updating split<1,3> were seen by nothing. (A2) the TOP line of (A) alone: the same six here (not run against the suite before).
(B) stage_load of kmeans_pass_native_kernel, `nt` arm: `st[1] = st[0]`: the six native cases here / none of 890 before."""
import time

import numpy as np
import pytest

import hot_banks as hb
from lloyd_ref import _caller_codebook, _pass_reference, as_float64, exact_assign_sums, exact_pass, updated
from slab_layout import flag_bytes, tile_geometry

KEEP_BYTES = 256 << 20             # csrc/lloyd_pass.h: KP_MALL_KEEP_DEFAULT
N_DRAWN = 100000

# id (starts with the name gcs_selftest_pass_kernel gives; banks as in PASS_CASES of tests/pass_cases.py),
# (n_scales, n_orient, ksize, shift, k), (B, H, W), G = workgroups of the launch with ONE global codebook - split<..>: parts * B
# (lloyd_mfma_launch: grid (parts, B), all working); native<NL,MINB,N0>: parts_eff * B (launch_native: 256 * MINB / B working
# workgroups per image) -, what the case runs: "pass" one pass through gcs_kmeans_assign_accumulate, "per_image" that and a pass with
# n_sets = B, "fused" the self-updating form through gcs_kmeans_pass_fused.
NT_CASES = [
    ("split<1,3,2>_D72", (4, 6, 13, 7, 8), (27, 321, 481), 783, "per_image"),
    ("split<1,3,2>_D72_self_updating", (4, 6, 13, 7, 8), (27, 321, 481), 783, "fused"),
    ("split<2,5>_D72", (4, 6, 13, 7, 16), (27, 321, 481), 783, "pass"),
    ("split<1,3>_D30", (2, 5, 11, 7, 8), (40, 321, 481), 800, "pass"),
    ("split<1,3>_D30_self_updating", (2, 5, 11, 7, 8), (40, 321, 481), 800, "fused"),
    ("split<1,5>_D78", (2, 13, 7, 7, 4), (17, 481, 321), 782, "pass"),
    ("native<2,3,0>_D84", (4, 7, 13, 7, 8), (18, 321, 481), 756, "pass"),
    ("native<2,3,6>_D96", (4, 8, 13, 7, 8), (16, 321, 481), 768, "pass"),
    ("native<3,3,0>_D90", (5, 6, 13, 7, 8), (20, 481, 321), 760, "pass"),
    ("native<3,3,6>_D144", (6, 8, 15, 7, 8), (15, 321, 481), 765, "pass"),
    ("native<4,3,6>_D192", (8, 8, 15, 7, 8), (15, 321, 481), 765, "per_image"),
    ("native<4,2,0>_D144", (8, 6, 13, 7, 8), (19, 321, 481), 494, "pass"),
]


def kernel_of(lib, case):
    _, (ns, no, _ks, _shift, k), (_b, h, w), _g, _what = case
    return lib.gcs_selftest_pass_kernel(h, w, ns, no, k).decode()


def launch_workgroups(lib, case):
    """G of the case's launch with one global codebook, restated from the two launchers (see NT_CASES)."""
    _, (ns, no, _ks, _shift, _k), (b, h, w), _g, _what = case
    name = kernel_of(lib, case)
    parts = lib.gcs_kmeans_parts_per_image(b, h, w)
    if name.startswith("split<"):
        return parts * b
    assert name.startswith("native<")
    minb = int(name.split(",")[1])
    need = -(-tile_geometry(lib, h, w, ns, no)[0] * 256 // 262144)           # lloyd_native.hip: native_parts_eff
    return min(max(256 * minb // b, 1, need), parts) * b


def preconditions(lib, case):
    """The three conditions on the global list, through the hook; -> (nt_limit, nlist, ntiles)."""
    case_id, (ns, no, _ks, _shift, k), (b, h, w), g, what = case
    name = kernel_of(lib, case)
    assert case_id == name or case_id.startswith(name + "_"), (case_id, name)
    assert launch_workgroups(lib, case) == g, (case_id, launch_workgroups(lib, case), g)
    ntiles = tile_geometry(lib, h, w, ns, no)[0]
    nlist = ntiles * b
    limit = lib.gcs_selftest_pass_nt_limit(b, h, w, ns, no, k, 1)
    assert 0 < limit < nlist, (case_id, limit, nlist)
    assert limit >= g + 1 and nlist - limit >= g + 1, (case_id, limit, nlist, g)
    assert limit % g != 0, (case_id, limit, g)
    if what == "per_image":
        assert 0 < lib.gcs_selftest_pass_nt_limit(b, h, w, ns, no, k, b) < ntiles, case_id
    if what == "fused":
        assert lib.gcs_kmeans_fused_workspace_bytes(b, h, w, ns, no, k, 1) != 0, case_id
    return limit, nlist, ntiles


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_STAGE = {}


class _Stage:
    """One (bank, batch) on the device: the slab, the canonical features read back from it, 100 000 drawn pixels on the host."""

    def __init__(self, torch, cfg, shape):
        from oracle import c_oracle as co
        b, h, w = shape
        self.bank = hb.hot_bank(*cfg)
        self.seg = hb.hot_segmenter(self.bank)
        ops = self.ops = self.seg.ops
        imgs = hb.hot_images(b, h, w, seed=b + h)
        # a black-region image (flagged beside unflagged tiles) at either end of the list: image 1 is one, the last becomes one
        assert b > 9 + 2 and 9 % len(hb.IMAGE_KINDS) == hb.BLACK_REGION
        imgs[[9, b - 1]] = imgs[[b - 1, 9]]
        self.feats = ops.feature_slab(b, h, w)
        ops.gabor_features(torch.from_numpy(imgs).cuda(), self.feats)
        self.canon = ops.features_unpack(self.feats, b, h, w)                                # (B, D, H, W) int16
        self.d = self.canon.shape[1]
        for i in (0, b // 2, b - 1):                      # unpacked == the C oracle: first, middle and last image of the batch
            want = co.gabor_features(imgs[i], self.bank.tapq, self.bank.shift, self.bank.n_orient)
            assert np.array_equal(self.canon[i].cpu().numpy().view(np.uint16), want), i
        assert int(as_float64(self.canon[0]).max()) >= 32768
        rng = np.random.default_rng(h + 7 * b)
        flat = np.sort(rng.choice(b * h * w, N_DRAWN, replace=False))
        self.drawn = flat
        self.drawn_img = flat // (h * w)
        bi, yi, xi = (torch.from_numpy(v).cuda() for v in (flat // (h * w), flat % (h * w) // w, flat % w))
        self.x_drawn = self.canon[bi, :, yi, xi].cpu().numpy().view(np.uint16).astype(np.int64)       # (n, D)

    def check_reference(self, torch, book, ref_lab):
        """exact_assign_sums on the drawn pixels (on the host) == _pass_reference (so.kmeans_assign, int64 sums); the batch's
        reference labels at those pixels == the same."""
        x = self.x_drawn
        vote = np.random.default_rng(1).random(len(x)) < 0.5
        want_lab, want_sums, want_cnt = _pass_reference(x[None], book, vote[None])
        lab, [(sums, cnt)] = exact_assign_sums(torch.from_numpy(x.T.astype(np.float64)), torch.from_numpy(book[0].astype(np.float64)),
                                               [torch.from_numpy(vote)])
        assert np.array_equal(lab.numpy(), want_lab[0])
        assert np.array_equal(sums.numpy().astype(np.int64), want_sums[0]) and np.array_equal(cnt.numpy().astype(np.int64), want_cnt[0])
        got = ref_lab.reshape(-1)[torch.from_numpy(self.drawn).cuda()].cpu().numpy()
        assert np.array_equal(got, want_lab[0])
        return want_lab[0]


def _stage(torch, cfg, shape):
    key = (cfg, shape)
    if key not in _STAGE:
        _STAGE.clear()                                       # one batch on the device at a time
        torch.cuda.empty_cache()
        _STAGE[key] = _Stage(torch, cfg, shape)
    return _STAGE[key]


def _both_kinds_below_the_limit(st, shape, limit, nlist, ntiles):
    """Among the tiles a sweep loads `nt` - physical list positions [0, limit) forward, [nlist - limit, nlist) in reverse - there are
    flagged and unflagged ones."""
    b, h, w = shape
    words, n = flag_bytes(st.seg, st.feats, b, h, w)
    assert n == ntiles
    flagged = words.any(axis=2).reshape(-1)                                                  # [image][tile] = the global list
    for name, part in (("forward", flagged[:limit]), ("reverse", flagged[nlist - limit:])):
        assert part.any() and not part.all(), (name, int(part.sum()), len(part))


@pytest.mark.parametrize("case", NT_CASES, ids=[c[0] for c in NT_CASES])
def test_both_load_arms_in_one_launch(torch_cuda, case):
    """See the module docstring. "pass": one pass from a caller-made codebook (a tie, extreme rows), one global codebook, forward and
    reverse, whole images and a row window (labelled-but-not-voting rows meet the `nt` arm): labels, sums and counts after
    gcs_kmeans_reduce and the centroids of gcs_kmeans_reduce_finalize == the reference. "per_image": also with n_sets = B, where the
    limit is per image list. "fused": three direct gcs_kmeans_pass_fused calls on a zeroed workspace, read back after every pass
    through tests/fused_workspace.py: the centroids == the update of the exact assignment of the pass before, the sums the pass left
    == the exact ones, the final labels == the reference's."""
    torch = torch_cuda
    t_start = time.perf_counter()
    case_id, (ns, no, ks, shift, k), shape, g, what = case
    b, h, w = shape
    st = _stage(torch, (ns, no, ks, shift), shape)
    ops, d = st.ops, st.d
    lib = ops.lib
    limit, nlist, ntiles = preconditions(lib, case)
    split = case_id.startswith("split<")
    if split:
        _both_kinds_below_the_limit(st, shape, limit, nlist, ntiles)
    book = _caller_codebook(st.x_drawn, k)[None]
    assert book.max() >= 32768

    if what == "fused":
        _fused_loop(torch, st, shape, k, book)
        print("%s: %.1f s" % (case_id, time.perf_counter() - t_start))
        return

    labels, partials = ops.label_slab(b, h, w), ops.partial_slab(b, h, w, k)
    window = (h // 4, h - h // 5)

    def run(cent_np, n_sets, rows, reverse, want_lab, want_sums, want_cnt):
        tag = (case_id, n_sets, rows, reverse)
        cent = torch.from_numpy(cent_np.astype(np.uint16).view(np.int16)).cuda().contiguous()
        sums = ops.new_sums(n_sets, k)
        labels.fill_(255)
        partials.zero_()
        ops.assign_accumulate(st.feats, cent, b, h, w, k, n_sets, labels, partials, rows=rows, reverse=reverse)
        ops.reduce(partials, b, h, w, k, n_sets, sums)
        got_lab = labels[:b * h * w].view(b, h, w)
        assert torch.equal(got_lab, want_lab), (tag, int((got_lab != want_lab).sum()))
        got = sums.cpu().numpy()
        assert np.array_equal(got[:, :, -1], want_cnt), tag
        assert np.array_equal(got[:, :, :-1], want_sums), tag
        new = cent.clone()
        ops.reduce_finalize(partials, b, h, w, k, n_sets, ops.new_sums(n_sets, k), new)
        assert np.array_equal(new.cpu().numpy().view(np.uint16), updated(want_sums, want_cnt, cent_np)), tag

    ref_lab, [whole, windowed] = exact_pass(st.canon, book, [(0, h), window])
    at_drawn = st.check_reference(torch, book, ref_lab)
    assert whole[1].sum() == b * h * w and windowed[1].sum() == b * (window[1] - window[0]) * w
    assert whole[1][0, 1] == 0 and not (at_drawn == 1).any()                # the duplicate row: the lowest index won every tie
    for reverse in (False, True):
        run(book, 1, (0, h), reverse, ref_lab, *whole)
        run(book, 1, window, reverse, ref_lab, *windowed)
    if what == "per_image":
        books = np.stack([_caller_codebook(st.x_drawn[st.drawn_img == i], k) for i in range(b)])
        ref_lab, [whole] = exact_pass(st.canon, books, [(0, h)])
        assert (whole[1].sum(axis=1) == h * w).all()
        for reverse in (False, True):
            run(books, b, (0, h), reverse, ref_lab, *whole)
    print("%s: %.1f s" % (case_id, time.perf_counter() - t_start))


def _fused_loop(torch, st, shape, k, book):
    import fused_workspace as fw
    b, h, w = shape
    ops, d = st.ops, st.d
    parts = int(ops.lib.gcs_kmeans_parts_per_image(b, h, w))
    lay = (1, fw.fold_rows(b, parts, 1, fw.env_fold_rows()), k, d)
    ws = ops.fused_workspace(b, h, w, k, 1)
    assert ws is not None and ws.numel() == fw.workspace_bytes(*lay)
    # the reference is itself checked on the drawn pixels, with the caller-made codebook (the loop makes its own centroids)
    st.check_reference(torch, book, exact_pass(st.canon, book, [(0, h)])[0])
    pixels = torch.tensor([((2 * j + 1) * h * w) // (2 * k) for j in range(k)], device="cuda")           # SPEC.md §4 init: image 0
    cent = as_float64(st.canon[0].reshape(d, -1)[:, pixels]).T.cpu().numpy().astype(np.int64)[None]     # (1, k, D)
    n_iter = 3
    for t in range(n_iter):
        last = t == n_iter - 1
        ref_lab, [(sums, cnt)] = exact_pass(st.canon, cent, [(0, h)])
        got_cent = torch.full((1, k, d), -1, dtype=torch.int16, device="cuda")
        out = torch.full((b, h, w), 99, dtype=torch.uint8, device="cuda") if last else None
        if last:
            ops.assign_raster(st.feats, got_cent, b, h, w, k, 1, out, reverse=bool(t & 1), fused=(ws, t))
        else:
            ops.assign_accumulate(st.feats, got_cent, b, h, w, k, 1, None, None, reverse=bool(t & 1), fused=(ws, t))
        v = fw.views(ws.cpu().numpy(), *lay)
        assert np.array_equal(got_cent.cpu().numpy().view(np.uint16), cent), t
        assert np.array_equal(v.cents[t & 1], cent), t
        if last:
            assert torch.equal(out, ref_lab), (t, int((out != ref_lab).sum()))
            assert fw.is_as_found(ws.cpu().numpy(), *lay)
        else:
            total = fw.totals(v.sums[t % 3])
            assert np.array_equal(total[:, :, -1], cnt) and np.array_equal(total[:, :, :-1], sums), t
            cent = updated(sums, cnt, cent)
