"""Slab kernels where byte offsets pass 2^31 and 2^32. No other test builds a feature slab above 0.9 GB, so a slab pointer, a tile
index times tile_bytes or `b * img_bytes` computed in 32 bits anywhere would pass the whole suite and label a 5 GB batch wrongly.

Part 1 - batches whose slab crosses both lines (tests/large_offsets.py: 81 x 130, B the smallest count with B * img_bytes >= 2^32 +
2^27: 4 576 images on the 4x6 bank, 3 391 on 3x9, 2 888 on 8x8, 2 324 on 7x10, 4.13 GiB each). The batch is base[idx]: sixteen hot
images (tests/hot_banks.py, every kind twice, `black_region` among them: flagged and unflagged split-slab tiles on both sides of
each line) in a fixed pseudo-random order in which the images below, across and above each line are three different base images.
Every entry point runs on the sixteen images alone, that small result is held to the existing references (the C oracle,
lloyd_ref._pass_reference / updated, smooth_ref, position_ref, feature_gradient_ref, gcs_region_tree on canonical features), and the
large run must equal the small one through idx: every byte of the slab (flag words and padding included: both slabs start as
0xA5), every label, every per-image sum; global sums == sum_j multiplicity_j * sums_j in int64. Comparisons run on the device in
chunks of images and leave out nothing.

Part 2 - ONE image whose own slab passes 2^31 (see there): (a) 47 000 x 1000 on the 4x6 bank, 4 230 740 224 bytes = 0.985 x 2^32
(top_off = 1.48 x 2^31), (b) 17 000 x 1000 on the 8x8 bank, 1.009 x 2^31: a pattern of 64 rows stacked; the reference is the slab's
own period between the ends and two crops, held to the C oracle (and tests/smooth_ref.py), at the ends. Both run gcs_gabor_features,
one Lloyd pass in both directions and gcs_smooth_features in place; (a) also the self-updating loop of three passes.

Entry points that take a feature slab (gabor_color_image_segmentation_amd/_lib.py: SIGNATURES) - covered here: gcs_gabor_features,
gcs_kmeans_assign_accumulate (+ gcs_kmeans_reduce), gcs_kmeans_assign_raster, gcs_kmeans_pass_fused, gcs_smooth_features,
gcs_position_features, gcs_feature_gradient, gcs_region_tree_slab, and Segmenter.segment_device above them. NOT covered, and
unverified above 4 GiB: gcs_features_unpack, gcs_features_gather and gcs_kmeans_init. They run here on the sixteen images and on the
crops only: called one after the other on the 4.13 GiB slab of the 3x9 bank (the last with n_sets = B = 3 391) they end in a GPU
memory fault whose cause is not known - every product in gcs_slab_value, gcs_slab_offset and the three kernels is 64-bit, and the
same calls on the 4x6 bank's slab give the right values - and a test may not run them there until it is. Part 2 therefore reads
no canonical tensor of the tall images; gcs_feature_gradient and gcs_region_tree_slab take H <= 4096 and cannot run on them; the
tall images have no packed strips (part 1 has them).

Seconds on an MI355X (the file: 20 s, every test below 24 GiB at its peak - asserted -, the largest 9.4 GiB): a bank's set-up 1.7
(twice 4.13 GiB written); the slab of a bank 0.2 - 0.3; one pass, each of the six kernels 0.4 - 1.1; the self-updating loop 0.6;
smoothing 0.3 / 0.5; position, edge map and tree 0.2 / 0.3; the segmenter 0.7; the tall images: Gabor and one pass 1.2 (a) and 2.9
(b, the host reference of 192 features), smoothing 0.6 / 1.4, the self-updating loop 2.6.

Mutants of the library, each built in a scratch copy and run once against this file (failed of 21). Every one truncates without
a sign, so every address it forms is below the right one by a multiple of 2^32 or 2^31 and not below the slab's start:
(1) gabor.hip, the image base `(size_t)b * img_bytes` kept in `unsigned` (three places): an image past 2^32 is stored at its offset
minus 2^32, i.e. at most 2^27 + img_bytes into a slab of more than 2^32 + 2^27 bytes: 16 failed (all of part 1; part 2 has b = 0).
(3) lloyd_native.hip, `(size_t)tile * lo.tile_bytes` kept in `unsigned` (loads only; offset + tile_bytes <= 2^32 + tile_bytes): 1
failed, test_one_lloyd_pass[native<4,3,6>].
(4) lloyd_mfma.hip, `mid_rel_l & 0x7fffffff` at the load: none failed (of the 18 tests the file had then), and none can: mid_rel =
mid_off - tin S / 2 <= mid_off = half an image, below 2^31 for every image gcs_make_layout admits - the mask is the identity on the
whole legal domain.
(5) in its place, `top_rel` masked to 31 bits (loads only; a smaller, non-negative offset from the same LO run, inside the image): 2
failed, test_one_image_past_2_31[split_4x6] and test_one_split_image_past_2_31_self_updating_loop - top_rel passes 2^31 only in an
image above 2.67 GiB.
(2) `d_lo[*]` with its magnitude kept in `unsigned` was not run: it is the identity here too - a stride is (G / ntiles) images +
less than one, 104 MB in part 1 and less than the image in part 2; only a batch of images of a GiB and more, with more workgroups
than an image has tiles, makes a stride of 2^32 (left for the test of such a batch). (With the sign inside the cast a reverse
sweep would leave the allocation: never run.)
Against the GPU suite as it was before this file, (1), (3) and (5) ran TOGETHER in one library: 0 failed of 1 349. They sit in three
different kernels (the Gabor stores, the deep-bank pass's loads, the split pass's TOP loads) and each is the identity below 2^32 -
the largest slab there is 0.9 GB -, so none of them alone can do otherwise; they were not run one by one.
"""
import time

import numpy as np
import pytest

import hot_banks as hb
import large_offsets as lo
from large_offsets import H, N_BASE, W
from lloyd_ref import _caller_codebook, _pass_reference, updated
from oracle import c_oracle as co
from oracle import spec_oracle as so

pytestmark = pytest.mark.gpu

P = H * W
PEAK_BYTES = 24 << 30               # what one test may hold on the shared device
CHUNK = 256                         # images per comparison


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(autouse=True)
def peak_memory(torch_cuda, request):
    """Every test of this file: at most 24 GiB of device memory at its peak, and its time printed."""
    torch = torch_cuda
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("%s: %.1f s, peak %.1f GiB" % (request.node.name, time.perf_counter() - t0, peak / 2 ** 30))
    assert peak <= PEAK_BYTES, peak


def first_difference(torch, big, small, idx, chunk=CHUNK):
    """big (B, ...) == small[idx] in every element, `chunk` images at a time on the device; -> None or (first image that
    differs, images that differ in its chunk)."""
    for i in range(0, big.shape[0], chunk):
        want = small[idx[i:i + chunk]]
        got = big[i:i + chunk]
        if not torch.equal(got, want):
            ne = (got != want).reshape(want.shape[0], -1).any(1)
            return i + int(ne.nonzero()[0]), int(ne.sum())
    return None


def _dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint16)).view(np.int16)).cuda()


class _Stage:
    """One bank: the sixteen base images, their slab and canonical features (held to the C oracle), and the large batch's slab."""

    def __init__(self, torch, bank_id, bank=None, ops=None):
        self.bank_id = bank_id
        self.bank = bank if bank is not None else hb.hot_bank(*lo.BANKS[bank_id])
        ops = self.ops = ops if ops is not None else hb.hot_segmenter(self.bank).ops
        ns, no = self.bank.n_scales, self.bank.n_orient
        self.img_bytes, self.b, idx, self.straddlers = lo.batch_geometry(ops.lib, ns, no)
        self.idx_np = idx
        self.idx = torch.from_numpy(idx).cuda()
        self.mult = lo.multiplicity(idx)
        self.base = hb.hot_images(N_BASE, H, W, seed=81)
        assert {hb.IMAGE_KINDS[i % 8] for i in range(N_BASE)} == set(hb.IMAGE_KINDS)
        self.base_dev = torch.from_numpy(self.base).cuda()
        self.imgs = self.base_dev[self.idx]                                         # (B, H, W, 3): the batch, built on the device
        self.small = self.new_slab(torch, N_BASE)
        ops.gabor_features(self.base_dev, self.small)
        self.big = self.new_slab(torch, self.b)
        ops.gabor_features(self.imgs, self.big)

    def new_slab(self, torch, b):
        n = self.ops.lib.gcs_feature_slab_bytes(b, H, W, self.bank.n_scales, self.bank.n_orient)
        assert n == b * self.img_bytes
        return torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")

    def oracle(self):
        """(N_BASE, D, H, W) uint16 of the C oracle, and the small slab's canonical features == it."""
        if not hasattr(self, "ref"):
            b = self.bank
            self.ref = np.stack([co.gabor_features(im, b.tapq, b.shift, b.n_orient) for im in self.base])
            self.small_canon = self.ops.features_unpack(self.small, N_BASE, H, W)
            assert np.array_equal(self.small_canon.cpu().numpy().view(np.uint16), self.ref)
            assert self.ref.max() >= 32768
            self.x = self.ref.reshape(N_BASE, self.ref.shape[1], P).transpose(0, 2, 1).astype(np.int64)      # (N_BASE, P, D)
        return self.ref


_STAGES = {}


@pytest.fixture(scope="module")
def stage(torch_cuda, request):
    """The stage of one bank; one at a time on the device."""
    bank_id = request.param
    if bank_id not in _STAGES:
        _STAGES.clear()
        torch_cuda.cuda.empty_cache()
        _STAGES[bank_id] = _Stage(torch_cuda, bank_id)
    yield _STAGES[bank_id]


@pytest.fixture(scope="module", autouse=True)
def _free_at_the_end(torch_cuda):
    yield
    _STAGES.clear()
    torch_cuda.cuda.empty_cache()


ALL_BANKS = list(lo.BANKS)


# ------------------------------------------------------------------------------------------ part 1: Gabor stores
@pytest.mark.parametrize("stage", ALL_BANKS, indirect=True)
def test_gabor_slab_every_byte(torch_cuda, stage):
    """gcs_gabor_features: the large slab viewed as [B, img_bytes] == small_slab[idx] in every byte (flag words, padding and the
    unused quarter of the last tile included: both started as 0xA5); the small slab, unpacked, == the C oracle."""
    torch, st = torch_cuda, stage
    st.oracle()
    assert st.big.numel() == st.b * st.img_bytes > lo.LINE32 + lo.MARGIN - 1
    small = st.small.view(N_BASE, st.img_bytes)
    assert len({bytes(r) for r in small[:, :4096].cpu().numpy()}) > 8                         # the base slabs differ from the start
    if st.bank_id == "split_4x6":                                                              # flagged beside unflagged tiles
        from slab_layout import flag_bytes
        words, _ = flag_bytes(st, st.small, N_BASE, H, W)
        flagged = words.any(axis=2)
        assert flagged[hb.BLACK_REGION].any() and not flagged[hb.BLACK_REGION].all()
    bad = first_difference(torch, st.big.view(st.b, st.img_bytes), small, st.idx)
    assert bad is None, (st.bank_id, bad, st.straddlers)


# ------------------------------------------------------------------------------------------ part 1: one Lloyd pass
# (kernel gcs_selftest_pass_kernel names, bank, k): one case per tile-addressing path (the banks are PASS_CASES' of
# tests/test_gpu_value_range.py; 8x8 at k = 13 takes wide<2,10> as its shift-8 twin there does)
PASS_CASES = [("split<1,3,2>", "split_4x6", 8), ("split<2,5>", "split_4x6", 16), ("wide8w<1,5>", "wide_3x9", 4),
              ("native<4,3,6>", "deep_8x8", 8), ("wide<2,10>", "deep_8x8", 13), ("generic", "generic_7x10", 4)]


def _run_pass(torch, st, feats, b, k, cent_np, n_sets, reverse):
    """gcs_kmeans_assign_accumulate + gcs_kmeans_reduce -> (labels (b, H, W) uint8 on the device, sums (n_sets, k, D + 1) int64)."""
    ops = st.ops
    labels = ops.label_slab(b, H, W).fill_(0xA5)
    partials = ops.partial_slab(b, H, W, k).zero_()
    sums = ops.new_sums(n_sets, k)
    ops.assign_accumulate(feats, _dev16(torch, cent_np), b, H, W, k, n_sets, labels, partials, reverse=reverse)
    ops.reduce(partials, b, H, W, k, n_sets, sums)
    return labels[:b * P].view(b, H, W), sums.cpu().numpy()


def _rasters(torch, st, feats, b, k, cent_np, n_sets, reverse):
    out = []
    scratch = st.ops.label_slab(b, H, W)                  # (written for the int32 map of the generic pass only: include/gcs.h)
    for dt in (torch.int32, torch.uint8):
        lab = torch.full((b, H, W), 99, dtype=dt, device="cuda")
        st.ops.assign_raster(feats, _dev16(torch, cent_np), b, H, W, k, n_sets, lab, scratch_labels=scratch, reverse=reverse)
        out.append(lab)
    return out


@pytest.mark.parametrize("name,stage,k", PASS_CASES, indirect=["stage"], ids=[c[0] for c in PASS_CASES])
def test_one_lloyd_pass(torch_cuda, name, stage, k):
    """gcs_kmeans_assign_accumulate + gcs_kmeans_reduce and gcs_kmeans_assign_raster (int32 and uint8), both sweep directions, one
    global codebook and n_sets = B (a codebook per base image, through idx). Small run == lloyd_ref._pass_reference; large labels ==
    small_labels[idx], per-image sums and counts == small[idx], global ones == sum_j multiplicity_j * sums_j (int64, exact: B P
    46 339 < 2^63)."""
    torch, st = torch_cuda, stage
    ops, b = st.ops, st.b
    st.oracle()
    x, d = st.x, st.x.shape[2]
    assert ops.lib.gcs_selftest_pass_kernel(H, W, st.bank.n_scales, st.bank.n_orient, k).decode() == name
    assert b * P * hb.G_MAX < 1 << 63
    vote = np.ones((N_BASE, P), bool)
    book = _caller_codebook(np.concatenate(list(x)), k)[None]                                  # (1, k, D): a tie, extreme rows
    books = np.stack([_caller_codebook(x[j], k) for j in range(N_BASE)])                       # (N_BASE, k, D)
    assert book.max() >= 32768
    # the small runs against the reference
    want_lab_g, sums_g, cnt_g = _pass_reference(x, np.repeat(book, N_BASE, 0), vote)           # per base image, the global codebook
    want_lab_p, sums_p, cnt_p = _pass_reference(x, books, vote)
    if k >= 2:
        assert not (want_lab_g == 1).any()                                                     # the lowest index won every tie
    total = np.concatenate([(st.mult[:, None, None] * sums_g).sum(0), (st.mult[:, None] * cnt_g).sum(0)[:, None]], 1)
    assert total[:, -1].sum() == b * P
    per_image = np.concatenate([sums_p, cnt_p[:, :, None]], 2)
    books_big = books[st.idx_np]
    for reverse in (False, True):
        tag = (name, reverse)
        small_lab_g, got = _run_pass(torch, st, st.small, N_BASE, k, np.repeat(book, N_BASE, 0), N_BASE, reverse)
        assert np.array_equal(small_lab_g.cpu().numpy().reshape(N_BASE, P), want_lab_g), tag
        assert np.array_equal(got, np.concatenate([sums_g, cnt_g[:, :, None]], 2)), tag
        small_lab_p, got = _run_pass(torch, st, st.small, N_BASE, k, books, N_BASE, reverse)
        assert np.array_equal(small_lab_p.cpu().numpy().reshape(N_BASE, P), want_lab_p), tag
        assert np.array_equal(got, per_image), tag
        small_lab_g, small_lab_p = small_lab_g.clone(), small_lab_p.clone()
        # the large runs through idx
        lab, got = _run_pass(torch, st, st.big, b, k, book, 1, reverse)
        bad = first_difference(torch, lab, small_lab_g, st.idx, chunk=1024)
        assert bad is None, (tag, "global", bad, st.straddlers)
        assert np.array_equal(got[0], total), (tag, "global sums")
        for out in _rasters(torch, st, st.big, b, k, book, 1, reverse):
            bad = first_difference(torch, out, small_lab_g.to(out.dtype), st.idx, chunk=1024)
            assert bad is None, (tag, "global raster", out.dtype, bad, st.straddlers)
        lab, got = _run_pass(torch, st, st.big, b, k, books_big, b, reverse)
        bad = first_difference(torch, lab, small_lab_p, st.idx, chunk=1024)
        assert bad is None, (tag, "per image", bad, st.straddlers)
        wrong = np.argwhere((got != per_image[st.idx_np]).any(axis=(1, 2)))
        assert wrong.size == 0, (tag, "per-image sums", wrong[:4].tolist(), st.straddlers)
        for out in _rasters(torch, st, st.big, b, k, books_big, b, reverse):
            bad = first_difference(torch, out, small_lab_p.to(out.dtype), st.idx, chunk=1024)
            assert bad is None, (tag, "per-image raster", out.dtype, bad, st.straddlers)


# ------------------------------------------------------------------------------------------ part 1: the self-updating loop
N_ITER = 3


def _reference_loop(x, k, idx, mult, mode, first=None):
    """SPEC.md §4 over the batch x[idx], N_ITER passes: `updated` applied to the multiplicity-weighted sums of the base images, pass
    by pass (global), or every base image on its own (per_image). -> (centroids each pass used, labels (N_BASE, P) of the last)."""
    if mode == "global":
        cent = so.kmeans_init(x[idx[0]] if first is None else first, k)[None]                  # image 0 of the batch
    else:
        cent = np.stack([so.kmeans_init(x[j], k) for j in range(N_BASE)])
    used = []
    vote = np.ones(x.shape[:2], bool)
    for t in range(N_ITER):
        used.append(cent)
        lab, sums, cnt = _pass_reference(x, cent if mode == "per_image" else np.repeat(cent, N_BASE, 0), vote)
        if t < N_ITER - 1:
            if mode == "global":
                sums, cnt = (mult[:, None, None] * sums).sum(0)[None], (mult[:, None] * cnt).sum(0)[None]
            cent = updated(sums, cnt, cent)
    return used, lab


def _fused_loop(torch, ops, feats, b, k, d, n_sets, dtype):
    """N_ITER direct gcs_kmeans_pass_fused calls on a zeroed workspace -> (centroids each pass wrote, the label map)."""
    ws = ops.fused_workspace(b, H, W, k, n_sets)
    assert ws is not None
    used = []
    out = torch.full((b, H, W), 99, dtype=dtype, device="cuda")
    for t in range(N_ITER):
        cent = torch.full((n_sets, k, d), -1, dtype=torch.int16, device="cuda")
        if t == N_ITER - 1:
            ops.assign_raster(feats, cent, b, H, W, k, n_sets, out, reverse=bool(t & 1), fused=(ws, t))
        else:
            ops.assign_accumulate(feats, cent, b, H, W, k, n_sets, None, None, reverse=bool(t & 1), fused=(ws, t))
        used.append(cent)
    return used, out


@pytest.mark.parametrize("stage", ["split_4x6"], indirect=True)
def test_self_updating_loop(torch_cuda, stage):
    """gcs_kmeans_pass_fused, three passes, one global codebook and n_sets = B, the label map as uint8 and as int32: the centroids
    every pass made for itself and every label == the reference loop (global: on the multiplicity-weighted sums; per image: the
    small loop == the reference, the large one == it through idx)."""
    torch, st = torch_cuda, stage
    ops, b, k = st.ops, st.b, 8
    st.oracle()
    d = st.x.shape[2]
    assert ops.lib.gcs_selftest_pass_kernel(H, W, st.bank.n_scales, st.bank.n_orient, k).decode() == "split<1,3,2>"
    want_used, want_lab = _reference_loop(st.x, k, st.idx_np, st.mult, "global")
    want_dev = torch.from_numpy(want_lab.reshape(N_BASE, H, W).astype(np.uint8)).cuda()
    assert max(c.max() for c in want_used) >= 32768 and len(np.unique(want_lab)) > 2
    for dtype in (torch.uint8, torch.int32):
        used, out = _fused_loop(torch, ops, st.big, b, k, d, 1, dtype)
        for t in range(N_ITER):
            assert np.array_equal(used[t].cpu().numpy().view(np.uint16), want_used[t]), ("global", dtype, t)
        bad = first_difference(torch, out, want_dev.to(dtype), st.idx, chunk=1024)
        assert bad is None, ("global", dtype, bad, st.straddlers)
    want_used, want_lab = _reference_loop(st.x, k, st.idx_np, st.mult, "per_image")
    want_dev = torch.from_numpy(want_lab.reshape(N_BASE, H, W).astype(np.uint8)).cuda()
    for dtype in (torch.uint8, torch.int32):
        small_used, small_out = _fused_loop(torch, ops, st.small, N_BASE, k, d, N_BASE, dtype)
        for t in range(N_ITER):
            assert np.array_equal(small_used[t].cpu().numpy().view(np.uint16), want_used[t]), ("per image, small", dtype, t)
        assert torch.equal(small_out, want_dev.to(dtype)), ("per image, small", dtype)
        used, out = _fused_loop(torch, ops, st.big, b, k, d, b, dtype)
        for t in range(N_ITER):
            assert torch.equal(used[t], small_used[t][st.idx]), ("per image", dtype, t)
        bad = first_difference(torch, out, small_out, st.idx, chunk=1024)
        assert bad is None, ("per image", dtype, bad, st.straddlers)


# ------------------------------------------------------------------------------------------ part 1: in-place stages, edge map, tree
@pytest.mark.parametrize("bank_id", ["split_4x6", "deep_8x8"])
def test_smoothing_in_place(torch_cuda, bank_id):
    """gcs_smooth_features on the large slab == the same call on the sixteen images through idx, every byte; the small slab,
    unpacked, == tests/smooth_ref.py on the C oracle's features."""
    import smooth_ref as sr
    torch = torch_cuda
    _STAGES.clear()
    torch.cuda.empty_cache()
    bank = hb.hot_bank(*lo.BANKS[bank_id])
    st = _Stage(torch, bank_id, bank, hb.hot_segmenter(bank, smoothing=1.0).ops)
    ref = st.oracle()
    ops, b = st.ops, st.b
    ops.smooth_features(st.small, N_BASE, H, W)
    got = ops.features_unpack(st.small, N_BASE, H, W).cpu().numpy().view(np.uint16)
    want = np.stack([sr.smooth_features(ref[j], 1.0, bank.n_scales, bank.n_orient) for j in range(N_BASE)])
    assert np.array_equal(got, want) and want.max() >= 32768 and not np.array_equal(want, ref)
    ops.smooth_features(st.big, b, H, W)
    bad = first_difference(torch, st.big.view(b, st.img_bytes), st.small.view(N_BASE, st.img_bytes), st.idx)
    assert bad is None, (bank_id, bad, st.straddlers)


POSITION_BANKS = {"split_4x5": dict(n_scales=4, n_orient=5), "deep_8x7": dict(n_scales=8, n_orient=7)}


def _position_stage(torch, bank_id):
    """A stage on the default taps with the coordinate slot of SPEC.md §12 (mu = 255: coordinates times 255 pass 4096 in every tile
    but the first columns', so TOP runs and flags are written); the slot is NOT yet filled."""
    from gabor_color_image_segmentation_amd import make_bank
    from gabor_color_image_segmentation_amd.segmenter import HipOps
    _STAGES.clear()
    torch.cuda.empty_cache()
    bank = make_bank(position_weight=255, **POSITION_BANKS[bank_id])
    assert bank.n_orient == POSITION_BANKS[bank_id]["n_orient"] + 1              # the coordinate slot is a slot of every scale
    return _Stage(torch, bank_id, bank, HipOps(bank, "cuda:0"))


@pytest.mark.parametrize("bank_id", list(POSITION_BANKS))
def test_position_edge_map_and_tree_on_the_slab(torch_cuda, bank_id):
    """gcs_position_features in place (the large slab afterwards == the small one through idx, every byte; the small one, unpacked,
    == tests/position_ref.py), then on that slab gcs_feature_gradient (small == tests/feature_gradient_ref.py) and
    gcs_region_tree_slab (small == gcs_region_tree on the canonical features, itself held to tests/region_tree_ref.py on two
    images): every output of the large call == the small call's through idx."""
    import feature_gradient_ref as fg
    import position_ref as pr
    import region_tree_ref as rt
    torch = torch_cuda
    st = _position_stage(torch, bank_id)
    ops, b, bank = st.ops, st.b, st.bank
    ns, slots = POSITION_BANKS[bank_id]["n_scales"], POSITION_BANKS[bank_id]["n_orient"]
    d = bank.n_features
    ops.position_features(st.small, N_BASE, H, W)
    canon = ops.features_unpack(st.small, N_BASE, H, W)
    x = canon.cpu().numpy().view(np.uint16)
    for j in range(N_BASE):
        assert np.array_equal(x[j], pr.features(st.base[j], 0.0, 0, 255, ns, slots)), j
    assert x.max() >= 255 * (W - 8) >= 4096
    ops.position_features(st.big, b, H, W)
    bad = first_difference(torch, st.big.view(b, st.img_bytes), st.small.view(N_BASE, st.img_bytes), st.idx)
    assert bad is None, (bank_id, "position", bad, st.straddlers)
    # the edge map
    small = torch.full((N_BASE, H, W), -7, dtype=torch.int32, device="cuda")
    ops.feature_gradient(st.small, N_BASE, H, W, small)
    want = np.stack([fg.gradient(x[j], ns, slots + 1) for j in range(N_BASE)])
    assert np.array_equal(small.cpu().numpy(), want) and want.max() > 0
    out = torch.full((b, H, W), -7, dtype=torch.int32, device="cuda")
    ops.feature_gradient(st.big, b, H, W, out)
    bad = first_difference(torch, out, small, st.idx, chunk=1024)
    assert bad is None, (bank_id, "gradient", bad, st.straddlers)
    del out
    # the tree: a map of 9 x 13 blocks, turned by the base image's number so that the maps differ
    yy, xx = np.mgrid[0:H, 0:W]
    blocks = (yy // 9) * (-(-W // 13)) + xx // 13
    K = int(blocks.max()) + 1
    maps = np.stack([(blocks + j) % K for j in range(N_BASE)]).astype(np.int32)

    def tree(feats, n, labels, slab=True):
        ws, merges, costs, alive = ops.region_tree_buffers(n, H, W, K)
        for t, v in ((ws, 0xAB), (merges, 7), (costs, 7), (alive, -5)):
            t.fill_(v)
        if slab:
            ops.region_tree_slab(feats, labels, n, H, W, K, ws, merges, costs, alive)
        else:
            ops.region_tree(feats, labels, n, H, W, K, ws, merges, costs, alive)
        return merges, costs, alive

    small_maps = torch.from_numpy(maps).cuda()
    small_tree = tree(st.small, N_BASE, small_maps)
    for got, want in zip(small_tree, tree(canon, N_BASE, small_maps, slab=False)):
        assert torch.equal(got, want)
    for j in (1, 7):
        rm, rc, ra = rt.build_tree(x[j], maps[j], K)
        assert int(small_tree[2][j]) == ra and np.array_equal(small_tree[0][j].cpu().numpy(), rm)
        assert np.array_equal(small_tree[1][j].cpu().numpy().view(np.uint64), rc)
    big_tree = tree(st.big, b, small_maps[st.idx])
    for what, got, want in zip(("merges", "costs", "alive"), big_tree, small_tree):
        bad = first_difference(torch, got, want, st.idx, chunk=1024)
        assert bad is None, (bank_id, what, bad, st.straddlers)


# ------------------------------------------------------------------------------------------ part 1: the segmenter
def test_segment_device_both_modes(torch_cuda):
    """Segmenter.segment_device on the default bank, mode "global" (the whole batch in one slab) and "per_image" (one group: the
    16 GiB budget holds it): every label == the reference loop on the C oracle's features (global: multiplicity-weighted sums;
    per image: the C oracle's own k-means, which the small call equals too)."""
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    _STAGES.clear()
    torch.cuda.empty_cache()
    seg = Segmenter(n_iter=N_ITER, device="cuda:0")
    bank = seg.bank
    img_bytes, b, idx, straddlers = lo.batch_geometry(seg.ops.lib, bank.n_scales, bank.n_orient)
    base = hb.hot_images(N_BASE, H, W, seed=81)
    ref = np.stack([co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient) for im in base])
    x = ref.reshape(N_BASE, ref.shape[1], P).transpose(0, 2, 1).astype(np.int64)
    base_dev, idx_dev = torch.from_numpy(base).cuda(), torch.from_numpy(idx).cuda()
    imgs = base_dev[idx_dev]
    for mode in ("global", "per_image"):
        assert seg.group_size(b, H, W, mode) == b                                              # one slab of b * img_bytes
        _, want = _reference_loop(x, seg.k, idx, lo.multiplicity(idx), mode)
        want = want.reshape(N_BASE, H, W).astype(np.int32)
        if mode == "per_image":
            assert np.array_equal(want, co.segment_batch(base, bank.tapq, bank.shift, bank.n_orient, k=seg.k, n_iter=N_ITER))
            assert np.array_equal(seg.segment_device(base_dev, mode=mode).cpu().numpy(), want)
        assert len(np.unique(want)) > 2
        got = seg.segment_device(imgs, mode=mode)
        bad = first_difference(torch, got, torch.from_numpy(want).cuda(), idx_dev, chunk=1024)
        assert bad is None, (mode, bad, straddlers)
        del got


# ------------------------------------------------------------------------------------------ part 2: one image past 2^31
# Only in ONE image whose own slab passes 2^31 do the Gabor kernels' lane offsets, the split pass's top_rel and a deep bank's
# tile * tile_bytes inside an image grow large. The image is a pattern of PERIOD rows stacked: stripes, noise and an all-black
# stretch side by side, so that every band holds flagged and unflagged tiles. H and W are multiples of 8 (no packed strip: part 1
# has them), so a band of PERIOD rows is PERIOD / 8 * W / 8 blocks = a whole number of tiles in raster order, and tile t of a crop
# that starts at a row r0 (a multiple of PERIOD) is tile t + r0 / 8 * W / 8 / 4 of the image.
PERIOD = 64
# (bank, H, W, k, the kernel): (a) a split image just below 4 GiB (top_off = 1.48 x 2^31); (b) a deep image past 2^31
SINGLE = [("split_4x6", 47000, 1000, 8, "split<1,3,2>"), ("deep_8x8", 17000, 1000, 8, "native<4,3,6>")]


def _reach(bank, smoothing=0.0):
    """Rows at either end of an image (or of a crop) that its border can reach, from the bank: per level L the filter radius at
    full resolution, (ksize // 2) << L, and the 2^L - 1 rows a level pixel covers beside its own (the 2 x 2 means); with smoothing,
    per scale s the radius of its taps (tests/smooth_ref.py) on its level s // 2, in the same way, on top of that."""
    import smooth_ref as sr
    levels = (bank.n_scales + 1) // 2
    gabor = max(((bank.ksize // 2) << L) + (1 << L) - 1 for L in range(levels))
    if not smoothing:
        return gabor
    return gabor + max((r << (s // 2)) + (1 << (s // 2)) - 1 for s, (r, _) in enumerate(sr.taps(smoothing, bank.n_scales)))


def _pattern(w):
    y, x = np.mgrid[0:PERIOD, 0:w]
    p = np.zeros((PERIOD, w, 3), np.uint8)
    third = w // 3
    stripes = np.where((x + 2 * y) % 18 < 9, 255, 0).astype(np.uint8)
    p[:, :third] = np.stack([stripes, stripes[::-1], stripes[:, ::-1]], -1)[:, :third]
    p[:, third:2 * third] = np.random.default_rng(64).integers(0, 256, (PERIOD, third, 3), dtype=np.uint8)
    return p                                                                                  # (the last third stays black)


def _tile_arrays(lib, slab, h, w, ns, no):
    """One image's slab as its arrays of per-tile rows: LO, MID, TOP, FLAG of a split slab (and the padding behind the flag
    words), the one run per tile of a wide slab; together they are every byte of the slab."""
    from slab_layout import tile_geometry
    nt, tile_bytes, split = tile_geometry(lib, h, w, ns, no)
    if not split:
        assert slab.numel() == nt * tile_bytes
        return nt, {"RUN": slab.view(nt, tile_bytes)}, slab[:0]
    s = tile_bytes // 2
    mid, top, flag = nt * s, nt * s + nt * s // 2, 2 * nt * s
    return nt, {"LO": slab[:mid].view(nt, s), "MID": slab[mid:top].view(nt, s // 2), "TOP": slab[top:flag].view(nt, s // 2),
                "FLAG": slab[flag:flag + 4 * nt].view(nt, 4)}, slab[flag + 4 * nt:]


def _rows_equal(torch, a, b, rows=4096):
    return all(torch.equal(a[i:i + rows], b[i:i + rows]) for i in range(0, a.shape[0], rows))


class _Tall:
    """One tall image and two crops of it. With m = the bands the borders reach (_reach, asserted against the bank): the top crop is
    bands [0, 2 m + 2) and answers for bands [0, m + 2) (its own bottom edge reaches the m behind them); band m + 1 is the period
    every band up to n_bands - m - 3 must repeat; the bottom crop starts at band n_bands - 2 m - 2 and answers for everything from
    its band m on. Nothing of the image is left out, and every compared row has its support inside its crop."""

    def __init__(self, torch, bank_id, h, w, k, name, smoothing=0.0):
        _STAGES.clear()
        torch.cuda.empty_cache()
        self.torch, self.bank_id, self.h, self.w, self.smoothing = torch, bank_id, h, w, smoothing
        bank = self.bank = hb.hot_bank(*lo.BANKS[bank_id])
        ops = self.ops = hb.hot_segmenter(bank, smoothing=smoothing).ops
        lib, ns, no = ops.lib, bank.n_scales, bank.n_orient
        assert lib.gcs_selftest_pass_kernel(h, w, ns, no, k).decode() == name
        img_bytes = lib.gcs_feature_slab_bytes(1, h, w, ns, no)
        assert lo.LINE31 < img_bytes < lo.LINE32 and h % 8 == 0 and w % 8 == 0 and PERIOD % 64 == 0
        assert (PERIOD // 8 * (w // 8)) % 4 == 0                                               # a band is whole tiles
        if bank_id == "split_4x6":
            assert img_bytes > 0.98 * lo.LINE32 and img_bytes * 3 // 4 > 1.47 * lo.LINE31      # top_off: far past 2^31
        self.per_band = PERIOD // 8 * (w // 8) // 4                                            # tiles per band
        self.n_bands, rest = divmod(h, PERIOD)
        reach = _reach(bank, smoothing)
        m = self.m = -(-reach // PERIOD)
        assert 0 < reach <= m * PERIOD and rest and rest % 8 == 0 and self.n_bands > 4 * m + 8
        self.image = np.tile(_pattern(w), (self.n_bands + 1, 1, 1))[:h]
        self.r0 = (self.n_bands - 2 * m - 2) * PERIOD
        self.crops = {"top": (0, self.image[:(2 * m + 2) * PERIOD]), "bottom": (self.r0, self.image[self.r0:])}
        # the rows a crop answers for, in the crop's own rows
        self.answers = {"top": (0, (m + 2) * PERIOD), "bottom": (m * PERIOD, h - self.r0)}
        self.n_between = self.n_bands - 2 * m - 4                                              # bands m + 2 .. n_bands - m - 3
        self.big = self.slab(self.image)
        self.small = {end: self.slab(crop) for end, (_, crop) in self.crops.items()}

    def slab(self, img_np):
        torch, ops, hh = self.torch, self.ops, img_np.shape[0]
        n = ops.lib.gcs_feature_slab_bytes(1, hh, self.w, self.bank.n_scales, self.bank.n_orient)
        slab = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        ops.gabor_features(torch.from_numpy(np.ascontiguousarray(img_np[None])).cuda(), slab)
        if self.smoothing:
            ops.smooth_features(slab, 1, hh, self.w)
        return slab

    def features(self):
        """end -> (rows * w, D) int64 of the reference (the C oracle, smoothed by tests/smooth_ref.py where the slabs are); the
        crops' own slabs, unpacked, == it."""
        import smooth_ref as sr
        bank, out = self.bank, {}
        for end, (_, crop) in self.crops.items():
            want = co.gabor_features(crop, bank.tapq, bank.shift, bank.n_orient)
            assert want.max() >= 32768
            if self.smoothing:
                raw, want = want, sr.smooth_features(want, self.smoothing, bank.n_scales, bank.n_orient)
                assert not np.array_equal(raw, want)
            got = self.ops.features_unpack(self.small[end], 1, crop.shape[0], self.w).cpu().numpy().view(np.uint16)[0]
            assert np.array_equal(got, want), (self.bank_id, end)
            out[end] = want.reshape(want.shape[0], -1).T.astype(np.int64)
        return out

    def check_slab(self):
        """Every byte of the tall image's slab: the ends == the crops' slabs, tile range by tile range in every array; every band
        between == band m + 1; the padding is as it was."""
        torch, lib, m, per_band = self.torch, self.ops.lib, self.m, self.per_band
        ns, no = self.bank.n_scales, self.bank.n_orient
        nt, arrays, pad = _tile_arrays(lib, self.big, self.h, self.w, ns, no)
        assert bool((pad == 0xA5).all())
        for what, a in arrays.items():
            ref = a[(m + 1) * per_band:(m + 2) * per_band].reshape(1, -1)
            for b0 in range(m + 2, self.n_bands - m - 2, 32):
                n = min(32, self.n_bands - m - 2 - b0)
                assert torch.equal(a[b0 * per_band:(b0 + n) * per_band].reshape(n, -1), ref.expand(n, -1)), (self.bank_id, what, b0)
        if "FLAG" in arrays:
            flagged = arrays["FLAG"][(m + 1) * per_band:(m + 2) * per_band].any(1)
            assert bool(flagged.any()) and not bool(flagged.all())
        for end, (row0, crop) in self.crops.items():
            hh = crop.shape[0]
            nt_crop, crop_arrays, _ = _tile_arrays(lib, self.small[end], hh, self.w, ns, no)
            shift_t = row0 // 8 * (self.w // 8) // 4
            t0, t1 = (self.answers[end][0] // PERIOD * per_band, min(self.answers[end][1] // PERIOD * per_band, nt_crop))
            if end == "bottom":
                t1 = nt_crop
                assert t1 + shift_t == nt
            else:
                assert t0 == 0 and t1 == (m + 2) * per_band and (m + 2) * PERIOD + m * PERIOD <= hh
            for what, a in arrays.items():
                assert _rows_equal(torch, a[t0 + shift_t:t1 + shift_t], crop_arrays[what][t0:t1]), (self.bank_id, end, what)

    def reference_pass(self, x, cent):
        """One pass over the tall image from the crops: end -> labels (rows, w) of the crop, and the image's exact sums and
        counts (k, D + 1) = top + n_between * band + bottom."""
        k, labs, total = cent.shape[1], {}, 0
        for end, (_, crop) in self.crops.items():
            rows = np.arange(crop.shape[0] * self.w) // self.w
            lab = so.kmeans_assign(x[end], cent[0])
            labs[end] = lab.reshape(crop.shape[0], self.w)
            parts = [(self.answers[end], 1)]
            if end == "top":
                parts.append((((self.m + 1) * PERIOD, (self.m + 2) * PERIOD), self.n_between))
            for (lo_r, hi_r), times in parts:
                keep = (rows >= lo_r) & (rows < hi_r)
                for j in range(k):
                    sel = keep & (lab == j)
                    total = total + times * np.concatenate([x[end][sel].sum(0), [sel.sum()]])[None] * (np.arange(k) == j)[:, None]
        assert total[:, -1].sum() == self.h * self.w
        return labs, total

    def check_labels(self, lab, labs, tag):
        """(H, W) labels of the tall image on the device == the crops' reference labels at the ends and band m + 1 between."""
        torch, m = self.torch, self.m
        for end, (row0, _) in self.crops.items():
            a, b = self.answers[end]
            want = torch.from_numpy(labs[end][a:b].astype(np.int64)).cuda()
            assert torch.equal(lab[row0 + a:row0 + b].to(torch.int64), want), (self.bank_id, tag, end)
        ref = lab[(m + 1) * PERIOD:(m + 2) * PERIOD].reshape(1, -1)
        between = lab[(m + 2) * PERIOD:(self.n_bands - m - 2) * PERIOD].reshape(self.n_between, -1)
        assert torch.equal(between, ref.expand(self.n_between, -1)), (self.bank_id, tag, "bands")


@pytest.mark.parametrize("bank_id,h,w,k,name", SINGLE, ids=[c[0] for c in SINGLE])
def test_one_image_past_2_31(torch_cuda, bank_id, h, w, k, name):
    """gcs_gabor_features and one Lloyd pass on one tall image: every byte of the slab (_Tall.check_slab; the crops' slabs, unpacked,
    == the C oracle), every label in both sweep directions (the pass on the crops == spec_oracle.kmeans_assign), sums and counts ==
    top + n * band + bottom, each part exact on the crops."""
    torch = torch_cuda
    tall = _Tall(torch, bank_id, h, w, k, name)
    ops = tall.ops
    tall.check_slab()
    x = tall.features()
    book = _caller_codebook(np.concatenate([x["top"], x["bottom"]]), k)[None]
    labs, total = tall.reference_pass(x, book)
    for end, (_, crop) in tall.crops.items():
        hh = crop.shape[0]
        lab = ops.label_slab(1, hh, w).fill_(0xA5)
        ops.assign_accumulate(tall.small[end], _dev16(torch, book), 1, hh, w, k, 1, lab, None)
        assert np.array_equal(lab[:hh * w].cpu().numpy().reshape(hh, w), labs[end]), end
    for reverse in (False, True):
        lab = ops.label_slab(1, h, w).fill_(0xA5)
        partials = ops.partial_slab(1, h, w, k).zero_()
        sums = ops.new_sums(1, k)
        ops.assign_accumulate(tall.big, _dev16(torch, book), 1, h, w, k, 1, lab, partials, reverse=reverse)
        ops.reduce(partials, 1, h, w, k, 1, sums)
        tall.check_labels(lab[:h * w].view(h, w), labs, reverse)
        assert np.array_equal(sums.cpu().numpy()[0], total), (bank_id, reverse, "sums")


@pytest.mark.parametrize("bank_id,h,w,k,name", SINGLE, ids=[c[0] for c in SINGLE])
def test_one_image_past_2_31_smoothed_in_place(torch_cuda, bank_id, h, w, k, name):
    """gcs_smooth_features in place on the tall image's slab: every byte as in test_one_image_past_2_31, with the borders' reach
    widened by the smoothing radii; the crops' smoothed slabs, unpacked, == tests/smooth_ref.py on the C oracle's features."""
    tall = _Tall(torch_cuda, bank_id, h, w, k, name, smoothing=1.0)
    assert _reach(tall.bank, 1.0) > _reach(tall.bank)
    tall.check_slab()
    tall.features()


def test_one_split_image_past_2_31_self_updating_loop(torch_cuda):
    """gcs_kmeans_pass_fused, three passes in alternating directions, on the split image of 0.985 x 2^32 bytes, the label map as
    uint8 and as int32: the centroids every pass made for itself == the SPEC.md §4 loop on sums put together from the crops (the init
    pixels lie in bands that repeat band m + 1), and every label == that loop's."""
    torch = torch_cuda
    bank_id, h, w, k, name = SINGLE[0]
    tall = _Tall(torch, bank_id, h, w, k, name)
    x = tall.features()
    d, m = x["top"].shape[1], tall.m
    pixels = [((2 * j + 1) * h * w) // (2 * k) for j in range(k)]
    assert all(m + 2 <= p // w // PERIOD <= tall.n_bands - m - 3 for p in pixels)
    cent = np.stack([x["top"][((p // w) % PERIOD + (m + 1) * PERIOD) * w + p % w] for p in pixels])[None]
    want_used = []
    for t in range(N_ITER):
        want_used.append(cent)
        labs, total = tall.reference_pass(x, cent)
        if t < N_ITER - 1:
            cent = updated(total[None, :, :-1], total[None, :, -1], cent)
    assert max(c.max() for c in want_used) >= 32768 and len(np.unique(labs["top"])) > 2
    for dtype in (torch.uint8, torch.int32):
        ws = tall.ops.fused_workspace(1, h, w, k, 1)
        assert ws is not None
        out = torch.full((1, h, w), 99, dtype=dtype, device="cuda")
        for t in range(N_ITER):
            got = torch.full((1, k, d), -1, dtype=torch.int16, device="cuda")
            if t == N_ITER - 1:
                tall.ops.assign_raster(tall.big, got, 1, h, w, k, 1, out, reverse=not (t & 1), fused=(ws, t))
            else:
                tall.ops.assign_accumulate(tall.big, got, 1, h, w, k, 1, None, None, reverse=not (t & 1), fused=(ws, t))
            assert np.array_equal(got.cpu().numpy().view(np.uint16), want_used[t]), (dtype, t)
        tall.check_labels(out[0], labs, dtype)
