"""Every stage on the FULL 16-bit feature range (SPEC.md §3: values up to 46339). The default banks cannot push a feature past
about 12 000 on any image, so bit 15 of a feature or a centroid, TOP nibbles above 2, the upper half of the square root's
domain and the smoothing bounds were never exercised. The legal, artificial banks of tests/hot_banks.py reach all of it through
the public C ABI. Stage by stage, so that a failure names its kernel; everything is bit-exact against the C oracle, the NumPy
oracle, tests/smooth_ref.py or plain int64 / Python integers, and every test asserts that its own inputs hold the values it
is about (e.g. ``ref.max() >= 32768``).

Lloyd-pass arms (csrc/lloyd_pass.h, gcs_pass_kernel): the ids of PASS_CASES name the instantiation each (bank, k) selects
(tests/test_pass_kernel_choice.py holds them to it). Of the 22 instantiations, narrow<1,9>, narrow<1,10> and narrow<2,10> cannot be
selected in the default build (a bank with D < 80 on three or more levels has at most 1 230 staging chunks per tile) and are
compiled into -DGCS_NO_SPLIT builds only; the other 19 and the generic pass each have a case here.

Mutants of the library, run once against this file and against the suite as it was before it (failed tests):
(a) the split pass's TOP unpack keeps 3 bits: 15 here, none before; (b) the Gabor split store keeps 3 bits of the TOP nibble: 30,
none; (c) smooth_pack_kernel packs `h >> 12 & 7`: 7, none; (d) smooth_planes_kernel drops the hi16 term: 13, and the earlier
smoothing tests fail too; (e) the native pass's centroid norm drops bit 15: 12, none; (f) kmeans_finalize divides in 32 bits: 4,
and four eight-rank tests of tests/test_distributed.py; (g) the Gabor flag bytes come from `top & 7`: 1
(test_most_negative_real_response: a white image whose every value is exactly 32768), none."""
import numpy as np
import pytest

import hot_banks as hb
import smooth_ref as sr
from oracle import c_oracle as co
from oracle import spec_oracle as so
from lloyd_ref import _caller_codebook, _pass_reference, _update_cases
from pass_cases import K_MAX, PASS_CASES
from slab_layout import flag_bytes, tile_of_pixels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_REF = {}


def _ref_features(cfg, imgs):
    """C-oracle features (B, D, H, W) uint16 of a hot bank, cached per (bank, images)."""
    key = (cfg, imgs.shape, imgs.tobytes())
    if key not in _REF:
        if len(_REF) > 6:
            _REF.pop(next(iter(_REF)))
        bank = hb.hot_bank(*cfg)
        _REF[key] = np.stack([co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient) for im in imgs])
    return _REF[key]


def _level_rows(ns, no, L):
    nf = ns * no
    return [c * nf + f for c in range(3) for f in range(nf) if (f // no) // 2 == L]


def _check_flags(seg, feats, ref, b, h, w):
    """Byte L of a tile's flag word is non-zero exactly where a level-L value of the tile is >= 4096; -> flagged tiles per image."""
    ns, no = seg.bank.n_scales, seg.bank.n_orient
    flags, ntiles = flag_bytes(seg, feats, b, h, w)
    tile = tile_of_pixels(h, w)
    assert tile.max() + 1 == ntiles
    counts = []
    for i in range(b):
        for L in range(4):
            want = np.zeros(ntiles, bool)
            if L < (ns + 1) // 2:
                want[np.unique(tile[(ref[i][_level_rows(ns, no, L)] >= 4096).any(axis=0)])] = True
            assert np.array_equal(flags[i, :, L] != 0, want), (i, L, int((flags[i, :, L] != 0).sum()), int(want.sum()))
        counts.append(int((flags[i] != 0).any(axis=1).sum()))
    return counts, ntiles


# ------------------------------------------------------------------------------------------ Gabor stores, unpack, flags
SPLIT_BANKS = [(4, 6, 13, 8), (4, 6, 13, 7), (2, 6, 13, 8), (2, 6, 15, 7), (2, 3, 7, 7), (2, 3, 7, 8)]
# shapes with and without packed edge strips (test_packed_edge_strips_features_and_labels), B = 1 (small-call launch forms) and 3
SPLIT_SHAPES = [(321, 481, 3), (481, 321, 1), (33, 41, 1), (34, 42, 3), (9, 10, 3), (65, 130, 1), (81, 121, 1), (81, 121, 3)]


@pytest.mark.parametrize("cfg", SPLIT_BANKS, ids=lambda c: "%dx%d_ks%d_shift%d" % c)
def test_split_slab_stores_unpack_and_flag_words(torch_cuda, cfg):
    """Both Gabor epilogues (shift 8: the short one; shift 7: the general one) into the split slab - LO, MID and TOP nibbles up to
    11, main blocks and packed edge strips - read back through gcs_features_unpack == the C oracle; flag byte L is set exactly
    where a level-L value of the tile is >= 4096. The black-region image has flagged and unflagged tiles side by side."""
    torch = torch_cuda
    seg = hb.hot_segmenter(hb.hot_bank(*cfg))
    nib, mixed = set(), 0
    for h, w, b in SPLIT_SHAPES:
        imgs = hb.hot_images(b, h, w, seed=h + w)
        ref = _ref_features(cfg, imgs)
        feats = seg.ops.feature_slab(b, h, w)
        seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
        got = seg.ops.features_unpack(feats, b, h, w).cpu().numpy().view(np.uint16)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, ((h, w, b), len(bad), bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        assert np.array_equal(seg.features_device(torch.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16), ref)
        counts, ntiles = _check_flags(seg, feats, ref, b, h, w)
        if b > hb.BLACK_REGION and 0 < counts[hb.BLACK_REGION] < ntiles:
            mixed += 1
        nib |= set(np.unique(ref >> 12).tolist())
        if h * w > 1000:
            assert ref.max() >= 32768, (h, w, int(ref.max()))
    assert nib == set(range(9 if cfg[3] == 8 else 12)), nib        # every TOP nibble the shift admits went through the stores
    assert mixed >= 2, mixed


WIDE_BANKS = [(4, 7, 13, 7), (4, 8, 7, 8), (5, 8, 13, 7), (5, 6, 15, 8), (6, 8, 15, 7), (8, 6, 13, 8), (8, 6, 7, 7), (8, 8, 15, 8),
              (8, 8, 15, 7), (7, 10, 13, 7), (3, 23, 9, 8)]


@pytest.mark.parametrize("cfg", WIDE_BANKS, ids=lambda c: "%dx%d_ks%d_shift%d" % c)
def test_wide_slab_stores_and_unpack(torch_cuda, cfg):
    """Wide two-level (D >= 80), three- and four-level banks, ksize 7 / 13 / 15, both epilogues, one image (gabor_pre01_kernel / the
    grouped launch forms of a small call) and three: gcs_features_unpack == the C oracle with bit 15 set in the reference."""
    torch = torch_cuda
    seg = hb.hot_segmenter(hb.hot_bank(*cfg))
    shapes = [(81, 121, 1), (72, 104, 3), (33, 41, 3), (9, 10, 1)] + ([(321, 481, 2)] if cfg[:2] in ((8, 8), (4, 7)) else [])
    for h, w, b in shapes:
        imgs = hb.hot_images(b, h, w, seed=h + w)
        ref = _ref_features(cfg, imgs)
        got = seg.features_device(torch.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, ((h, w, b), len(bad), bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        if h * w > 1000:
            assert ref.max() >= 32768 and (ref >= 4096).mean() > 0.5, (h, w, int(ref.max()))


@pytest.mark.parametrize("cfg", [(4, 6, 13, 8), (8, 8, 15, 8), (5, 6, 13, 8)], ids=lambda c: "%dx%d_ks%d_shift%d" % c)
def test_most_negative_real_response(torch_cuda, cfg):
    """`>> shift` is a floor: real taps that are all negative with sum|tapq_re| = 32 896 give v_re = -255 * 32 896 and a_re =
    floor(-32767.5) = -32768 on a white image - the one 16-bit value whose magnitude is not a positive int16. The short epilogue
    adds the digits in 16-bit arithmetic and squares them signed: g = 32768 exactly where the window is white. Flag words and labels
    (both codebook modes) of that batch are checked too."""
    torch = torch_cuda
    bank = hb.hot_bank(*cfg)
    t = bank.tapq.copy()
    t[:, 0] = -t[:, 0]
    for f in range(len(t)):                                       # top one tap up: sum|tapq_re| = 32 896 exactly
        y, x = np.argwhere(t[f, 0] != 0)[0]
        t[f, 0, y, x] -= 32896 + int(t[f, 0].astype(np.int64).sum())
    assert np.all(t[:, 0].astype(np.int64).sum(axis=(1, 2)) == -32896) and t.min() >= -32639
    import dataclasses
    bank = dataclasses.replace(bank, tapq=t)
    seg = hb.hot_segmenter(bank)
    imgs = hb.hot_images(4, 72, 104, seed=9)
    ref = np.stack([co.gabor_features(im, bank.tapq, bank.shift, bank.n_orient) for im in imgs])
    for im, r in zip(imgs[:2], ref[:2]):
        assert np.array_equal(so.gabor_features(im, t.astype(np.int64), bank.shift, bank.n_orient), r)
    got = seg.features_device(torch.from_numpy(imgs).cuda()).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, ref)
    assert (ref[3] == 32768).all() and ref.max() >= 36000         # image 3 is white; the stripes reach sqrt(32768^2 + a_im^2)
    # every value of the white image has the TOP nibble 8 and nothing else: a flag taken from three of the nibble's four bits would
    # leave its tiles unflagged, and a pass would read them as zeros
    b, h, w = imgs.shape[:3]
    if cfg[:2] == (4, 6):
        feats = seg.ops.feature_slab(b, h, w)
        seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
        counts, ntiles = _check_flags(seg, feats, ref, b, h, w)
        assert counts[3] == ntiles
    for mode in ("per_image", "global"):
        want = co.segment_batch(imgs, bank.tapq, bank.shift, bank.n_orient, k=8, n_iter=3, mode=mode)
        seg.n_iter = 3
        assert np.array_equal(seg.segment_batch(imgs, mode=mode), want), mode
    assert len(np.unique(want[3])) == 1 and want[3, 0, 0] != want[1, 0, w - 1]      # white is not labelled like black


# ------------------------------------------------------------------------------------------ init, gather
@pytest.mark.parametrize("cfg", [(4, 6, 13, 7), (2, 3, 7, 7), (4, 7, 13, 7), (8, 8, 15, 8), (7, 10, 13, 7)],
                         ids=lambda c: "%dx%d_ks%d_shift%d" % c)
def test_kmeans_init_and_features_gather(torch_cuda, cfg):
    """gcs_kmeans_init == the oracle's features at the SPEC.md §4 pixels (per-image and global); gcs_features_gather == the
    features at random (b, y, x) triples, every edge-strip pixel of the shape among them, b < 0 -> a zero row."""
    torch = torch_cuda
    seg = hb.hot_segmenter(hb.hot_bank(*cfg))
    b, h, w = 3, 81, 122
    imgs = hb.hot_images(b, h, w, seed=5)
    ref = _ref_features(cfg, imgs)
    d = ref.shape[1]
    feats = seg.ops.feature_slab(b, h, w)
    seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
    x = ref.reshape(b, d, -1).transpose(0, 2, 1)
    for k in (1, 8, 16):
        for n_sets in (1, b):
            cent = torch.full((n_sets, k, d), -1, dtype=torch.int16, device="cuda")
            seg.ops.kmeans_init(feats, b, h, w, k, n_sets, cent)
            want = np.stack([so.kmeans_init(x[i], k) for i in range(n_sets)])
            assert np.array_equal(cent.cpu().numpy().view(np.uint16), want), (k, n_sets)
            if k == 16:
                assert want.max() >= 32768
    rng = np.random.default_rng(17)
    n = 4000
    byx = np.stack([rng.integers(-1, b, n), rng.integers(0, h, n), rng.integers(0, w, n)], 1).astype(np.int32)
    strip = np.array([(i % b, y, xx) for i, (y, xx) in enumerate([(y, xx) for y in range(h) for xx in (w - 2, w - 1)] +
                                                                  [(h - 1, xx) for xx in range(w)])], np.int32)
    byx = np.concatenate([byx, strip])
    got = seg.ops.features_gather(feats, b, h, w, torch.from_numpy(byx).cuda()).cpu().numpy().view(np.uint16)
    want = np.where(byx[:, :1] >= 0, ref[np.maximum(byx[:, 0], 0), :, byx[:, 1], byx[:, 2]], 0)
    assert np.array_equal(got, want)
    assert (byx[:, 0] < 0).sum() > 100 and want.max() >= 32768 and (want[len(want) - len(strip):] >= 32768).any()


# ------------------------------------------------------------------------------------------ one Lloyd pass, kernel level
@pytest.mark.parametrize("case", [c for c, _ in PASS_CASES], ids=[i for _, i in PASS_CASES])
def test_one_lloyd_pass(torch_cuda, case):
    """gcs_kmeans_assign_accumulate + gcs_kmeans_reduce (and gcs_kmeans_reduce_finalize, gcs_kmeans_assign_raster) on hot features:
    labels == so.kmeans_assign, sums and counts == NumPy int64, new centroids == so.kmeans_update. (a) from the init centroids, one
    global and one per-image codebook; (b) from a caller-made codebook (see _caller_codebook) with a row window, both sweep
    directions, either output alone, and as int32 / uint8 raster maps."""
    torch = torch_cuda
    ns, no, ks, shift, k = case
    cfg = (ns, no, ks, shift)
    seg = hb.hot_segmenter(hb.hot_bank(*cfg), k=k)
    ops = seg.ops
    b, h, w = 3, 41, 74
    imgs = hb.hot_images(b, h, w, seed=13)
    ref = _ref_features(cfg, imgs).astype(np.int64)
    d = ref.shape[1]
    x = ref.reshape(b, d, -1).transpose(0, 2, 1)                              # (b, P, D)
    assert ref.max() >= 32768
    feats = ops.feature_slab(b, h, w)
    ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
    labels, partials = ops.label_slab(b, h, w), ops.partial_slab(b, h, w, k)

    def run(cent_np, n_sets, rows, reverse):
        cent = torch.from_numpy(cent_np.astype(np.uint16).view(np.int16)).cuda().contiguous()
        sums = ops.new_sums(n_sets, k)
        labels.fill_(255)
        partials.zero_()
        ops.assign_accumulate(feats, cent, b, h, w, k, n_sets, labels, partials, rows=rows, reverse=reverse)
        ops.reduce(partials, b, h, w, k, n_sets, sums)
        vote = np.zeros((b, h, w), bool)
        vote[:, rows[0]:rows[1]] = True
        want_lab, want_sums, want_cnt = _pass_reference(x, cent_np, vote.reshape(b, -1))
        got_lab = labels[:b * h * w].view(b, h * w).cpu().numpy()
        got = sums.cpu().numpy()
        assert np.array_equal(got_lab, want_lab), (n_sets, rows, reverse, int((got_lab != want_lab).sum()))
        assert np.array_equal(got[:, :, -1], want_cnt), (n_sets, rows, reverse)
        assert np.array_equal(got[:, :, :-1], want_sums), (n_sets, rows, reverse)
        new = cent.clone()
        ops.reduce_finalize(partials, b, h, w, k, n_sets, ops.new_sums(n_sets, k), new)
        want_new = cent_np.copy()
        nz = want_cnt > 0
        want_new[nz] = (2 * want_sums[nz] + want_cnt[nz][:, None]) // (2 * want_cnt[nz][:, None])
        assert np.array_equal(new.cpu().numpy().view(np.uint16), want_new), (n_sets, rows, reverse)
        return cent, want_lab, want_cnt, want_new

    for n_sets in (1, b):                                                      # (a) init centroids
        init = np.stack([so.kmeans_init(x[i], k) for i in range(n_sets)])
        _, _, _, new = run(init, n_sets, (0, h), False)
        if k >= 4 and n_sets == 1:
            assert new.max() >= 32768, int(new.max())                          # a centroid with bit 15 set came out of the update
            run(new, 1, (0, h), True)                                          # ... and goes into the next pass's patterns
    book = _caller_codebook(np.concatenate(list(x)), k)[None]                  # (b) caller-made codebook
    assert book.max() >= 32768
    for reverse in (False, True):
        cent, want_lab, want_cnt, _ = run(book, 1, (h // 4, h - h // 5), reverse)
        if k >= 2:
            assert want_cnt[0, 1] == 0 and not (want_lab == 1).any()           # the duplicate row: the lowest index won every tie
        lab2, par2 = torch.full_like(labels, 255), torch.zeros_like(partials)
        partials.zero_()
        ops.assign_accumulate(feats, cent, b, h, w, k, 1, labels, partials, reverse=reverse)
        ops.assign_accumulate(feats, cent, b, h, w, k, 1, lab2, None, reverse=reverse)
        ops.assign_accumulate(feats, cent, b, h, w, k, 1, None, par2, reverse=reverse)
        assert torch.equal(lab2, labels) and torch.equal(par2, partials)
        for dt in (torch.int32, torch.uint8):
            out = torch.full((b, h, w), 99, dtype=dt, device="cuda")
            ops.assign_raster(feats, cent, b, h, w, k, 1, out, scratch_labels=labels, reverse=reverse)
            assert np.array_equal(out.cpu().numpy().reshape(b, -1), want_lab), (dt, reverse)


# ------------------------------------------------------------------------------------------ finalize / reduce_finalize alone
@pytest.mark.parametrize("d,k", [(72, 16), (3, 4), (192, 8), (210, 5)])
def test_finalize_on_written_sums(torch_cuda, d, k):
    """gcs_kmeans_finalize alone: floor((2 S + n) / (2 n)) in Python integers; 2 S + n reaches 9.2e11 (n = 64 x 481 x 321 pixels of
    46339), far past 32 bits; empty clusters keep their centroid."""
    torch = torch_cuda
    seg = hb.hot_segmenter(hb.hot_bank(2, 3, 7, 7))
    old, sums, want = _update_cases(d, k)
    n_sets = 2
    s = torch.tensor([sums, sums[::-1]], dtype=torch.int64, device="cuda")
    cent = torch.from_numpy(np.array([old, old[::-1]], np.uint16).view(np.int16)).cuda()
    from gabor_color_image_segmentation_amd import _lib
    _lib.check(seg.ops.lib.gcs_kmeans_finalize(s.data_ptr(), n_sets, k, d, cent.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "gcs_kmeans_finalize")
    got = cent.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, np.array([want, want[::-1]], np.uint16))
    assert max(max(r[:-1]) for r in sums) >= (1 << 38) and np.array(want).max() == hb.G_MAX and 32768 in np.array(want)


@pytest.mark.parametrize("b,h,w,n_sets", [(64, 321, 481, 1), (3, 64, 96, 1), (3, 64, 96, 3), (64, 321, 481, 64)])
def test_reduce_finalize_on_written_partials(torch_cuda, b, h, w, n_sets):
    """gcs_kmeans_reduce_finalize and gcs_kmeans_reduce alone, on partial rows the test writes (layout: csrc/common.h, [set][chunk
    of 16 elements][row][16] uint64): the sums of _update_cases cut into random per-row shares, for the 64-row-group form (more than
    64 rows per set) and the 16-row-group form; sums == the totals, centroids == floor((2 S + n) / (2 n)) in Python integers."""
    torch = torch_cuda
    d, k = 72, 16
    seg = hb.hot_segmenter(hb.hot_bank(4, 6, 13, 7), k=k)
    lib = seg.ops.lib
    parts = lib.gcs_kmeans_parts_per_image(b, h, w)
    rows = parts if n_sets == b else b * parts
    row_len = k * (d + 1)
    nch = (row_len + 15) // 16
    assert lib.gcs_kmeans_partial_bytes(b, h, w, d, k) == n_sets * nch * rows * 16 * 8
    old, sums, want = _update_cases(d, k)
    flat = np.array([v for r in sums for v in r], np.int64)                              # (row_len,)
    rng = np.random.default_rng(b + n_sets)
    par = np.zeros((n_sets, nch, rows, 16), np.uint64)
    for s in range(n_sets):
        cuts = np.sort(rng.integers(0, flat + 1, (rows - 1, row_len)), axis=0)          # random shares that add up exactly
        share = np.diff(np.concatenate([np.zeros((1, row_len), np.int64), cuts, flat[None]]), axis=0)
        padded = np.zeros((rows, nch * 16), np.int64)
        padded[:, :row_len] = share
        par[s] = padded.reshape(rows, nch, 16).transpose(1, 0, 2).astype(np.uint64)
    partials = torch.from_numpy(par.view(np.int64)).cuda()
    cent = torch.from_numpy(np.array([old] * n_sets, np.uint16).view(np.int16)).cuda()
    out = seg.ops.new_sums(n_sets, k)
    seg.ops.reduce_finalize(partials, b, h, w, k, n_sets, out, cent)
    assert np.array_equal(out.cpu().numpy().reshape(n_sets, -1), np.tile(flat, (n_sets, 1)))
    assert np.array_equal(cent.cpu().numpy().view(np.uint16), np.array([want] * n_sets, np.uint16))
    out2 = seg.ops.new_sums(n_sets, k)
    seg.ops.reduce(partials, b, h, w, k, n_sets, out2)
    assert torch.equal(out2, out)
    assert (rows > 64) == (b == 64 and n_sets == 1) and np.array(want).max() == hb.G_MAX


# ------------------------------------------------------------------------------------------ end to end
# one bank per pass family: (n_scales, n_orient, ksize, shift, k)
E2E_CASES = [((4, 6, 13, 7, 8), "split_k8"), ((4, 6, 13, 8, 16), "split_k16"), ((2, 3, 7, 7, 8), "split_one_level"),
             ((5, 5, 13, 7, 8), "wide_slab_narrow"), ((5, 6, 13, 7, 8), "native_3_levels"), ((8, 8, 15, 8, 8), "native_4_levels"),
             ((3, 9, 15, 7, 4), "wide_8_waves"), ((8, 8, 15, 7, 13), "wide_k13"), ((7, 10, 13, 7, 4), "generic")]


@pytest.mark.parametrize("case", [c for c, _ in E2E_CASES], ids=[i for _, i in E2E_CASES])
def test_labels_end_to_end(torch_cuda, case):
    """segment_batch and segment_device == the C oracle on a hot bank, both codebook modes, five passes (forward and reverse
    sweeps, centroids with bit 15 set from the second pass on)."""
    torch = torch_cuda
    ns, no, ks, shift, k = case
    bank = hb.hot_bank(ns, no, ks, shift)
    seg = hb.hot_segmenter(bank, k=k, n_iter=5)
    b, h, w = 5, 81, 121
    imgs = hb.hot_images(b, h, w, seed=23)
    feats = _ref_features((ns, no, ks, shift), imgs).reshape(b, 3 * ns * no, -1)
    assert feats.max() >= 32768
    for mode in ("per_image", "global"):
        if mode == "global":
            want, cent = co.kmeans(feats, k, 5)
            assert cent.max() >= 32768
            want = want.reshape(b, h, w)
        else:
            want = np.stack([co.kmeans(feats[i:i + 1], k, 5)[0].reshape(h, w) for i in range(b)])
        got = seg.segment_device(torch.from_numpy(imgs).cuda(), mode=mode).cpu().numpy()
        assert np.array_equal(got, want), (mode, "device", int((got != want).sum()))
        got = seg.segment_batch(imgs, mode=mode)
        assert np.array_equal(got, want), (mode, "host", int((got != want).sum()))
        assert np.array_equal(seg.segment_batch(imgs, mode=mode, out_dtype=np.uint8), want), (mode, "uint8")


def test_labels_through_the_captured_graph_and_the_chunked_host_path(torch_cuda):
    """B = 1 called twice (capture, then replay, on different images) and 8 x 321x481 (more than 2^20 pixels: the chunked upload
    path of segment_batch) on the 4x6 shift-8 bank == the C oracle."""
    bank = hb.hot_bank(4, 6, 13, 8)
    seg = hb.hot_segmenter(bank, n_iter=4)
    for seed in (1, 2):
        img = hb.hot_images(3, 321, 481, seed=seed)[seed:seed + 1]
        want = co.segment_batch(img, bank.tapq, bank.shift, 6, k=8, n_iter=4)
        assert np.array_equal(seg.segment_batch(img), want), seed
    assert len(seg._graphs) == 1
    imgs = hb.hot_images(8, 321, 481, seed=4)
    assert _ref_features((4, 6, 13, 8), imgs).max() >= 32768
    for mode in ("per_image", "global"):
        want = co.segment_batch(imgs, bank.tapq, bank.shift, 6, k=8, n_iter=4, mode=mode)
        assert np.array_equal(seg.segment_batch(imgs, mode=mode), want), mode


def test_batch_64_global_codebook_every_label(torch_cuda):
    """The timed shape, 64 x 321x481, on the 4x6 shift-7 bank with one global codebook: every label == the C oracle. The only size at
    which the split pass's `nt` loads and full accumulators meet large values (a cluster sum reaches 1e11 here)."""
    bank = hb.hot_bank(4, 6, 13, 7)
    imgs = hb.hot_images(64, 321, 481, seed=0)
    x = np.stack([co.gabor_features(im, bank.tapq, bank.shift, 6) for im in imgs]).reshape(64, 72, -1)
    assert x.max() >= 46000 and (x >= 32768).mean() > 0.01
    want, cent = co.kmeans(x, 8, 6)
    assert cent.max() >= 32768 and len(np.unique(want)) == 8
    got = hb.hot_segmenter(bank, n_iter=6).segment_batch(imgs, "global")
    assert np.array_equal(got.reshape(64, -1), want), int((got.reshape(64, -1) != want).sum())


# ------------------------------------------------------------------------------------------ smoothing
SMOOTH_BANKS = [(4, 6, 13, 7), (2, 6, 13, 8), (8, 8, 15, 8), (5, 6, 13, 7)]          # split 2 levels, split 1 level, wide 4 and 3 levels


@pytest.mark.parametrize("cfg", SMOOTH_BANKS, ids=lambda c: "%dx%d_ks%d_shift%d" % c)
@pytest.mark.parametrize("K", [0.5, 1.0, K_MAX])
def test_smoothed_hot_slabs(torch_cuda, cfg, K):
    """gcs_smooth_features on hot slabs == tests/smooth_ref.py: row sums of 4096 * 46 000 in 32 bits, column sums on their 16-bit
    halves, TOP nibbles up to 11 through smooth.hip's unpack and pack. For the split banks the flag words after smoothing are
    again set exactly where a smoothed level-L value is >= 4096."""
    torch = torch_cuda
    ns, no = cfg[:2]
    seg = hb.hot_segmenter(hb.hot_bank(*cfg), smoothing=K)
    top = 0
    for h, w, b in ((8, 8, 3), (9, 13, 3), (81, 121, 3), (321, 481, 1)):
        imgs = hb.hot_images(b, h, w, seed=h * w)
        raw = _ref_features(cfg, imgs)
        feats = seg.ops.feature_slab(b, h, w)
        seg.ops.gabor_features(torch.from_numpy(imgs).cuda(), feats)
        seg.ops.smooth_features(feats, b, h, w)
        got = seg.ops.features_unpack(feats, b, h, w).cpu().numpy().view(np.uint16)
        want = np.stack([sr.smooth_features(raw[i], K, ns, no) for i in range(b)])
        assert np.array_equal(got, want), ((h, w), K, int((got != want).sum()))
        if ns <= 4:
            _check_flags(seg, feats, want, b, h, w)
        if h * w > 1000:
            assert raw.max() >= 32768
        top = max(top, int(want.max()))
    assert top >= 32768, top                                                   # bit 15 survives the smoothing somewhere


def test_labels_with_smoothing(torch_cuda):
    """Segmenter(smoothing=1.0) on a hot bank == restated features + co.kmeans, both codebook modes."""
    cfg = (4, 6, 13, 7)
    seg = hb.hot_segmenter(hb.hot_bank(*cfg), smoothing=1.0, n_iter=5)
    b, h, w = 4, 97, 131
    imgs = hb.hot_images(b, h, w, seed=41)
    x = np.stack([sr.smooth_features(f, 1.0, 4, 6) for f in _ref_features(cfg, imgs)]).reshape(b, 72, -1)
    assert x.max() >= 32768
    want = co.kmeans(x, 8, 5)[0].reshape(b, h, w)
    assert np.array_equal(seg.segment_batch(imgs, "global"), want)
    want = np.stack([co.kmeans(x[i:i + 1], 8, 5)[0].reshape(h, w) for i in range(b)])
    assert np.array_equal(seg.segment_batch(imgs), want)
