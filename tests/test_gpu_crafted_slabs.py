"""Every kernel that reads the feature slab, on slabs the TESTS wrote (tests/slab_codec.py) instead of the Gabor stage: the whole
16-bit range - SPEC.md §3 and include/gcs.h call everything downstream of the Gabor stage exact for every uint16, and the Gabor
stage itself never writes a value above 46 340 -, flagged beside unflagged tiles and levels, no-pixel slots holding either filler,
and shapes below the Gabor stage's 8 x 8. Everything is compared bit for bit with integer references.

First the codec is held to the library (random-byte slabs through gcs_features_unpack; Gabor-written slabs against pack(C oracle)),
then it defines what a slab means. Contents, each asserted on the input: *any16* (uniform over all 65 536 values, 0xFFFF planted),
*edges* (draws from EDGE_VALUES with the values >= 0x1000 confined to chosen (image, level, tile) triples) and *ceiling* (every
feature 0xFFFF); each packed with filler 0x00 and 0xFF in the no-pixel slots (non-zero TOP nibbles there set no flag).

Mutants of the library that change a value and never an address, a loop bound, a barrier or a launch shape, run once against this
file (failed tests here) and against the earlier tests of the mutated kernel (failed tests there; the files are named in DESIGN.md
§7, "Crafted slabs"):
(a) the split pass's TOP unpack masks the nibble with 7: 15 here (9 test_lloyd_pass, 6 test_self_updating_loop), 58 before - the
    suite caught it already;
(b) the same unpack swaps bits 2 and 3 of the nibble: 15 here, 60 before (nibbles 4 .. 11 change too, and the hot banks reach them);
(c) the same unpack reads the nibbles 12 .. 15 as 8 .. 11: 15 here, none before - no slab the library writes holds a value of 49 152;
(d) KM_CHUNK = 192 in the generic pass: 1 here (test_lloyd_pass[generic_D210_k16], on the near-tie rows of the ceiling codebook: its
    four constant rows alone are too far apart for an error of 2^15 in x . c to move a label), none before;
(e) ke_level squares |x - c| as a signed 32-bit number: 14 here, 21 before (the earlier codebooks hold an all-65535 row);
(f) slab_next reads the TOP nibble whatever the flag says: none here, none before - equivalent on every legal slab, where a pixel's
    TOP nibble under an unset flag is zero;
(g) gcs_kmeans_init keeps 15 bits: 6 here, 14 before."""
import functools

import numpy as np
import pytest

import feature_gradient_ref as fg
import fused_workspace as fw
import hot_banks as hb
import kmeans_model_ref as km
import position_ref as pr
import slab_codec as sc
import smooth_ref as sr
from lloyd_ref import _pass_reference, updated
from oracle import spec_oracle as so
from pass_cases import K_MAX, PASS_CASES

pytestmark = pytest.mark.gpu

B = 3
SHAPES = [(1, 1), (5, 9), (9, 10), (16, 17), (17, 16), (13, 21), (33, 41)]    # below the Gabor stage; both strips and the corner; one
GABOR_SHAPES = SHAPES[2:]                                                      # strip each; ragged, unpacked; several tiles
CONTENTS = ("any16", "edges", "ceiling")
FILLERS = (0x00, 0xFF)
EDGE_VALUES = np.array([0, 0xFF, 0x100, 0xFFF, 0x1000, 0x7FFF, 0x8000, 0xB504, 0xB505, 0xFF00, 0xFFFF], np.uint16)
CEILING_ROWS = (0, 0x00FF, 0xFF00, 0xFFFF)
# one bank per slab format and pyramid depth: (n_scales, n_orient, ksize, shift) of tests/hot_banks.py
READER_BANKS = {"split_4x6": (4, 6, 13, 7),            # split slab, two levels
                "split_2x3": (2, 3, 7, 7),             # split slab, one level
                "wide_3x9": (3, 9, 15, 7),             # wide slab, two levels (D = 81), packed strips
                "three_5x6": (5, 6, 13, 7),            # three levels
                "deep_8x8": (8, 8, 15, 7),             # four levels, D = 192
                "d207_3x23": (3, 23, 9, 7)}            # D = 207: the most gcs_feature_gradient and gcs_region_tree_slab take
EVALUATE_BANKS = dict(READER_BANKS, generic_6x12=(6, 12, 13, 7))              # D = 216: past the matrix-core passes


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_OPS = {}


def _ops(cfg, smoothing=0.0):
    key = (cfg, smoothing)
    if key not in _OPS:
        from gabor_color_image_segmentation_amd.segmenter import HipOps
        _OPS[key] = HipOps(hb.hot_bank(*cfg), "cuda:0", smoothing)
    return _OPS[key]


# ------------------------------------------------------------------------------------------ crafted contents
class Crafted:
    """levels, canon (B, D, H, W) uint16, x (B, P, D) int64 and the slab bytes raw[filler] (B, img_bytes) of one content."""

    def __init__(self, geo, levels, content):
        self.geo, self.levels, self.content = geo, levels, content
        self.canon = geo.canonical(levels)
        self.h, self.w, self.d = geo.h, geo.w, geo.d
        self.x = self.canon.reshape(B, geo.d, -1).transpose(0, 2, 1).astype(np.int64)
        self.raw = {f: geo.pack(levels, filler=f) for f in FILLERS}
        nop = geo.no_pixel_bits()
        assert np.array_equal(self.raw[0x00] ^ self.raw[0xFF], np.broadcast_to(nop[None], self.raw[0].shape))
        self.holds_no_pixel_slot = bool(nop.any())
        for f in FILLERS:
            assert np.array_equal(geo.unpack(self.raw[f]), self.canon)


def _tile_level_hot(geo, levels):
    """(B, n_levels, ntiles) bool: does level L of tile t hold a value >= 0x1000."""
    hot = np.zeros((B, geo.n_levels, geo.ntiles), bool)
    for lev in range(geo.n_levels):
        for t in range(geo.ntiles):
            hot[:, lev, t] = (levels[lev][:, :, geo.tile[lev] == t] >= 0x1000).any(axis=(1, 2))
    return hot


@functools.lru_cache(maxsize=12)         # (a test walks contents inside shapes: the last few are what the next bank's test reuses)
def crafted(shape, ns, no, content, top=65535):
    """The content of the module docstring for one (shape, bank), made once; every content is asserted here. ``top``: the largest
    value of any16 (46 340 for the one entry point whose domain ends there)."""
    geo = sc.geometry(shape[0], shape[1], ns, no)
    rng = np.random.default_rng([shape[0], shape[1], ns, no, CONTENTS.index(content)])
    sizes = [(B, len(geo.planes[lev]), geo.hl[lev], geo.wl[lev]) for lev in range(geo.n_levels)]
    if content == "any16":
        levels = [rng.integers(0, top + 1, s).astype(np.uint16) for s in sizes]
        levels[0][0, 0, 0, 0] = top                              # both ends, whatever the size (1 x 1 on D = 3 holds 9 values)
        levels[0][1, 0, 0, 0] = 0
        assert max(int(v.max()) for v in levels) == top and min(int(v.min()) for v in levels) == 0
        if top == 65535:
            assert levels[0].max() > 46340 and (levels[0] >> 12 == 15).any()
    elif content == "edges":
        hot = rng.random((B, geo.n_levels, geo.ntiles)) < 0.5
        hot[0] = True                                            # image 0: tile 0 flagged on every level, tile 1 (if any) on none
        hot[0, :, 1:2] = False
        hot[1, :, 0] = [lev == 0 for lev in range(geo.n_levels)]  # image 1, tile 0: level 0 flagged, the deeper ones not
        hot[2, :, 0] = False
        levels = []
        for lev, s in enumerate(sizes):
            v = EDGE_VALUES[rng.integers(0, len(EDGE_VALUES), s)]
            low = EDGE_VALUES[rng.integers(0, 4, s)]
            keep = hot[:, lev][:, geo.tile[lev]]                 # (B, H_L, W_L)
            v = np.where(keep[:, None], v, low)
            for i in range(B):
                for t in np.flatnonzero(hot[i, lev]):
                    y, x = np.argwhere(geo.tile[lev] == t)[0]
                    v[i, 0, y, x] = 0xB505
            levels.append(v.astype(np.uint16))
        got = _tile_level_hot(geo, levels)
        assert np.array_equal(got, hot) and got[0, :, 0].all() and not got[2, :, 0].any()
        assert geo.ntiles == 1 or not got[0, :, 1].any()         # flagged beside unflagged tiles
        assert geo.n_levels == 1 or (got[1, 0, 0] and not got[1, 1:, 0].any())     # ... and levels of one tile
        assert set(np.unique(np.concatenate([v.reshape(-1) for v in levels])).tolist()) <= set(EDGE_VALUES.tolist())
    else:
        levels = [np.full(s, 0xFFFF, np.uint16) for s in sizes]
    cr = Crafted(geo, levels, content)
    if geo.split:
        hot = _tile_level_hot(geo, levels)
        for f in FILLERS:
            assert np.array_equal(geo.flags(cr.raw[f])[:, :, :geo.n_levels] != 0, hot.transpose(0, 2, 1))
    if content == "ceiling":
        assert (cr.canon == 0xFFFF).all()
    assert cr.holds_no_pixel_slot                                # every shape here leaves slots without a pixel: the fillers differ
    return cr


def codebook(cr, k, n_sets, seed=0):
    """(n_sets, k, D) int64. ceiling: rows 0 .. 3 are all-0, all-0x00FF, all-0xFF00, all-0xFFFF, rotated by the set; the rows behind
    them are all-0xFFFF with ONE plane 0xFFFE, the plane moving through the physical planes from row to row: distance 1 from every
    pixel where the all-0xFFFF row is at distance 0, so a digit sum of x . c that loses one bit anywhere (the fp32 sums of the generic
    pass past 2^24: with a chunk of 192 planes instead of 128 every such row from physical plane 129 on wins) changes every label.
    Otherwise pixel vectors of the set's own images with row 1 a duplicate of row 0 (a tie: the lowest index wins), then the four
    constant rows."""
    d = cr.d
    if cr.content == "ceiling":
        physical = np.concatenate(cr.geo.planes)                 # logical feature of every physical plane (level-major)
        out = np.full((n_sets, k, d), 0xFFFF, np.int64)
        for s in range(n_sets):
            for j in range(min(k, 4)):
                out[s, j] = CEILING_ROWS[(j + s) % 4]
            for j in range(4, k):
                out[s, j, physical[((2 * (j - 4) + 1) * d) // (2 * (k - 4))]] = 0xFFFE
        return out
    rng = np.random.default_rng(seed + k)
    out = np.empty((n_sets, k, d), np.int64)
    for s in range(n_sets):
        pix = cr.x[s] if n_sets > 1 else cr.x.reshape(-1, d)
        rows = [pix[i] for i in rng.integers(0, len(pix), k)]
        rows[1:1] = [rows[0]]
        rows[2:2] = [np.full(d, v, np.int64) for v in (0xFFFF, 0, 0xFF00, 0x00FF)]
        out[s] = np.stack(rows[:k])
    return out


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cent_dev(torch, cent):
    return _dev(torch, cent.astype(np.uint16).view(np.int16))


def _diff(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {np.asarray(got).size} differ, first at {i}: got {np.asarray(got)[i]}, want {np.asarray(want)[i]}"


def _same(got, want, tag):
    assert np.array_equal(got, want), (tag, _diff(got, want))


# ------------------------------------------------------------------------------------------ B: the codec against the library
@pytest.mark.parametrize("bank", list(EVALUATE_BANKS))
def test_random_byte_slabs_unpack_like_the_codec(torch_cuda, bank):
    """Slabs of random bytes with every flag byte set (a legal slab's flag is set wherever a TOP nibble is non-zero, so every nibble
    counts for every reader): gcs_features_unpack == slab_codec.unpack."""
    torch = torch_cuda
    cfg = EVALUATE_BANKS[bank]
    ops = _ops(cfg)
    for h, w in SHAPES:
        geo = sc.geometry(h, w, cfg[0], cfg[1])
        assert geo.img_bytes == ops.lib.gcs_feature_slab_bytes(1, h, w, cfg[0], cfg[1])
        rng = np.random.default_rng(h * 100 + w)
        raw = rng.integers(0, 256, (B, geo.img_bytes), dtype=np.uint8)
        geo.set_flags(raw, 1)
        want = geo.unpack(raw)
        got = ops.features_unpack(_dev(torch, raw.reshape(-1)), B, h, w).cpu().numpy().view(np.uint16)
        _same(got, want, (bank, (h, w)))
        if h * w * geo.d > 100:
            assert want.max() > 46340 and (want >> 12 == 15).any()


@pytest.mark.parametrize("bank", list(READER_BANKS))
def test_gabor_written_slabs_are_the_packed_oracle_features(torch_cuda, bank):
    """gcs_gabor_features on hot images into poison-filled memory == pack(C-oracle features) on every bit that holds a pixel and
    on every flag word."""
    from fused_stages import ref_features
    torch = torch_cuda
    cfg = READER_BANKS[bank]
    ops = _ops(cfg)
    top = 0
    for h, w in [(8, 8)] + GABOR_SHAPES:
        geo = sc.geometry(h, w, cfg[0], cfg[1])
        imgs = hb.hot_images(B, h, w, seed=h + w)
        ref = ref_features(cfg, imgs)
        want = geo.pack(geo.levels_of(ref))
        assert np.array_equal(geo.unpack(want), ref)                # (the oracle's levels replicate as the codec says)
        pix = geo.pixel_bits()
        for poison in (0xA5, 0x5A):
            slab = torch.full((B * geo.img_bytes,), poison, dtype=torch.uint8, device="cuda")
            ops.gabor_features(_dev(torch, imgs), slab)
            got = slab.cpu().numpy().reshape(B, geo.img_bytes)
            _same((got ^ want) & pix[None], np.zeros_like(got), (bank, (h, w), poison, "pixel bits"))
            if geo.split:
                _same(geo.flags(got) != 0, geo.flags(want) != 0, (bank, (h, w), poison, "flag words"))
        top = max(top, int(ref.max()))
    assert top >= 32768


# ------------------------------------------------------------------------------------------ C: the Lloyd passes
def _window(h):
    return (h // 3, h - h // 4) if h >= 4 else (0, h)             # cuts a block wherever a block has four rows


@pytest.mark.parametrize("case", [c for c, _ in PASS_CASES], ids=[i for _, i in PASS_CASES])
def test_lloyd_pass_on_crafted_slabs(torch_cuda, case):
    """gcs_kmeans_assign_accumulate + gcs_kmeans_reduce and gcs_kmeans_assign_raster (int32, uint8): labels, every sum and every count
    == _pass_reference in int64, on every content, filler and shape; one codebook over whole images and one per image under a row
    window, each swept forward and backward. ceiling on the generic pass is 2 * 255 * 255 * 128 = 16 646 400 per digit sum, 0.8 %
    below 2^24."""
    torch = torch_cuda
    ns, no, ks, shift, k = case
    ident = dict(PASS_CASES)[case]
    ops = _ops((ns, no, ks, shift))
    for h, w in SHAPES:
        assert ops.lib.gcs_selftest_pass_kernel(h, w, ns, no, k).decode() == ident.split("_D")[0], (ident, (h, w))
        labels, partials = ops.label_slab(B, h, w), ops.partial_slab(B, h, w, k)
        for content in CONTENTS:
            cr = crafted((h, w), ns, no, content)
            runs = []
            for n_sets, rows in ((1, (0, h)), (B, _window(h))):
                cent = codebook(cr, k, n_sets)
                vote = np.zeros((B, h, w), bool)
                vote[:, rows[0]:rows[1]] = True
                want = _pass_reference(cr.x, cent, vote.reshape(B, -1))
                if content == "ceiling":
                    assert k < 4 or (cent.min(axis=2) == 0xFFFF).any(axis=1).all()       # both bytes 255 on both sides
                elif k >= 2:
                    assert not (want[0] == 1).any() and (want[0] == 0).any()      # the duplicate row lost every tie
                runs.append((n_sets, rows, _cent_dev(torch, cent), want))
            for filler in FILLERS:
                slab = _dev(torch, cr.raw[filler].reshape(-1))
                for n_sets, rows, cent, (want_lab, want_sums, want_cnt) in runs:
                    for reverse in (False, True):
                        tag = (ident, (h, w), content, filler, n_sets, rows, reverse)
                        sums = ops.new_sums(n_sets, k)
                        labels.fill_(255)
                        ops.assign_accumulate(slab, cent, B, h, w, k, n_sets, labels, partials, rows=rows, reverse=reverse)
                        ops.reduce(partials, B, h, w, k, n_sets, sums)
                        got = sums.cpu().numpy()
                        _same(labels[:B * h * w].view(B, h * w).cpu().numpy(), want_lab, tag + ("labels",))
                        _same(got[:, :, -1], want_cnt, tag + ("counts",))
                        _same(got[:, :, :-1], want_sums, tag + ("sums",))
                    for dt in (torch.int32, torch.uint8):
                        out = torch.full((B, h, w), 99, dtype=dt, device="cuda")
                        ops.assign_raster(slab, cent, B, h, w, k, n_sets, out, scratch_labels=labels, reverse=dt == torch.uint8)
                        _same(out.cpu().numpy().reshape(B, -1), want_lab, (ident, (h, w), content, filler, n_sets, str(dt)))


FUSED_CASES = [(c, i) for c, i in PASS_CASES if i.split("_D")[0] in ("split<1,3>", "split<1,3,2>")]


@pytest.mark.parametrize("case", [c for c, _ in FUSED_CASES], ids=[i for _, i in FUSED_CASES])
def test_self_updating_loop_of_two_passes_on_any16(torch_cuda, case):
    """gcs_kmeans_pass_fused, a complete loop of two passes == init / assign / update / assign in NumPy; afterwards every byte of the
    workspace but the two centroid arrays is zero, and the arrays hold the two passes' centroids."""
    torch = torch_cuda
    ns, no, ks, shift, k = case
    ops = _ops((ns, no, ks, shift))
    for h, w in SHAPES:
        cr = crafted((h, w), ns, no, "any16")
        parts = int(ops.lib.gcs_kmeans_parts_per_image(B, h, w))
        everything = np.ones((B, h * w), bool)
        for n_sets in (1, B):
            assert ops.lib.gcs_kmeans_fused_workspace_bytes(B, h, w, ns, no, k, n_sets) != 0
            init = np.stack([so.kmeans_init(cr.x[s], k) for s in range(n_sets)])
            _, sums, cnt = _pass_reference(cr.x, init, everything)
            second = updated(sums, cnt, init)
            want_lab = _pass_reference(cr.x, second, everything)[0]
            lay = (n_sets, fw.fold_rows(B, parts, n_sets, fw.env_fold_rows()), k, cr.d)
            for filler in FILLERS:
                tag = (dict(PASS_CASES)[case], (h, w), n_sets, filler)
                slab = _dev(torch, cr.raw[filler].reshape(-1))
                ws = ops.fused_workspace(B, h, w, k, n_sets)
                assert ws.numel() == fw.workspace_bytes(*lay)
                c0 = torch.full((n_sets, k, cr.d), -3, dtype=torch.int16, device="cuda")
                c1 = torch.full((n_sets, k, cr.d), -3, dtype=torch.int16, device="cuda")
                out = torch.full((B, h, w), 99, dtype=torch.int32, device="cuda")
                ops.assign_accumulate(slab, c0, B, h, w, k, n_sets, None, None, reverse=False, fused=(ws, 0))
                ops.assign_raster(slab, c1, B, h, w, k, n_sets, out, reverse=True, fused=(ws, 1))
                _same(c0.cpu().numpy().view(np.uint16), init, tag + ("centroids of pass 0",))
                _same(c1.cpu().numpy().view(np.uint16), second, tag + ("centroids of pass 1",))
                _same(out.cpu().numpy().reshape(B, -1), want_lab, tag + ("labels",))
                after = ws.cpu().numpy()
                v = fw.views(after, *lay)
                assert fw.is_as_found(after, *lay) and not any(p.any() for p in v.cent_pad), tag
                _same(v.cents[0], init, tag + ("centroid array 0",))
                _same(v.cents[1], second, tag + ("centroid array 1",))


@pytest.mark.parametrize("d,k", [(72, 16), (3, 4), (207, 8), (216, 5)])
def test_finalize_on_sums_of_0xffff_features(torch_cuda, d, k):
    """gcs_kmeans_finalize where every summed feature was 0xFFFF or just below: floor((2 S + n) / (2 n)) == lloyd_ref.updated, with
    n from 1 to 64 x 481 x 321 and empty clusters between full ones."""
    torch = torch_cuda
    ops = _ops(READER_BANKS["split_2x3"])
    n_big = 64 * 481 * 321
    counts = np.array([[1, 0, 2, n_big, 0, n_big - 1, 3, 1 << 20][j % 8] for j in range(k)], np.int64)
    rng = np.random.default_rng(d)
    old = rng.integers(0, 65536, (2, k, d))
    cnt = np.stack([counts, counts[::-1]])
    e = np.arange(d)[None, None, :] % 4
    n = cnt[:, :, None]
    # S = 65535 n (mean 65535), 65535 n - n // 2 (the half that rounds up to 65535), one less (65534), 65535 n - n (65534 exactly)
    cases = [65535 * n + 0 * e, 65535 * n - n // 2, np.maximum(65535 * n - n // 2 - 1, 0), 65534 * n + 0 * e]
    sums = np.where(n == 0, 0, np.choose(e, cases))
    want = updated(sums, cnt, old)
    assert want.max() == 65535 and (want == 65534).any() and int(sums.max()) > 1 << 39 and (want[cnt == 0] == old[cnt == 0]).all()
    s = _dev(torch, np.concatenate([sums, cnt[:, :, None]], axis=2).astype(np.int64))
    cent = _cent_dev(torch, old)
    from gabor_color_image_segmentation_amd import _lib
    _lib.check(ops.lib.gcs_kmeans_finalize(s.data_ptr(), 2, k, d, cent.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "gcs_kmeans_finalize")
    _same(cent.cpu().numpy().view(np.uint16), want, (d, k))


# ------------------------------------------------------------------------------------------ C: the other readers
@pytest.mark.parametrize("bank", list(READER_BANKS))
def test_init_and_gather_on_crafted_slabs(torch_cuda, bank):
    """gcs_kmeans_init == the SPEC.md §4 pixels and gcs_features_gather == every pixel of every image, with rows of b < 0 between."""
    torch = torch_cuda
    cfg = READER_BANKS[bank]
    ops = _ops(cfg)
    for h, w in SHAPES:
        yy, xx = (a.reshape(-1) for a in np.mgrid[0:h, 0:w])
        byx = np.concatenate([np.stack([np.full(h * w, i if i < B else -1 - i), yy, xx], 1) for i in (0, B, 1, 2, B + 1)]).astype(np.int32)
        assert (byx[:, 0] < 0).sum() == 2 * h * w
        for content in CONTENTS:
            cr = crafted((h, w), cfg[0], cfg[1], content)
            want_rows = np.where(byx[:, :1] >= 0, cr.canon[np.maximum(byx[:, 0], 0), :, byx[:, 1], byx[:, 2]], 0)
            for filler in FILLERS:
                slab = _dev(torch, cr.raw[filler].reshape(-1))
                for k in (1, 8, 16):
                    for n_sets in (1, B):
                        cent = torch.full((n_sets, k, cr.d), -1, dtype=torch.int16, device="cuda")
                        ops.kmeans_init(slab, B, h, w, k, n_sets, cent)
                        want = np.stack([so.kmeans_init(cr.x[i], k) for i in range(n_sets)])
                        _same(cent.cpu().numpy().view(np.uint16), want, (bank, (h, w), content, filler, k, n_sets))
                got = ops.features_gather(slab, B, h, w, _dev(torch, byx)).cpu().numpy().view(np.uint16)
                _same(got, want_rows, (bank, (h, w), content, filler, "gather"))
            if content != "edges":
                assert want_rows.max() > 46340


@pytest.mark.parametrize("bank", list(EVALUATE_BANKS))
def test_evaluate_on_crafted_slabs(torch_cuda, bank):
    """gcs_kmeans_evaluate: labels, best, second and the table == kmeans_model_ref.evaluate_batch, k = 1, 2, 3, 8, 16, one codebook
    and one per image; a pixel ON a centroid and a tie in every run off the ceiling."""
    torch = torch_cuda
    cfg = EVALUATE_BANKS[bank]
    ops = _ops(cfg)
    for h, w in SHAPES:
        for content in CONTENTS:
            cr = crafted((h, w), cfg[0], cfg[1], content)
            slabs = [_dev(torch, cr.raw[f].reshape(-1)) for f in FILLERS]
            for k in (1, 2, 3, 8, 16):
                for n_sets in (1, B):
                    cent = codebook(cr, k, n_sets, seed=h + w)
                    lab, best, second, stats = km.evaluate_batch(cr.x, cent)
                    if content != "ceiling":
                        assert (best == 0).any() and (k == 1 or (second == best).any())
                    elif k >= 4:
                        assert not best.any() and ((second == 1).all() if k > 4 else (second > 1).all())
                    cdev = _cent_dev(torch, cent)
                    for filler, slab in zip(FILLERS, slabs):
                        outs = dict(labels=torch.full((B, h, w), -77, dtype=torch.int32, device="cuda"),
                                    best=torch.full((B, h, w), -77, dtype=torch.int64, device="cuda"),
                                    second=torch.full((B, h, w), -77, dtype=torch.int64, device="cuda"),
                                    stats=torch.full((n_sets, k, 2), -77, dtype=torch.int64, device="cuda"))
                        ops.kmeans_evaluate(slab, cdev, B, h, w, k, n_sets, **outs)
                        tag = (bank, (h, w), content, k, n_sets, filler)
                        _same(outs["labels"].cpu().numpy().reshape(B, -1), lab, tag + ("labels",))
                        _same(outs["best"].cpu().numpy().reshape(B, -1), best, tag + ("best",))
                        _same(outs["second"].cpu().numpy().reshape(B, -1), second, tag + ("second",))
                        _same(outs["stats"].cpu().numpy(), stats, tag + ("stats",))


@pytest.mark.parametrize("bank", list(EVALUATE_BANKS))
def test_evaluate_distance_at_the_ceiling(torch_cuda, bank):
    """Every feature 0xFFFF against an all-zero centroid (and the reverse): best = D * 65535^2, the largest distance there is."""
    torch = torch_cuda
    cfg = EVALUATE_BANKS[bank]
    ops = _ops(cfg)
    h, w = 13, 21
    cr = crafted((h, w), cfg[0], cfg[1], "ceiling")
    cent = np.zeros((1, 2, cr.d), np.int64)
    cent[0, 1, 0] = 1
    lab, best, second, stats = km.evaluate_batch(cr.x, cent)
    assert (best == cr.d * 65535 ** 2 - 2 * 65535 + 1).all() and (lab == 1).all()
    for filler in FILLERS:
        outs = dict(labels=torch.full((B, h, w), -77, dtype=torch.int32, device="cuda"),
                    best=torch.full((B, h, w), -77, dtype=torch.int64, device="cuda"),
                    second=torch.full((B, h, w), -77, dtype=torch.int64, device="cuda"),
                    stats=torch.full((1, 2, 2), -77, dtype=torch.int64, device="cuda"))
        ops.kmeans_evaluate(_dev(torch, cr.raw[filler].reshape(-1)), _cent_dev(torch, cent), B, h, w, 2, 1, **outs)
        _same(outs["labels"].cpu().numpy().reshape(B, -1), lab, (bank, filler, "labels"))
        _same(outs["best"].cpu().numpy().reshape(B, -1), best, (bank, filler, "best"))
        _same(outs["second"].cpu().numpy().reshape(B, -1), second, (bank, filler, "second"))
        _same(outs["stats"].cpu().numpy(), stats, (bank, filler, "stats"))


@pytest.mark.parametrize("bank", list(READER_BANKS))
def test_feature_gradient_on_crafted_slabs(torch_cuda, bank):
    torch = torch_cuda
    cfg = READER_BANKS[bank]
    ops = _ops(cfg)
    for h, w in SHAPES:
        for content in CONTENTS:
            cr = crafted((h, w), cfg[0], cfg[1], content)
            want = np.stack([fg.gradient(cr.canon[i], cfg[0], cfg[1]) for i in range(B)])
            for filler in FILLERS:
                out = torch.full((B, h, w), -7, dtype=torch.int32, device="cuda")
                ops.feature_gradient(_dev(torch, cr.raw[filler].reshape(-1)), B, h, w, out)
                _same(out.cpu().numpy(), want, (bank, (h, w), content, filler))
            if content == "ceiling":
                assert not want.any()                            # a constant slab has no gradient
            elif content == "any16" and h * w > 100:
                assert int(want.max()) ** 2 > 1 << 32


@pytest.mark.parametrize("K", [1.0, K_MAX], ids=["K1", "Kmax"])
@pytest.mark.parametrize("bank", list(READER_BANKS))
def test_smoothing_on_crafted_slabs(torch_cuda, bank, K):
    """gcs_smooth_features in place: the canonical features afterwards == smooth_ref of those before; no-pixel bits keep what they
    held; flag bytes are set exactly where a smoothed value is >= 4096; and every bit that holds a pixel is pack() of the smoothed
    features - the TOP nibbles under an unset flag too, which gcs_slab_value (init, gather, unpack) reads whatever the flag says."""
    torch = torch_cuda
    cfg = READER_BANKS[bank]
    ops = _ops(cfg, smoothing=K)
    ns, no = cfg[:2]
    mixed = False
    for h, w in GABOR_SHAPES:
        geo = sc.geometry(h, w, ns, no)
        nop, pix = geo.no_pixel_bits(), geo.pixel_bits()
        for content in CONTENTS:
            cr = crafted((h, w), ns, no, content)
            want = np.stack([sr.smooth_features(cr.canon[i], K, ns, no) for i in range(B)])
            if content == "ceiling":
                assert (want == 0xFFFF).all()                    # taps that sum to 4096 twice: the largest accumulator there is
            for filler in FILLERS:
                tag = (bank, (h, w), content, filler, K)
                slab = _dev(torch, cr.raw[filler].reshape(-1))
                ops.smooth_features(slab, B, h, w)
                got = slab.cpu().numpy().reshape(B, geo.img_bytes)
                _same(geo.unpack(got), want, tag + ("values",))
                _same((got ^ cr.raw[filler]) & nop[None], np.zeros_like(got), tag + ("no-pixel bits",))
                packed = geo.pack(geo.levels_of(want), filler=filler)
                _same((got ^ packed) & pix[None], np.zeros_like(got), tag + ("pixel bits",))
                if geo.split:
                    _same(geo.flags(got) != 0, geo.flags(packed) != 0, tag + ("flag words",))
                    mixed = mixed or (0 < int((geo.flags(packed)[:, :, :geo.n_levels] != 0).sum()) < B * geo.ntiles * geo.n_levels)
    assert mixed or not geo.split                                # flagged beside unflagged (tile, level) pairs after smoothing too


@pytest.mark.parametrize("bank", list(READER_BANKS))
def test_position_features_on_any16_slabs(torch_cuda, bank):
    """gcs_position_features on an any16 slab: the coordinate planes are position_ref's, every other bit of the value bytes - the other
    planes, channel 2 of the slot, the no-pixel slots - is unchanged, and no flag byte is cleared."""
    torch = torch_cuda
    cfg = READER_BANKS[bank]
    ops = _ops(cfg)
    ns, no = cfg[:2]
    mu, top = 255, 0
    for h, w in GABOR_SHAPES:
        geo = sc.geometry(h, w, ns, no)
        cr = crafted((h, w), ns, no, "any16")
        for y0 in (0, 8):
            assert pr.in_domain(mu, y0 + h, w)
            f_n = ns * no
            slot = [c * f_n + s * no + no - 1 for c in range(2) for s in range(ns)]
            others = [d for d in range(cr.d) if d not in slot]
            want = np.stack([pr.fill_slot(cr.canon[i].copy(), ns, no, mu, y0) for i in range(B)])
            want[:, others] = cr.canon[:, others]                # (fill_slot zeroes channel 2 of the slot; the kernel keeps it)
            assert int(want[:, slot].max()) == mu * (max(y0 + h, w) - 1) and not np.array_equal(want[:, slot], cr.canon[:, slot])
            top = max(top, int(want[:, slot].max()))
            if geo.split:                                        # every TOP run counts, so every byte is held below
                assert (geo.flags(cr.raw[0])[:, :, :geo.n_levels] != 0).all()
            for filler in FILLERS:
                tag = (bank, (h, w), y0, filler)
                slab = _dev(torch, cr.raw[filler].reshape(-1))
                from gabor_color_image_segmentation_amd import _lib
                _lib.check(ops.lib.gcs_position_features(slab.data_ptr(), B, h, w, ns, no, mu, y0, torch.cuda.current_stream().cuda_stream),
                           "gcs_position_features")
                got = slab.cpu().numpy().reshape(B, geo.img_bytes)
                packed = geo.pack(geo.levels_of(want), filler=filler)
                _same(got[:, :geo.value_bytes], packed[:, :geo.value_bytes], tag + ("value bytes",))
                if geo.split:
                    before = geo.flags(cr.raw[filler]) != 0
                    _same(geo.flags(got) != 0, before | (geo.flags(packed) != 0), tag + ("flag words",))
    assert top >= 4096                                           # coordinates that reach the TOP nibbles


@pytest.mark.parametrize("bank", list(READER_BANKS))
def test_region_tree_slab_on_values_up_to_46340(torch_cuda, bank):
    """gcs_region_tree_slab in its own domain (SPEC.md §14: x <= 46 340), both ends present: merges, costs and alive ==
    cluster_tree_ref on the connected node map of a random blocky label map, on every shape (gcs_region_tree_slab takes any
    1 <= H, W <= 4096). 1 x 1 is one node: K = 1, no merge list (the entry point takes NULL then), and the sums at the head of the
    workspace are the pixel's features and a count of one; 5 x 9 may come out as one node per image as well."""
    import cluster_tree_ref as ctr
    torch = torch_cuda
    cfg = READER_BANKS[bank]
    ops = _ops(cfg)
    lib = ops.lib
    ns, no = cfg[:2]
    most = 0
    for h, w in SHAPES:
        cr = crafted((h, w), ns, no, "any16", top=46340)
        assert cr.canon.max() == 46340 and cr.canon.min() == 0
        rng = np.random.default_rng(h * w)
        coarse = rng.integers(0, 3, (B, -(-h // 4), -(-w // 5)))
        lab = coarse.repeat(4, axis=1).repeat(5, axis=2)[:, :h, :w].astype(np.int32)
        trees = [ctr.tree(cr.canon[i], lab[i]) for i in range(B)]
        k = max(int(t[0].max()) + 1 for t in trees)
        assert k >= 2 or h * w < 64
        most = max(most, k)
        nodes = np.stack([t[0] for t in trees]).astype(np.int32)
        nodes_dev = _dev(torch, nodes)
        for filler in FILLERS:
            slab = _dev(torch, cr.raw[filler].reshape(-1))
            ws = torch.full((lib.gcs_region_tree_workspace_bytes(B, h, w, cr.d, k),), 0xAB, dtype=torch.uint8, device="cuda")
            merges = torch.full((B, k - 1, 2), 7, dtype=torch.int32, device="cuda")
            costs = torch.full((B, k - 1), 7, dtype=torch.int64, device="cuda")
            alive = torch.full((B,), -5, dtype=torch.int32, device="cuda")
            mp, cp = (merges.data_ptr(), costs.data_ptr()) if k > 1 else (None, None)
            rc = lib.gcs_region_tree_slab(slab.data_ptr(), nodes_dev.data_ptr(), B, h, w, ns, no, k, ws.data_ptr(), mp, cp,
                                          alive.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.gcs_last_error()
            torch.cuda.synchronize()
            for i, (n_map, m, c, a) in enumerate(trees):
                tag = (bank, (h, w), filler, i)
                n = len(m)
                assert int(alive[i]) == a, tag
                _same(merges[i, :n].cpu().numpy(), m, tag + ("merges",))
                _same(costs[i, :n].cpu().numpy().view(np.uint64), c, tag + ("costs",))
                assert bool((merges[i, n:] == -1).all()) and not bool(costs[i, n:].any()), tag
            if k == 1:                                           # nothing merged: the head of the workspace is what the statistics wrote
                head = ws[:B * (cr.d + 1) * 8].cpu().numpy().view(np.uint64).reshape(B, cr.d + 1)
                _same(head[:, :-1], cr.x.sum(axis=1).astype(np.uint64), (bank, (h, w), filler, "sums"))
                assert (head[:, -1] == h * w).all()
    assert most >= 30
