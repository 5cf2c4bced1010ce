"""Every scorer entry off the BSD image shape: the fixture of tests/golden/make_scoring_edge_golden.py (13 shapes from 1x70 to
65x129 around the 16 x 64 tiles of boundary_counts_kernel and the 64-bit words of the bit-plane scorer; noise, stripes,
checkerboards, block grids, tile-seam and corner maps; 1 / 3 / 9 annotators, labels above 255) through

* the integer entries (gcs_boundary_counts[_batch|_resident], gcs_region_counts[_batch[_u8]], gcs_region_reduce,
  gcs_score_batch_resident), bit for bit against NumPy / scipy restatements written here, outputs pre-filled with -1, and
* the scoring functions of evaluate_gpu against the numbers the reference's own metrics class gave for the same cases
  (tests/golden/scoring_edge_golden.json), raising cases included.

The label-side bit planes are READ from the scratch gcs_boundary_counts_resident leaves behind ([2][B][H][wp] words: boundary
planes, then dilated planes). gcs.h does not promise that layout to callers; this test pins it on purpose, because the planes are
otherwise only seen through sums."""
import numpy as np
import pytest

import scoring_edge
from scoring_edge import _assemble, _np_counts, _np_planes, _np_reduce, _np_tables, _np_tables_batch

pytestmark = pytest.mark.gpu
CASES = scoring_edge.load()
SHAPES = sorted({c[0].split("/")[0] for c in CASES}, key=lambda s: tuple(int(v) for v in s.split("x")))
EXACT_KEYS = ("regions", "recall", "precision", "underseg", "undersegNP", "density")
AGREE_KEYS = ("PRI", "VoI", "covering")
LDS_LIMIT = 48 * 1024           # region_counts_launch: workgroup-private tables while
                                # (max_annotators * n_segments * n_truth_labels + 2 * n_segments) * 4 <= 48 * 1024


# ------------------------------------------------------------------------------------------------ plumbing
def _lib():
    from gabor_color_image_segmentation_amd import _lib as L
    return L, L.load()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _dirty(n, dtype):
    """An output buffer that starts at -1 everywhere: nothing may rely on zeros."""
    import torch
    return torch.full((max(int(n), 1),), -1, dtype=dtype, device="cuda")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _by_shape(shape, want=lambda key, gold: True):
    return [(k, l, t, g) for k, l, t, g in CASES if k.startswith(shape + "/") and want(k, g)]


def _unpack(words, m, h, w):
    """uint64 plane words [2][m][h][wp] -> bits [2][m][h][wp * 64]."""
    wp = (w + 63) // 64
    raw = words.cpu().numpy().view(np.uint64)[:2 * m * h * wp].reshape(2, m, h, wp)
    return np.unpackbits(raw.view(np.uint8), axis=-1, bitorder="little").reshape(2, m, h, wp * 64).astype(bool)


def _assert_planes(words, maps, what):
    m, h, w = maps.shape
    bits = _unpack(words, m, h, w)
    assert not bits[..., w:].any(), (what, "a bit at or beyond column W")
    want = _np_planes(maps)
    for p, name in enumerate(("boundary", "dilated")):
        bad = np.argwhere(bits[p][..., :w] != want[p])
        assert bad.size == 0, (what, name, "first differing (map, y, x):", bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ raw entries (device)
def _boundary_counts(lab, truth):
    import torch
    L, lib = _lib()
    a, h, w = truth.shape
    scratch = _dirty(lib.gcs_boundary_scratch_bytes(a, h, w), torch.uint8)
    counts = _dirty(1 + 3 * a, torch.int64)
    lab_d, truth_d = _dev(lab.astype(np.int32)), _dev(truth)         # (named: an input must outlive the call that reads it)
    L.check(lib.gcs_boundary_counts(lab_d.data_ptr(), truth_d.data_ptr(), a, h, w, scratch.data_ptr(), counts.data_ptr(),
                                    _stream()), "gcs_boundary_counts")
    return counts.cpu().numpy()


def _boundary_counts_batch(labs, truth, img_of):
    import torch
    L, lib = _lib()
    (b, h, w), t = labs.shape, len(truth)
    scratch = _dirty(lib.gcs_boundary_batch_scratch_bytes(b, t, h, w), torch.uint8)
    counts = _dirty(b + 3 * t, torch.int64)
    labs_d, truth_d, img_of_d = _dev(labs), _dev(truth), _dev(img_of)
    L.check(lib.gcs_boundary_counts_batch(labs_d.data_ptr(), truth_d.data_ptr(), img_of_d.data_ptr(), b, t, h, w,
                                          scratch.data_ptr(), counts.data_ptr(), _stream()), "gcs_boundary_counts_batch")
    return counts.cpu().numpy()


def _boundary_counts_resident(labs, dt):
    """counts [B + 3T], seg_max [B], and the scratch words the call leaves behind."""
    import torch
    L, lib = _lib()
    b, h, w = labs.shape
    scratch = _dirty(lib.gcs_bit_planes_bytes(b, h, w) // 8, torch.int64)
    counts, smax = _dirty(b + 3 * dt.t, torch.int64), _dirty(b, torch.int32)
    labs_d = _dev(labs)
    L.check(lib.gcs_boundary_counts_resident(labs_d.data_ptr(), dt.planes.data_ptr(), dt.bd_counts.data_ptr(),
                                             dt.img_of_d.data_ptr(), b, dt.t, h, w, scratch.data_ptr(), counts.data_ptr(),
                                             smax.data_ptr(), _stream()), "gcs_boundary_counts_resident")
    return counts.cpu().numpy(), smax.cpu().numpy(), scratch


def _region_counts(lab, truth, n_seg, stride):
    import torch
    L, lib = _lib()
    a, h, w = truth.shape
    hist, area, perim = _dirty(a * n_seg * stride, torch.int32), _dirty(n_seg, torch.int32), _dirty(n_seg, torch.int32)
    lab_d, truth_d = _dev(lab.astype(np.int32)), _dev(truth)
    L.check(lib.gcs_region_counts(lab_d.data_ptr(), truth_d.data_ptr(), a, h, w, n_seg, stride, hist.data_ptr(), area.data_ptr(),
                                  perim.data_ptr(), _stream()), "gcs_region_counts")
    return hist.cpu().numpy().reshape(a, n_seg, stride), area.cpu().numpy(), perim.cpu().numpy()


def _region_counts_batch(labs, truth, first, a_max, n_seg, stride, u8=False):
    import torch
    L, lib = _lib()
    (b, h, w), t = labs.shape, len(truth)
    hist, area, perim = _dirty(t * n_seg * stride, torch.int32), _dirty(b * n_seg, torch.int32), _dirty(b * n_seg, torch.int32)
    if u8:
        assert int(truth.max()) < 256
        fn, td = lib.gcs_region_counts_batch_u8, _dev(truth.astype(np.uint8))
    else:
        fn, td = lib.gcs_region_counts_batch, _dev(truth.astype(np.uint16))
    labs_d, first_d = _dev(labs), _dev(first)
    L.check(fn(labs_d.data_ptr(), td.data_ptr(), first_d.data_ptr(), b, t, a_max, h, w, n_seg, stride, hist.data_ptr(),
               area.data_ptr(), perim.data_ptr(), _stream()), "gcs_region_counts_batch" + ("_u8" if u8 else ""))
    return (hist.cpu().numpy().reshape(t, n_seg, stride), area.cpu().numpy().reshape(b, n_seg),
            perim.cpu().numpy().reshape(b, n_seg))


def _region_reduce(hist, area, img_of):
    import torch
    L, lib = _lib()
    t, n_seg, stride = hist.shape
    under, under_np = _dirty(t, torch.int64), _dirty(t, torch.int64)
    hist_d, area_d, img_of_d = _dev(hist.astype(np.int32)), _dev(area.astype(np.int32)), _dev(img_of)
    L.check(lib.gcs_region_reduce(hist_d.data_ptr(), area_d.data_ptr(), img_of_d.data_ptr(), t, n_seg, stride, under.data_ptr(),
                                  under_np.data_ptr(), _stream()), "gcs_region_reduce")
    return under.cpu().numpy(), under_np.cpu().numpy()


def _score_batch_resident(labs, dt, n_seg):
    """Every output of gcs_score_batch_resident at a table capacity of n_seg segments (host arrays, by name)."""
    import torch
    L, lib = _lib()
    b, h, w = labs.shape
    t, stride = dt.t, dt.stride
    scratch = _dirty(lib.gcs_bit_planes_bytes(b, h, w) // 8, torch.int64)
    hist, counts, smax = _dirty(t * n_seg * stride, torch.int32), _dirty(b + 3 * t, torch.int64), _dirty(b, torch.int32)
    area, perim = _dirty(b * n_seg, torch.int32), _dirty(b * n_seg, torch.int32)
    under, under_np = _dirty(t, torch.int64), _dirty(t, torch.int64)
    labs_d = _dev(labs)
    L.check(lib.gcs_score_batch_resident(labs_d.data_ptr(), dt.planes.data_ptr(), dt.bd_counts.data_ptr(), dt.maps.data_ptr(),
                                         1 if dt.u8 else 0, dt.first_d.data_ptr(), dt.img_of_d.data_ptr(), b, t, dt.a_max, h, w,
                                         n_seg, stride, scratch.data_ptr(), hist.data_ptr(), counts.data_ptr(), smax.data_ptr(),
                                         area.data_ptr(), perim.data_ptr(), under.data_ptr(), under_np.data_ptr(), _stream()),
            "gcs_score_batch_resident")
    return {"hist": hist.cpu().numpy().reshape(t, n_seg, stride), "counts": counts.cpu().numpy(), "seg_max": smax.cpu().numpy(),
            "area": area.cpu().numpy().reshape(b, n_seg), "perim": perim.cpu().numpy().reshape(b, n_seg),
            "under": under.cpu().numpy(), "under_np": under_np.cpu().numpy(), "scratch": scratch}


def _device_truth(truth, first, img_of):
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth
    return DeviceTruth(truth, first, img_of, [int(m.max()) + 1 for m in truth])


def _wide_batch(shape):
    """All cases of a shape that have annotators (ragged 1 / 3 / 9 / 3 maps per image) plus four more images that pair a
    label map with another case's annotators: 18 images, so that B > 16."""
    cs = _by_shape(shape, lambda k, g: not k.endswith("/a0"))
    items = [(l, t) for _, l, t, _ in cs]
    items += [(cs[(i + 5) % len(cs)][1], cs[i][2]) for i in range(4)]
    assert len(items) >= 17
    return cs, items


# ------------------------------------------------------------------------------------------------ integers, bit for bit
@pytest.mark.parametrize("shape", SHAPES)
def test_boundary_count_entries_bit_for_bit(built, shape):
    """gcs_boundary_counts per case; gcs_boundary_counts_batch and gcs_boundary_counts_resident on the shape's 18-image ragged
    batch: every one of the B + 3T words, seg_max, the resident annotator planes and the label planes in the scratch."""
    L, lib = _lib()
    cs, items = _wide_batch(shape)
    checked = 0
    for key, lab, truth, _ in cs:
        got = _boundary_counts(lab, truth)
        assert np.array_equal(got, _np_counts(lab[None], truth, np.zeros(len(truth), np.int32))), key
        checked += 1
    for key, lab, truth, _ in _by_shape(shape, lambda k, g: k.endswith("/a0")):    # no annotators: the entry refuses, writes nothing
        with pytest.raises(L.GcsError):
            _boundary_counts(lab, np.zeros((0,) + lab.shape, np.uint16))
        checked += 1
    assert checked == len(_by_shape(shape))
    labs, truth, first, img_of = _assemble(items)
    want = _np_counts(labs, truth, img_of)
    assert np.array_equal(_boundary_counts_batch(labs, truth, img_of), want), shape
    dt = _device_truth(truth, first, img_of)
    _assert_planes(dt.planes, truth, (shape, "annotator planes"))
    assert np.array_equal(dt.bd_counts.cpu().numpy(), want[len(labs) + 1::3])
    counts, smax, scratch = _boundary_counts_resident(labs, dt)
    assert np.array_equal(counts, want), shape
    assert smax.tolist() == [int(l.max()) for l in labs]
    _assert_planes(scratch, labs, (shape, "label planes"))


def test_label_maximum_in_the_last_partly_filled_word(built):
    """seg_max with large labels, the maximum alone in the last column of the last row (W % 64 = 1, 2, 63), and a batch whose
    plane words are no multiple of 4 (a workgroup of bits_boundary_kernel whose last waves have no word)."""
    rng = np.random.default_rng(5)
    for h, w in ((3, 65), (5, 130), (7, 63), (1, 70)):
        labs = rng.integers(0, 3, (3, h, w)).astype(np.int32)
        labs[0, h - 1, w - 1] = 2 ** 31 - 1
        labs[1, 0, w - 1] = 70000
        labs[2, h // 2, 0] = 300
        assert (3 * h * ((w + 63) // 64)) % 4 != 0
        truth = rng.integers(1, 4, (3, h, w)).astype(np.uint16)
        first, img_of = np.array([0, 1, 2, 3], np.int32), np.arange(3, dtype=np.int32)
        counts, smax, scratch = _boundary_counts_resident(labs, _device_truth(truth, first, img_of))
        assert smax.tolist() == [2 ** 31 - 1, 70000, 300]
        assert np.array_equal(counts, _np_counts(labs, truth, img_of))
        _assert_planes(scratch, labs, (h, w))


@pytest.mark.parametrize("shape", SHAPES)
def test_region_table_entries_bit_for_bit(built, shape):
    """gcs_region_counts per case, gcs_region_counts_batch on the 18-image batch (labels above 255: uint16 alone), and both the
    uint8 and the uint16 entry on the images whose annotator labels fit a byte - once with every label map (tables of up to
    338 segments) and once with the few-segment maps only (workgroup-private tables, B > 16)."""
    cs, items = _wide_batch(shape)
    for key, lab, truth, _ in cs:
        n_seg, stride = int(lab.max()) + 1, int(truth.max()) + 1
        got = _region_counts(lab, truth, n_seg, stride)
        for g, w, name in zip(got, _np_tables(lab, truth, n_seg, stride), ("hist", "area", "perim")):
            assert np.array_equal(g, w), (key, name)
    labs, truth, first, img_of = _assemble(items)
    n_seg, stride, a_max = int(labs.max()) + 1, int(truth.max()) + 1, int(np.diff(first).max())
    assert stride > 256 and a_max == 9
    want = _np_tables_batch(labs, truth, first, n_seg, stride)
    for g, w, name in zip(_region_counts_batch(labs, truth, first, a_max, n_seg, stride), want, ("hist", "area", "perim")):
        assert np.array_equal(g, w), (shape, name)
    narrow = [(l, t) for l, t in items if int(t.max()) < 256]
    few = [(l, t) for l, t in narrow if int(l.max()) < 5]
    for sub in (narrow, few):
        sub = (sub * 18)[:max(len(sub), 18)]                        # repeated to 18 images where fewer fit a byte
        labs, truth, first, img_of = _assemble(sub)
        n_seg, stride, a_max = int(labs.max()) + 1, int(truth.max()) + 1, int(np.diff(first).max())
        want = _np_tables_batch(labs, truth, first, n_seg, stride)
        g16 = _region_counts_batch(labs, truth, first, a_max, n_seg, stride)
        g8 = _region_counts_batch(labs, truth, first, a_max, n_seg, stride, u8=True)
        for a, b, w, name in zip(g16, g8, want, ("hist", "area", "perim")):
            assert np.array_equal(a, w), (shape, name, "uint16")
            assert np.array_equal(b, w), (shape, name, "uint8")


def _triples(words):
    """(max_annotators, n_segments, n_truth_labels) with max_annotators * n_segments * n_truth_labels + 2 * n_segments == words."""
    out = []
    for a in range(1, 12):
        for stride in range(1, 2001):
            if words % (a * stride + 2) == 0:
                out.append((a, words // (a * stride + 2), stride))
    return out


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_region_tables_at_the_edge_of_the_private_table_limit(built, delta):
    """Table sizes of exactly the limit of region_counts_launch, one counter below and one above it (the triples are DERIVED
    from its formula, so they follow the constant): the last size with workgroup-private tables and the first with global
    atomics count the same. uint16 entry, and the uint8 entry where the labels fit a byte."""
    words = LDS_LIMIT // 4 + delta
    found = _triples(words)
    assert found, words
    proper = [t for t in found if t[1] >= 2 and t[2] >= 2] or found     # (12 289 words is prime: one segment, 1 117 columns)
    picks = {}
    for t in sorted(proper, key=lambda t: -t[2]):                        # three of them, different annotator counts
        picks.setdefault(t[0], t)
    picks = list(picks.values())[:3] + [t for t in sorted(proper, key=lambda t: -t[2]) if t[2] <= 256][:1]   # and one for uint8
    rng = np.random.default_rng(words)
    h, w = 33, 193
    for a, n_seg, stride in picks:
        assert (a * n_seg * stride + 2 * n_seg) * 4 == LDS_LIMIT + 4 * delta
        items = [(rng.integers(0, n_seg, (h, w)), rng.integers(0, stride, (n, h, w))) for n in (a, 1, a)]
        labs, truth, first, img_of = _assemble(items)
        want = _np_tables_batch(labs, truth, first, n_seg, stride)
        forms = [False] + ([True] if stride <= 256 else [])
        for u8 in forms:
            got = _region_counts_batch(labs, truth, first, a, n_seg, stride, u8=u8)
            for g, wv, name in zip(got, want, ("hist", "area", "perim")):
                assert np.array_equal(g, wv), (a, n_seg, stride, name, u8)
        if a == 1:                                                   # the single-image entry sizes its tables by A
            got = _region_counts(labs[1], truth[first[1]:first[2]], n_seg, stride)
            for g, wv in zip(got, _np_tables(labs[1], truth[first[1]:first[2]], n_seg, stride)):
                assert np.array_equal(g, wv), (a, n_seg, stride)


@pytest.mark.parametrize("h,w", [(2, 2), (1, 70), (70, 1), (17, 65), (33, 193)])
def test_region_tables_skip_what_lies_outside_them(built, h, w):
    """max_annotators understated (1 where images bring 3: the private table for 1 fits, the kernel must not use it); labels
    >= n_segments (those pixels are in no table, all others are counted); annotator labels >= n_truth_labels (missing from
    hist alone). Each with small tables (workgroup-private) and with tables beyond the limit (global atomics)."""
    rng = np.random.default_rng(h * 1000 + w)
    items = [(rng.integers(0, 6, (h, w)), rng.integers(0, 10, (n, h, w))) for n in (3, 1, 3)]
    for lab, t in items:
        lab[0, 0], lab[h - 1, w - 1], t[:, 0, 0], t[:, h - 1, w - 1] = 5, 0, 9, 0
    labs, truth, first, img_of = _assemble(items)
    for n_seg, stride, a_max in ((6, 10, 1),            # understated max_annotators
                                 (3, 10, 3), (3, 10, 1),                     # labels 3, 4, 5 lie outside the tables
                                 (6, 4, 3), (4, 7, 1),                       # annotator labels 4 .. 9 (7 .. 9) lie outside hist
                                 (3, 2100, 3), (6, 2100, 1), (900, 10, 3)):  # the same beyond the private-table limit
        private = (a_max * n_seg * stride + 2 * n_seg) * 4 <= LDS_LIMIT
        assert private == (stride < 2100 and n_seg < 900)
        want = _np_tables_batch(labs, truth, first, n_seg, stride)
        if n_seg < 6:
            assert want[1].sum() < labs.size
        for u8 in (False, True) if stride <= 256 else (False,):
            got = _region_counts_batch(labs, truth, first, a_max, n_seg, stride, u8=u8)
            for g, wv, name in zip(got, want, ("hist", "area", "perim")):
                assert np.array_equal(g, wv), (n_seg, stride, a_max, name, u8)


@pytest.mark.parametrize("stride", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("n_seg", [1, 2, 3, 5, 8, 9])
def test_region_reduce_and_the_fused_scorer_against_numpy(built, n_seg, stride):
    """gcs_region_reduce on NumPy's tables, and every output of gcs_score_batch_resident (counts, seg_max, tables, under,
    under_np), at the exact table size and at a capacity above the largest label (rows of zeros), against NumPy."""
    rng = np.random.default_rng(100 * n_seg + stride)
    h, w = 17, 65
    items = [(rng.integers(0, n_seg, (h, w)), rng.integers(0, stride, (n, h, w))) for n in (1, 3, 2)]
    for lab, t in items:
        lab[0, 0] = n_seg - 1
        t[:, h - 1, w - 1] = stride - 1                            # every image uses the last row, every map the last column
    labs, truth, first, img_of = _assemble(items)
    dt = _device_truth(truth, first, img_of)
    assert dt.stride == stride and dt.u8 == (stride <= 256)
    counts = _np_counts(labs, truth, img_of)
    for cap in (n_seg, n_seg + 3):
        hist, area, perim = _np_tables_batch(labs, truth, first, cap, stride)
        under, under_np = _np_reduce(hist, area, img_of)
        got_u, got_n = _region_reduce(hist, area, img_of)
        assert np.array_equal(got_u, under) and np.array_equal(got_n, under_np), (cap, "gcs_region_reduce")
        got = _score_batch_resident(labs, dt, cap)
        for name, wv in (("counts", counts), ("seg_max", labs.reshape(len(labs), -1).max(axis=1)), ("hist", hist), ("area", area),
                         ("perim", perim), ("under", under), ("under_np", under_np)):
            assert np.array_equal(got[name], wv), (cap, name)
        _assert_planes(got["scratch"], labs, (n_seg, stride, "label planes of the fused scorer"))


# ------------------------------------------------------------------------------------------------ scores against the reference
def _assert_scores(got, ref, what):
    """The comparison of tests/test_gpu_scoring.py against the reference's numbers: the same floats, compactness to 1e-15."""
    for k in EXACT_KEYS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    assert abs(got["compactness"] - ref["compactness"]) <= 1e-15 * max(1.0, abs(ref["compactness"])), (what, "compactness")


def _assert_agreement(got, lab, truth, what):
    """The rule of tests/test_gpu_region_agreement.py against the host definition: PRI the same float, the rest within 1e-12."""
    from gabor_color_image_segmentation_amd.evaluate import region_agreement
    ref = region_agreement(lab, list(truth))
    assert got["PRI"] == ref["PRI"], what
    for k in AGREE_KEYS:
        assert abs(got[k] - ref[k]) <= 1e-12, (what, k, got[k], ref[k])


def _batched_forms(labs, truth, first, img_of, n_seg_exact):
    """Every batched way to score (name, callable returning the list of dicts); the resident ones build their DeviceTruth inside,
    because building it is where an image without annotators raises."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device, all_scores_batch_resident
    n_truth = [int(m.max()) + 1 for m in truth]
    dev = lambda: _dev(labs)
    dtf = lambda: _device_truth(truth, first, img_of)
    return [("host stack", lambda: all_scores_batch_device(dev(), truth, first, img_of, n_truth)),
            ("host stack, n_segments", lambda: all_scores_batch_device(dev(), truth, first, img_of, n_truth, n_segments=n_seg_exact)),
            ("DeviceTruth", lambda: all_scores_batch_device(dev(), dtf())),
            ("resident, n_segments=None", lambda: all_scores_batch_resident(dev(), dtf())),
            ("resident, exact", lambda: all_scores_batch_resident(dev(), dtf(), n_segments=n_seg_exact)),
            ("resident, larger", lambda: all_scores_batch_resident(dev(), dtf(), n_segments=2 * n_seg_exact + 7))]


def test_scores_equal_the_reference_on_every_fixture_case(built):
    """Single-image, batched (host stack and DeviceTruth) and resident scorers on every case of the fixture, one image at a time:
    the reference's numbers, or the exception the reference raised. Every case is checked; none is filtered out."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_device, boundary_scores_device
    seen = set()
    for key, lab, truth, ref in CASES:
        labs, first = lab[None], np.array([0, len(truth)], np.int32)
        img_of = np.zeros(len(truth), np.int32)
        forms = [("boundary_scores_device", lambda: [boundary_scores_device(_dev(lab), list(truth))]),
                 ("all_scores_device", lambda: [all_scores_device(_dev(lab), list(truth))])]
        forms += _batched_forms(labs, truth, first, img_of, int(lab.max()) + 1)
        for name, run in forms:
            if "raises" in ref:
                with pytest.raises(scoring_edge.ERRORS[ref["raises"]]):
                    run()
            elif name == "boundary_scores_device":
                got = run()[0]
                assert got["recall"] == ref["recall"] and got["precision"] == ref["precision"], (key, name)
            else:
                _assert_scores(run()[0], ref, (key, name))
        seen.add(key)
    assert len(seen) == len(CASES) == 195


@pytest.mark.parametrize("shape", SHAPES)
def test_batches_of_fixture_cases_equal_the_reference(built, shape):
    """All scoring cases of a shape in ONE batch (1, 3 and 9 annotators side by side; repeated to 17 images or more, past the grid
    change at B > 16) through every batched form: the reference's numbers per image; with agreement=True also PRI / VoI /
    covering of the host definition. Then the same batch with one degenerate image in its middle - a constant label map, an
    annotator map without a boundary, an image without annotators - raises what the reference raised for that image, and a
    label above n_segments raises ValueError in the resident form."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_device, all_scores_batch_resident
    good = _by_shape(shape, lambda k, g: "raises" not in g)
    assert {len(t) for _, _, t, _ in good} == {1, 3, 9}
    batch = (good * 17)[:max(17, len(good))]
    labs, truth, first, img_of = _assemble([(l, t) for _, l, t, _ in batch])
    n_seg = int(labs.max()) + 1
    for name, run in _batched_forms(labs, truth, first, img_of, n_seg):
        got = run()
        assert len(got) == len(batch)
        for (key, _, _, ref), g in zip(batch, got):
            _assert_scores(g, ref, (key, name))
    n_truth = [int(m.max()) + 1 for m in truth]
    dt = _device_truth(truth, first, img_of)
    for name, got in (("host stack", all_scores_batch_device(_dev(labs), truth, first, img_of, n_truth, agreement=True)),
                      ("resident", all_scores_batch_resident(_dev(labs), dt, agreement=True)),
                      ("resident, larger", all_scores_batch_resident(_dev(labs), dt, n_segments=3 * n_seg, agreement=True))):
        for (key, lab, t, ref), g in zip(batch, got):
            _assert_scores(g, ref, (key, name, "agreement=True"))
            _assert_agreement(g, lab, t, (key, name))
    for agreement in (False, True):                                  # one label too many for the stated n_segments
        with pytest.raises(ValueError):
            all_scores_batch_resident(_dev(labs), dt, n_segments=n_seg - 1, agreement=agreement)
    bad = _by_shape(shape, lambda k, g: "raises" in g)
    kinds = {"constant label map": [c for c in bad if "/constant/" in c[0]][0],
             "annotator without a boundary": [c for c in bad if c[0].endswith("/a3const")][0],
             "no annotators": [c for c in bad if c[0].endswith("/a0")][0]}
    for what, (key, lab, t, ref) in kinds.items():
        mixed = batch[:5] + [(key, lab, t, ref)] + batch[5:9]
        labs, truth, first, img_of = _assemble([(l, t) for _, l, t, _ in mixed])
        for name, run in _batched_forms(labs, truth, first, img_of, int(labs.max()) + 1):
            with pytest.raises(scoring_edge.ERRORS[ref["raises"]]):
                run()
        healthy = mixed[:5] + mixed[6:]                              # the same batch without that image scores
        labs, truth, first, img_of = _assemble([(l, t) for _, l, t, _ in healthy])
        for (k2, _, _, r2), g in zip(healthy, all_scores_batch_resident(_dev(labs), _device_truth(truth, first, img_of))):
            _assert_scores(g, r2, (k2, "after", what))


# ------------------------------------------------------------------------------------------------ one result block per DeviceTruth
def test_one_uncollected_submission_per_device_truth(built):
    """A second submission against the SAME DeviceTruth while the first is uncollected raises (it would overwrite the first one's
    result block); collecting, or dropping, the first clears the way; submissions against DIFFERENT DeviceTruth objects stay
    pipelined and give what their separate, synchronous runs give."""
    from gabor_color_image_segmentation_amd.evaluate_gpu import all_scores_batch_resident, submit_scores_batch_resident
    good = _by_shape("33x193", lambda k, g: "raises" not in g)
    one, two = good[:5], good[5:10]
    labs1, truth, first, img_of = _assemble([(l, t) for _, l, t, _ in one])
    labs2 = np.stack([l for _, l, _, _ in two]).astype(np.int32)      # other label maps, the same annotators
    assert not np.array_equal(labs1, labs2)
    dt = _device_truth(truth, first, img_of)
    ref1, ref2 = all_scores_batch_resident(_dev(labs1), dt), all_scores_batch_resident(_dev(labs2), dt)
    assert ref1 != ref2
    for (key, _, _, ref), g in zip(one, ref1):
        _assert_scores(g, ref, key)
    p1 = submit_scores_batch_resident(_dev(labs1), dt)
    with pytest.raises(RuntimeError, match="one result block per DeviceTruth"):
        submit_scores_batch_resident(_dev(labs2), dt)
    assert p1.result() == ref1                                       # the refused submission left the first one's numbers alone
    with pytest.raises(RuntimeError):
        p1.result()                                                  # collected once: the block belongs to the next submission
    p2 = submit_scores_batch_resident(_dev(labs2), dt)               # collected: the next one goes through
    assert p2.result() == ref2
    p3 = submit_scores_batch_resident(_dev(labs1), dt)
    del p3                                                           # dropped uncollected: clears the way as well
    assert submit_scores_batch_resident(_dev(labs2), dt).result() == ref2
    # a submission that raises on collection (a constant label map) is collected all the same
    p4 = submit_scores_batch_resident(_dev(np.zeros_like(labs1)), dt)
    with pytest.raises(ZeroDivisionError):
        p4.result()
    assert submit_scores_batch_resident(_dev(labs1), dt).result() == ref1
    # two DeviceTruth objects: both enqueued before either is collected, collected in either order
    labs_b, truth_b, first_b, img_of_b = _assemble([(l, t) for _, l, t, _ in two])
    dt_b = _device_truth(truth_b, first_b, img_of_b)
    ref_b = all_scores_batch_resident(_dev(labs_b), dt_b)
    for (key, _, _, ref), g in zip(two, ref_b):
        _assert_scores(g, ref, key)
    for order in ((0, 1), (1, 0)):
        pend = [submit_scores_batch_resident(_dev(labs1), dt), submit_scores_batch_resident(_dev(labs_b), dt_b)]
        got = {i: pend[i].result() for i in order}
        assert got[0] == ref1 and got[1] == ref_b, order
