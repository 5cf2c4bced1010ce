"""gcs_cue_gradient (SPEC.md §25, include/gcs_cues.h) on the GPU: every value compared with ``==`` against the NumPy restatement
(tests/cue_gradient_ref.py). Three different images per call. Shapes: 1 x 1, 1 x 7, 5 x 3 (several reflections at r = 8), 8 x 32
(exactly one tile), 9 x 33 (one pixel into the next tile both ways), 23 x 71 (ragged, several tiles); r in {1, 8, 15}, n in
{1, 3, 8, 16} (the three kernel instantiations), bins in {2, 16, 64}, K in {1, 8, 64}; every cue alone, four distinct weights, the
cues whose pointer is NULL; crafted images and maps (constant, a step in one channel, two cues stepping at right angles, noise
with all 64 bins in every window, 0 / 255 only, labels -1 and K), crafted mask tables (corner taps of the 31 x 31 frame, all
ones), the join with G (negative entries, the largest product), the buffer contract behind canary bands (tests/arena.py), the
argument rules, and the host paths on 64 x 48 crops of two val fixture images (``cue_edges_device`` against the restated chain,
a global codebook, PB alone, no Lloyd launch without the texton cue, replay from a captured graph, ``segment_cue_edges``, the
threshold sweep). The restatement's chi-squares of a plane are computed once per (plane, K, r, n, table) and shared."""
import importlib.util
import os

import numpy as np
import pytest

import cue_gradient_ref as cg
import texton_gradient_ref as tg
from arena import Arena, POISONS, ptr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (1, 7), (5, 3), (8, 32), (9, 33), (23, 71)]
# (r, n, bins, K): every value at least once, every pair of extremes once, n = 3 (chunk of 4), 8 (chunk of 8), 16 (two chunks)
COMBOS = [(1, 1, 2, 1), (8, 8, 16, 8), (15, 16, 64, 64), (1, 16, 64, 1), (15, 1, 2, 64), (1, 3, 2, 64), (15, 3, 64, 1),
          (8, 16, 2, 8), (8, 1, 64, 8), (15, 8, 16, 1), (1, 8, 16, 64), (8, 3, 16, 64)]
CACHE = {}                                                    # the restatement's chi-squares, shared by every test of the file


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    return Segmenter().ops


def _labels(shape, K, seed):
    """Three label maps of one shape: iid, blocky, and iid with -1 and K sprinkled."""
    h, w = shape
    rng = np.random.default_rng(seed)
    iid = rng.integers(0, K, size=shape).astype(np.int32)
    y, x = np.mgrid[0:h, 0:w]
    blocky = ((y // 11 * 3 + x // 13 + (y // 5) * (x // 29)) % K).astype(np.int32)
    holes = iid.copy()
    pick = rng.random(shape)
    holes[pick < 0.15] = -1
    holes[pick > 0.85] = K
    return np.stack([iid, blocky, holes])


def _images(shape, seed):
    """Three images of one shape: a dense one (64-bin value = a per-channel shuffle of (x % 8) + 8 (y % 8), random low bits: ANY
    8 x 8 pixels hold all 64 bins, so no bin is absent from a window that large), a smooth ramp with a different slope per channel
    (few bins per window: the skip), and iid 0 / 255 only."""
    h, w = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    dense = np.stack([rng.permutation(64)[x % 8 + 8 * (y % 8)] * 4 + rng.integers(0, 4, size=shape) for _ in range(3)],
                     axis=-1).astype(np.uint8)
    ramp = np.stack([(3 * x + y) % 256, (40 + 5 * y) % 256, (200 - 2 * x - 3 * y) % 256], axis=-1).astype(np.uint8)
    ends = (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    return np.stack([dense, ramp, ends])


def _st(torch):
    return torch.cuda.current_stream().cuda_stream


def _run(torch, ops, lab, img, K, bins, wts, r, n, grad=None, dirs=True, table=None):
    """The raw entry point on fresh device copies; ``lab`` / ``img`` None: a NULL pointer. Returns (out, dir or None)."""
    b, h, w = (lab if lab is not None else img).shape[:3]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dl, di, g = up(lab), up(img), up(grad)
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    d = torch.full((b, h, w), 77, dtype=torch.uint8, device="cuda") if dirs else None
    m = ops.texton_masks(r, n) if table is None else torch.from_numpy(np.ascontiguousarray(table).view(np.int32)).cuda()
    rc = ops.lib.gcs_cue_gradient(ptr(dl), ptr(di), b, h, w, K, cg.shift_of(bins), *wts, r, n, m.data_ptr(), ptr(g), out.data_ptr(),
                                  ptr(d), _st(torch))
    assert rc == 0, ops.lib.gcs_last_error()
    return out.cpu().numpy(), (d.cpu().numpy() if dirs else None)


def _want(lab, img, K, bins, wts, r, n, table=None):
    """(PB, dir) of every image of a batch by the restatement."""
    b = len(lab if lab is not None else img)
    res = [cg.cue_gradient(None if lab is None else lab[i], None if img is None else img[i], K, bins, wts, r, n, table, CACHE)
           for i in range(b)]
    return np.stack([p for p, _ in res]), np.stack([d for _, d in res])


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "r%d_n%d_b%d_K%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_and_parameter(torch_cuda, ops, shape, combo):
    """Four distinct weights (a swapped cue or channel shows), three different images and maps in one call; PB, dir, and the map
    joined with a G that has negative entries."""
    r, n, bins, K = combo
    wts = (1, 2, 3, 16)
    lab, img = _labels(shape, K, shape[0] * 1000 + shape[1] + r), _images(shape, shape[0] * 77 + shape[1] + n)
    want, wdir = _want(lab, img, K, bins, wts, r, n)
    got, dirs = _run(torch_cuda, ops, lab, img, K, bins, wts, r, n)
    _same(got, want, "PB")
    _same(dirs, wdir, "dir")
    grad = np.random.default_rng(r + n).integers(-3, 1 << 20, size=lab.shape).astype(np.int32)
    grad[:, 0, 0] = (1 << 20) - 1
    joined, dirs2 = _run(torch_cuda, ops, lab, img, K, bins, wts, r, n, grad=grad)
    _same(joined, np.stack([tg.joined(want[i], np.maximum(grad[i], 0)) for i in range(3)]), "E'")
    _same(dirs2, wdir, "dir beside the joined map")
    if shape == (1, 1):
        assert not got.any() and not dirs.any()               # one pixel mirrored everywhere: both halves agree
    elif shape == (23, 71):
        assert got.max(axis=(1, 2)).min() > 0 and len({a.tobytes() for a in got}) == 3
        if bins == 64:                                        # the dense image: no bin is absent from any tile's window
            for c in range(3):
                q = cg.quantise(img[0, ..., c], 64)
                assert all(len(np.unique(q[max(0, y - r):y + 8 + r, max(0, x - r):x + 32 + r])) == 64
                           for y in range(0, 23, 8) for x in range(0, 71, 32))


WEIGHT_CASES = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 1, 1, 1), (2, 2, 1, 1), (16, 16, 16, 16), (3, 0, 5, 0)]


@pytest.mark.parametrize("wts", WEIGHT_CASES, ids=lambda t: "w%d_%d_%d_%d" % t)
def test_weights_and_null_cues(torch_cuda, ops, wts):
    """Each cue alone and mixtures, at n = 8 and n = 16; a cue of weight 0 is given as a NULL pointer AND as a tensor of another
    content (it is not read either way). (1, 0, 0, 0) is gcs_texton_gradient's output on the same labels, dir included."""
    torch = torch_cuda
    shape, K, bins, r = (23, 71), 8, 16, 8
    lab, img = _labels(shape, K, 3), _images(shape, 4)
    for n in (8, 16):
        want, wdir = _want(lab, img, K, bins, wts, r, n)
        null_lab, null_img = (None if not wts[0] else lab), (None if not any(wts[1:]) else img)
        got, dirs = _run(torch, ops, null_lab, null_img, K, bins, wts, r, n)
        _same(got, want, ("NULL for unused cues", n))
        _same(dirs, wdir, ("dir", n))
        other_lab = lab if wts[0] else lab[::-1]
        other_img = img if any(wts[1:]) else img[::-1]
        got2, dirs2 = _run(torch, ops, other_lab, other_img, K, bins, wts, r, n)
        assert np.array_equal(got2, got) and np.array_equal(dirs2, dirs)
        if wts == (1, 0, 0, 0):
            dev = torch.from_numpy(lab).cuda()
            out = torch.full(lab.shape, -7, dtype=torch.int32, device="cuda")
            d = torch.full(lab.shape, 77, dtype=torch.uint8, device="cuda")
            ops.texton_gradient(dev, 3, shape[0], shape[1], K, r, n, None, out, d)
            assert np.array_equal(out.cpu().numpy(), got) and np.array_equal(d.cpu().numpy(), dirs)


@pytest.mark.parametrize("r", [1, 15])
@pytest.mark.parametrize("n", [3, 8, 16])
@pytest.mark.parametrize("shape", [(9, 33), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_texton_weight_alone_is_the_texton_kernel_byte_for_byte(torch_cuda, ops, shape, n, r):
    """gcs_cue_gradient at (1, 0, 0, 0) against gcs_texton_gradient on the same K = 64 maps: the map, dir, and the map joined with
    a G that has negative entries, at every dispatch arm of both kernels (n = 3, 8, 16) and both radius limits; 9 x 33 is two
    tiles each way, every one partial. The texton side is held to tests/texton_gradient_ref.py, so the two cannot be wrong
    together."""
    torch, K = torch_cuda, 64
    lab = _labels(shape, K, 500 + 10 * n + r)
    ref = [tg.texton_gradient(lab[i], K, r, n) for i in range(3)]
    want, wdir = np.stack([t for t, _ in ref]), np.stack([d for _, d in ref])
    # G: positive values with the sign flipped on a checkerboard, and -1, -5, INT32_MIN where TG > 0 in every map; a negative
    # entry joins as 0 (a kernel that dropped the clamp, or read G differently from the other, shows at those pixels)
    grad = np.random.default_rng(n * 31 + r).integers(1, 1 << 20, size=lab.shape).astype(np.int32)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    grad[:, (y + x) % 2 == 1] *= -1
    grad[:, 0, 0] = -1 if shape == (1, 1) else (1 << 20) - 1
    if shape == (9, 33):
        for i in range(3):
            at = np.argwhere(want[i] > 0)
            for (py, px), v in zip(at[[0, len(at) // 2, -1]], (-1, -5, np.iinfo(np.int32).min)):
                grad[i, py, px] = v
            assert (want[i][grad[i] < 0] > 0).sum() >= 3 and (want[i][grad[i] > 0] > 0).any()
    assert (grad < 0).any()
    dev, masks = torch.from_numpy(lab).cuda(), ops.texton_masks(r, n)
    for g, expect in ((None, want), (grad, np.stack([tg.joined(want[i], np.maximum(grad[i], 0)) for i in range(3)]))):
        out = torch.full(lab.shape, -7, dtype=torch.int32, device="cuda")
        d = torch.full(lab.shape, 77, dtype=torch.uint8, device="cuda")
        dg = None if g is None else torch.from_numpy(g).cuda()
        rc = ops.lib.gcs_texton_gradient(dev.data_ptr(), 3, shape[0], shape[1], K, r, n, masks.data_ptr(), ptr(dg), out.data_ptr(),
                                         d.data_ptr(), _st(torch))
        assert rc == 0, ops.lib.gcs_last_error()
        tex, tdir = out.cpu().numpy(), d.cpu().numpy()
        _same(tex, expect, "the texton kernel against the restatement")
        _same(tdir, wdir, "the texton kernel's dir against the restatement")
        got, dirs = _run(torch, ops, lab, None, K, 16, (1, 0, 0, 0), r, n, grad=g)
        assert got.tobytes() == tex.tobytes() and dirs.tobytes() == tdir.tobytes(), ("joined" if g is not None else "alone")
        if g is not None:
            assert not got[g < 0].any() and (shape == (1, 1) or got[g > 0].any())
    if shape == (9, 33):
        assert want.max(axis=(1, 2)).min() > 0                # (at 1 x 1 every value is 0: both halves agree)


def test_crafted_images(torch_cuda, ops):
    """A constant image and map; a step in one channel only, for each of the three (only that cue answers); two cues stepping at
    right angles (at the crossing the maximum of the sums is half the sum of the maxima); two cues whose edges lie 45 degrees
    apart (at the crossing PB is more than either cue's own maximum and less than their sum)."""
    torch = torch_cuda
    h, w, K, bins, r, n = 23, 71, 4, 16, 8, 8
    flat_lab = np.full((3, h, w), 2, np.int32)
    flat_img = np.stack([np.full((h, w, 3), v, np.uint8) for v in (0, 131, 255)])
    got, dirs = _run(torch, ops, flat_lab, flat_img, K, bins, (16, 16, 16, 16), r, n)
    assert not got.any() and not dirs.any()
    for ch in range(3):
        img = np.full((3, h, w, 3), 100, np.uint8)
        img[0, :, 30:, ch] = 180                              # a vertical edge, a horizontal edge, a diagonal one
        img[1, 11:, :, ch] = 180
        img[2, ...][np.add.outer(np.arange(h), np.arange(w)) > 40, ch] = 180
        for c in range(4):
            wts = tuple(5 if i == c else 0 for i in range(4))
            got, dirs = _run(torch, ops, flat_lab, img, K, bins, wts, r, n)
            want, wdir = _want(flat_lab, img, K, bins, wts, r, n)
            _same(got, want, (ch, c))
            _same(dirs, wdir, (ch, c, "dir"))
            assert bool(got.any()) == (c == ch + 1)
            if c == ch + 1:
                at_top = [int(np.bincount(dirs[i][got[i] == got[i].max()]).argmax()) for i in range(3)]
                assert at_top == [0, n // 2, n // 4]          # the direction whose normal crosses the edge
    lab = np.zeros((3, h, w), np.int32)
    lab[:, :, 35:] = 1                                         # the labels step across a vertical edge ...
    img = np.full((3, h, w, 3), 60, np.uint8)
    img[:, 12:, :, 0] = 200                                    # ... channel 0 across a horizontal one
    wts = (1, 1, 0, 0)
    got, dirs = _run(torch, ops, lab, img, K, bins, wts, r, n)
    want, wdir = _want(lab, img, K, bins, wts, r, n)
    _same(got, want, "right angles")
    _same(dirs, wdir, "right angles, dir")
    apart = cg.summed_maxima(lab[0], img[0], K, bins, wts, r, n, cache=CACHE)
    assert (apart >= want[0]).all() and apart[12, 35] == 2 * want[0][12, 35] > 0   # at the crossing the two readings differ
    img = np.full((3, h, w, 3), 60, np.uint8)
    img[:, np.add.outer(np.arange(h), np.arange(w)) > 12 + 35, 0] = 200            # channel 0 across the diagonal through (12, 35)
    got, dirs = _run(torch, ops, lab, img, K, bins, wts, r, n)
    want, wdir = _want(lab, img, K, bins, wts, r, n)
    _same(got, want, "45 degrees apart")
    _same(dirs, wdir, "45 degrees apart, dir")
    own = cg.cue_chi_squares(lab[0], img[0], K, bins, wts, r, n, cache=CACHE)
    tops = own[0][:, 12, 35].max(), own[1][:, 12, 35].max()  # PB is neither cue's maximum nor their sum
    assert own[0][:, 12, 35].argmax() == 0 and own[1][:, 12, 35].argmax() == n // 4
    assert max(tops) < want[0][12, 35] < sum(tops)


def test_crafted_mask_tables(torch_cuda, ops):
    """Single-tap tables: the four corner taps of the 31 x 31 frame at r = 15 against the centre, one direction per corner (every
    cue sees the same tap). The all-ones table: the largest numerators, and with weights 16 and G = 2^20 - 1 the largest product."""
    torch = torch_cuda
    r, K, bins = 15, 5, 16
    shape = (9, 33)
    lab, img = _labels(shape, K, 8), _images(shape, 9)
    corners = [(-r, -r), (-r, r), (r, -r), (r, r)]
    table = np.zeros((4, 2, 31), np.uint32)
    for i, (dy, dx) in enumerate(corners):
        table[i, 0, dy + r] = 1 << (dx + r)
        table[i, 1, r] = 1 << r
    wts = (1, 2, 3, 16)
    got, dirs = _run(torch, ops, lab, img, K, bins, wts, r, 4, table=table)
    want, wdir = _want(lab, img, K, bins, wts, r, 4, table)
    _same(got, want, "corner taps")
    _same(dirs, wdir, "corner taps, dir")
    y, x = np.arange(shape[0]), np.arange(shape[1])
    planes = [lab[0]] + [cg.quantise(img[0, ..., c], bins) for c in range(3)]
    planes[0] = np.where((planes[0] >= 0) & (planes[0] < K), planes[0], -1)
    by_hand = []
    for dy, dx in corners:                                    # a tap against the centre: 128 where the two bins differ
        p = 0
        for wc, pl in zip(wts, planes):
            tap = pl[tg.mirror(y + dy, shape[0])][:, tg.mirror(x + dx, shape[1])]
            p = p + wc * np.where(tap != pl, 64 * (tap >= 0) + 64 * (pl >= 0), 0)
        by_hand.append(p)
    _same(got[0], np.max(by_hand, axis=0).astype(np.int32), "corner taps by hand")
    full = np.zeros((1, 2, 31), np.uint32)
    full[0, 0] = (1 << 31) - 1
    wts = (16, 16, 16, 16)
    clean = _labels(shape, K, 8)[:2]                           # (no label outside 0 .. K-1: every pixel counts in a bin)
    top = np.full((2,) + shape, (1 << 20) - 1, np.int32)
    got, _ = _run(torch, ops, clean, img[:2], K, bins, wts, r, 1, table=full)
    assert (got == 4 * 16 * 64 * 961).all()                   # each cue: the sum over its bins of 64 g_j = 64 * 961
    _same(got, _want(clean, img[:2], K, bins, wts, r, 1, full)[0], "all ones")
    joined, _ = _run(torch, ops, clean, img[:2], K, bins, wts, r, 1, grad=top, table=full)
    assert (joined == tg.joined(np.int64(4 * 16 * 64 * 961), np.int64((1 << 20) - 1))).all()
    assert 4 * 16 * 64 * 961 * ((1 << 20) - 1) > 1 << 41


@pytest.mark.parametrize("shape,combo,wts", [((9, 33), (15, 16, 64, 64), (1, 2, 3, 16)), ((23, 71), (8, 8, 16, 8), (2, 2, 1, 1)),
                                             ((5, 3), (8, 3, 2, 1), (0, 1, 1, 1)), ((1, 7), (1, 1, 16, 8), (1, 0, 0, 0))])
def test_buffer_contract(torch_cuda, ops, shape, combo, wts):
    """Inputs and outputs are arena views of exact size between 4096-byte canary bands; each case runs on outputs filled with 0x00
    and with 0xA5: both runs equal the restatement and each other, the bands are intact, the inputs unchanged; ``dir_out`` and
    ``grad`` may be NULL. Correct sizes only."""
    torch, lib = torch_cuda, ops.lib
    r, n, bins, K = combo
    h, w = shape
    lab, img = _labels(shape, K, 21), _images(shape, 22)
    grad = np.random.default_rng(5).integers(-2, 1 << 20, size=lab.shape).astype(np.int32)
    want, wdir = _want(lab if wts[0] else None, img if any(wts[1:]) else None, K, bins, wts, r, n)
    want_joined = np.stack([tg.joined(want[i], np.maximum(grad[i], 0)) for i in range(3)])
    runs = []
    for poison in POISONS:
        a = Arena(torch, "cuda", capacity=1 << 20)
        dl = a.put(lab, name="labels") if wts[0] else None
        di = a.put(img, align=1, name="image") if any(wts[1:]) else None          # (a uint8 image starts at any byte)
        dg = a.put(grad, name="grad")
        dm = a.put(tg.masks(r, n), name="masks")
        out = {}
        for with_grad in (0, 1):
            for with_dir in (0, 1):
                o = a.take(3 * h * w * 4, fill=poison, name="map")
                d = a.take(3 * h * w, align=1, fill=poison, name="direction map") if with_dir else None
                rc = lib.gcs_cue_gradient(ptr(dl), ptr(di), 3, h, w, K, cg.shift_of(bins), *wts, r, n, dm.data_ptr(),
                                          dg.data_ptr() if with_grad else None, o.data_ptr(), ptr(d), _st(torch))
                assert rc == 0, lib.gcs_last_error()
                key = "%d%d" % (with_grad, with_dir)
                out["map " + key] = a.read(o, np.int32, lab.shape)
                _same(out["map " + key], want_joined if with_grad else want, key)
                if with_dir:
                    out["dir " + key] = a.read(d, np.uint8, lab.shape)
                    _same(out["dir " + key], wdir, key)
        a.check()
        a.unchanged()
        runs.append(out)
    assert runs[0].keys() == runs[1].keys() and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_bad_arguments_launch_nothing(torch_cuda, ops):
    torch, lib = torch_cuda, ops.lib
    b, h, w, K, r, n = 1, 16, 24, 4, 3, 5
    # every buffer is a view of ONE allocation with room behind it: a check that failed to refuse would still write inside it
    px = b * h * w
    pool = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    cut = lambda at, nbytes: pool[at:at + nbytes]
    lab, grad, img = cut(0, 4 * px).view(torch.int32), cut(8192, 4 * px).view(torch.int32), cut(16384, 3 * px).view(b, h, w, 3)
    masks = cut(24576, n * 2 * (2 * r + 1) * 4).view(torch.int32)
    masks.copy_(ops.texton_masks(r, n).reshape(-1))
    out, dirs = cut(32768, 4 * px).view(torch.int32).view(b, h, w), cut(40960, px).view(b, h, w)
    out.fill_(-7)
    dirs.fill_(77)
    before = pool.clone()
    st = _st(torch)
    #        0 labels        1 img           2  3  4  5  6 shift 7-10 weights 11 12  13 masks          14 grad          15 out
    good = [lab.data_ptr(), img.data_ptr(), b, h, w, K, 4, 1, 2, 3, 4, r, n, masks.data_ptr(), grad.data_ptr(), out.data_ptr(),
            dirs.data_ptr(), st]
    bad = [(0, None), (1, None), (13, None), (15, None), (2, 0), (2, 65536), (3, 0), (3, 4097), (4, 0), (4, 4097), (5, 0), (5, 65),
           (6, 1), (6, 8), (6, 0), (7, -1), (7, 17), (8, 17), (9, -1), (10, 17), (11, 0), (11, 16), (12, 0), (12, 17)]
    for pos, val in bad:
        args = list(good)
        args[pos] = val
        assert lib.gcs_cue_gradient(*args) == 1, (pos, val)
        assert b"gcs_cue_gradient" in lib.gcs_last_error()
    zero = list(good)
    zero[7:11] = [0, 0, 0, 0]
    assert lib.gcs_cue_gradient(*zero) == 1                   # every weight 0
    # an output range that overlaps an input that is read (the output views are the poisoned tensors' own memory otherwise)
    for pos, val in ((15, lab.data_ptr()), (15, grad.data_ptr() + 4), (15, img.data_ptr()), (15, masks.data_ptr()),
                     (16, lab.data_ptr() + 8), (16, img.data_ptr() + 3 * b * h * w - 1), (16, grad.data_ptr()),
                     (16, out.data_ptr() + 4 * b * h * w - 1)):
        args = list(good)
        args[pos] = val
        assert lib.gcs_cue_gradient(*args) == 1, ("overlap", pos)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(pool, before)                         # nothing was launched
    # a cue of weight 0 is not read: its pointer may be NULL, and it may overlap an output
    for args in ([None] + good[1:7] + [0] + good[8:], good[:1] + [None] + good[2:7] + [3, 0, 0, 0] + good[11:],
                 [out.data_ptr()] + good[1:7] + [0] + good[8:]):
        assert lib.gcs_cue_gradient(*args) == 0, lib.gcs_last_error()
    assert lib.gcs_cue_gradient(*good) == 0
    torch.cuda.current_stream().synchronize()
    assert not bool(out.any()) and not bool(dirs.any())       # a constant map and image
    new = lambda dt=torch.int32: torch.zeros((b, h, w), dtype=dt, device="cuda")
    for kw in (dict(out=new(torch.int64)), dict(dir_out=new()), dict(imgs=img[..., :2]), dict(labels=None), dict(imgs=None),
               dict(bins=3), dict(weights=(1, 2, 3)), dict(weights=(0, 0, 0, 0)), dict(weights=(1, 1, 1, 17)),
               dict(masks=ops.texton_masks(r, n + 1))):
        a = dict(labels=new(), imgs=img, b=b, h=h, w=w, K=K, bins=16, weights=(1, 2, 3, 4), r=r, n=n, grad=None, out=new(), dir_out=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.cue_gradient(**a)


# ---- the host paths on 64 x 48 crops of two val fixture images

COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4, k=8)


@pytest.fixture(scope="module")
def crops(torch_cuda):
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"][:2]]
    imgs = np.stack([np.ascontiguousarray(val["img_" + i][100:164, 120:168]) for i in ids])
    return imgs, torch_cuda.from_numpy(imgs).cuda()


def _chain(seg, dev, imgs, mode="per_image", **kw):
    """The restated chain: the plan's own labels and G, and I_0 = the image its Gabor stage sees."""
    import colour_ref
    labels = seg.segment_device(dev, mode=mode).cpu().numpy()
    grad = seg.edges_device(dev).cpu().numpy() if kw.pop("joined", True) else None
    i0 = np.stack([colour_ref.opponent(im, seg.chroma_gain) for im in imgs]).astype(np.uint8) if seg.chroma_gain else imgs
    a = dict(K=seg.k, bins=16, weights=(2, 2, 1, 1), r=8, n=8)
    a.update(kw)
    return np.stack([cg.cue_edges(labels[i], i0[i], None if grad is None else grad[i], a["K"], a["bins"], a["weights"], a["r"],
                                  a["n"], cache=CACHE) for i in range(len(imgs))])


@pytest.mark.parametrize("plan", ["colour", "default"])
def test_cue_edges_device_equals_the_restated_chain(torch_cuda, crops, plan):
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    imgs, dev = crops
    seg = Segmenter(**COLOUR) if plan == "colour" else Segmenter()
    got = seg.cue_edges_device(dev)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 64, 48) and int(got.max()) > 0
    _same(got.cpu().numpy(), _chain(seg, dev, imgs), "E'")
    _same(seg.cue_edges_device(dev, joined=False).cpu().numpy(), _chain(seg, dev, imgs, joined=False), "PB")
    _same(seg.cue_edges_device(dev, mode="global").cpu().numpy(), _chain(seg, dev, imgs, mode="global"), "global codebook")
    _same(seg.cue_edges_device(dev, radius=3, n_directions=5, bins=4, weights=(1, 0, 16, 3)).cpu().numpy(),
          _chain(seg, dev, imgs, bins=4, weights=(1, 0, 16, 3), r=3, n=5), "other arguments")
    # the label-map entry point on the same planes
    lab, g = seg.segment_device(dev), seg.edges_device(dev)
    i0 = dev
    if plan == "colour":
        i0 = torch.empty_like(dev)
        seg.ops.colour_opponent(dev, i0)
    out, dirs = seg.cue_gradient_device(lab, i0, K=seg.k, gradient=g, directions=True)
    assert torch.equal(out, got) and dirs.dtype == torch.uint8 and int(dirs.max()) < 8
    assert torch.equal(seg.cue_gradient_device(lab, None, weights=(1, 0, 0, 0)), seg.texton_gradient_device(lab))
    assert torch.equal(seg.cue_gradient_device(None, i0, weights=(0, 1, 1, 1), gradient=g),
                       seg.cue_edges_device(dev, weights=(0, 1, 1, 1)))


@pytest.mark.parametrize("plan", ["colour", "default", "superpixels"])
def test_without_the_texton_cue_no_lloyd_pass_is_enqueued(torch_cuda, crops, plan):
    """weights[0] == 0: equality with the restatement, and - through the recorder of the host call trace - no Lloyd entry point
    is called; the refusals that exist only for the k-means map do not apply (a superpixel plan runs)."""
    from gabor_color_image_segmentation_amd import Segmenter
    spec = importlib.util.spec_from_file_location("make_host_call_traces", os.path.join(GOLD, "make_host_call_traces.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    imgs, dev = crops
    seg = Segmenter(**{"colour": COLOUR, "default": {}, "superpixels": dict(n_superpixels=12, n_regions=4)}[plan])
    want = _chain(Segmenter(**COLOUR) if plan == "colour" else Segmenter(), dev, imgs, weights=(0, 1, 1, 1))
    lloyd = {"kmeans_init", "assign_raster", "assign_accumulate", "reduce", "finalize", "reduce_finalize", "pass_fused",
             "labels_widen", "label_slab", "partial_slab", "new_centroids"}
    seg.ops = log = rec.Recorder(seg.ops)
    got = seg.cue_edges_device(dev, weights=(0, 1, 1, 1))
    names = [name for name, _ in log.log]
    _same(got.cpu().numpy(), want, "E' without textons")
    assert names[-1] == "cue_gradient" and "gabor_features" in names and "feature_gradient" in names
    assert not lloyd & set(names), names
    if plan == "superpixels":
        with pytest.raises(ValueError):
            seg.cue_edges_device(dev)                         # with the texton cue the plain k-means map is needed
    else:
        del log.log[:]
        seg.cue_edges_device(dev)
        assert lloyd & {name for name, _ in log.log}          # the recorder does see the Lloyd loop when there is one


def test_replay_from_a_captured_graph_and_segment_cue_edges(torch_cuda, crops):
    from gabor_color_image_segmentation_amd import Segmenter, segment_cue_edges
    from gabor_color_image_segmentation_amd import segmenter as sg
    torch = torch_cuda
    imgs, dev = crops
    seg = Segmenter(**COLOUR)
    src = dev[:1].clone()
    eager = [seg.cue_edges_device(dev[i:i + 1]).clone() for i in range(2)]        # (also: masks and scratch exist before the capture)
    torch.cuda.current_stream().synchronize()
    graph, held = torch.cuda.CUDAGraph(), {}
    assert sg._CAPTURES.capture(torch, graph, lambda: held.update(out=seg.cue_edges_device(src)), device=seg.ops.device)
    out = held["out"]
    for i in (1, 0):
        src.copy_(dev[i:i + 1])
        out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), i
    one = segment_cue_edges(imgs[0], **COLOUR)
    assert one.dtype == np.float32 and one.shape == (64, 48) and one.max() == 1.0
    assert np.array_equal(one, tg.normalised(_chain(seg, dev[:1], imgs[:1])[0]))
    assert not segment_cue_edges(np.full((16, 16, 3), 9, np.uint8), **COLOUR).any()
    for kw in (dict(bins=12), dict(weights=(0, 0, 0, 0)), dict(weights=(1, 2)), dict(radius=0), dict(radius=16),
               dict(n_directions=17), dict(n_directions=0)):
        with pytest.raises(ValueError):
            segment_cue_edges(imgs[0], **kw)
        with pytest.raises(ValueError):
            seg.cue_edges_device(dev, **kw)


def test_sweep_of_a_cue_map_equals_edge_scores(torch_cuda):
    """``evaluate_gpu.edge_sweep_resident`` on one cue map == ``evaluate.edge_scores`` at the sweep's thresholds (16 levels)."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    torch = torch_cuda
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    i = str(val["ids"][0])
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    e = Segmenter(**COLOUR).cue_edges_device(torch.from_numpy(val["img_" + i][None]).cuda(), weights=(0, 1, 1, 1))
    levels = 16
    rec, prec, f, step = edge_sweep_resident(e, truth.to_device([i]), levels=levels)
    eh = e[0].cpu().numpy()
    assert step == -(-(int(eh.max()) + 1) // levels)
    want = edge_scores(eh, truth[i], [step * (tau + 1) - 1 for tau in range(levels)])
    assert rec[0].tolist() == want["recall"].tolist() and prec[0].tolist() == want["precision"].tolist()
    assert f[0].tolist() == want["fmeasure"].tolist() and 0.2 < f.max() < 1.0
