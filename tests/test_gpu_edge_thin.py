"""gcs_edge_thin (SPEC.md §26, include/gcs_thin.h) on the GPU: every value compared with ``==`` against the NumPy restatement
(tests/edge_thin_ref.py). Three different maps per call: small signed values (negatives and zeros), three distinct values (ties and
plateaus everywhere) and the full int32 range (INT32_MIN, INT32_MAX, values above 2^30). Shapes: 1 x 1, 1 x 9, 9 x 1, 2 x 2,
3 x 3, 17 x 23, 32 x 62 (exactly one tile), 33 x 63 (one pixel into the next tile both ways) and 71 x 135 (three tiles each way,
the last one ragged: the kernel's tile is 32 rows of 62 pixels); every n in 1 .. 16; dir random, values >= n and 255 among them;
crafted step tables (all the weight on each of the eight ring offsets, as q1 and as q2; w1 + w2 = 2048 on the full range; offsets
outside -1 .. 1, which are clamped); the buffer contract behind canary bands (tests/arena.py); the argument rules; the stream
contract (tests/stream_order.py: late-written inputs, no host wait); one batch whose int32 maps pass bytes 2^31 and 2^32; and the
host chains on the 64 x 48 crops tests/test_gpu_cue_gradient.py uses (``cue_edges_device(thin=True)`` and
``texton_edges_device(thin=True)`` against the restatement applied to the label-map entry points' map and direction map, replay
from a captured graph, ``thin=False`` against the call without the argument, ``segment_cue_edges(thin=True)``, the sweep).
Nothing here looks at a kernel's assembly."""
import importlib.util
import os

import numpy as np
import pytest

import edge_thin_ref as et
import texton_gradient_ref as tg
from arena import Arena, POISONS

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE_H, TILE_W = 32, 62                                       # et_kernel's tile (csrc/edge_thin.hip)
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (17, 23), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1),
          (2 * TILE_H + 7, 2 * TILE_W + 11)]
RING = [(0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)]
I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    ops = Segmenter().ops
    assert hasattr(ops.lib, "gcs_edge_thin") and hasattr(ops.lib, "gcs_thin_steps")
    return ops


def _maps(shape, seed):
    """Three maps of one shape: small signed values, three distinct values, the full int32 range."""
    rng = np.random.default_rng(seed)
    small = rng.integers(-4, 6, size=shape)
    three = rng.choice([0, 7, 9], size=shape)
    wide = rng.integers(1 << 30, 1 << 31, size=shape)
    pick = rng.random(shape)
    wide[pick < 0.1] = I32.max
    wide[(pick >= 0.1) & (pick < 0.2)] = I32.min
    wide[(pick >= 0.2) & (pick < 0.3)] = rng.integers(-9, 10, size=shape)[(pick >= 0.2) & (pick < 0.3)]
    return np.stack([small, three, wide]).astype(np.int32)


def _dirs(shape3, n, seed):
    """Random directions 0 .. n + 1 (two values out of range) with 255 sprinkled."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, n + 2, size=shape3)
    d[rng.random(shape3) < 0.05] = 255
    return d.astype(np.uint8)


def _st(torch):
    return torch.cuda.current_stream().cuda_stream


def _run(torch, ops, e, d, n, table=None):
    """The raw entry point on fresh device copies; ``table`` None: ``ops.thin_steps(n)``."""
    b, h, w = e.shape
    de, dd = torch.from_numpy(np.ascontiguousarray(e)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
    steps = ops.thin_steps(n) if table is None else torch.from_numpy(np.ascontiguousarray(table, np.int32)).cuda()
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    rc = ops.lib.gcs_edge_thin(de.data_ptr(), dd.data_ptr(), b, h, w, n, steps.data_ptr(), out.data_ptr(), _st(torch))
    assert rc == 0, ops.lib.gcs_last_error()
    got = out.cpu().numpy()
    assert np.array_equal(de.cpu().numpy(), e) and np.array_equal(dd.cpu().numpy(), d)       # inputs are read only
    return got


def _want(e, d, n, table=None):
    """The restatement, image by image: the pixel loop on small maps, whole arrays on large ones (held to the loop in
    tests/test_edge_thin.py and on 17 x 23 here)."""
    fn = et.thin if e.shape[1] * e.shape[2] <= 400 else et.thin_fast
    return np.stack([fn(e[i], d[i], n, table) for i in range(len(e))])


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_and_every_n(torch_cuda, ops, shape):
    e = _maps(shape, shape[0] * 1000 + shape[1])
    kept = 0
    for n in range(1, 17):
        d = _dirs(e.shape, n, 31 * n + shape[1])
        table = np.zeros((n, 8), np.int32)
        assert ops.lib.gcs_thin_steps(n, table.ctypes.data) == 0 and np.array_equal(table, et.steps(n))
        assert np.array_equal(ops.thin_steps(n).cpu().numpy(), table)
        got, want = _run(torch_cuda, ops, e, d, n), _want(e, d, n)
        _same(got, want, ("T", n))
        assert not got[d >= n].any() and not got[e <= 0].any() and (got[got != 0] == e[got != 0]).all()
        kept += np.count_nonzero(got)
    if shape == (17, 23):
        d = _dirs(e.shape, 8, 5)
        assert np.array_equal(_want(e, d, 8), np.stack([et.thin_fast(e[i], d[i], 8) for i in range(3)]))
    if shape == (1, 1):
        assert kept == 0                                      # every neighbour is the pixel itself: minus is never below
    elif shape[0] * shape[1] > 100:
        assert kept > 16 * 3


def _crafted_tables():
    """n = 16: rows 0 - 7 put all the weight on q1 = ring offset k (q2 another offset, weight 0), rows 8 - 15 on q2."""
    table = np.zeros((16, 8), np.int32)
    for k, (dy, dx) in enumerate(RING):
        oy, ox = RING[(k + 3) % 8]
        table[k] = [dy, dx, oy, ox, 5, 0, 0, 0]
        table[8 + k] = [oy, ox, dy, dx, 0, 3, 0, 0]
    return table


@pytest.mark.parametrize("shape", [(3, 3), (17, 23), (2 * TILE_H + 7, 2 * TILE_W + 11)], ids=lambda s: "%dx%d" % s)
def test_crafted_step_tables(torch_cuda, ops, shape):
    torch = torch_cuda
    e = _maps(shape, 9 + shape[0])
    table = _crafted_tables()
    d = _dirs(e.shape, 16, 77)
    got = _run(torch, ops, e, d, 16, table)
    _same(got, _want(e, d, 16, table), "single-offset rows")
    # by hand: with all the weight on one offset q, T = V where V > V(p - q) and V >= V(p + q), clamped
    v = np.maximum(e.astype(np.int64), 0)
    pad = np.pad(v, ((0, 0), (1, 1), (1, 1)), mode="edge")
    h, w = shape
    for k, (dy, dx) in enumerate(RING):
        for row in (k, 8 + k):
            plus, minus = pad[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w], pad[:, 1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
            hand = np.where((v > 0) & (v > minus) & (v >= plus), v, 0)
            assert np.array_equal(got[d == row], hand[d == row]), (k, row)
    # w1 + w2 = 2048 on the full int32 range: the products reach 2^42
    big = np.zeros((8, 8), np.int32)
    for k, (dy, dx) in enumerate(RING):
        oy, ox = RING[(k + 1) % 8]
        big[k] = [dy, dx, oy, ox, 1000 + k, 1048 - k, 0, 0]
    top = np.stack([np.random.default_rng(s).integers(I32.max - 3, I32.max, size=shape, endpoint=True) for s in (1, 2, 3)]).astype(np.int32)
    d = _dirs(e.shape, 8, 78)
    for maps in (e, top):
        _same(_run(torch, ops, maps, d, 8, big), _want(maps, d, 8, big), "w1 + w2 = 2048")
    assert 2048 * int(I32.max) > 1 << 41
    # offsets outside -1 .. 1 are the caller's error: clamped, and nothing is read out of bounds (the maps sit in an arena)
    wild = big.copy()
    wild[:, :4] = [[(-1) ** (k + j) * (2 + 3 * j + k) * 1000 for j in range(4)] for k in range(8)]
    wild[3, :4] = [I32.max, I32.min, I32.min, I32.max]
    a = Arena(torch, "cuda", capacity=1 << 20)
    de, dd, dt = a.put(e, name="edges"), a.put(d, align=1, name="dir"), a.put(wild, name="steps")
    o = a.take(e.size * 4, fill=0xA5, name="T")
    assert ops.lib.gcs_edge_thin(de.data_ptr(), dd.data_ptr(), 3, h, w, 8, dt.data_ptr(), o.data_ptr(), _st(torch)) == 0
    _same(a.read(o, np.int32, e.shape), _want(e, d, 8, wild), "clamped offsets")
    a.check()
    a.unchanged()


@pytest.mark.parametrize("shape,n", [((1, 1), 1), ((9, 1), 3), ((17, 23), 8), ((TILE_H + 1, TILE_W + 1), 16),
                                     ((2 * TILE_H + 7, 2 * TILE_W + 11), 5)])
def test_buffer_contract(torch_cuda, ops, shape, n):
    """Inputs and the output are arena views of exact size between 4096-byte canary bands; each case runs on an output filled
    with 0x00 and with 0xA5: both runs equal the restatement, the bands are intact, the inputs unchanged."""
    torch, lib = torch_cuda, ops.lib
    h, w = shape
    e, d = _maps(shape, 21), _dirs((3,) + shape, n, 22)
    want = _want(e, d, n)
    runs = []
    for poison in POISONS:
        a = Arena(torch, "cuda", capacity=1 << 20)
        de = a.put(e, name="edges")
        dd = a.put(d, align=1, name="dir")                    # (a uint8 map starts at any byte)
        dt = a.put(et.steps(n), name="steps")
        o = a.take(3 * h * w * 4, fill=poison, name="T")
        assert lib.gcs_edge_thin(de.data_ptr(), dd.data_ptr(), 3, h, w, n, dt.data_ptr(), o.data_ptr(), _st(torch)) == 0, lib.gcs_last_error()
        runs.append(a.read(o, np.int32, e.shape))
        _same(runs[-1], want, hex(poison))
        a.check()
        a.unchanged()
    assert np.array_equal(runs[0], runs[1])


def test_bad_arguments_launch_nothing(torch_cuda, ops):
    torch, lib = torch_cuda, ops.lib
    b, h, w, n = 2, 16, 24, 5
    px = b * h * w
    # every buffer is a view of ONE allocation with room behind it: a check that failed to refuse would still write inside it
    pool = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    cut = lambda at, nbytes: pool[at:at + nbytes]
    e, d = cut(0, 4 * px).view(torch.int32).view(b, h, w), cut(8192, px).view(b, h, w)
    steps = cut(16384, n * 32).view(torch.int32).view(n, 8)
    out = cut(24576, 4 * px).view(torch.int32).view(b, h, w)
    e.copy_(torch.from_numpy(_maps((h, w), 3)[:2]).cuda())
    d.copy_(torch.from_numpy(_dirs((b, h, w), n, 4)).cuda())
    steps.copy_(ops.thin_steps(n))
    out.fill_(-7)
    before = pool.clone()
    good = [e.data_ptr(), d.data_ptr(), b, h, w, n, steps.data_ptr(), out.data_ptr(), _st(torch)]
    bad = [(0, None), (1, None), (6, None), (7, None), (2, 0), (2, 65536), (3, 0), (3, 4097), (4, 0), (4, 4097), (5, 0), (5, 17),
           (7, e.data_ptr()), (7, e.data_ptr() + 4 * px - 4), (7, e.data_ptr() - 4 * px + 4), (7, d.data_ptr()),
           (7, d.data_ptr() + px - 1), (7, steps.data_ptr()), (7, steps.data_ptr() + n * 32 - 4)]
    for pos, val in bad:
        args = list(good)
        args[pos] = val
        assert lib.gcs_edge_thin(*args) == 1, (pos, val)
        assert b"gcs_edge_thin" in lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert torch.equal(pool, before)                         # nothing was launched
    # ranges that only touch do not overlap: out right behind edges, and right in front of it
    tight = torch.zeros(12 * px + 64, dtype=torch.uint8, device="cuda")
    te = tight[4 * px:8 * px].view(torch.int32).view(b, h, w)
    te.copy_(e)
    want = _want(e.cpu().numpy(), d.cpu().numpy(), n)
    for at in (8 * px, 0):
        to = tight[at:at + 4 * px].view(torch.int32).view(b, h, w)
        to.fill_(-7)
        assert lib.gcs_edge_thin(te.data_ptr(), d.data_ptr(), b, h, w, n, steps.data_ptr(), to.data_ptr(), _st(torch)) == 0
        _same(to.cpu().numpy(), want, ("touching", at))
    assert lib.gcs_edge_thin(*good) == 0
    _same(out.cpu().numpy(), want, "the good call")
    # the Python layer's own checks
    new = lambda dt=torch.int32: torch.zeros((b, h, w), dtype=dt, device="cuda")
    for kw in (dict(out=new(torch.int64)), dict(dirs=new()), dict(edges=new()[:, :8]), dict(edges=None), dict(out=None), dict(n=17),
               dict(steps=ops.thin_steps(n + 1)), dict(edges=torch.zeros((b, h, w), dtype=torch.int32))):
        a = dict(edges=new(), dirs=new(torch.uint8), b=b, h=h, w=w, n=n, out=new())
        a.update(kw)
        with pytest.raises(ValueError):
            ops.edge_thin(**a)
    for bad_n in (0, 17):
        with pytest.raises(ValueError):
            ops.thin_steps(bad_n)
    assert ops.thin_steps(n) is ops.thin_steps(n) and tuple(ops.thin_steps(16).shape) == (16, 8)


# ---- the stream contract (include/gcs.h, "Streams"), in the manner of tests/test_gpu_stream_contract.py

def test_late_inputs_are_honoured_and_the_call_does_not_wait(torch_cuda, ops):
    """QUIET on the true inputs == the restatement, on the decoys a different map; LATE: on a side stream behind a gate, every
    input (edges, dir and the step table) holding its decoy until a copy behind the gate puts the true bytes in place; the call
    returns while the gate runs and the output equals the quiet run."""
    import stream_order as so
    torch = torch_cuda
    shape, n = (37, 53), 8
    e, d = _maps(shape, 41), _dirs((3,) + shape, n, 42)
    e2, d2 = _maps(shape, 43), _dirs((3,) + shape, n, 44)
    table, table2 = et.steps(n), et.steps(n)[::-1].copy()
    case = so.Case("edge_thin", ["gcs_edge_thin"],
                   dict(edges=so.late(e, e2), dirs=so.late(d, d2), steps=so.late(table, table2), out=so.out(e.size * 4)),
                   lambda lib, p, st: _ok(lib, lib.gcs_edge_thin(p["edges"], p["dirs"], 3, shape[0], shape[1], n, p["steps"], p["out"], st)),
                   lambda o: so.same(so.view(o["out"], np.int32, e.shape), _want(e, d, n), "quiet run"))
    run = so.Runner(torch, ops.lib)
    case.quiet["true"], dt = run.quiet_run(case, "true")
    case.check(case.quiet["true"])
    case.quiet["decoy"], _ = run.quiet_run(case, "decoy")
    so.same(so.view(case.quiet["decoy"]["out"], np.int32, e.shape), _want(e2, d2, n, table2), "quiet run on the decoys")
    assert not np.array_equal(case.quiet["decoy"]["out"], case.quiet["true"]["out"])
    for swap, tab in ((dict(edges=e2), table), (dict(dirs=d2), table), (dict(), table2)):          # each input alone changes the output
        assert not np.array_equal(_want(swap.get("edges", e), swap.get("dirs", d), n, tab), _want(e, d, n))
    run.calibrate()
    run.settle([dt])
    run.hold_late(case)
    run.release(case)


def _ok(lib, rc):
    assert rc == 0, lib.gcs_last_error()


# ---- byte offsets past 2^31 and 2^32

def test_offsets_past_two_to_the_thirty_one_and_thirty_two(torch_cuda, ops):
    """65 maps of 4095 x 4093: edges and T (int32) pass bytes 2^31 (inside image 32) and 2^32 (inside image 64); 9.4 GiB in all.
    The maps are zero but for a few small patches: at the two lines, in the first and last image and at the corners of the images
    that straddle the lines. Every patch == the restatement on its surroundings, and no other element of T is non-zero (the
    output is poisoned on entry: an element that was not written, or written from another image's pixels, shows)."""
    torch = torch_cuda
    b, h, w, n = 65, 4095, 4093, 8
    p = h * w
    assert 32 * p < 1 << 29 < 33 * p and 64 * p < 1 << 30 < 65 * p and 4 * b * p > (1 << 32) + (1 << 20)
    free, _ = torch.cuda.mem_get_info()
    assert free > 11 << 30, "this case holds 9.4 GiB"
    e = torch.zeros((b, h, w), dtype=torch.int32, device="cuda")
    d = torch.zeros((b, h, w), dtype=torch.uint8, device="cuda")
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(2)
    spots = []
    for line in (1 << 29, 1 << 30):                           # the element at the line and its surroundings
        img, rest = divmod(line, p)
        spots.append((img, rest // w, rest % w))
    spots += [(0, 0, 0), (b - 1, h - 1, w - 1), (32, 0, 0), (32, h - 1, w - 1), (33, 0, w - 1), (63, h - 1, 0), (64, 0, 0), (64, h - 1, 0)]
    assert len(set(spots)) == len(spots)
    boxes = []
    for img, y, x in spots:
        y0, x0 = min(max(y - 4, 0), h - 9), min(max(x - 6, 0), w - 13)
        patch = rng.integers(-50, 1000, size=(9, 13)).astype(np.int32)         # (at an image corner the patch reaches the corner)
        dirs = rng.integers(0, n + 1, size=(9, 13)).astype(np.uint8)
        e[img, y0:y0 + 9, x0:x0 + 13] = torch.from_numpy(patch).cuda()
        d[img, y0:y0 + 9, x0:x0 + 13] = torch.from_numpy(dirs).cuda()
        boxes.append((img, y0, x0))
    steps = ops.thin_steps(n)
    rc = ops.lib.gcs_edge_thin(e.data_ptr(), d.data_ptr(), b, h, w, n, steps.data_ptr(), out.data_ptr(), _st(torch))
    assert rc == 0, ops.lib.gcs_last_error()
    torch.cuda.synchronize()
    total = 0
    for img, y0, x0 in boxes:
        # a window two pixels wider than the patch's box (where the image has them): zeros around the patch, so the clamp of the
        # restatement at the window's edge sees what the kernel sees in the image
        ya, yb, xa, xb = max(y0 - 2, 0), min(y0 + 11, h), max(x0 - 2, 0), min(x0 + 15, w)
        got = out[img, ya:yb, xa:xb].cpu().numpy()
        want = et.thin(e[img, ya:yb, xa:xb].cpu().numpy(), d[img, ya:yb, xa:xb].cpu().numpy(), n)
        _same(got, want, (img, y0, x0))
        assert np.count_nonzero(want) > 0
        total += np.count_nonzero(want)
    assert int(torch.count_nonzero(out)) == total            # everything else was written, with 0
    del e, d, out
    torch.cuda.empty_cache()


# ---- the host chains on 64 x 48 crops of two val fixture images

COLOUR = dict(n_orient=5, color_weight=0.125, chroma_gain=4, k=8)


@pytest.fixture(scope="module")
def crops(torch_cuda):
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"][:2]]
    imgs = np.stack([np.ascontiguousarray(val["img_" + i][100:164, 120:168]) for i in ids])
    return imgs, torch_cuda.from_numpy(imgs).cuda()


def _recorder():
    spec = importlib.util.spec_from_file_location("make_host_call_traces", os.path.join(GOLD, "make_host_call_traces.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec.Recorder


def _thinned(e, d, n):
    e, d = e.cpu().numpy(), d.cpu().numpy()
    return np.stack([et.thin_fast(e[i], d[i], n) for i in range(len(e))])


@pytest.mark.parametrize("plan", ["colour", "default"])
def test_cue_edges_device_thin(torch_cuda, crops, plan):
    """``cue_edges_device(thin=True)`` == the restatement applied to ``cue_gradient_device(..., directions=True)`` on the plan's
    own labels, G and I_0; ``thin=False`` == the call without the argument, launch for launch."""
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    imgs, dev = crops
    seg = Segmenter(**COLOUR) if plan == "colour" else Segmenter()
    lab, g = seg.segment_device(dev), seg.edges_device(dev)
    i0 = dev
    if plan == "colour":
        i0 = torch.empty_like(dev)
        seg.ops.colour_opponent(dev, i0)
    for kw, joined in ((dict(), True), (dict(joined=False), False), (dict(radius=3, n_directions=5, bins=4, weights=(1, 0, 16, 3)), True)):
        n = kw.get("n_directions", 8)
        args = {k: v for k, v in kw.items() if k != "joined"}
        thick, dirs = seg.cue_gradient_device(lab, i0, K=seg.k, gradient=g if joined else None, directions=True, **args)
        got = seg.cue_edges_device(dev, thin=True, **kw)
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, 64, 48)
        _same(got.cpu().numpy(), _thinned(thick, dirs, n), ("T", kw))
        assert 0 < int(torch.count_nonzero(got)) < int(torch.count_nonzero(thick))
        assert torch.equal(seg.cue_edges_device(dev, **kw), thick) and torch.equal(seg.cue_edges_device(dev, thin=False, **kw), thick)
        both = seg.cue_gradient_device(lab, i0, K=seg.k, gradient=g if joined else None, directions=True, thin=True, **args)
        assert torch.equal(both[0], got) and torch.equal(both[1], dirs)
        assert torch.equal(seg.cue_gradient_device(lab, i0, K=seg.k, gradient=g if joined else None, thin=True, **args), got)
        assert torch.equal(seg.thin_edges_device(thick, dirs, n_directions=n), got)
    real, names = seg.ops, {}
    seg.ops = log = _recorder()(real)
    try:
        for key, kw in (("none", dict()), ("false", dict(thin=False)), ("true", dict(thin=True))):
            del log.log[:]
            seg.cue_edges_device(dev, **kw)
            names[key] = [name for name, _ in log.log]
    finally:
        seg.ops = real
    assert names["false"] == names["none"] and "edge_thin" not in names["none"] and names["none"][-1] == "cue_gradient"
    assert [x for x in names["true"] if x != "thin_steps"] == names["none"] + ["edge_thin"]


def test_texton_edges_device_thin(torch_cuda, crops):
    from gabor_color_image_segmentation_amd import Segmenter, segment_texton_edges
    torch = torch_cuda
    imgs, dev = crops
    seg = Segmenter(**COLOUR)
    lab, g = seg.segment_device(dev), seg.edges_device(dev)
    for kw, joined in ((dict(), True), (dict(joined=False), False), (dict(radius=4, n_directions=16), True)):
        n = kw.get("n_directions", 8)
        args = {k: v for k, v in kw.items() if k != "joined"}
        thick, dirs = seg.texton_gradient_device(lab, K=seg.k, gradient=g if joined else None, directions=True, **args)
        got = seg.texton_edges_device(dev, thin=True, **kw)
        _same(got.cpu().numpy(), _thinned(thick, dirs, n), ("T", kw))
        assert 0 < int(torch.count_nonzero(got)) < int(torch.count_nonzero(thick))
        assert torch.equal(seg.texton_edges_device(dev, **kw), thick) and torch.equal(seg.texton_edges_device(dev, thin=False, **kw), thick)
        assert torch.equal(seg.texton_gradient_device(lab, K=seg.k, gradient=g if joined else None, thin=True, **args), got)
    one = segment_texton_edges(imgs[0], thin=True, **COLOUR)
    assert one.dtype == np.float32 and one.max() == 1.0
    assert np.array_equal(one, tg.normalised(seg.texton_edges_device(dev[:1], thin=True)[0].cpu().numpy()))


def test_replay_from_a_captured_graph_and_segment_cue_edges(torch_cuda, crops):
    from gabor_color_image_segmentation_amd import Segmenter, segment_cue_edges
    from gabor_color_image_segmentation_amd import segmenter as sg
    torch = torch_cuda
    imgs, dev = crops
    seg = Segmenter(**COLOUR)
    src = dev[:1].clone()
    eager = [seg.cue_edges_device(dev[i:i + 1], thin=True).clone() for i in range(2)]      # (also: tables and scratch exist before the capture)
    assert not torch.equal(eager[0], eager[1])
    torch.cuda.current_stream().synchronize()
    graph, held = torch.cuda.CUDAGraph(), {}
    assert sg._CAPTURES.capture(torch, graph, lambda: held.update(out=seg.cue_edges_device(src, thin=True)), device=seg.ops.device)
    out = held["out"]
    for i in (1, 0):
        src.copy_(dev[i:i + 1])
        out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), i
    one = segment_cue_edges(imgs[0], thin=True, **COLOUR)
    assert one.dtype == np.float32 and one.shape == (64, 48) and one.max() == 1.0
    assert np.array_equal(one, tg.normalised(eager[0][0].cpu().numpy()))
    thick = segment_cue_edges(imgs[0], **COLOUR)
    assert np.count_nonzero(one) < np.count_nonzero(thick) and not segment_cue_edges(np.full((16, 16, 3), 9, np.uint8), thin=True, **COLOUR).any()


def test_sweep_of_a_thinned_map_equals_edge_scores(torch_cuda):
    """``evaluate_gpu.edge_sweep_resident`` scores a thinned map unchanged: == ``evaluate.edge_scores`` at the sweep's thresholds."""
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    torch = torch_cuda
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    i = str(val["ids"][0])
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    t = Segmenter(**COLOUR).cue_edges_device(torch.from_numpy(val["img_" + i][None]).cuda(), weights=(0, 1, 1, 1), thin=True)
    levels = 16
    rec, prec, f, step = edge_sweep_resident(t, truth.to_device([i]), levels=levels)
    th = t[0].cpu().numpy()
    want = edge_scores(th, truth[i], [step * (tau + 1) - 1 for tau in range(levels)])
    assert rec[0].tolist() == want["recall"].tolist() and prec[0].tolist() == want["precision"].tolist()
    assert f[0].tolist() == want["fmeasure"].tolist() and 0.2 < f.max() < 1.0
