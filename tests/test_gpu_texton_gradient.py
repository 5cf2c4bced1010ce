"""gcs_texton_gradient (SPEC.md §24) on the GPU: every value compared with ``==`` against the NumPy restatement
(tests/texton_gradient_ref.py). Shapes: 1 x 1, 1 x 9 and 5 x 9 (several reflections), 8 x 8, 8 x 32 (exactly one tile), 9 x 33 (a
one-pixel second tile both ways), 33 x 41, 40 x 70 (at r = 15 the halo reaches across two tiles and past both borders); radii
1, 2, 8, 15, direction counts 1, 3, 8, 16 (both kernel instantiations), K from 1 to 64; iid maps, blocky maps (most planes absent
from most tiles: the skip), a map with -1 and K; three distinct images in one call against their single calls; crafted mask tables
(one tap against the centre for every offset of the 31 x 31 frame, all 961 bits in one half, random tables); the joined map with
products past 2^32; the optional arguments; the argument rules; ``texton_edges_device`` on a val fixture image against restatement
o (``segment_device`` labels, ``edges_device`` map), per image, with a global codebook and replayed from a captured graph; the
threshold sweep of that map against ``evaluate.edge_scores``."""
import os

import numpy as np
import pytest

import texton_gradient_ref as tg

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (1, 9), (5, 9), (8, 8), (8, 32), (9, 33), (33, 41), (40, 70)]
# (r, n, K): every radius, direction count and K of the section's test list at least once, n <= 4 and n > 4 at every radius
COMBOS = [(1, 1, 2), (2, 3, 8), (8, 8, 16), (15, 16, 64), (8, 16, 1), (15, 8, 2), (2, 1, 64), (1, 3, 16), (15, 3, 8), (8, 1, 8),
          (1, 16, 8), (2, 8, 16)]


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def ops(torch_cuda):
    from gabor_color_image_segmentation_amd import Segmenter
    return Segmenter().ops


def _maps(shape, K, seed):
    """Three label maps of one shape: iid (every bin populated where the shape allows), blocky, and iid with -1 and K sprinkled."""
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


def _run(torch, ops, lab, K, r, n, grad=None, dirs=True, table=None):
    b, h, w = lab.shape
    dev = torch.from_numpy(np.ascontiguousarray(lab)).cuda()
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    d = torch.full((b, h, w), 77, dtype=torch.uint8, device="cuda") if dirs else None
    g = None if grad is None else torch.from_numpy(np.ascontiguousarray(grad)).cuda()
    m = None if table is None else torch.from_numpy(np.ascontiguousarray(table).view(np.int32)).cuda()
    ops.texton_gradient(dev, b, h, w, K, r, n, g, out, d, masks=m)
    return out.cpu().numpy(), (d.cpu().numpy() if dirs else None)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "r%d_n%d_K%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_and_parameter(torch_cuda, ops, shape, combo):
    r, n, K = combo
    lab = _maps(shape, K, shape[0] * 1000 + shape[1] + r)
    got, dirs = _run(torch_cuda, ops, lab, K, r, n)
    for i, name in enumerate(("iid", "blocky", "holes")):
        want, wdir = tg.texton_gradient(lab[i], K, r, n)
        _same(got[i], want, (name, "TG"))
        _same(dirs[i], wdir, (name, "dir"))
    if shape == (1, 1) or K == 1:
        assert not got[:2].any() and not dirs[:2].any()      # one label: both halves agree everywhere
    elif min(shape) >= 8:
        assert got[0].max() > 0


@pytest.mark.parametrize("shape,combo", [((9, 33), (2, 3, 8)), ((33, 41), (8, 8, 16)), ((40, 70), (15, 16, 64))])
def test_three_distinct_images_equal_their_single_calls(torch_cuda, ops, shape, combo):
    r, n, K = combo
    lab = _maps(shape, K, 5)
    got, dirs = _run(torch_cuda, ops, lab, K, r, n)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])
    for i in range(3):
        one, d1 = _run(torch_cuda, ops, lab[i:i + 1], K, r, n)
        assert np.array_equal(one[0], got[i]) and np.array_equal(d1[0], dirs[i])


@pytest.mark.parametrize("shape", [(5, 9), (33, 41)], ids=lambda s: "%dx%d" % s)
def test_one_tap_against_the_centre_for_every_offset(torch_cuda, ops, shape):
    """A = {one offset}, B = {(0, 0)}, for every offset of the 31 x 31 frame in turn: 128 where the two labels differ, 0 where they
    agree - every tap's addressing and mirror on its own. 961 launches, one read."""
    torch = torch_cuda
    h, w = shape
    r, K = 15, 5
    lab = np.random.default_rng(h).integers(0, K, size=shape).astype(np.int32)
    offsets = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
    tables = np.zeros((len(offsets), 1, 2, 2 * r + 1), np.uint32)
    for t, (dy, dx) in enumerate(offsets):
        tables[t, 0, 0, dy + r] = 1 << (dx + r)
        tables[t, 0, 1, r] = 1 << r
    dev = torch.from_numpy(lab[None]).cuda()
    m = torch.from_numpy(tables.view(np.int32)).cuda()
    out = torch.full((len(offsets), 1, h, w), -7, dtype=torch.int32, device="cuda")
    for t in range(len(offsets)):
        ops.texton_gradient(dev, 1, h, w, K, r, 1, None, out[t], None, masks=m[t])
    got = out.cpu().numpy()[:, 0]
    y, x = np.arange(h), np.arange(w)
    for t, (dy, dx) in enumerate(offsets):
        tap = lab[tg.mirror(y + dy, h)][:, tg.mirror(x + dx, w)]
        _same(got[t], np.where(tap != lab, 128, 0).astype(np.int32), (dy, dx))


def test_the_largest_numerator_and_tables_without_symmetry(torch_cuda, ops):
    """All 961 bits in A and none in B: g = the label's count in the whole frame, h = 0, a bin adds 64 g; with one label the
    division sees 64 * 961^2 / 961. Then random tables (B is not the mirror image of A, rows of any bit pattern)."""
    r = 15
    full = np.zeros((1, 2, 31), np.uint32)
    full[0, 0] = (1 << 31) - 1
    one = np.zeros((1, 33, 41), np.int32)
    got, _ = _run(torch_cuda, ops, one, 1, r, 1, table=full)
    assert (got == 64 * 961).all()
    lab = _maps((33, 41), 3, 9)
    got, dirs = _run(torch_cuda, ops, lab, 3, r, 1, table=full)
    for i in range(3):
        want, _ = tg.texton_gradient(lab[i], 3, r, 1, full)
        _same(got[i], want, "full frame")
    assert (got[:2] == 64 * 961).all() and got[2].max() < 64 * 961
    rng = np.random.default_rng(31)
    for rr, n, K in ((15, 5, 4), (8, 3, 16), (2, 16, 3)):
        table = rng.integers(0, 1 << (2 * rr + 1), size=(n, 2, 2 * rr + 1)).astype(np.uint32)
        lab = _maps((40, 70), K, rr)
        got, dirs = _run(torch_cuda, ops, lab, K, rr, n, table=table)
        for i in range(3):
            want, wdir = tg.texton_gradient(lab[i], K, rr, n, table)
            _same(got[i], want, ("random table", rr))
            _same(dirs[i], wdir, ("random table dir", rr))
    high = full.copy()                                       # bits above 2r of a row are ignored
    lab = _maps((9, 33), 4, 2)
    a, _ = _run(torch_cuda, ops, lab, 4, 2, 1, table=np.ascontiguousarray(high[:, :, :5]))
    b, _ = _run(torch_cuda, ops, lab, 4, 2, 1, table=np.ascontiguousarray(high[:, :, :5] & 31))
    assert np.array_equal(a, b) and (a[0] == 64 * 25).all()


@pytest.mark.parametrize("shape,combo", [((33, 41), (8, 8, 16)), ((40, 70), (15, 3, 2)), ((1, 9), (2, 8, 8))])
def test_joined_map_and_optional_arguments(torch_cuda, ops, shape, combo):
    r, n, K = combo
    lab = _maps(shape, K, 77)
    rng = np.random.default_rng(shape[1])
    grad = rng.integers(0, 2 ** 20, size=lab.shape).astype(np.int32)
    grad[:, 0, 0] = 2 ** 20 - 1
    grad[:, -1, -1] = 0
    alone, dirs = _run(torch_cuda, ops, lab, K, r, n)
    got, dirs2 = _run(torch_cuda, ops, lab, K, r, n, grad=grad)
    assert np.array_equal(dirs, dirs2)
    for i in range(3):
        _same(got[i], tg.joined(tg.texton_gradient(lab[i], K, r, n)[0], grad[i]), "E")
    if min(shape) > 1:
        assert int((alone.astype(np.int64) * grad).max()) > 2 ** 32      # the product passes 32 bits: the corrected root
    below = grad.copy()
    below[:, -1, -1] = -5                                    # a negative G counts as 0
    assert np.array_equal(_run(torch_cuda, ops, lab, K, r, n, grad=below)[0], got)
    no_dir, none = _run(torch_cuda, ops, lab, K, r, n, grad=grad, dirs=False)
    assert none is None and np.array_equal(no_dir, got)
    no_dir, _ = _run(torch_cuda, ops, lab, K, r, n, dirs=False)
    assert np.array_equal(no_dir, alone)


def test_bad_arguments_launch_nothing(torch_cuda, ops):
    torch = torch_cuda
    lib = ops.lib
    b, h, w, K, r, n = 1, 16, 24, 4, 3, 5
    lab = torch.zeros((b, h, w), dtype=torch.int32, device="cuda")
    out = torch.full((b, h, w), -7, dtype=torch.int32, device="cuda")
    masks = ops.texton_masks(r, n)
    assert masks is ops.texton_masks(r, n) and tuple(masks.shape) == (n, 2, 2 * r + 1)           # cached per (r, n)
    assert np.array_equal(masks.cpu().numpy().view(np.uint32), tg.masks(r, n))
    st = torch.cuda.current_stream().cuda_stream
    good = [lab.data_ptr(), b, h, w, K, r, n, masks.data_ptr(), None, out.data_ptr(), None, st]
    for pos, val in ((0, None), (7, None), (9, None), (1, 0), (1, 65536), (2, 0), (2, 4097), (3, 0), (3, 4097), (4, 0), (4, 65),
                     (5, 0), (5, 16), (6, 0), (6, 17)):
        args = list(good)
        args[pos] = val
        assert lib.gcs_texton_gradient(*args) == 1, (pos, val)
        assert b"gcs_texton_gradient" in lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert bool((out == -7).all())                           # nothing was launched
    assert lib.gcs_texton_gradient(*good) == 0
    torch.cuda.current_stream().synchronize()
    assert not bool(out.any())                               # a constant map
    with pytest.raises(ValueError):
        ops.texton_gradient(lab, b, h, w, K, r, n, None, out.to(torch.int64), None)
    with pytest.raises(ValueError):
        ops.texton_gradient(lab, b, h, w, K, r, n, None, out, out)           # dir_out must be uint8
    with pytest.raises(ValueError):
        ops.texton_gradient(lab, b, h, w, K, r, n, None, out, None, masks=ops.texton_masks(r, n + 1))
    with pytest.raises(ValueError):
        ops.texton_masks(16, 8)


# ---- the chain on a val fixture image (481 x 321, colour bank, k = 8)

@pytest.fixture(scope="module")
def chain(torch_cuda):
    """The plan, two portrait val images on the device, and - computed once - the plan's own labels and G of the first."""
    from gabor_color_image_segmentation_amd import Segmenter
    torch = torch_cuda
    val = np.load(os.path.join(GOLD, "bsd_val_images.npz"))
    ids = [str(i) for i in val["ids"] if val["img_" + str(i)].shape[:2] == (481, 321)][:2]
    seg = Segmenter(n_orient=5, color_weight=0.125, chroma_gain=4, k=8)
    dev = torch.from_numpy(np.stack([val["img_" + i] for i in ids])).cuda()
    labels = seg.segment_device(dev[:1]).cpu().numpy()[0]
    grad = seg.edges_device(dev[:1]).cpu().numpy()[0]
    want_tg = tg.texton_gradient(labels, 8, 8, 8)[0]
    return seg, dev, ids, grad, want_tg


def test_texton_edges_device_equals_the_restated_chain(torch_cuda, chain):
    torch = torch_cuda
    seg, dev, ids, grad, want_tg = chain
    got = seg.texton_edges_device(dev[:1])
    assert got.dtype == torch.int32 and tuple(got.shape) == (1, 481, 321)
    _same(got[0].cpu().numpy(), tg.joined(want_tg, grad), "E")
    _same(seg.texton_edges_device(dev[:1], joined=False)[0].cpu().numpy(), want_tg, "TG")
    assert want_tg.max() > 0 and grad.max() > 0
    # the label-map entry point on the same labels, with the direction map
    lab = seg.segment_device(dev[:1])
    out, dirs = seg.texton_gradient_device(lab, K=8, directions=True)
    assert torch.equal(out, seg.texton_edges_device(dev[:1], joined=False)) and dirs.dtype == torch.uint8 and int(dirs.max()) < 8
    assert torch.equal(seg.texton_gradient_device(lab, gradient=seg.edges_device(dev[:1])), got)       # K from the map's maximum


def test_texton_edges_device_with_a_global_codebook(torch_cuda, chain):
    seg, dev, ids, _, _ = chain
    labels = seg.segment_device(dev, mode="global").cpu().numpy()
    grad = seg.edges_device(dev).cpu().numpy()
    got = seg.texton_edges_device(dev, mode="global").cpu().numpy()
    for i in range(2):
        _same(got[i], tg.joined(tg.texton_gradient(labels[i], 8, 8, 8)[0], grad[i]), ("global", i))


def test_texton_edges_device_replayed_from_a_captured_graph(torch_cuda, chain):
    from gabor_color_image_segmentation_amd import segmenter as sg
    torch = torch_cuda
    seg, dev, ids, _, _ = chain
    src = dev[:1].clone()
    eager = [seg.texton_edges_device(dev[i:i + 1]).clone() for i in range(2)]     # (also: masks and scratch exist before the capture)
    torch.cuda.current_stream().synchronize()
    graph, held = torch.cuda.CUDAGraph(), {}
    # the module's own capture guard: collector off, a helper thread and a stream of its own, a refused capture kept alive
    assert sg._CAPTURES.capture(torch, graph, lambda: held.update(out=seg.texton_edges_device(src)), device=seg.ops.device)
    out = held["out"]
    for i in (1, 0):
        src.copy_(dev[i:i + 1])
        out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), i


def test_sweep_of_the_joined_map_equals_edge_scores(torch_cuda, chain):
    from gabor_color_image_segmentation_amd.evaluate import edge_scores
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_sweep_resident
    from gabor_color_image_segmentation_amd.groundtruth import PackedTruth
    seg, dev, ids, _, _ = chain
    truth = PackedTruth(os.path.join(GOLD, "bsd500_truth.npz"))
    e = seg.texton_edges_device(dev[:1])
    levels = 256
    rec, prec, f, step = edge_sweep_resident(e, truth.to_device(ids[:1]), levels=levels)
    eh = e[0].cpu().numpy()
    assert step == -(-(int(eh.max()) + 1) // levels)
    want = edge_scores(eh, truth[ids[0]], [step * (tau + 1) - 1 for tau in range(levels)])
    assert rec[0].tolist() == want["recall"].tolist() and prec[0].tolist() == want["precision"].tolist()
    assert f[0].tolist() == want["fmeasure"].tolist() and 0.2 < f.max() < 1.0
