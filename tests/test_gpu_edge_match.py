"""gcs_truth_thin and gcs_edge_match (SPEC.md §27, include/gcs_match.h) on the GPU: every integer compared with ``==`` against
``evaluate.match_count`` (scipy's Hopcroft-Karp, one matching per level) and ``evaluate.thin_boundaries``. The worked examples
through the raw C calls; random maps of 1 x 1, 1 x 9, 9 x 1, 13 x 17 and 33 x 47 with levels 1, 4 and 256, D2 0, 1, 18, 20 (69
offsets: a second lane chunk) and, on 24 x 31, 160 (505 offsets), three images with 1, 3 and 2 annotators, uint8 and 16-bit
truth, q below 0 and above ``levels``; the chain (searches 199 deep, one of which fails and kills it; a staircase whose last
search augments along 198 pixels); ``cap`` exact and too small; the host calls against ``evaluate.match_scores`` float for float
on two BSD fixture images; the buffer contract behind canary bands (tests/arena.py); the stream contract
(tests/stream_order.py); capture and replay in a child process (tests/checkers/edge_match_capture_child.py); one batch whose
maps pass element 2^31. Every buffer of every raw call here is an arena view between canary bands. Nothing here looks at a
kernel's assembly.

Measured on an MI355X: the whole file, 20 tests, in 11.6 s; the slowest are the 33 x 47 random maps (2.8 s, most of it the
reference's matchings), the capture child (2.6 s) and the two BSD fixture cases (1.4 and 1.0 s); the 2^31 case (13 GiB) takes
less than a second."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import edge_match_ref as em
from arena import Arena, POISONS
from test_edge_match import em_chain

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def lib(torch_cuda):
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    for name in _lib.MATCH_EXTENSIONS:
        assert hasattr(lib, name), name
    return lib


def _st(torch):
    return torch.cuda.current_stream().cuda_stream


def _thin(torch, lib, maps, poison=0xA5):
    """gcs_truth_thin on (T,H,W) uint8 or uint16 maps in an arena -> (thin uint8 (T,H,W), counts int32 (T,))."""
    t, h, w = maps.shape
    a = Arena(torch, "cuda", capacity=maps.nbytes + t * h * w + 4 * t + (1 << 16))
    dm = a.put(maps, name="maps")
    dt = a.take(t * h * w, align=1, fill=poison, name="thin")
    dc = a.take(4 * t, align=4, fill=poison, name="counts")
    rc = lib.gcs_truth_thin(dm.data_ptr(), t, h, w, int(maps.dtype == np.uint8), dt.data_ptr(), dc.data_ptr(), _st(torch))
    assert rc == 0, lib.gcs_last_error()
    thin, counts = a.read(dt, np.uint8, maps.shape), a.read(dc, np.int32, (t,))
    a.check()
    a.unchanged()
    return thin, counts


def _match(torch, lib, q, thin, img_of, levels, offs, cap, poison=0xA5):
    """gcs_edge_match in an arena -> (matched (T,levels), above (B,levels), counters uint32 (T,4))."""
    b, h, w = q.shape
    t = thin.shape[0]
    nbytes = lib.gcs_edge_match_bytes(b, t, h, w, cap)
    assert nbytes > 0
    a = Arena(torch, "cuda", capacity=nbytes + q.nbytes + thin.nbytes + 4 * (t + b) * levels + (1 << 17))
    dq = a.put(np.ascontiguousarray(q, np.int32), name="q")
    dt = a.put(np.ascontiguousarray(thin, np.uint8), align=1, name="thin")
    di = a.put(np.ascontiguousarray(img_of, np.int32), align=4, name="img_of")
    do = a.put(np.ascontiguousarray(offs, np.int32), align=4, name="offsets")
    ws = a.take(nbytes, fill=poison, name="workspace")
    dm = a.take(4 * t * levels, align=4, fill=poison, name="matched")
    da = a.take(4 * b * levels, align=4, fill=poison, name="above")
    rc = lib.gcs_edge_match(dq.data_ptr(), dt.data_ptr(), di.data_ptr(), b, t, h, w, levels, do.data_ptr(), len(offs), cap,
                            ws.data_ptr(), dm.data_ptr(), da.data_ptr(), _st(torch))
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.synchronize()
    got = a.read(dm, np.int32, (t, levels)), a.read(da, np.int32, (b, levels)), a.read(ws[:16 * t], np.uint32, (t, 4))
    a.check()
    a.unchanged()
    return got


def _want(q, truth, levels, d2):
    """M[tau] and above[tau] of one image and one contour from ``match_count``, one matching per DISTINCT level set."""
    from gabor_color_image_segmentation_amd.evaluate import match_count
    qc = np.clip(q, 0, levels)
    m, above, seen = np.zeros(levels, np.int64), np.zeros(levels, np.int64), {}
    for tau in range(levels):
        p = qc > tau
        above[tau] = n = int(p.sum())
        if n not in seen:                                     # the sets are nested: equal size, equal set
            seen[n] = match_count(p, truth, d2)
        m[tau] = seen[n]
    return m, above


def _labels(rng, shape, kind):
    h, w = shape
    if kind == 0:
        return rng.integers(0, 3, size=shape)
    if kind == 1:
        return np.cumsum(rng.random(shape) < 0.12, axis=1) + (np.arange(h)[:, None] // 5)
    return (np.arange(h)[:, None] // 4 + np.arange(w)[None, :] // 6) * 7 % 300       # blocks; labels above 255 on 16-bit maps


def _batch(rng, shape, levels):
    """Three images with 1, 3 and 2 annotator maps; q in -3 .. levels + 3 out of at most 12 distinct values."""
    palette = np.unique(np.concatenate([[-3, 0, levels, levels + 3], rng.integers(0, levels + 1, size=8)]))
    q = rng.choice(palette, size=(3,) + shape) * (rng.random((3,) + shape) < np.array([0.25, 0.7, 1.0])[:, None, None])
    img_of = np.array([0, 1, 1, 1, 2, 2], np.int32)
    maps = np.stack([_labels(rng, shape, k % 3) for k in range(6)])
    return q.astype(np.int32), img_of, maps


def _check_batch(torch, lib, q, img_of, maps, levels, d2, cap=None):
    from gabor_color_image_segmentation_amd.evaluate import thin_boundaries
    thin, counts = _thin(torch, lib, maps)
    for t in range(len(maps)):
        assert np.array_equal(thin[t].astype(bool), thin_boundaries(maps[t])) and thin.max() <= 1, t
        assert counts[t] == thin[t].sum()
    cap = int(counts.max()) + 1 if cap is None else cap
    matched, above, counters = _match(torch, lib, q, thin, img_of, levels, em.offsets(d2), cap)
    for t in range(len(maps)):
        m, a = _want(q[img_of[t]], thin[t].astype(bool), levels, d2)
        assert matched[t].tolist() == m.tolist(), (t, levels, d2, matched[t].tolist(), m.tolist())
        assert above[img_of[t]].tolist() == a.tolist(), (t, levels, d2)
    return matched, counters


# ---- the definition

def test_worked_examples_through_the_c_calls(torch_cuda, lib):
    row = np.array([[[0, 0, 1, 0]]], np.uint8)
    thin, counts = _thin(torch_cuda, lib, row)
    assert thin.tolist() == [[[0, 1, 1, 0]]] and counts.tolist() == [2]
    for q in ([1, 2, 0, 0], [0, 0, 2, 1]):
        matched, above, _ = _match(torch_cuda, lib, np.array([[q]], np.int32), thin, [0], 2, em.offsets(1), 3)
        assert matched.tolist() == [[2, 1]] and above.tolist() == [[2, 1]], q
    labels = np.repeat(np.array([0, 0, 0, 1, 1], np.uint16), 9).reshape(1, 5, 9)
    thin, counts = _thin(torch_cuda, lib, labels)
    assert counts.tolist() == [9] and thin[0, 2].all() and thin.sum() == 9
    q = np.zeros((1, 5, 9), np.int32)
    q[0, 1:4] = 1
    matched, above, _ = _match(torch_cuda, lib, q, thin, [0], 1, em.offsets(1), 10)
    assert matched.tolist() == [[9]] and above.tolist() == [[27]]


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (13, 17), (33, 47)], ids=lambda s: "%dx%d" % s)
def test_random_maps_equal_match_count_at_every_level(torch_cuda, lib, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    some = 0
    for levels in (1, 4, 256):
        for d2 in (0, 1, 18, 20):
            q, img_of, maps = _batch(rng, shape, levels)
            maps = maps.astype(np.uint8 if (levels + d2) % 2 else np.uint16)
            matched, _ = _check_batch(torch_cuda, lib, q, img_of, maps, levels, d2)
            some += int(matched.sum())
    assert some > 0 or shape == (1, 1)
    assert len(em.offsets(20)) == 69 and len(em.offsets(18)) == 61


def test_the_largest_disc(torch_cuda, lib):
    """D2 = 160: 505 offsets, eight lane chunks, on a 24 x 31 map (the disc covers most of it from anywhere)."""
    assert len(em.offsets(160)) == 505
    rng = np.random.default_rng(160)
    for levels in (4, 256):
        q, img_of, maps = _batch(rng, (24, 31), levels)
        _check_batch(torch_cuda, lib, q, img_of, maps.astype(np.uint16), levels, 160)


def _staircase():
    """The chain's contour under a map whose pixels arrive one per level from the right: x = 200 first, x = 3 last of them, each
    taking the contour pixel on its left; then x = 1, whose only contour pixel is taken: its search runs to the free pixel at the
    far end, 198 deep, and augments."""
    labels, _ = em_chain()
    q = np.zeros((1, 204), np.int32)
    q[0, 3:201] = np.arange(3, 201) - 1
    q[0, 1] = 1
    return labels, q


def test_the_chain_and_cap(torch_cuda, lib):
    """Image 0: the chain (the last level's search from x = 1 runs the chain's length and fails). Image 1: the staircase (a search
    198 deep that augments). Image 2: a small random map. ``cap`` = max |Q| + 1 exactly: right. ``cap`` = 2: the two long maps get
    -1 in their whole rows, the third is right, the canaries are intact."""
    torch = torch_cuda
    labels, q_chain = em_chain()
    _, q_stairs = _staircase()
    rng = np.random.default_rng(7)
    small = np.zeros((1, 204), np.int64)
    small[0, 100:] = 1
    q = np.stack([q_chain, q_stairs, (rng.integers(0, 4, size=(1, 204)) * 60).astype(np.int32)])
    maps = np.stack([labels, labels, small]).astype(np.uint8)
    img_of = np.array([0, 1, 2], np.int32)
    levels = 256
    matched, counters = _check_batch(torch, lib, q, img_of, maps, levels, 1)           # cap = 199 + 1
    assert matched[0, 0] == 199 and matched[0, 1] == 199 and matched[1, 0] == 199 and matched[1, 1] == 198
    assert counters[0, 2] > 64 and counters[0, 3] >= 1 and counters[1, 2] > 64, counters.tolist()       # deepest stack, failed searches
    thin, counts = _thin(torch, lib, maps)
    assert counts.tolist() == [199, 199, 1]
    got, above, _ = _match(torch, lib, q, thin, img_of, levels, em.offsets(1), 2)
    assert (got[:2] == -1).all() and got[2].tolist() == matched[2].tolist()
    assert above.tolist() == [_want(q[i], thin[i].astype(bool), levels, 1)[1].tolist() for i in range(3)]
    # the reference's own restatement overflows where the kernel does
    assert em.sweep(q[0], thin[0], levels, em.offsets(1), cap=2)[0][0] == -1
    # a map whose image does not exist: its row is -1, the others are right
    got, _, _ = _match(torch, lib, q, thin, np.array([0, 3, 2], np.int32), levels, em.offsets(1), 200)
    assert got[0].tolist() == matched[0].tolist() and (got[1] == -1).all() and got[2].tolist() == matched[2].tolist()
    got, _, _ = _match(torch, lib, q, thin, np.array([-1, 1, 2], np.int32), levels, em.offsets(1), 200)
    assert (got[0] == -1).all() and got[1].tolist() == matched[1].tolist()


def test_any_offset_table_is_exact(torch_cuda, lib):
    """A table that is no disc (three offsets, one of them far outside any image, one twice): pairs are allowed by the table alone."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    rng = np.random.default_rng(3)
    h, w = 11, 14
    q = (rng.random((1, h, w)) < 0.5).astype(np.int32)
    thin = (rng.random((1, h, w)) < 0.3).astype(np.uint8)
    table = np.array([[0, 2], [-1, -1], [0, 2], [1 << 30, -(1 << 30)], [2, 0]], np.int32)
    matched, _, _ = _match(torch_cuda, lib, q, thin, [0], 1, table, int(thin.sum()) + 1)
    rows, cols = [], []
    for y, x in np.argwhere(q[0] > 0):
        for dy, dx in ((0, 2), (-1, -1), (2, 0)):
            if 0 <= y + dy < h and 0 <= x + dx < w and thin[0, y + dy, x + dx]:
                rows.append(y * w + x)
                cols.append((y + dy) * w + x + dx)
    graph = csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(h * w, h * w))
    assert matched[0, 0] == int(np.sum(maximum_bipartite_matching(graph, perm_type="column") >= 0)) > 5


# ---- the buffer contract

@pytest.mark.parametrize("shape,levels,d2", [((1, 1), 1, 0), ((9, 1), 4, 1), ((13, 17), 256, 18), ((33, 47), 7, 20)])
def test_buffer_contract(torch_cuda, lib, shape, levels, d2):
    """Every buffer is an exact-size arena view between 4096-byte canary bands (``_thin`` and ``_match`` check them and the
    inputs); outputs and workspace filled with 0x00 and with 0xA5 give the same bytes and the reference's values."""
    rng = np.random.default_rng(11)
    q, img_of, maps = _batch(rng, shape, levels)
    maps = maps.astype(np.uint8)
    runs = []
    for poison in POISONS:
        thin, counts = _thin(torch_cuda, lib, maps, poison)
        matched, above, _ = _match(torch_cuda, lib, q, thin, img_of, levels, em.offsets(d2), int(counts.max()) + 1, poison)
        runs.append((thin, counts, matched, above))
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    for t in range(6):
        m, a = _want(q[img_of[t]], runs[0][0][t].astype(bool), levels, d2)
        assert runs[0][2][t].tolist() == m.tolist() and runs[0][3][img_of[t]].tolist() == a.tolist()


def test_ranges_that_only_touch_do_not_overlap(torch_cuda, lib):
    """matched right behind q, above right behind matched, the workspace right behind the thin planes: accepted, and right."""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    shape, levels, d2 = (16, 16), 4, 2
    q, img_of, maps = _batch(rng, shape, levels)
    thin, counts = _thin(torch, lib, maps.astype(np.uint8))
    cap, offs = int(counts.max()) + 1, em.offsets(d2)
    nbytes = lib.gcs_edge_match_bytes(3, 6, 16, 16, cap)
    pool = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    at = {"q": 0, "matched": q.nbytes, "above": q.nbytes + 4 * 6 * levels, "thin": 8192, "ws": 8192 + thin.nbytes, "img_of": 1 << 19,
          "offs": (1 << 19) + 256}
    assert (8192 + thin.nbytes) % 256 == 0 and at["above"] + 4 * 3 * levels <= 8192 and at["ws"] + nbytes < 1 << 19
    for name, arr in (("q", q), ("thin", thin), ("img_of", img_of), ("offs", offs)):
        raw = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()).cuda()
        pool[at[name]:at[name] + raw.numel()].copy_(raw)
    p = {k: pool.data_ptr() + v for k, v in at.items()}
    rc = lib.gcs_edge_match(p["q"], p["thin"], p["img_of"], 3, 6, 16, 16, levels, p["offs"], len(offs), cap, p["ws"], p["matched"],
                            p["above"], _st(torch))
    assert rc == 0, lib.gcs_last_error()
    host = pool.cpu().numpy()
    matched = host[at["matched"]:at["matched"] + 4 * 6 * levels].view(np.int32).reshape(6, levels)
    for t in range(6):
        assert matched[t].tolist() == _want(q[img_of[t]], thin[t].astype(bool), levels, d2)[0].tolist()
    # one byte closer and it is refused
    assert lib.gcs_edge_match(p["q"], p["thin"], p["img_of"], 3, 6, 16, 16, levels, p["offs"], len(offs), cap, p["ws"], p["matched"] - 4,
                              p["above"], _st(torch)) == 1


# ---- the stream contract (include/gcs.h, "Streams"), in the manner of tests/test_gpu_stream_contract.py

def _ok(lib, rc):
    assert rc == 0, lib.gcs_last_error()


def stream_cases(lib):
    """The two capturable entry points as cases of tests/stream_order.py: true inputs and decoys (other legal inputs of the same
    size that give other outputs), the check of the quiet run against the references."""
    import stream_order as so
    from gabor_color_image_segmentation_amd.evaluate import thin_boundaries
    rng = np.random.default_rng(21)
    shape, levels, d2 = (29, 37), 16, 18
    h, w = shape
    q, img_of, maps = _batch(rng, shape, levels)
    q2, _, maps2 = _batch(rng, shape, levels)
    maps, maps2 = maps.astype(np.uint8), maps2.astype(np.uint8)
    thin, thin2 = (np.stack([thin_boundaries(m) for m in mm]).astype(np.uint8) for mm in (maps, maps2))
    img_of2 = np.array([0, 0, 1, 2, 2, 2], np.int32)
    offs = em.offsets(d2)
    offs2 = np.concatenate([em.offsets(1)] * 13)[:len(offs)]                  # 61 rows again, the disc of D2 = 1 over and over
    cap = int(max(thin.sum(axis=(1, 2)).max(), thin2.sum(axis=(1, 2)).max())) + 1
    nbytes = lib.gcs_edge_match_bytes(3, 6, h, w, cap)

    def want_match(q, thin, img_of, d2):
        got = [_want(q[img_of[t]], thin[t].astype(bool), levels, d2) for t in range(6)]
        above = np.zeros((3, levels), np.int64)
        for t in range(6):
            above[img_of[t]] = got[t][1]
        return np.stack([g[0] for g in got]), above

    def check_match(o):
        m, a = want_match(q, thin, img_of, d2)
        so.same(so.view(o["matched"], np.int32, (6, levels)), m, "matched")
        so.same(so.view(o["above"], np.int32, (3, levels)), a, "above")

    def check_thin(o):
        so.same(so.view(o["thin"], np.uint8, maps.shape), thin, "thin")
        so.same(so.view(o["counts"], np.int32), thin.sum(axis=(1, 2)), "counts")

    match = so.Case("edge_match", ["gcs_edge_match"],
                    dict(q=so.late(q, q2), thin=so.late(thin, thin2), img_of=so.late(img_of, img_of2), offsets=so.late(offs, offs2),
                         ws=so.scratch(nbytes), matched=so.out(4 * 6 * levels), above=so.out(4 * 3 * levels)),
                    lambda lib, p, st: _ok(lib, lib.gcs_edge_match(p["q"], p["thin"], p["img_of"], 3, 6, h, w, levels, p["offsets"],
                                                                   len(offs), cap, p["ws"], p["matched"], p["above"], st)),
                    check_match)
    match.want_decoy = lambda: want_match(q2, thin2, img_of2, 1)
    match.shapes = ((6, levels), (3, levels))
    truth = so.Case("truth_thin", ["gcs_truth_thin"],
                    dict(maps=so.late(maps, maps2), thin=so.out(maps.size), counts=so.out(4 * 6)),
                    lambda lib, p, st: _ok(lib, lib.gcs_truth_thin(p["maps"], 6, h, w, 1, p["thin"], p["counts"], st)), check_thin)
    return [match, truth]


def test_late_inputs_are_honoured_and_the_calls_do_not_wait(torch_cuda, lib):
    """QUIET on the true inputs == the references, on the decoys other values; LATE: on a side stream behind a gate, every input
    holding its decoy until a copy behind the gate puts the true bytes in place; the call returns while the gate runs and the
    outputs equal the quiet run."""
    import stream_order as so
    torch = torch_cuda
    cases = stream_cases(lib)
    run = so.Runner(torch, lib)
    times = []
    for case in cases:
        case.quiet["true"], dt = run.quiet_run(case, "true")
        case.check(case.quiet["true"])
        case.quiet["decoy"], _ = run.quiet_run(case, "decoy")
        times.append(dt)
        for name in case.outputs():
            assert not np.array_equal(case.quiet["decoy"][name], case.quiet["true"][name]), (case.name, name)
    m, a = cases[0].want_decoy()
    so.same(so.view(cases[0].quiet["decoy"]["matched"], np.int32, m.shape), m, "matched on the decoys")
    so.same(so.view(cases[0].quiet["decoy"]["above"], np.int32, a.shape), a, "above on the decoys")
    run.calibrate()
    run.settle(times)
    for case in cases:
        run.hold_late(case)
        run.release(case)


def test_capture_and_replay_on_other_inputs():
    """One child process (a failed capture leaves its thread unable to launch: it must not take this process with it): both entry
    points captured on a side stream and replayed on the second input set."""
    child = os.path.join(HERE, "checkers", "edge_match_capture_child.py")
    r = subprocess.run([sys.executable, child], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    lines = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(OK|FAIL) (gcs_\w+)(.*)", line)
        if m:
            lines[m.group(2)] = (m.group(1), m.group(3))
    for sym in ("gcs_edge_match", "gcs_truth_thin"):
        assert sym in lines, (sym, "the child printed no line for it", r.returncode, r.stdout[-2000:])
        assert lines[sym][0] == "OK", (sym, lines[sym][1])
    assert r.returncode == 0, r.stdout[-2000:]


# ---- element offsets past 2^31

def test_maps_past_element_two_to_the_thirty_one(torch_cuda, lib):
    """129 annotator maps of 4096 x 4096: T H W = 2^31 + 2^24 elements (the thin planes pass byte 2^31, the state words byte
    2^33). Two images; map 0 belongs to image 0, the other 128 to image 1. Only the first and the last map carry a contour, in the
    image's first and last rows; both images carry map pixels there alone. Both maps == the reference on their patches (every
    pair lies inside them), every other row is zero."""
    torch = torch_cuda
    t, b, side, levels, d2 = 129, 2, 4096, 8, 18
    hw = side * side
    assert t * hw > 1 << 31 and (t - 1) * hw <= 1 << 31
    free, _ = torch.cuda.mem_get_info()
    need = 2 * t * hw + 4 * t * hw + 4 * 2 * b * hw + (2 << 30)
    if free < need:
        pytest.skip("this case holds %.1f GiB" % (need / 2 ** 30))
    rng = np.random.default_rng(31)
    ph, pw = 20, 40
    patch_maps = [np.cumsum(rng.random((ph, pw)) < 0.2, axis=1).astype(np.uint8) % 5 for _ in range(2)]
    patch_q = [(rng.integers(0, levels + 2, size=(ph, pw)) * (rng.random((ph, pw)) < 0.5)).astype(np.int32) for _ in range(2)]
    for m in patch_maps:                                      # a ring of the background label: no contour outside the patch
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 0
    maps = torch.zeros((t, side, side), dtype=torch.uint8, device="cuda")
    q = torch.zeros((b, side, side), dtype=torch.int32, device="cuda")
    where = [(0, 0, 0, 0), (t - 1, 1, side - ph, side - pw)]
    for k, (ti, bi, y0, x0) in enumerate(where):
        maps[ti, y0:y0 + ph, x0:x0 + pw] = torch.from_numpy(patch_maps[k]).cuda()
        q[bi, y0:y0 + ph, x0:x0 + pw] = torch.from_numpy(patch_q[k]).cuda()
    thin = torch.full((t, side, side), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((t,), -7, dtype=torch.int32, device="cuda")
    assert lib.gcs_truth_thin(maps.data_ptr(), t, side, side, 1, thin.data_ptr(), counts.data_ptr(), _st(torch)) == 0, lib.gcs_last_error()
    counts_h = counts.cpu().numpy()
    wants = []
    for k, (ti, bi, y0, x0) in enumerate(where):
        want_thin = em.thin(patch_maps[k])
        assert np.array_equal(thin[ti, y0:y0 + ph, x0:x0 + pw].cpu().numpy().astype(bool), want_thin) and want_thin.sum() > 20
        assert counts_h[ti] == want_thin.sum()
        wants.append(_want(patch_q[k], want_thin, levels, d2))
    assert not counts_h[1:-1].any() and int(thin.sum(dtype=torch.int64)) == int(counts_h.sum())
    del maps
    torch.cuda.empty_cache()
    cap = int(counts_h.max()) + 1
    ws = torch.empty(lib.gcs_edge_match_bytes(b, t, side, side, cap), dtype=torch.uint8, device="cuda")
    out = torch.full((t + b, levels), -7, dtype=torch.int32, device="cuda")
    img_of = torch.ones(t, dtype=torch.int32, device="cuda")
    img_of[0] = 0
    offs = torch.from_numpy(em.offsets(d2)).cuda()
    rc = lib.gcs_edge_match(q.data_ptr(), thin.data_ptr(), img_of.data_ptr(), b, t, side, side, levels, offs.data_ptr(), len(offs), cap,
                            ws.data_ptr(), out.data_ptr(), out[t:].data_ptr(), _st(torch))
    assert rc == 0, lib.gcs_last_error()
    got = out.cpu().numpy()
    for k, (ti, bi, _, _) in enumerate(where):
        assert got[ti].tolist() == wants[k][0].tolist() and got[t + bi].tolist() == wants[k][1].tolist(), k
        assert wants[k][0][0] > 10
    assert not got[1:t - 1].any()
    del ws, thin, q, out
    torch.cuda.empty_cache()


# ---- the host calls on two BSD fixture images

@pytest.fixture(scope="module")
def bsd(torch_cuda):
    """Images 100075 and 100098 (321 x 481) of tests/golden/bsd_inputs.npz with their 6 + 5 annotator maps, resident; a thick
    synthetic ribbon (strength falling off with the distance from the first annotator's contour, eleven pixels wide, with noise)
    and its direction map (the normal of the nearest contour pixel in 8 directions)."""
    from scipy import ndimage as ndi
    from gabor_color_image_segmentation_amd.evaluate import thin_boundaries
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth
    z = np.load(os.path.join(GOLD, "bsd_inputs.npz"))
    ids = ["100075", "100098"]
    truths = [[z["seg_%s_%d" % (i, k)] for k in range(int(z["nseg_" + i]))] for i in ids]
    stack = np.stack([s for ts in truths for s in ts])
    first = np.cumsum([0] + [len(ts) for ts in truths]).astype(np.int32)
    img_of = np.repeat(np.arange(2), np.diff(first)).astype(np.int32)
    truth = DeviceTruth(stack, first, img_of, [int(s.max()) + 1 for s in stack], "cuda")
    rng = np.random.default_rng(75)
    edges, dirs = [], []
    for ts in truths:
        dist, (iy, ix) = ndi.distance_transform_edt(~thin_boundaries(ts[0]), return_indices=True)
        yy, xx = np.mgrid[:dist.shape[0], :dist.shape[1]]
        angle = np.arctan2(yy - iy, xx - ix) % np.pi
        dirs.append((np.rint(angle / np.pi * 8).astype(np.int64) % 8).astype(np.uint8))
        edges.append((np.maximum(0, 6 - dist) * 150 + rng.integers(0, 90, size=dist.shape) * (dist < 6)).astype(np.int32))
    return truths, truth, np.stack(edges), np.stack(dirs)


def _hold_to_match_scores(torch, truths, truth, edges, taus):
    from gabor_color_image_segmentation_amd.evaluate import match_scores
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_match_resident
    rec, prec, f, step = edge_match_resident(torch.from_numpy(edges).cuda(), truth)
    assert rec.shape == (2, 256) and rec.dtype == np.float64 and step == -(-(int(edges.max()) + 1) // 256)
    for i in range(2):
        want = match_scores(edges[i], truths[i], [step * (tau + 1) - 1 for tau in taus])
        assert rec[i, taus].tolist() == want["recall"].tolist(), i
        assert prec[i, taus].tolist() == want["precision"].tolist(), i
        assert f[i, taus].tolist() == want["fmeasure"].tolist(), i
    return f


TAUS = [0, 5, 20, 60, 120, 180, 230, 255]


def test_edge_match_resident_on_a_thick_ribbon(torch_cuda, bsd):
    truths, truth, edges, _ = bsd
    f = _hold_to_match_scores(torch_cuda, truths, truth, edges, TAUS)
    assert 0.0 < f.max() < 1.0


def test_edge_match_resident_on_the_thinned_ribbon(torch_cuda, bsd):
    from gabor_color_image_segmentation_amd import Segmenter
    from gabor_color_image_segmentation_amd.evaluate_gpu import edge_match_counts_resident
    torch = torch_cuda
    truths, truth, edges, dirs = bsd
    thin = Segmenter().thin_edges_device(torch.from_numpy(edges).cuda(), torch.from_numpy(dirs).cuda(), n_directions=8)
    assert 0 < int(torch.count_nonzero(thin)) < np.count_nonzero(edges) // 3
    f = _hold_to_match_scores(torch, truths, truth, thin.cpu().numpy(), TAUS)
    assert f.max() > 0.2
    # the counts call by itself, the lazily built planes, an explicit D2, and the kernel's counters
    from gabor_color_image_segmentation_amd.evaluate import match_count, thin_boundaries
    planes, counts, n_thin = truth.thin_planes()
    assert truth.thin_planes()[0] is planes and n_thin.tolist() == [int(thin_boundaries(s).sum()) for ts in truths for s in ts]
    q = torch.clamp(thin // 200, max=4).to(torch.int32)
    matched, above, n, counters = edge_match_counts_resident(q, truth, 4, max_dist2=5, stats=True)
    assert n.tolist() == n_thin.tolist() and matched.shape == (11, 4) and above.shape == (2, 4) and counters.shape == (11, 4)
    qh = q.cpu().numpy()
    for t in (0, 10):
        i = 0 if t < 6 else 1
        assert matched[t, 1] == match_count(qh[i] > 1, thin_boundaries(truths[i][t - 6 * i]), 5)
        assert above[i, 1] == np.count_nonzero(qh[i] > 1)
    assert (counters[:, 0] >= matched[:, 0]).all()                    # at least one step per matched pixel
    with pytest.raises(ValueError, match="max_dist2"):
        edge_match_counts_resident(q, truth, 4, max_dist2=161)
    with pytest.raises(ValueError, match="levels"):
        edge_match_counts_resident(q, truth, 257)
    with pytest.raises(ValueError):
        edge_match_counts_resident(q[:1], truth, 4)


def test_an_annotator_without_a_contour_raises_as_the_host_does(torch_cuda):
    from gabor_color_image_segmentation_amd.evaluate import match_scores
    from gabor_color_image_segmentation_amd.evaluate_gpu import DeviceTruth, edge_match_resident
    torch = torch_cuda
    maps = np.zeros((2, 6, 8), np.uint16)
    maps[0, :, 4:] = 1
    truth = DeviceTruth(maps, [0, 2], [0, 0], [2, 1], "cuda")
    edges = np.zeros((1, 6, 8), np.int32)
    edges[0, :, 3] = 9
    with pytest.raises(ZeroDivisionError):
        match_scores(edges[0], list(maps), [0])
    with pytest.raises(ZeroDivisionError):
        edge_match_resident(torch.from_numpy(edges).cuda(), truth, levels=4)
    rec, prec, f, step = edge_match_resident(torch.zeros((1, 6, 8), dtype=torch.int32, device="cuda"), truth, levels=4)
    assert not rec.any() and not f.any() and step == 1       # no map pixel at any level: the zero rule, before any division
