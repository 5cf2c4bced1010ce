"""One-to-one matching at every level at once (SPEC.md §27) on the CPU: the section's worked examples, gcs_match_offsets against a
Python disc for every d2, the restatement (tests/edge_match_ref.py) against ``evaluate.match_count`` level by level on random
maps, the contract the frozen symbol tables cannot carry (include/gcs_match.h <-> ``_lib.MATCH_EXTENSIONS`` <-> the built
library's exports), every GCS_EINVAL case of the three entry points (refused before anything is launched, so they run without a
GPU) and the host calls' ValueErrors through stand-ins. No GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import edge_match_ref as em

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = {"gcs_match_offsets", "gcs_truth_thin", "gcs_edge_match_bytes", "gcs_edge_match"}


def _counts(q, labels, levels, d2):
    """(the restatement's M, above) after holding them to ``match_count`` at every level."""
    from gabor_color_image_segmentation_amd.evaluate import match_count, thin_boundaries
    truth = thin_boundaries(labels)
    assert np.array_equal(truth, em.thin(labels))
    m, above, _ = em.sweep(q, truth, levels, em.offsets(d2))
    qc = np.clip(q, 0, levels)
    for tau in range(levels):
        assert m[tau] == match_count(qc > tau, truth, d2), (tau, d2)
        assert above[tau] == np.count_nonzero(qc > tau)
    return m.tolist(), above.tolist()


# ---- the definition

def test_worked_examples():
    """SPEC.md §27: the row that needs an augmenting path, its mirror, and §26's ribbon."""
    from gabor_color_image_segmentation_amd.evaluate import match_scores
    labels = np.array([[0, 0, 1, 0]])
    assert np.flatnonzero(em.thin(labels)).tolist() == [1, 2]
    assert em.offsets(1).tolist() == [[-1, 0], [0, -1], [0, 0], [0, 1], [1, 0]]
    assert _counts(np.array([[1, 2, 0, 0]]), labels, 2, 1) == ([2, 1], [2, 1])       # pixel 0 reaches only contour pixel 1
    assert _counts(np.array([[0, 0, 2, 1]]), labels, 2, 1) == ([2, 1], [2, 1])
    labels = np.repeat(np.array([0, 0, 0, 1, 1]), 9).reshape(5, 9)
    assert np.array_equal(em.thin(labels), np.arange(5)[:, None].repeat(9, 1) == 2)
    q = np.zeros((5, 9), np.int32)
    q[1:4] = 1
    assert _counts(q, labels, 1, 1) == ([9], [27])
    sc = match_scores(q, [labels], [0], 1)
    assert sc["recall"][0] == 1.0 and sc["precision"][0] == 9 / 27
    # values outside 0 .. levels are clamped
    assert _counts(np.array([[-5, 9, 0, 0]]), np.array([[0, 0, 1, 0]]), 2, 1) == ([1, 1], [1, 1])


@pytest.mark.parametrize("d2", [0, 1, 2, 5, 18, 20])
def test_the_restatement_is_match_count_at_every_level(d2):
    """36 random maps per D2 (216 in all), up to 13 x 13, levels 1 .. 6, values below 0 and above ``levels`` among them."""
    rng = np.random.default_rng(100 + d2)
    for i in range(36):
        h, w = (int(v) for v in rng.integers(1, 14, size=2))
        levels = int(rng.integers(1, 7))
        labels = rng.integers(0, 3, size=(h, w)) if i % 3 else np.cumsum(rng.random((h, w)) < 0.15, axis=1)
        q = rng.integers(-1, levels + 2, size=(h, w)) * (rng.random((h, w)) < rng.choice([0.2, 0.6, 1.0]))
        _counts(q.astype(np.int32), labels, levels, d2)


def test_the_chain():
    """A 1 x 204 row at D2 = 1: |Q| = 199; the interior arrives first and the two end pixels last, so the last searches run the
    chain's length and one of them fails."""
    from gabor_color_image_segmentation_amd.evaluate import match_count
    labels, q = em_chain()
    truth = em.thin(labels)
    assert truth.sum() == 199
    m, above, steps = em.sweep(q, truth, 2, em.offsets(1))
    assert m.tolist() == [match_count(q > 0, truth, 1), match_count(q > 1, truth, 1)] and above.tolist() == [q.size - 3, q.size - 5]
    assert em.sweep(q, truth, 2, em.offsets(1), cap=2)[0].tolist() == [-1, -1]
    assert em.sweep(q, truth, 2, em.offsets(1), cap=200)[0].tolist() == m.tolist()


def em_chain():
    """-> (labels (1,204), q (1,204)): labels alternate on x = 2 .. 201 and are constant at both ends; q = 2 on x = 3 .. 201, 1 on
    x = 1 and x = 202, else 0."""
    labels = np.zeros((1, 204), np.int64)
    labels[0, 2:202] = np.arange(200) % 2
    labels[0, 202:] = 1
    q = np.zeros((1, 204), np.int32)
    q[0, 3:202] = 2
    q[0, 1] = q[0, 202] = 1
    return labels, q


# ---- the library: symbols and argument rules

@pytest.fixture(scope="module")
def lib(built):
    from gabor_color_image_segmentation_amd import _lib
    return _lib.load()


def test_gcs_match_offsets_is_the_disc(lib):
    sizes = {}
    for d2 in range(161):
        got, n = np.full((513, 2), -77, np.int32), np.full(2, -77, np.int32)
        assert lib.gcs_match_offsets(d2, got.ctypes.data, n.ctypes.data) == 0
        want = [(dy, dx) for dy in range(-13, 14) for dx in range(-13, 14) if dy * dy + dx * dx <= d2]
        assert n.tolist() == [len(want), -77] and got[:len(want)].tolist() == [list(p) for p in want] and (got[len(want):] == -77).all()
        assert np.array_equal(em.offsets(d2), got[:len(want)])
        sizes[d2] = len(want)
    assert (sizes[0], sizes[1], sizes[18], sizes[20], sizes[160]) == (1, 5, 61, 69, 505) and max(sizes.values()) <= 512


def test_gcs_match_offsets_refuses_bad_arguments(lib):
    room, n = np.zeros((512, 2), np.int32), np.full(1, -77, np.int32)
    for d2 in (-1, 161, 1 << 30):
        assert lib.gcs_match_offsets(d2, room.ctypes.data, n.ctypes.data) == 1 and b"gcs_match_offsets" in lib.gcs_last_error()
    assert lib.gcs_match_offsets(18, None, n.ctypes.data) == 1 and b"NULL" in lib.gcs_last_error()
    assert lib.gcs_match_offsets(18, room.ctypes.data, None) == 1 and b"NULL" in lib.gcs_last_error()
    assert not room.any() and n[0] == -77


def test_header_table_and_exports_agree(lib):
    from gabor_color_image_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gcs_match.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gcs_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.MATCH_EXTENSIONS) == SYMBOLS, declared ^ set(_lib.MATCH_EXTENSIONS)
    assert 'extern "C"' in hdr and "ABI 18" in hdr and '#include "gcs.h"' in hdr
    assert "torch" not in hdr.lower() and "at::" not in hdr
    for name, (res, args) in _lib.MATCH_EXTENSIONS.items():
        fn = getattr(lib, name)                               # exported by the built library
        assert fn.restype is res and list(fn.argtypes) == args
        kind, decl = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, code).groups()
        assert (kind == "size_t") == (res is C.c_size_t)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):                        # pointers and the stream are void pointers, the rest ints
            assert (a is C.c_void_p) == ("*" in p or p.startswith("gcs_stream_t")), (name, p)
    others = set(_lib.SIGNATURES) | set(_lib.EXTENSIONS) | set(_lib.THIN_EXTENSIONS)
    assert not set(_lib.MATCH_EXTENSIONS) & others
    assert lib.gcs_abi_version() == 18 and _lib.ABI_VERSION == 18


def test_the_frozen_headers_and_tables_do_not_know_the_symbols():
    from gabor_color_image_segmentation_amd import _lib
    for name in ("gcs.h", "gcs_cues.h", "gcs_thin.h"):
        hdr = open(os.path.join(ROOT, "include", name)).read()
        assert not [s for s in SYMBOLS if s in hdr] and "gcs_match" not in hdr, name
    assert not SYMBOLS & (set(_lib.SIGNATURES) | set(_lib.EXTENSIONS) | set(_lib.THIN_EXTENSIONS))
    assert set(_lib.EXTENSIONS) == {"gcs_cue_gradient"} and set(_lib.THIN_EXTENSIONS) == {"gcs_thin_steps", "gcs_edge_thin"}


def test_a_library_without_the_symbols_still_loads_and_the_host_calls_refuse(built, monkeypatch):
    from gabor_color_image_segmentation_amd import _lib, evaluate_gpu
    saved, held = dict(_lib.MATCH_EXTENSIONS), _lib._lib
    try:
        _lib.MATCH_EXTENSIONS["gcs_not_in_this_library"] = (C.c_int, [])
        _lib._lib = None
        lib = _lib.load()
        assert not hasattr(lib, "gcs_not_in_this_library") and all(hasattr(lib, s) for s in SYMBOLS)
    finally:
        _lib.MATCH_EXTENSIONS.clear()
        _lib.MATCH_EXTENSIONS.update(saved)
        _lib._lib = held
    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace())       # a library of ABI 18 from before the header
    import torch
    truth = _standin_truth()
    q = torch.zeros((2, 5, 7), dtype=torch.int32)
    with pytest.raises(ValueError, match="needs a library that has it"):
        evaluate_gpu.edge_match_counts_resident(q, truth, 4)
    with pytest.raises(ValueError, match="needs a library that has it"):
        evaluate_gpu.edge_match_resident(q, truth, levels=4)


P = [C.c_void_p(q << 36) for q in range(1, 9)]               # non-NULL dummies far apart, 256-byte aligned, never dereferenced


def _at(q, off):
    return C.c_void_p(q.value + off)


def test_truth_thin_validates_before_launching(lib):
    good = dict(maps=P[0], T=3, H=19, W=23, u8=1, thin=P[1], counts=P[2])

    def call(**bad):
        a = dict(good, **bad)
        return lib.gcs_truth_thin(a["maps"], a["T"], a["H"], a["W"], a["u8"], a["thin"], a["counts"], None)
    for bad in (dict(maps=None), dict(thin=None), dict(counts=None)):
        assert call(**bad) == 1 and b"NULL" in lib.gcs_last_error(), bad
    for bad in (dict(T=0), dict(T=-1), dict(T=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097)):
        assert call(**bad) == 1 and b"shape" in lib.gcs_last_error(), bad
    px = 3 * 19 * 23
    for bad in (dict(thin=P[0]), dict(thin=_at(P[0], px - 1)), dict(thin=_at(P[0], -px + 1)), dict(counts=_at(P[0], px - 1)),
                dict(counts=_at(P[0], -11)), dict(counts=P[1]), dict(counts=_at(P[1], px - 1)), dict(thin=_at(P[2], 11)),
                dict(u8=0, thin=_at(P[0], 2 * px - 1))):
        assert call(**bad) == 1 and b"overlaps" in lib.gcs_last_error(), bad
    assert b"gcs_truth_thin" in lib.gcs_last_error()


def test_edge_match_validates_before_launching(lib):
    """Argument errors are reported without touching the GPU (so this runs on the CPU box)."""
    B, T, H, W, L, N, CAP = 2, 5, 19, 23, 7, 61, 40
    good = dict(q=P[0], thin=P[1], img_of=P[2], B=B, T=T, H=H, W=W, levels=L, offsets=P[3], n_off=N, cap=CAP, ws=P[4], matched=P[5],
                above=P[6])

    def call(**bad):
        a = dict(good, **bad)
        return lib.gcs_edge_match(a["q"], a["thin"], a["img_of"], a["B"], a["T"], a["H"], a["W"], a["levels"], a["offsets"], a["n_off"],
                                  a["cap"], a["ws"], a["matched"], a["above"], None)
    for name in ("q", "thin", "img_of", "offsets", "ws", "matched", "above"):
        assert call(**{name: None}) == 1 and b"NULL" in lib.gcs_last_error(), name
    for bad in (dict(B=0), dict(B=65536), dict(T=0), dict(T=-2), dict(T=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097),
                dict(cap=0), dict(cap=-1), dict(cap=4096 * 4096 + 2)):
        assert call(**bad) == 1 and b"shape" in lib.gcs_last_error(), bad
        a = dict(good, **bad)
        assert lib.gcs_edge_match_bytes(a["B"], a["T"], a["H"], a["W"], a["cap"]) == 0
    for bad in (dict(levels=0), dict(levels=-1), dict(levels=257), dict(n_off=0), dict(n_off=513)):
        assert call(**bad) == 1 and b"argument" in lib.gcs_last_error(), bad
    assert call(ws=_at(P[4], 64)) == 1 and b"aligned" in lib.gcs_last_error()
    nbytes = lib.gcs_edge_match_bytes(B, T, H, W, CAP)
    hw = H * W
    # what the workspace has to hold at the least: the counters, two histogram rows per image, the sorted list, the state, the
    # stack (two words per entry) and the visit log
    assert nbytes >= 16 * T + 2 * B * 257 * 4 + 4 * B * hw + 4 * T * hw + 12 * T * CAP and nbytes % 256 == 0
    assert lib.gcs_edge_match_bytes(B, T, H, W, CAP + 64) > nbytes
    sizes = dict(q=4 * B * hw, thin=T * hw, img_of=4 * T, offsets=8 * N)
    outs = dict(ws=nbytes, matched=4 * T * L, above=4 * B * L)
    for o, on in outs.items():
        step = 256 if o == "ws" else 1
        for i, n in sizes.items():
            for off in (0, (n - 1) // step * step, -((on - 1) // step * step)):
                assert call(**{o: _at(good[i], off)}) == 1 and b"overlaps an input" in lib.gcs_last_error(), (o, i, off)
        for p, pn in outs.items():
            if p != o and o != "ws":
                for off in (0, (pn - 1) // 4 * 4, -(on - 4)):
                    assert call(**{o: _at(good[p], off)}) == 1 and b"overlap" in lib.gcs_last_error(), (o, p, off)
    assert b"gcs_edge_match" in lib.gcs_last_error()
    # (ranges that only touch do not overlap; such a call would launch, so it is made on the GPU: tests/test_gpu_edge_match.py)


# ---- the host calls' own checks, through stand-ins: a truth without a device, CPU tensors

def _standin_truth(b=2, h=5, w=7, t=3):
    import torch
    return types.SimpleNamespace(b=b, h=h, w=w, t=t, device=torch.device("cpu"), first=np.array([0, 2, 3], np.int32))


def test_host_calls_refuse_before_any_launch(built, monkeypatch):
    import torch
    from gabor_color_image_segmentation_amd import _lib, evaluate_gpu as eg

    def no_library():
        raise AssertionError("an argument error must be raised before the library is touched")
    monkeypatch.setattr(_lib, "load", no_library)
    truth = _standin_truth()
    q = torch.zeros((2, 5, 7), dtype=torch.int32)
    for fn, kw in ((eg.edge_match_counts_resident, dict(levels=4)), (eg.edge_match_resident, dict(levels=4, step=1))):
        for bad_q in (q[:1], q[:, :4], q[:, :, :6], q.to(torch.int64), q[0]):
            with pytest.raises(ValueError):
                fn(bad_q, truth, **kw)
        for levels in (0, -1, 257):
            with pytest.raises(ValueError, match="levels"):
                fn(q, truth, **dict(kw, levels=levels))
        for d2 in (161, -1, 1 << 20):
            with pytest.raises(ValueError, match="max_dist2"):
                fn(q, truth, max_dist2=d2, **kw)
    big = types.SimpleNamespace(b=1, h=4097, w=3, t=1, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="4096"):
        eg.edge_match_counts_resident(torch.zeros((1, 4097, 3), dtype=torch.int32), big, 4, max_dist2=18)
    # match_distance2 of a large image passes 160: refused by default, taken with an explicit D2 (further checks then need a device)
    from gabor_color_image_segmentation_amd.evaluate import match_distance2
    assert match_distance2(321, 481) == 18 and match_distance2(1700, 1700) > 160
    wide = types.SimpleNamespace(b=1, h=1700, w=1700, t=1, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="max_dist2"):
        eg.edge_match_counts_resident(torch.zeros((1, 1700, 1700), dtype=torch.int32), wide, 4)
