"""The self-updating Lloyd passes (gcs_kmeans_pass_fused): a single-rank loop over whole images is n_iter launches -
every pass makes its own centroids (the SPEC.md §4 init pixels, or the §4 update from the sums the previous pass added into the
shared rows of the workspace with 64-bit atomics) - instead of init + n_iter passes + (n_iter - 1) reduce launches. Everything
here is checked against the C oracle (and the centroids against the init / pass / reduce path, bit for bit): both codebook modes,
every residue of the three-buffer rotation, the one-pass loop that never accumulates, loops that follow one another on one
workspace (the state a loop leaves is the state it found), the captured graph, and a library that lacks the entry points."""
import numpy as np
import pytest

import fused_workspace as fw
import hot_banks as hb
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

FUSED_SYMBOLS = ("gcs_kmeans_fused_workspace_bytes", "gcs_kmeans_pass_fused")


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _synth(b, h, w, seed):
    from gabor_color_image_segmentation_amd.synthetic import synthetic_batch
    return synthetic_batch(b, h, w, seed=seed)


def _grating(h, w, f=0.4, lo=0, hi=255, vertical=True):
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.where(np.sin(2 * np.pi * f * (xx if vertical else yy)) >= 0, hi, lo).astype(np.uint8)
    return np.stack([g, g, g], -1)


class _Spy:
    """Counts the launches of a HipOps by kind, and keeps the loop on the path the test is about."""

    def __init__(self, seg):
        self.n = dict(init=0, reduce=0, fused=0, plain=0)
        ops = seg.ops
        for name, key in (("kmeans_init", "init"), ("reduce_finalize", "reduce"), ("reduce", "reduce")):
            setattr(ops, name, self._count(getattr(ops, name), key))
        for name in ("assign_accumulate", "assign_raster"):
            setattr(ops, name, self._count_pass(getattr(ops, name)))

    def _count(self, fn, key):
        def wrapped(*a, **kw):
            self.n[key] += 1
            return fn(*a, **kw)
        return wrapped

    def _count_pass(self, fn):
        def wrapped(*a, **kw):
            self.n["fused" if kw.get("fused") is not None else "plain"] += 1
            return fn(*a, **kw)
        return wrapped


def _segmenter(**kw):
    from gabor_color_image_segmentation_amd import Segmenter
    seg = Segmenter(**kw)
    return seg, _Spy(seg)


def _device_labels(torch, seg, imgs, mode):
    return seg.segment_device(torch.from_numpy(imgs).cuda(), mode=mode).cpu().numpy()


def _oracle(seg, imgs, mode, n_iter=None):
    return co.segment_batch(imgs, seg.bank.tapq, seg.bank.shift, seg.bank.n_orient, k=seg.k,
                            n_iter=seg.n_iter if n_iter is None else n_iter, mode=mode)


def _workspace_is_as_found(seg):
    """White box (include/gcs.h: 'every complete loop leaves the workspace as it found it'): the three sum buffers and the ticket
    are zero again; only the two centroid arrays behind the sums (each a multiple of 256 bytes) hold data. The layout is that of
    tests/fused_workspace.py."""
    n = 0
    for (g, h, w, mode), ws in seg._ws.items():
        fold = ws["fold"]
        assert fold is not None
        n_sets = g if mode == "per_image" else 1
        rows = fw.fold_rows(g, seg.ops.lib.gcs_kmeans_parts_per_image(g, h, w), n_sets, fw.env_fold_rows())
        v = fw.views(fold.cpu().numpy(), n_sets, rows, seg.k, seg.bank.n_features)
        for i in range(3):
            assert not v.sum_raw[i].any(), "a sum buffer was left dirty"
        assert not v.ticket_raw.any(), "the ticket was left set"
        n += 1
    assert n > 0


@pytest.mark.parametrize("mode", ["per_image", "global"])
@pytest.mark.parametrize("n_iter", [1, 2, 3, 4, 10])
def test_labels_equal_the_c_oracle_for_every_rotation_residue(torch_cuda, mode, n_iter):
    """B = 5 on a shape with both packed edge strips, one image a grating (every tile flagged): n_iter = 1 never accumulates,
    2 .. 4 end on every residue of the buffer rotation, 10 is the flagship's count. No init and no reduce launch is made."""
    h, w = 81, 121
    imgs = _synth(5, h, w, seed=31)
    imgs[3] = _grating(h, w)
    seg, spy = _segmenter(n_iter=n_iter)
    got = _device_labels(torch_cuda, seg, imgs, mode)
    assert spy.n == dict(init=0, reduce=0, fused=n_iter, plain=0), spy.n
    assert np.array_equal(got, _oracle(seg, imgs, mode))
    _workspace_is_as_found(seg)


@pytest.mark.parametrize("mode", ["per_image", "global"])
@pytest.mark.parametrize("h,w", [(321, 481), (137, 82)])
def test_one_image_and_the_portrait_shape(torch_cuda, mode, h, w):
    imgs = _synth(1, h, w, seed=h)
    seg, spy = _segmenter(n_iter=5)
    got = _device_labels(torch_cuda, seg, imgs, mode)
    assert spy.n["fused"] == 5 and spy.n["init"] == spy.n["reduce"] == spy.n["plain"] == 0
    assert np.array_equal(got, _oracle(seg, imgs, mode))
    _workspace_is_as_found(seg)


def test_the_portrait_batch(torch_cuda):
    imgs = _synth(5, 481, 321, seed=12)
    seg, spy = _segmenter(n_iter=4)
    for mode in ("global", "per_image"):
        assert np.array_equal(_device_labels(torch_cuda, seg, imgs, mode), _oracle(seg, imgs, mode)), mode
    assert spy.n == dict(init=0, reduce=0, fused=8, plain=0)


@pytest.mark.parametrize("mode,n_iter", [("global", 10), ("per_image", 4)])
def test_the_timed_batch(torch_cuda, mode, n_iter):
    """B = 64 at 321 x 481: 768 workgroups fold into the shared rows (global: the flagship of bench.py)."""
    from gabor_color_image_segmentation_amd.synthetic import synthetic_shard
    imgs = synthetic_shard(0, 64, 321, 481)
    seg, spy = _segmenter(n_iter=n_iter)
    got = _device_labels(torch_cuda, seg, imgs, mode)
    assert spy.n == dict(init=0, reduce=0, fused=n_iter, plain=0)
    assert np.array_equal(got, _oracle(seg, imgs, mode))
    _workspace_is_as_found(seg)


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_a_hot_bank(torch_cuda, mode):
    """Values up to 46 339 (tests/hot_banks.py): the largest sums the 64-bit fold sees per pixel, flagged and clean tiles mixed."""
    bank = hb.hot_bank(4, 6, 13, 8)
    seg = hb.hot_segmenter(bank, n_iter=4)
    spy = _Spy(seg)
    imgs = hb.hot_images(5, 81, 121, seed=7)
    got = _device_labels(torch_cuda, seg, imgs, mode)
    assert spy.n == dict(init=0, reduce=0, fused=4, plain=0)
    want = co.segment_batch(imgs, bank.tapq, bank.shift, bank.n_orient, k=8, n_iter=4, mode=mode)
    assert np.array_equal(got, want) and len(np.unique(want)) > 1


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_empty_clusters_keep_their_centroid(torch_cuda, mode):
    """A constant image and a two-colour image have fewer distinct pixels than k = 8: most clusters are empty after the first
    pass and must keep the centroid of the pass before (read back from the other centroid array), pass after pass."""
    h, w = 64, 96
    flat = np.full((h, w, 3), 90, np.uint8)
    two = flat.copy()
    two[:, w // 2:] = (200, 30, 120)
    imgs = np.stack([flat, two, _grating(h, w)])
    seg, spy = _segmenter(n_iter=5)
    got = _device_labels(torch_cuda, seg, imgs, mode)
    assert spy.n["fused"] == 5 and spy.n["plain"] == 0
    want = _oracle(seg, imgs, mode)
    assert np.array_equal(got, want)
    if mode == "per_image":
        assert len(np.unique(want[0])) < 8


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_centroids_after_t_passes_equal_the_two_launch_path(torch_cuda, mode):
    """``cent`` after a loop = the centroids its last pass used: n_iter = t + 1 leaves the result of t updates. Bit for bit the
    same as init / pass / reduce_finalize leave, t = 1 .. 4."""
    torch = torch_cuda
    h, w = 81, 121
    imgs = _synth(5, h, w, seed=5)
    dev = torch.from_numpy(imgs).cuda()
    for t in range(1, 5):
        new, spy_new = _segmenter(n_iter=t + 1)
        old, spy_old = _segmenter(n_iter=t + 1)
        old.ops.has_fused = False
        lab_new = new.segment_device(dev, mode=mode)
        lab_old = old.segment_device(dev, mode=mode)
        assert spy_new.n["fused"] == t + 1 and spy_old.n == dict(init=1, reduce=t, fused=0, plain=t + 1)
        c_new, c_old = new._ws[(5, h, w, mode)]["cent"], old._ws[(5, h, w, mode)]["cent"]
        assert torch.equal(c_new, c_old), t
        assert c_new.any() and torch.equal(lab_new, lab_old)


@pytest.mark.parametrize("mode", ["per_image", "global"])
def test_loops_follow_one_another_on_one_workspace(torch_cuda, mode):
    """Two calls in a row, then calls with other pass counts, all on one Segmenter (one workspace): n_iter = 2 twice is the case in
    which the buffer the last pass reads is the one the next call's first pass adds into."""
    h, w = 81, 121
    seg, spy = _segmenter(n_iter=2)
    total = 0
    for i, n_iter in enumerate([2, 2, 5, 1, 4, 3, 3]):
        seg.n_iter = n_iter
        imgs = _synth(5, h, w, seed=100 + i)
        assert np.array_equal(_device_labels(torch_cuda, seg, imgs, mode), _oracle(seg, imgs, mode)), (i, n_iter)
        _workspace_is_as_found(seg)
        total += n_iter
    assert len(seg._ws) == 1 and spy.n == dict(init=0, reduce=0, fused=total, plain=0)


@pytest.mark.parametrize("n_iter", [2, 4])
def test_the_graph_replayed_small_call_equals_the_eager_one(torch_cuda, n_iter):
    """segment_batch on a small call replays a captured graph of the whole step: replay after replay finds the workspace as the
    loop before left it. == the eager launches (GCS_DEBUG no_graph) == the C oracle."""
    from gabor_color_image_segmentation_amd.segmenter import DebugSwitches
    h, w = 72, 104
    graph, spy_g = _segmenter(n_iter=n_iter)
    eager, spy_e = _segmenter(n_iter=n_iter)
    eager.debug = DebugSwitches("no_graph")
    for mode in ("per_image", "global"):
        for i in range(3):
            imgs = _synth(2, h, w, seed=40 + i)
            want = _oracle(graph, imgs, mode)
            assert np.array_equal(graph.segment_batch(imgs, mode=mode), want), (mode, i)
            assert np.array_equal(eager.segment_batch(imgs, mode=mode), want), (mode, i)
    assert any(ent["graph"] is not None for ent in graph._graphs.values()), "no graph was captured: nothing was replayed"
    assert spy_g.n["init"] == spy_g.n["reduce"] == spy_g.n["plain"] == 0 and spy_g.n["fused"] > 0
    assert spy_e.n == dict(init=0, reduce=0, fused=6 * n_iter, plain=0)


def test_a_library_without_the_entry_points_takes_the_launch_sequence_of_before(torch_cuda, monkeypatch):
    from gabor_color_image_segmentation_amd import _lib
    monkeypatch.setattr(_lib, "SIGNATURES", {k: v for k, v in _lib.SIGNATURES.items() if k not in FUSED_SYMBOLS})
    h, w = 81, 121
    imgs = _synth(3, h, w, seed=9)
    seg, spy = _segmenter(n_iter=4)
    assert not seg.ops.has_fused
    for mode in ("per_image", "global"):
        assert np.array_equal(_device_labels(torch_cuda, seg, imgs, mode), _oracle(seg, imgs, mode)), mode
        assert np.array_equal(seg.segment_batch(imgs[:1], mode=mode), _oracle(seg, imgs[:1], mode)), mode
    assert all(ws["fold"] is None for ws in seg._ws.values())
    assert spy.n["fused"] == 0 and spy.n["init"] > 0 and spy.n["reduce"] > 0 and spy.n["plain"] > 0


def test_banks_without_a_self_updating_pass_keep_their_launches(torch_cuda):
    """k > 8 and the deep bank have no such pass (gcs_kmeans_fused_workspace_bytes == 0): the loop falls back, results unchanged."""
    imgs = _synth(2, 64, 96, seed=3)
    for kw in (dict(k=12, n_iter=3), dict(n_scales=8, n_orient=8, n_iter=3)):
        seg, spy = _segmenter(**kw)
        assert np.array_equal(_device_labels(torch_cuda, seg, imgs, "global"), _oracle(seg, imgs, "global")), kw
        assert spy.n["fused"] == 0 and spy.n["init"] == 1 and spy.n["reduce"] == 2, (kw, spy.n)
