"""The buffer contract of include/gcs.h, entry point by entry point, on the raw C calls (``_lib.load()`` and ``data_ptr()``s, no
HipOps): every device output and workspace is an arena view (tests/arena.py) of EXACTLY the size the header or its ``*_bytes()``
function gives, with a canary band of 4096 bytes on either side; every input is an arena view of its exact size too. Each call
runs twice, on outputs and workspaces filled with 0x00 and with 0xA5, and each time

  (a) every output ``==`` the existing reference (C oracle features, tests/lloyd_ref.py, tests/smooth_ref.py, ...),
  (b) no canary byte is damaged (``arena.check``),
  (c) no input has changed (``arena.unchanged``),
  (d) the outputs of the two runs are identical.

A buffer whose entry contents the header prescribes gets them (the zeroed workspace of gcs_kmeans_pass_fused, the previous
centroids of the two finalize calls, the slab under the in-place stages); a buffer the header describes as partly kept is compared
with its bytes from before. No buffer is ever smaller than the header asks: the tests probe the contract, they provoke nothing.

CONTRACT (below) names, for every symbol of ``_lib.SIGNATURES`` and ``_lib.EXTENSIONS``, the case that holds it here, the file that already holds it behind
bands, or that it is a host-only function; a CPU test keeps the table complete."""
import inspect
import os
import re

import numpy as np
import pytest

import arena as ar
from arena import Arena, ptr

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# ---- the table (step 4 of the issue): symbol -> the test of this file that holds its buffers
CONTRACT = {
    "gcs_gabor_features": "test_gabor_unpack_gather_gradient_tree",
    "gcs_features_unpack": "test_gabor_unpack_gather_gradient_tree",
    "gcs_features_gather": "test_gabor_unpack_gather_gradient_tree",
    "gcs_feature_gradient": "test_gabor_unpack_gather_gradient_tree",
    "gcs_region_tree_slab": "test_gabor_unpack_gather_gradient_tree",
    "gcs_smooth_features": "test_smoothing_in_place",
    "gcs_kmeans_init": "test_lloyd_entries",
    "gcs_kmeans_assign_accumulate": "test_lloyd_entries",
    "gcs_kmeans_assign_raster": "test_lloyd_entries",
    "gcs_kmeans_reduce": "test_lloyd_entries",
    "gcs_kmeans_finalize": "test_lloyd_entries",
    "gcs_kmeans_reduce_finalize": "test_lloyd_entries",
    "gcs_kmeans_pass_fused": "test_lloyd_entries",
    "gcs_labels_widen": "test_lloyd_entries",
    "gcs_connected_regions": "test_connected_and_merged_regions",
    "gcs_merge_small_regions": "test_connected_and_merged_regions",
    "gcs_region_tree": "test_region_tree_cut_contours_sweep",
    "gcs_region_tree_cut": "test_region_tree_cut_contours_sweep",
    "gcs_region_tree_contours": "test_region_tree_cut_contours_sweep",
    "gcs_boundary_sweep_resident": "test_region_tree_cut_contours_sweep",
    "gcs_texton_gradient": "test_texton_gradient",
    "gcs_boundary_counts": "test_scoring_entries",
    "gcs_boundary_counts_batch": "test_scoring_entries",
    "gcs_truth_prepare": "test_scoring_entries",
    "gcs_boundary_counts_resident": "test_scoring_entries",
    "gcs_region_counts": "test_scoring_entries",
    "gcs_region_counts_batch": "test_scoring_entries",
    "gcs_region_counts_batch_u8": "test_scoring_entries",
    "gcs_region_reduce": "test_scoring_entries",
    "gcs_score_batch_resident": "test_scoring_entries",
    "gcs_region_agreement": "test_scoring_entries",
    "gcs_download": "test_download_into_pinned_memory",
    "gcs_selftest_isqrt": "test_isqrt_counter",
}
# entry points whose band test lives in another file
ELSEWHERE = {
    "gcs_region_nodes": "test_gpu_region_nodes.py",
    "gcs_colour_opponent": "test_gpu_colour_features.py",
    "gcs_position_features": "test_gpu_position_features.py",
    "gcs_superpixel_segment": "superpixel_raw.py",
    "gcs_region_sweep": "test_gpu_region_sweep.py",
    "gcs_region_sweep_under": "test_gpu_cut_metrics.py",
    "gcs_cut_shapes": "test_gpu_cut_metrics.py",
    "gcs_region_props": "test_gpu_region_props.py",
    "gcs_region_props_cuts": "test_gpu_region_props.py",
    "gcs_region_paint": "test_gpu_region_props.py",
    "gcs_region_adjacency": "test_gpu_region_adjacency.py",
    "gcs_region_adjacency_cuts": "test_gpu_region_adjacency.py",
    "gcs_region_tree_edges": "test_gpu_region_tree_edges.py",
    "gcs_label_used": "test_gpu_region_tree_edges.py",
    "gcs_cue_gradient": "test_gpu_cue_gradient.py",
}
# functions that take no device pointer
HOST_ONLY = {
    "gcs_abi_version", "gcs_last_error", "gcs_device_cu_count", "gcs_bank_packed_bytes", "gcs_bank_bias_count", "gcs_bank_pack",
    "gcs_feature_slab_bytes", "gcs_feature_pass_bytes", "gcs_label_slab_bytes", "gcs_kmeans_parts_per_image",
    "gcs_kmeans_partial_bytes", "gcs_gabor_workspace_bytes", "gcs_kmeans_fused_workspace_bytes", "gcs_selftest_native_parts",
    "gcs_selftest_pass_kernel", "gcs_selftest_pass_nt_limit", "gcs_selftest_gabor_plan", "gcs_boundary_scratch_bytes",
    "gcs_boundary_batch_scratch_bytes", "gcs_bit_planes_bytes", "gcs_region_agreement_scratch_bytes", "gcs_connected_scratch_bytes",
    "gcs_merge_scratch_bytes", "gcs_region_nodes_scratch_bytes", "gcs_smooth_workspace_bytes", "gcs_superpixel_grid",
    "gcs_superpixel_workspace_bytes", "gcs_region_tree_workspace_bytes", "gcs_region_tree_contours_workspace_bytes",
    "gcs_region_sweep_workspace_bytes", "gcs_region_sweep_under_workspace_bytes", "gcs_cut_shapes_workspace_bytes",
    "gcs_region_adjacency_workspace_bytes", "gcs_region_tree_edges_workspace_bytes", "gcs_texton_masks",
}


def _source_with_helpers(fn, seen=None):
    """The source of a function of this file and, transitively, of the module-level helpers (functions, classes) it names."""
    seen = set() if seen is None else seen
    seen.add(fn.__name__)
    text = inspect.getsource(fn)
    for name in sorted(set(re.findall(r"\b(_[A-Za-z]\w*)\(", text)) - seen):
        obj = globals().get(name)
        if (inspect.isfunction(obj) or inspect.isclass(obj)) and getattr(obj, "__module__", None) == __name__ and name not in seen:
            text += _source_with_helpers(obj, seen)
    return text


def test_every_entry_point_has_a_home():
    """CPU: the three sets partition ``_lib.SIGNATURES`` and ``_lib.EXTENSIONS`` together; every case named is a test of this file that mentions the symbol; every
    other file named exists, mentions the symbol and poisons or guards its buffers (or holds them in an arena). A new entry point fails here until its contract has a home."""
    from gabor_color_image_segmentation_amd import _lib
    sets = (set(CONTRACT), set(ELSEWHERE), HOST_ONLY)
    assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])
    assert not set(_lib.SIGNATURES) & set(_lib.EXTENSIONS)
    symbols = set(_lib.SIGNATURES) | set(_lib.EXTENSIONS)
    assert "gcs_cue_gradient" in symbols
    missing, extra = symbols - set.union(*sets), set.union(*sets) - symbols
    assert not missing and not extra, (sorted(missing), sorted(extra))
    for sym, case in CONTRACT.items():
        assert case.startswith("test_") and callable(globals().get(case)), (sym, case)
        text = _source_with_helpers(globals()[case])
        assert re.search(r"lib\.%s\b" % sym, text), (sym, case, "neither the case nor a helper it calls makes this call")
    for sym, name in ELSEWHERE.items():
        path = os.path.join(HERE, name)
        assert os.path.isfile(path), (sym, name)
        text = open(path).read()
        # (poisoned or guarded buffers, or views of tests/arena.py between its canary bands, as in this file)
        assert sym in text and ("0xAB" in text or "guard" in text.lower() or ("Arena(" in text and ".check()" in text)), (sym, name)


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _lib():
    from gabor_color_image_segmentation_amd import _lib as L
    return L.load()


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == 0, (what, _lib().gcs_last_error())


def _twice(torch, body, capacity=8 << 20):
    """``body(arena, poison) -> {name: array}`` on a fresh arena per poison byte: (b), (c) and (d); (a) is the body's."""
    runs = []
    for poison in ar.POISONS:
        a = Arena(torch, "cuda", capacity)
        out = body(a, poison)
        torch.cuda.synchronize()
        a.check()
        a.unchanged()
        runs.append(out)
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), (key, "differs between outputs that held 0x00 and 0xA5 on entry")
    return runs


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _all(view_bytes, byte, what):
    bad = np.flatnonzero(view_bytes != byte)
    assert bad.size == 0, (what, "written: first at", int(bad[0]), len(bad))


@gpu
def test_the_arena_sees_device_writes(torch_cuda):
    """One byte past a view, through a plain torch fill of a view that is one byte longer (no library kernel; inside the arena)."""
    a = Arena(torch_cuda, "cuda", 1 << 16)
    a.take(100, name="u")
    v = a.take(1001, fill=0xA5, name="v")
    start = v.data_ptr() - a.base
    a.check()
    a.buf[start:start + 1002].fill_(0x11)
    with pytest.raises(AssertionError, match=r"^v \(1001 bytes\): the band behind it was written, first at \+0 \(1 bytes"):
        a.check()
    a.buf[start + 1001:start + 1002].fill_(ar.CANARY)
    a.buf[start - 1:start + 5].fill_(0x11)
    with pytest.raises(AssertionError, match=r"^v \(1001 bytes\): the band in front of it was written, first at -1 \(1 bytes"):
        a.check()


# ------------------------------------------------------------------------------------------------------------ slab stages
# name -> (n_scales, n_orient, ksize, shift): one hot bank (tests/hot_banks.py: values of 4096 and more, so that the TOP runs and the
# flag words of the split slab are written) per slab format and depth, and D = 210 for the generic pass
BANKS = {"split2": (4, 6, 13, 8), "split1": (2, 6, 13, 7), "wide2": (4, 7, 13, 7), "three": (6, 4, 13, 7), "four": (8, 8, 13, 8),
         "generic": (7, 10, 13, 7)}
SLAB_SHAPES = [(8, 8), (9, 10), (13, 11), (33, 41)]
B = 3
_PACKED, _STAGES = {}, {}


def _packed(cfg):
    if cfg not in _PACKED:
        import hot_banks as hb
        lib = _lib()
        ns, no, ks, _ = cfg
        tapq = np.ascontiguousarray(hb.hot_bank(*cfg).tapq, np.int16)
        packed = np.zeros(lib.gcs_bank_packed_bytes(ns, no), np.int8)
        bias = np.zeros(lib.gcs_bank_bias_count(ns, no), np.int32)
        _ok(lib.gcs_bank_pack(tapq.ctypes.data, ns, no, ks, packed.ctypes.data, bias.ctypes.data), "gcs_bank_pack")
        _PACKED[cfg] = (packed, bias)
    return _PACKED[cfg]


def _gabor(a, poison, cfg, imgs):
    """gcs_gabor_features into a poisoned slab through a poisoned workspace -> the slab view."""
    lib = _lib()
    ns, no, ks, shift = cfg
    b, h, w = imgs.shape[:3]
    packed, bias = _packed(cfg)
    img_d, pk, bi = a.put(imgs, name="images"), a.put(packed, name="packed bank"), a.put(bias, name="bias")
    need = lib.gcs_gabor_workspace_bytes(b, h, w, ns)
    per = lib.gcs_feature_slab_bytes(1, h, w, ns, no)
    assert need > 0 and per > 0 and lib.gcs_feature_slab_bytes(b, h, w, ns, no) == b * per
    ws = a.take(need, fill=poison, name="gabor workspace")
    slab = a.take(b * per, fill=poison, name="feature slab")
    _ok(lib.gcs_gabor_features(img_d.data_ptr(), b, h, w, pk.data_ptr(), bi.data_ptr(), ns, no, ks, shift, ws.data_ptr(),
                               slab.data_ptr(), _st()), "gcs_gabor_features")
    return slab


def _unpack(a, poison, cfg, slab, b, h, w, name="canonical features"):
    lib = _lib()
    ns, no = cfg[:2]
    d = 3 * ns * no
    out = a.take(b * d * h * w * 2, fill=poison, name=name)
    _ok(lib.gcs_features_unpack(slab.data_ptr(), b, h, w, ns, no, out.data_ptr(), _st()), "gcs_features_unpack")
    return out


class _Stage:
    """One (bank, shape): the images, the C oracle's features, and the slab bytes gcs_gabor_features wrote over either poison -
    made by the contract run of gcs_gabor_features and gcs_features_unpack itself."""

    def __init__(self, torch, bank, shape):
        import hot_banks as hb
        from fused_stages import ref_features
        self.cfg = cfg = BANKS[bank]
        self.ns, self.no = cfg[:2]
        self.b, (self.h, self.w) = B, shape
        self.d = 3 * self.ns * self.no
        self.imgs = hb.hot_images(B, shape[0], shape[1], seed=shape[0] * shape[1])
        self.ref = ref_features(cfg, self.imgs)                                             # (B, D, H, W) uint16
        self.x = self.ref.reshape(B, self.d, -1).transpose(0, 2, 1).astype(np.int64)      # (B, P, D)
        self.slab = {}

        def body(a, poison):
            slab = _gabor(a, poison, cfg, self.imgs)
            canon = _unpack(a, poison, cfg, slab, B, self.h, self.w)
            self.slab[poison] = a.read(slab)
            got = a.read(canon, np.uint16, self.ref.shape)
            _eq(got, self.ref, (bank, shape, "gcs_gabor_features -> gcs_features_unpack", hex(poison)))
            return {"canonical": got}
        _twice(torch, body)
        self.kept = self.slab[0x00] != self.slab[0xA5]      # slab bytes the Gabor stage does not write (slots without a pixel)
        if shape == (8, 8):                                  # one 8 x 8 block of a tile of four: the other three hold no pixel
            assert 2 * int(self.kept.sum()) > self.kept.size, (bank, int(self.kept.sum()), self.kept.size)
        self._cent = {}

    def cent(self, k, n_sets):
        from oracle import spec_oracle as so
        if (k, n_sets) not in self._cent:
            self._cent[k, n_sets] = np.stack([so.kmeans_init(self.x[i], k) for i in range(n_sets)]).astype(np.int64)
        return self._cent[k, n_sets]


def _stage(torch, bank, shape):
    if (bank, shape) not in _STAGES:
        _STAGES[bank, shape] = _Stage(torch, bank, shape)
    return _STAGES[bank, shape]


def _label_maps(shape, k, seed, b=B):
    """(b, H, W) int32: blocks of 3 x 3 with a tenth of the pixels redrawn; values from -1 .. k (both ends outside 0 .. k-1), at most
    40 different ones, 0 and k - 1 among them."""
    rng = np.random.default_rng(seed)
    h, w = shape
    vals = np.unique(np.concatenate([[-1, 0, k - 1, k], rng.integers(0, k, 36)])).astype(np.int32)
    coarse = vals[rng.integers(0, len(vals), (b, -(-h // 3), -(-w // 3)))]
    lab = coarse.repeat(3, axis=1).repeat(3, axis=2)[:, :h, :w].copy()
    noise = rng.random(lab.shape) < 0.1
    lab[noise] = vals[rng.integers(0, len(vals), int(noise.sum()))]
    lab[:, 0, 0], lab[:, h - 1, w - 1] = 0, k - 1
    return np.ascontiguousarray(lab, np.int32)


@gpu
@pytest.mark.parametrize("shape", SLAB_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bank", list(BANKS))
def test_gabor_unpack_gather_gradient_tree(torch_cuda, bank, shape):
    """gcs_gabor_features (slab and workspace) and gcs_features_unpack == the C oracle (in ``_Stage``); on the slab as an exact-size
    input: gcs_features_gather, gcs_feature_gradient == tests/feature_gradient_ref.py and gcs_region_tree_slab ==
    tests/region_tree_ref.py on the oracle's features (both for D <= 207)."""
    import feature_gradient_ref as fg
    import region_tree_ref as rt
    torch, lib = torch_cuda, _lib()
    s = _stage(torch, bank, shape)
    b, h, w, ns, no, d = s.b, s.h, s.w, s.ns, s.no, s.d
    rng = np.random.default_rng(h * w)
    n = 37
    byx = np.stack([rng.integers(-1, b, n), rng.integers(0, h, n), rng.integers(0, w, n)], 1).astype(np.int32)
    byx[:4] = [(0, 0, 0), (b - 1, h - 1, w - 1), (-1, 0, 0), (1, h - 1, 0)]
    want_rows = np.where(byx[:, :1] >= 0, s.ref[np.maximum(byx[:, 0], 0), :, byx[:, 1], byx[:, 2]], 0)
    K = 33
    lab = _label_maps(shape, K, seed=h + w)
    if d <= 207:
        want_grad = np.stack([fg.gradient(s.ref[i], ns, no) for i in range(b)])
        trees = [rt.build_tree(s.ref[i], lab[i], K) for i in range(b)]

    def body(a, poison):
        slab = a.put(s.slab[poison], name="feature slab")
        triples = a.put(byx, name="byx")
        rows = a.take(n * d * 2, fill=poison, name="gathered rows")
        _ok(lib.gcs_features_gather(slab.data_ptr(), b, h, w, ns, no, n, triples.data_ptr(), rows.data_ptr(), _st()), "gather")
        out = {"rows": a.read(rows, np.uint16, (n, d))}
        _eq(out["rows"], want_rows, (bank, shape, "gcs_features_gather"))
        if d > 207:
            return out
        grad = a.take(b * h * w * 4, fill=poison, name="gradient map")
        _ok(lib.gcs_feature_gradient(slab.data_ptr(), b, h, w, ns, no, grad.data_ptr(), _st()), "gcs_feature_gradient")
        labels = a.put(lab, name="labels")
        need = lib.gcs_region_tree_workspace_bytes(b, h, w, d, K)
        assert need > 0
        ws = a.take(need, fill=poison, name="tree workspace")
        merges = a.take(b * (K - 1) * 8, fill=poison, name="merges")
        costs = a.take(b * (K - 1) * 8, fill=poison, name="costs")
        alive = a.take(b * 4, fill=poison, name="alive")
        _ok(lib.gcs_region_tree_slab(slab.data_ptr(), labels.data_ptr(), b, h, w, ns, no, K, ws.data_ptr(), merges.data_ptr(),
                                     costs.data_ptr(), alive.data_ptr(), _st()), "gcs_region_tree_slab")
        out.update(grad=a.read(grad, np.int32, (b, h, w)), merges=a.read(merges, np.int32, (b, K - 1, 2)),
                   costs=a.read(costs, np.uint64, (b, K - 1)), alive=a.read(alive, np.int32, (b,)))
        _eq(out["grad"], want_grad, (bank, shape, "gcs_feature_gradient"))
        for i, (wm, wc, wa) in enumerate(trees):
            assert int(out["alive"][i]) == wa, (bank, shape, i)
            _eq(out["merges"][i], wm, (bank, shape, i, "merges"))
            _eq(out["costs"][i], wc, (bank, shape, i, "costs"))
        return out
    _twice(torch, body)


@gpu
@pytest.mark.parametrize("shape", SLAB_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bank", list(BANKS))
def test_smoothing_in_place(torch_cuda, bank, shape):
    """gcs_smooth_features on the slab in place through a poisoned workspace == tests/smooth_ref.py (through gcs_features_unpack);
    the slab bytes the Gabor stage does not write (slots that hold no pixel: they still hold the poison) keep their bytes."""
    import smooth_ref as sr
    torch, lib = torch_cuda, _lib()
    s = _stage(torch, bank, shape)
    b, h, w, ns, no = s.b, s.h, s.w, s.ns, s.no
    taps, radius = sr.taps_array(1.0, ns)
    want = np.stack([sr.smooth_features(s.ref[i], 1.0, ns, no) for i in range(b)])
    assert not np.array_equal(want, s.ref)

    def body(a, poison):
        before = s.slab[poison]
        slab = a.take(before.size, fill=before, name="feature slab (in place)")
        t, r = a.put(taps, name="taps"), a.put(radius, name="radius")
        need = lib.gcs_smooth_workspace_bytes(b, h, w, ns, no)
        assert need > 0
        ws = a.take(need, fill=poison, name="smoothing workspace")
        _ok(lib.gcs_smooth_features(slab.data_ptr(), b, h, w, ns, no, t.data_ptr(), r.data_ptr(), ws.data_ptr(), _st()), "smooth")
        canon = _unpack(a, poison, s.cfg, slab, b, h, w)
        got = a.read(canon, np.uint16, s.ref.shape)
        _eq(got, want, (bank, shape, "gcs_smooth_features", hex(poison)))
        after = a.read(slab)
        _eq(after[s.kept], before[s.kept], (bank, shape, "slab bytes that hold no pixel"))
        return {"canonical": got}
    _twice(torch, body)


# ------------------------------------------------------------------------------------------------------------ Lloyd passes
def _fused_loop(a, poison, s, slab, k, n_sets, out_u8, ws, n_iter):
    """A complete loop of ``n_iter`` gcs_kmeans_pass_fused calls on the workspace ``ws`` -> (centroid views of every pass, label view)."""
    lib = _lib()
    b, h, w, ns, no, d = s.b, s.h, s.w, s.ns, s.no, s.d
    cents, out = [], None
    for t in range(n_iter):
        last = t == n_iter - 1
        c = a.take(n_sets * k * d * 2, fill=poison, name="centroids of fused pass %d" % t)
        if last:
            out = a.take(b * h * w * (1 if out_u8 else 4), fill=poison, name="label map of the fused loop")
        _ok(lib.gcs_kmeans_pass_fused(slab.data_ptr(), b, h, w, ns, no, k, n_sets, t & 1, t, 1 if last else 0, ws.data_ptr(),
                                      c.data_ptr(), ptr(out), 1 if out_u8 else 0, _st()), "gcs_kmeans_pass_fused")
        cents.append(c)
    return cents, out


def _lloyd_body(s, k, n_sets, reverse, tag):
    """Every Lloyd entry point on the stage's slab for one (k, n_sets, sweep direction); the references are computed once."""
    import fused_workspace as fw
    from lloyd_ref import _pass_reference, updated
    lib = _lib()
    b, h, w, ns, no, d = s.b, s.h, s.w, s.ns, s.no, s.d
    p = h * w
    lo, hi = 1, h - 2                                                   # a row window that is not the whole image
    cent_np = s.cent(k, n_sets)                                         # the SPEC.md §4 init pixels
    book = cent_np.copy()                                               # the codebook of the passes: for k = 16 with rows 0 and 1
    if k == 16:                                                         # identical - the lowest index wins every tie, so cluster 1
        book[:, 1] = book[:, 0]                                         # is empty in every set and keeps its centroid in the update
    vote = np.zeros((b, h, w), bool)
    vote[:, lo:hi] = True
    want_lab, want_sums, want_cnt = _pass_reference(s.x, book, vote.reshape(b, -1))
    assert k != 16 or ((want_cnt[:, 1] == 0).all() and not (want_lab == 1).any()), tag
    want_table = np.concatenate([want_sums, want_cnt[..., None]], axis=2)
    want_new = updated(want_sums, want_cnt, book)
    assert k != 16 or np.array_equal(want_new[:, 1], book[:, 1])
    pbytes = lib.gcs_kmeans_partial_bytes(b, h, w, d, k)
    fbytes = lib.gcs_kmeans_fused_workspace_bytes(b, h, w, ns, no, k, n_sets)
    assert pbytes > 0
    if fbytes:                                                          # the loop of three self-updating passes, restated
        whole = np.ones((b, p), bool)
        loop_cent, loop_lab, c = [], [], cent_np
        for t in range(3):
            loop_cent.append(c)
            lab_t, sm, cn = _pass_reference(s.x, c, whole)
            loop_lab.append(lab_t)
            c = updated(sm, cn, c)
        parts = int(lib.gcs_kmeans_parts_per_image(b, h, w))
        lay = (n_sets, fw.fold_rows(b, parts, n_sets, fw.env_fold_rows()), k, d)
        assert fw.workspace_bytes(*lay) == fbytes

    def body(a, poison):
        st = _st()
        slab = a.put(s.slab[poison], name="feature slab")
        init = a.take(n_sets * k * d * 2, fill=poison, name="init centroids")
        _ok(lib.gcs_kmeans_init(slab.data_ptr(), b, h, w, ns, no, k, n_sets, init.data_ptr(), st), "gcs_kmeans_init")
        cent = a.put(book.astype(np.uint16), name="centroids")

        def assign(labels, partials):
            _ok(lib.gcs_kmeans_assign_accumulate(slab.data_ptr(), cent.data_ptr(), b, h, w, ns, no, k, n_sets, lo, hi, reverse,
                                                 ptr(labels), ptr(partials), st), "gcs_kmeans_assign_accumulate")
        lab2, par2 = a.take(b * p, fill=poison, name="labels (both outputs)"), a.take(pbytes, fill=poison, name="partials (both)")
        assign(lab2, par2)
        lab1 = a.take(b * p, fill=poison, name="labels (alone)")
        assign(lab1, None)
        par1 = a.take(pbytes, fill=poison, name="partials (alone)")
        assign(None, par1)
        sums = {}
        for name, par in (("both", par2), ("alone", par1)):
            sums[name] = a.take(n_sets * k * (d + 1) * 8, fill=poison, name="sums of partials (%s)" % name)
            _ok(lib.gcs_kmeans_reduce(par.data_ptr(), b, h, w, d, k, n_sets, sums[name].data_ptr(), st), "gcs_kmeans_reduce")
        old = book.astype(np.uint16)
        new_f = a.take(old.nbytes, fill=old, name="centroids (finalize, in place)")
        _ok(lib.gcs_kmeans_finalize(sums["both"].data_ptr(), n_sets, k, d, new_f.data_ptr(), st), "gcs_kmeans_finalize")
        new_rf, sums_rf = a.take(old.nbytes, fill=old, name="centroids (reduce_finalize)"), a.take(n_sets * k * (d + 1) * 8,
                                                                                                 fill=poison, name="sums (rf)")
        _ok(lib.gcs_kmeans_reduce_finalize(par2.data_ptr(), b, h, w, d, k, n_sets, sums_rf.data_ptr(), new_rf.data_ptr(), st), "rf")
        new_rf0 = a.take(old.nbytes, fill=old, name="centroids (reduce_finalize, no sums)")
        _ok(lib.gcs_kmeans_reduce_finalize(par1.data_ptr(), b, h, w, d, k, n_sets, None, new_rf0.data_ptr(), st), "rf, sums NULL")
        rast, scratch = {}, {}
        for u8 in (0, 1):
            rast[u8] = a.take(b * p * (1 if u8 else 4), fill=poison, name="raster map (%s)" % ("uint8" if u8 else "int32"))
            scratch[u8] = a.take(lib.gcs_label_slab_bytes(b, h, w), fill=poison, name="scratch labels (%d)" % u8)
            _ok(lib.gcs_kmeans_assign_raster(slab.data_ptr(), cent.data_ptr(), b, h, w, ns, no, k, n_sets, reverse,
                                             rast[u8].data_ptr(), u8, scratch[u8].data_ptr(), st), "gcs_kmeans_assign_raster")
        rast_ns = a.take(b * p, fill=poison, name="raster map (uint8, no scratch)")
        _ok(lib.gcs_kmeans_assign_raster(slab.data_ptr(), cent.data_ptr(), b, h, w, ns, no, k, n_sets, reverse, rast_ns.data_ptr(),
                                         1, None, st), "gcs_kmeans_assign_raster(scratch NULL)")
        narrow = a.put(want_lab.astype(np.uint8), align=4, name="uint8 labels (widen)")
        wide = a.take(b * p * 4, align=4, fill=poison, name="widened labels")
        _ok(lib.gcs_labels_widen(narrow.data_ptr(), b, h, w, wide.data_ptr(), st), "gcs_labels_widen")
        out = {"init": a.read(init, np.uint16, cent_np.shape), "labels both": a.read(lab2), "labels alone": a.read(lab1),
               "sums both": a.read(sums["both"], np.int64, want_table.shape), "sums alone": a.read(sums["alone"], np.int64, want_table.shape),
               "sums rf": a.read(sums_rf, np.int64, want_table.shape), "new f": a.read(new_f, np.uint16, cent_np.shape),
               "new rf": a.read(new_rf, np.uint16, cent_np.shape), "new rf0": a.read(new_rf0, np.uint16, cent_np.shape),
               "raster i32": a.read(rast[0], np.int32), "raster u8": a.read(rast[1]), "raster u8 ns": a.read(rast_ns),
               "wide": a.read(wide, np.int32)}
        _eq(out["init"], cent_np, (tag, "gcs_kmeans_init"))
        for name in ("labels both", "labels alone", "raster i32", "raster u8", "raster u8 ns", "wide"):
            _eq(out[name].reshape(b, p), want_lab, (tag, name))
        for name in ("sums both", "sums alone", "sums rf"):
            _eq(out[name], want_table, (tag, name))
        for name in ("new f", "new rf", "new rf0"):
            _eq(out[name], want_new, (tag, name))
        for u8 in (0, 1):
            raw = a.read(scratch[u8])
            if d >= 208 and not u8:                                     # the generic pass: needed, and then also filled
                _eq(raw[:b * p].reshape(b, p), want_lab, (tag, "scratch labels of the generic pass"))
            else:
                _all(raw, poison, (tag, "scratch_labels_dev (never written here)", u8))
        if fbytes:
            ws = a.take(fbytes, fill=np.zeros(fbytes, np.uint8), name="fused workspace (zeroed by the caller)")
            for u8, n_iter in ((0, 3), (1, 2), (0, 3)):                 # complete loops of either length, one behind the other
                cents, lab = _fused_loop(a, poison, s, slab, k, n_sets, u8, ws, n_iter)
                for t, c in enumerate(cents):
                    out["fused cent %d %d" % (n_iter, t)] = a.read(c, np.uint16, cent_np.shape)
                    _eq(out["fused cent %d %d" % (n_iter, t)], loop_cent[t], (tag, "centroids of fused pass", t, n_iter))
                out["fused labels %d" % n_iter] = a.read(lab, np.uint8 if u8 else np.int32)
                _eq(out["fused labels %d" % n_iter].reshape(b, p), loop_lab[n_iter - 1], (tag, "labels of the fused loop", n_iter))
                # every byte of the workspace after a complete loop: what the caller zeroed is zero again - the sum buffers, the
                # ticket and all padding -, and the two centroid arrays (which no pass 0 reads) hold the loop's last two codebooks
                want_ws = np.zeros(fbytes, np.uint8)
                v = fw.views(want_ws, *lay)
                for t in (n_iter - 2, n_iter - 1):
                    v.cents[t & 1][...] = loop_cent[t].astype(np.uint16)
                _eq(a.read(ws), want_ws, (tag, "the fused workspace after a complete loop", n_iter))
        return out
    return body, 4 * pbytes + (16 << 20)


@gpu
@pytest.mark.parametrize("shape", SLAB_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bank", list(BANKS))
def test_lloyd_entries(torch_cuda, bank, shape):
    """gcs_kmeans_init, gcs_kmeans_assign_accumulate (both outputs, either alone; rows 1 .. H-3 vote), gcs_kmeans_reduce of either
    partial buffer, gcs_kmeans_finalize, gcs_kmeans_reduce_finalize (with and without sums), gcs_kmeans_assign_raster (int32 and uint8;
    scratch_labels_dev given and NULL), gcs_labels_widen and, where the bank has one, complete loops of gcs_kmeans_pass_fused ==
    tests/lloyd_ref.py on the oracle's features: k = 3 and 16, one and B codebooks, both sweep directions. The uint8 maps are
    B H W bytes exactly (3 * 13 * 11 = 429 and 3 * 9 * 10 = 270: an end that is no multiple of 4)."""
    torch = torch_cuda
    s = _stage(torch, bank, shape)
    fused = 0
    for k in (3, 16):
        for n_sets in (1, B):
            for reverse in (0, 1):
                body, capacity = _lloyd_body(s, k, n_sets, reverse, (bank, shape, k, n_sets, reverse))
                runs = _twice(torch, body, capacity)
                fused += any(key.startswith("fused") for key in runs[0])
    assert fused == (4 if bank in ("split2", "split1") else 0), fused   # the split-slab banks have the self-updating pass at k = 3


# ------------------------------------------------------------------------------------------------------------ sub-batch slabs
@gpu
@pytest.mark.parametrize("bank", ["split2", "wide2", "three"])
def test_a_sub_batch_of_a_slab(torch_cuda, bank):
    """A slab of four 13 x 11 images; every entry point that takes a slab pointer, called on ``slab + per_image`` with B = 2, gives
    what the call on the whole slab gives for images 1 and 2, and the in-place stages leave images 0 and 3 untouched."""
    import hot_banks as hb
    import smooth_ref as sr
    torch, lib = torch_cuda, _lib()
    cfg = BANKS[bank]
    ns, no = cfg[:2]
    d = 3 * ns * no
    h, w, k, K = 13, 11, 3, 33
    imgs = hb.hot_images(4, h, w, seed=4)
    per = lib.gcs_feature_slab_bytes(1, h, w, ns, no)
    taps, radius = sr.taps_array(1.0, ns)
    lab = _label_maps((h, w), K, seed=8, b=4)
    rng = np.random.default_rng(2)
    byx = np.stack([rng.integers(0, 2, 19), rng.integers(0, h, 19), rng.integers(0, w, 19)], 1).astype(np.int32)
    fbytes = {nb: lib.gcs_kmeans_fused_workspace_bytes(nb, h, w, ns, no, k, nb) for nb in (2, 4)}
    assert all(bool(v) == (bank == "split2") for v in fbytes.values()), fbytes    # the split slab has the self-updating pass at k = 3

    def calls(a, poison, slab_ptr, nb, first):
        """Every read-only slab entry on ``nb`` images from ``slab_ptr`` (``first`` = the batch's first image) -> arrays."""
        st = _st()
        p = h * w
        out = {}
        canon = a.take(nb * d * p * 2, fill=poison, name="canonical")
        _ok(lib.gcs_features_unpack(slab_ptr, nb, h, w, ns, no, canon.data_ptr(), st), "gcs_features_unpack")
        out["canonical"] = a.read(canon, np.uint16, (nb, d, h, w))
        triples = a.put(byx + np.array([0 if nb == 2 else 1, 0, 0], np.int32), name="byx")
        rows = a.take(len(byx) * d * 2, fill=poison, name="rows")
        _ok(lib.gcs_features_gather(slab_ptr, nb, h, w, ns, no, len(byx), triples.data_ptr(), rows.data_ptr(), st), "gather")
        out["rows"] = a.read(rows, np.uint16, (len(byx), d))
        cent = a.take(nb * k * d * 2, fill=poison, name="init centroids")
        _ok(lib.gcs_kmeans_init(slab_ptr, nb, h, w, ns, no, k, nb, cent.data_ptr(), st), "gcs_kmeans_init")
        out["init"] = a.read(cent, np.uint16, (nb, k, d))
        labels = a.take(nb * p, fill=poison, name="labels")
        partials = a.take(lib.gcs_kmeans_partial_bytes(nb, h, w, d, k), fill=poison, name="partials")
        _ok(lib.gcs_kmeans_assign_accumulate(slab_ptr, cent.data_ptr(), nb, h, w, ns, no, k, nb, 0, h, 0, labels.data_ptr(),
                                             partials.data_ptr(), st), "gcs_kmeans_assign_accumulate")
        sums = a.take(nb * k * (d + 1) * 8, fill=poison, name="sums")
        _ok(lib.gcs_kmeans_reduce(partials.data_ptr(), nb, h, w, d, k, nb, sums.data_ptr(), st), "gcs_kmeans_reduce")
        out["labels"], out["sums"] = a.read(labels).reshape(nb, p), a.read(sums, np.int64, (nb, k, d + 1))
        rast = a.take(nb * p * 4, fill=poison, name="raster map")
        _ok(lib.gcs_kmeans_assign_raster(slab_ptr, cent.data_ptr(), nb, h, w, ns, no, k, nb, 1, rast.data_ptr(), 0, None, st), "raster")
        out["raster"] = a.read(rast, np.int32, (nb, p))
        if fbytes[nb]:
            ws = a.take(fbytes[nb], fill=np.zeros(fbytes[nb], np.uint8), name="fused workspace")
            for t in range(2):
                c = a.take(nb * k * d * 2, fill=poison, name="fused centroids %d" % t)
                fl = a.take(nb * p * 4, fill=poison, name="fused labels") if t else None
                _ok(lib.gcs_kmeans_pass_fused(slab_ptr, nb, h, w, ns, no, k, nb, t, t, t, ws.data_ptr(), c.data_ptr(), ptr(fl), 0, st),
                    "gcs_kmeans_pass_fused")
                out["fused cent %d" % t] = a.read(c, np.uint16, (nb, k, d))
            out["fused labels"] = a.read(fl, np.int32, (nb, p))
        grad = a.take(nb * p * 4, fill=poison, name="gradient")
        _ok(lib.gcs_feature_gradient(slab_ptr, nb, h, w, ns, no, grad.data_ptr(), st), "gcs_feature_gradient")
        out["grad"] = a.read(grad, np.int32, (nb, h, w))
        maps = a.put(lab[first:first + nb], name="label maps")
        tws = a.take(lib.gcs_region_tree_workspace_bytes(nb, h, w, d, K), fill=poison, name="tree workspace")
        merges, costs = a.take(nb * (K - 1) * 8, fill=poison, name="merges"), a.take(nb * (K - 1) * 8, fill=poison, name="costs")
        alive = a.take(nb * 4, fill=poison, name="alive")
        _ok(lib.gcs_region_tree_slab(slab_ptr, maps.data_ptr(), nb, h, w, ns, no, K, tws.data_ptr(), merges.data_ptr(), costs.data_ptr(),
                                     alive.data_ptr(), st), "gcs_region_tree_slab")
        out.update(merges=a.read(merges, np.int32, (nb, K - 1, 2)), costs=a.read(costs, np.uint64, (nb, K - 1)),
                   alive=a.read(alive, np.int32, (nb,)))
        return out

    def in_place(a, poison, slab, off, nb):
        """gcs_smooth_features, then gcs_position_features, on ``nb`` images from byte ``off`` of the view ``slab``."""
        st = _st()
        t, r = a.put(taps, name="taps"), a.put(radius, name="radius")
        ws = a.take(lib.gcs_smooth_workspace_bytes(nb, h, w, ns, no), fill=poison, name="smoothing workspace")
        _ok(lib.gcs_smooth_features(slab.data_ptr() + off, nb, h, w, ns, no, t.data_ptr(), r.data_ptr(), ws.data_ptr(), st), "smooth")
        _ok(lib.gcs_position_features(slab.data_ptr() + off, nb, h, w, ns, no, 5, 0, st), "gcs_position_features")

    def body(a, poison):
        slab = _gabor(a, poison, cfg, imgs)
        before = a.read(slab).reshape(4, per)
        full = calls(a, poison, slab.data_ptr(), 4, 0)
        sub = calls(a, poison, slab.data_ptr() + per, 2, 1)
        for key in full:
            _eq(sub[key], full[key] if key == "rows" else full[key][1:3], (bank, key, "images 1 and 2 through a sub-batch pointer"))
        assert np.array_equal(a.read(slab).reshape(4, per), before), "a read-only slab entry wrote to the slab"
        whole = a.take(4 * per, fill=before, name="slab (in place, whole)")
        part = a.take(4 * per, fill=before, name="slab (in place, images 1 and 2)")
        in_place(a, poison, whole, 0, 4)
        in_place(a, poison, part, per, 2)
        got_w, got_p = a.read(whole).reshape(4, per), a.read(part).reshape(4, per)
        assert not np.array_equal(got_w, before)
        _eq(got_p[1:3], got_w[1:3], (bank, "images 1 and 2 of the in-place stages"))
        _eq(got_p[[0, 3]], before[[0, 3]], (bank, "images 0 and 3 under a sub-batch call"))
        return sub
    _twice(torch, body, 16 << 20)


# ------------------------------------------------------------------------------------------------------------ label-map kernels
MAP_SHAPES = [(1, 1), (1, 9), (13, 11), (37, 53)]


@gpu
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_connected_and_merged_regions(torch_cuda, shape):
    """gcs_connected_regions == spec_oracle.connected_regions, gcs_merge_small_regions == tests/merge_ref.py."""
    import merge_ref
    from oracle import spec_oracle as so
    torch, lib = torch_cuda, _lib()
    h, w = shape
    lab = _label_maps(shape, 7, seed=h * w)
    want_cc = np.stack([so.connected_regions(m) for m in lab])
    want_m = np.stack([merge_ref.merge_small_regions(m, 3) for m in lab])

    def body(a, poison):
        labels = a.put(lab, name="labels")
        sc = a.take(lib.gcs_connected_scratch_bytes(B, h, w), fill=poison, name="connected scratch")
        cc = a.take(B * h * w * 4, fill=poison, name="connected regions")
        _ok(lib.gcs_connected_regions(labels.data_ptr(), B, h, w, sc.data_ptr(), cc.data_ptr(), _st()), "gcs_connected_regions")
        need = lib.gcs_merge_scratch_bytes(B, h, w, 3)
        assert need > 0
        sm = a.take(need, fill=poison, name="merge scratch")
        mm = a.take(B * h * w * 4, fill=poison, name="merged regions")
        _ok(lib.gcs_merge_small_regions(labels.data_ptr(), B, h, w, 3, sm.data_ptr(), mm.data_ptr(), _st()), "gcs_merge_small_regions")
        out = {"cc": a.read(cc, np.int32, lab.shape), "merged": a.read(mm, np.int32, lab.shape)}
        _eq(out["cc"], want_cc, (shape, "gcs_connected_regions"))
        _eq(out["merged"], want_m, (shape, "gcs_merge_small_regions"))
        return out
    _twice(torch, body)


def _truths(shape, seed):
    """Ragged annotator maps (1, 3, 2 per image): truth uint16 [6][H][W], first [B + 1], img_of [6]."""
    rng = np.random.default_rng(seed)
    h, w = shape
    counts = (1, 3, 2)
    truth = np.stack([np.kron(rng.integers(1, 5, (-(-h // 4), -(-w // 4))), np.ones((4, 4), np.int64))[:h, :w] for _ in range(6)])
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return truth.astype(np.uint16), first, np.repeat(np.arange(B), counts).astype(np.int32)


def _truth_prepare(a, poison, truth, want8=True):
    """gcs_truth_prepare -> (planes, bd_counts, truth8) views."""
    lib = _lib()
    t, h, w = truth.shape
    src = a.put(truth, name="annotator maps")
    planes = a.take(lib.gcs_bit_planes_bytes(t, h, w), fill=poison, name="annotator bit planes")
    bd = a.take(t * 8, fill=poison, name="bd_counts")
    t8 = a.take(t * h * w, fill=poison, name="truth8") if want8 else None
    _ok(lib.gcs_truth_prepare(src.data_ptr(), t, h, w, planes.data_ptr(), bd.data_ptr(), ptr(t8), _st()), "gcs_truth_prepare")
    return src, planes, bd, t8


@gpu
@pytest.mark.parametrize("K", [1, 33, 4096])
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_region_tree_cut_contours_sweep(torch_cuda, shape, K):
    """gcs_region_tree (with and without costs) == region_tree_ref.build_tree; gcs_region_tree_cut out of place and in place ==
    region_tree_ref.cut; gcs_region_tree_contours == contour_map_ref.contour_map; gcs_boundary_sweep_resident on planes of
    gcs_truth_prepare == contour_map_ref.histograms. K = 1 (no rows), 33 (the tile accumulator's overflow form), 4096 (the most)."""
    import contour_map_ref as cm
    import region_tree_ref as rt
    torch, lib = torch_cuda, _lib()
    h, w = shape
    d, R = 5, 2
    lab = _label_maps(shape, K, seed=h * w + K)
    x = np.random.default_rng(K).integers(0, 46340, (B, d, h, w)).astype(np.uint16)
    truth, first, img_of = _truths(shape, seed=K + h)
    t = len(truth)
    trees = [rt.build_tree(x[i], lab[i], K) for i in range(B)]
    want_cut = np.stack([rt.cut(lab[i], trees[i][0], trees[i][2], R) for i in range(B)])
    want_u = np.stack([cm.contour_map(lab[i], trees[i][0], trees[i][2]) for i in range(B)])
    want_h = np.zeros((B + 2 * t, K + 1), np.uint32)
    for i in range(B):
        hm, rec, prec = cm.histograms(want_u[i], truth[first[i]:first[i + 1]], K)
        want_h[i] = hm
        want_h[B + 2 * first[i]:B + 2 * first[i + 1]:2], want_h[B + 2 * first[i] + 1:B + 2 * first[i + 1]:2] = rec, prec
    need = lib.gcs_region_tree_workspace_bytes(B, h, w, d, K)
    cneed = lib.gcs_region_tree_contours_workspace_bytes(B, K)
    assert need > 0 and cneed > 0

    def body(a, poison):
        st = _st()
        feats, labels = a.put(x, name="canonical features"), a.put(lab, name="labels")
        out = {}
        for costs_given in (1, 0):
            ws = a.take(need, fill=poison, name="tree workspace")
            merges = a.take(B * (K - 1) * 8, fill=poison, name="merges")
            costs = a.take(B * (K - 1) * 8, fill=poison, name="costs") if costs_given else None
            alive = a.take(B * 4, fill=poison, name="alive")
            _ok(lib.gcs_region_tree(feats.data_ptr(), labels.data_ptr(), B, h, w, d, K, ws.data_ptr(), ptr(merges), ptr(costs),
                                    alive.data_ptr(), st), "gcs_region_tree")
            got_m, got_a = a.read(merges, np.int32, (B, K - 1, 2)), a.read(alive, np.int32, (B,))
            for i in range(B):
                assert int(got_a[i]) == trees[i][2], (shape, K, i)
                _eq(got_m[i], trees[i][0], (shape, K, i, "merges"))
            if costs_given:
                out["costs"] = a.read(costs, np.uint64, (B, K - 1))
                _eq(out["costs"], np.stack([tr[1] for tr in trees]), (shape, K, "costs"))
            out["merges %d" % costs_given], out["alive %d" % costs_given] = got_m, got_a
        cut = a.take(B * h * w * 4, fill=poison, name="cut")
        _ok(lib.gcs_region_tree_cut(labels.data_ptr(), ptr(merges), alive.data_ptr(), B, h, w, K, R, cut.data_ptr(), st), "cut")
        same = a.take(lab.nbytes, fill=lab, name="labels (cut in place)")
        _ok(lib.gcs_region_tree_cut(same.data_ptr(), ptr(merges), alive.data_ptr(), B, h, w, K, R, same.data_ptr(), st), "cut in place")
        cws = a.take(cneed, fill=poison, name="contour workspace")
        u = a.take(B * h * w * 4, fill=poison, name="contour map")
        _ok(lib.gcs_region_tree_contours(labels.data_ptr(), ptr(merges), alive.data_ptr(), B, h, w, K, cws.data_ptr(), u.data_ptr(),
                                         st), "gcs_region_tree_contours")
        _, planes, _, _ = _truth_prepare(a, poison, truth, want8=False)
        iof = a.put(img_of, name="img_of")
        hist = a.take((B + 2 * t) * (K + 1) * 4, fill=poison, name="sweep histograms")
        _ok(lib.gcs_boundary_sweep_resident(u.data_ptr(), planes.data_ptr(), iof.data_ptr(), B, t, h, w, K, hist.data_ptr(), st),
            "gcs_boundary_sweep_resident")
        out.update(cut=a.read(cut, np.int32, lab.shape), same=a.read(same, np.int32, lab.shape), u=a.read(u, np.int32, lab.shape),
                   hist=a.read(hist, np.uint32, want_h.shape))
        _eq(out["cut"], want_cut, (shape, K, "gcs_region_tree_cut"))
        _eq(out["same"], want_cut, (shape, K, "gcs_region_tree_cut in place"))
        _eq(out["u"], want_u, (shape, K, "gcs_region_tree_contours"))
        _eq(out["hist"], want_h, (shape, K, "gcs_boundary_sweep_resident"))
        return out
    _twice(torch, body, 2 * need + (8 << 20))


@gpu
@pytest.mark.parametrize("K,r,n", [(1, 1, 4), (33, 15, 5), (64, 1, 16), (64, 15, 4)])
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_texton_gradient(torch_cuda, shape, K, r, n):
    """gcs_texton_gradient with and without ``grad`` and ``dir_out`` == tests/texton_gradient_ref.py; the uint8 direction map is
    B H W bytes exactly."""
    import texton_gradient_ref as tg
    torch, lib = torch_cuda, _lib()
    h, w = shape
    lab = _label_maps(shape, K, seed=h * w + K + r)
    masks = np.zeros((n, 2, 2 * r + 1), np.uint32)
    _ok(lib.gcs_texton_masks(r, n, masks.ctypes.data), "gcs_texton_masks")
    assert np.array_equal(masks, tg.masks(r, n))
    g = np.random.default_rng(r).integers(0, 1 << 20, lab.shape).astype(np.int32)
    want = [tg.texton_gradient(m, K, r, n) for m in lab]
    want_tg, want_dir = np.stack([t for t, _ in want]), np.stack([d for _, d in want])
    want_joined = np.stack([tg.joined(want_tg[i], g[i]) for i in range(B)])

    def body(a, poison):
        labels, table, grad = a.put(lab, name="labels"), a.put(masks, name="masks"), a.put(g, name="grad")
        out = {}
        for with_grad in (0, 1):
            for with_dir in (0, 1):
                o = a.take(B * h * w * 4, fill=poison, name="texton map")
                dm = a.take(B * h * w, fill=poison, name="direction map") if with_dir else None
                _ok(lib.gcs_texton_gradient(labels.data_ptr(), B, h, w, K, r, n, table.data_ptr(), grad.data_ptr() if with_grad else None,
                                            o.data_ptr(), ptr(dm), _st()), "gcs_texton_gradient")
                key = "%d%d" % (with_grad, with_dir)
                out["map " + key] = a.read(o, np.int32, lab.shape)
                _eq(out["map " + key], want_joined if with_grad else want_tg, (shape, K, r, n, key))
                if with_dir:
                    out["dir " + key] = a.read(dm, np.uint8, lab.shape)
                    _eq(out["dir " + key], want_dir, (shape, K, r, n, key, "dir"))
        return out
    _twice(torch, body)


# ------------------------------------------------------------------------------------------------------------ scoring
LDS_LIMIT = 48 * 1024           # tests/test_gpu_scoring_edge.py: workgroup-private tables while
                                # (max_annotators * n_segments * n_truth_labels + 2 * n_segments) * 4 <= 48 * 1024
STRIDE, A_MAX = 10, 3
SEG_AT = LDS_LIMIT // 4 // (A_MAX * STRIDE + 2)            # 384 segments: exactly at the limit; 385: just past it


def _agreement(hist):
    """sums uint64 [T][4] (exact) and terms float64 [T][4] of gcs.h from the tables [T][n_seg][stride], in NumPy."""
    hist = hist.astype(np.int64)
    sums, terms = np.zeros((len(hist), 4), np.uint64), np.zeros((len(hist), 4), np.float64)
    xlog = lambda v: float((v[v > 0] * np.log2(v[v > 0].astype(np.float64))).sum())
    for t, n in enumerate(hist):
        ai, bj = n.sum(axis=1), n.sum(axis=0)
        sums[t] = [bj.sum(), (ai * ai).sum(), (bj * bj).sum(), (n * n).sum()]
        union = ai[:, None] + bj[None, :] - n
        ratio = np.where(n > 0, n / np.maximum(union, 1), 0.0).max(axis=0)
        terms[t] = [xlog(ai), xlog(bj), xlog(n), float((bj * ratio).sum())]
    return sums, terms


@gpu
@pytest.mark.parametrize("n_seg", [SEG_AT, SEG_AT + 1])
@pytest.mark.parametrize("shape", [(1, 1), (1, 64), (1, 65), (13, 1), (13, 64), (13, 65)], ids=lambda s: "%dx%d" % s)
def test_scoring_entries(torch_cuda, shape, n_seg):
    """The ten scorer entry points == the NumPy / scipy restatements of tests/scoring_edge.py (region agreement: NumPy here, the
    integer sums ``==``, the float terms within 1e-11 relative: sums of at most 4000 non-negative float64 terms, each within an ulp
    or two), at W = 1, 64, 65 and H = 1, 13, annotators 1 / 3 / 2, tables at and just past the private-table limit."""
    from scoring_edge import _np_counts, _np_planes, _np_reduce, _np_tables, _np_tables_batch
    torch, lib = torch_cuda, _lib()
    assert (A_MAX * SEG_AT * STRIDE + 2 * SEG_AT) * 4 == LDS_LIMIT
    h, w = shape
    rng = np.random.default_rng(h * 100 + w + n_seg)
    labs = rng.integers(0, n_seg, (B, h, w)).astype(np.int32)
    labs[:, h - 1, w - 1] = n_seg - 1
    truth, first, img_of = _truths(shape, seed=n_seg + w)
    truth = (truth + rng.integers(0, STRIDE - 4, truth.shape)).astype(np.uint16)
    truth[:, 0, 0] = STRIDE - 1
    t = len(truth)
    one, a1 = 1, 3                                                       # the image of three annotators, for the single-image entries
    truth1 = truth[first[one]:first[one + 1]]
    want_c1 = _np_counts(labs[one][None], truth1, np.zeros(a1, np.int32))
    want_c = _np_counts(labs, truth, img_of)
    want_t1 = _np_tables(labs[one], truth1, n_seg, STRIDE)
    want_t = _np_tables_batch(labs, truth, first, n_seg, STRIDE)
    want_under = _np_reduce(want_t[0], want_t[1], img_of)
    want_sums, want_terms = _agreement(want_t[0])
    smax = labs.reshape(B, -1).max(axis=1).astype(np.int32)
    want_planes = _np_planes(truth)                                      # bd and dil5 planes [2][T][H][W]
    wp = (w + 63) // 64
    assert lib.gcs_bit_planes_bytes(t, h, w) == 2 * t * h * wp * 8
    tbytes = t * n_seg * STRIDE * 4

    def tables(a, poison, rows, name):
        return (a.take(rows * n_seg * STRIDE * 4, fill=poison, name="hist " + name), a.take((B if rows == t else 1) * n_seg * 4,
                fill=poison, name="area " + name), a.take((B if rows == t else 1) * n_seg * 4, fill=poison, name="perim " + name))

    def body(a, poison):
        st = _st()
        out = {}
        lab_d, lab1_d, truth1_d = a.put(labs, name="label maps"), a.put(labs[one], name="label map"), a.put(truth1, name="annotators of one")
        first_d, iof = a.put(first, name="first"), a.put(img_of, name="img_of")
        # one image
        sc = a.take(lib.gcs_boundary_scratch_bytes(a1, h, w), fill=poison, name="boundary scratch")
        c1 = a.take((1 + 3 * a1) * 8, fill=poison, name="counts of one")
        _ok(lib.gcs_boundary_counts(lab1_d.data_ptr(), truth1_d.data_ptr(), a1, h, w, sc.data_ptr(), c1.data_ptr(), st), "gcs_boundary_counts")
        h1, ar1, pe1 = tables(a, poison, a1, "of one")
        _ok(lib.gcs_region_counts(lab1_d.data_ptr(), truth1_d.data_ptr(), a1, h, w, n_seg, STRIDE, h1.data_ptr(), ar1.data_ptr(),
                                  pe1.data_ptr(), st), "gcs_region_counts")
        out.update(c1=a.read(c1, np.int64), h1=a.read(h1, np.uint32, (a1, n_seg, STRIDE)), ar1=a.read(ar1, np.uint32), pe1=a.read(pe1, np.uint32))
        _eq(out["c1"], want_c1, (shape, "gcs_boundary_counts"))
        for key, wv in zip(("h1", "ar1", "pe1"), want_t1):
            _eq(out[key], wv, (shape, n_seg, "gcs_region_counts", key))
        # the batch, truth uploaded
        truth_d, planes, bd, t8 = _truth_prepare(a, poison, truth)
        scb = a.take(lib.gcs_boundary_batch_scratch_bytes(B, t, h, w), fill=poison, name="batch scratch")
        cb = a.take((B + 3 * t) * 8, fill=poison, name="counts of the batch")
        _ok(lib.gcs_boundary_counts_batch(lab_d.data_ptr(), truth_d.data_ptr(), iof.data_ptr(), B, t, h, w, scb.data_ptr(), cb.data_ptr(),
                                          st), "gcs_boundary_counts_batch")
        out["cb"] = a.read(cb, np.int64)
        _eq(out["cb"], want_c, (shape, "gcs_boundary_counts_batch"))

        def prepared(when):
            """What gcs_truth_prepare wrote, every bit of it: planes == scoring_edge._np_planes, no bit at or beyond column W."""
            got = {"planes": a.read(planes, np.uint64, (2, t, h, wp)), "bd": a.read(bd, np.int64), "t8": a.read(t8, np.uint8, truth.shape)}
            bits = np.unpackbits(got["planes"].view(np.uint8), axis=-1, bitorder="little").reshape(2, t, h, wp * 64).astype(bool)
            assert not bits[..., w:].any(), (shape, when, "a plane bit at or beyond column W")
            _eq(bits[..., :w], want_planes, (shape, when, "bit planes of gcs_truth_prepare"))
            _eq(got["bd"], want_c[B + 1::3], (shape, when, "bd_counts of gcs_truth_prepare"))
            _eq(got["t8"], truth.astype(np.uint8), (shape, when, "truth8 of gcs_truth_prepare"))
            return got
        out.update(prepared("after gcs_truth_prepare"))
        # resident
        scr = a.take(lib.gcs_bit_planes_bytes(B, h, w), fill=poison, name="label planes")
        cr, sm = a.take((B + 3 * t) * 8, fill=poison, name="counts (resident)"), a.take(B * 4, fill=poison, name="seg_max")
        _ok(lib.gcs_boundary_counts_resident(lab_d.data_ptr(), planes.data_ptr(), bd.data_ptr(), iof.data_ptr(), B, t, h, w, scr.data_ptr(),
                                             cr.data_ptr(), sm.data_ptr(), st), "gcs_boundary_counts_resident")
        crn = a.take((B + 3 * t) * 8, fill=poison, name="counts (resident, no seg_max)")
        _ok(lib.gcs_boundary_counts_resident(lab_d.data_ptr(), planes.data_ptr(), bd.data_ptr(), iof.data_ptr(), B, t, h, w, scr.data_ptr(),
                                             crn.data_ptr(), None, st), "gcs_boundary_counts_resident(seg_max NULL)")
        out.update(cr=a.read(cr, np.int64), crn=a.read(crn, np.int64), sm=a.read(sm, np.int32))
        _eq(out["cr"], want_c, (shape, "gcs_boundary_counts_resident"))
        _eq(out["crn"], want_c, (shape, "gcs_boundary_counts_resident, seg_max NULL"))
        _eq(out["sm"], smax, (shape, "seg_max"))
        for u8, fn, maps in ((0, lib.gcs_region_counts_batch, truth_d), (1, lib.gcs_region_counts_batch_u8, t8)):
            hb_, arb, peb = tables(a, poison, t, "of the batch (%d)" % u8)
            _ok(fn(lab_d.data_ptr(), maps.data_ptr(), first_d.data_ptr(), B, t, A_MAX, h, w, n_seg, STRIDE, hb_.data_ptr(), arb.data_ptr(),
                   peb.data_ptr(), st), "gcs_region_counts_batch" + "_u8" * u8)
            got = (a.read(hb_, np.uint32, (t, n_seg, STRIDE)), a.read(arb, np.uint32, (B, n_seg)), a.read(peb, np.uint32, (B, n_seg)))
            for key, gv, wv in zip(("hist", "area", "perim"), got, want_t):
                out["%s %d" % (key, u8)] = gv
                _eq(gv, wv, (shape, n_seg, "gcs_region_counts_batch", u8, key))
        under, under_np = a.take(t * 8, fill=poison, name="under"), a.take(t * 8, fill=poison, name="under_np")
        _ok(lib.gcs_region_reduce(hb_.data_ptr(), arb.data_ptr(), iof.data_ptr(), t, n_seg, STRIDE, under.data_ptr(), under_np.data_ptr(),
                                  st), "gcs_region_reduce")
        out.update(under=a.read(under, np.int64), under_np=a.read(under_np, np.int64))
        _eq(out["under"], want_under[0], (shape, n_seg, "under"))
        _eq(out["under_np"], want_under[1], (shape, n_seg, "under_np"))
        _eq(a.read(hb_, np.uint32, want_t[0].shape), want_t[0], (shape, "hist_dev after gcs_region_reduce (read only)"))
        _eq(a.read(arb, np.uint32, want_t[1].shape), want_t[1], (shape, "area_dev after gcs_region_reduce (read only)"))
        # the fused scorer
        for u8, maps in ((1, t8), (0, truth_d)):
            f = {key: a.take(size, fill=poison, name="%s (fused scorer)" % key) for key, size in
                 (("scratch", lib.gcs_bit_planes_bytes(B, h, w)), ("hist", tbytes), ("counts", (B + 3 * t) * 8), ("seg_max", B * 4),
                  ("area", B * n_seg * 4), ("perim", B * n_seg * 4), ("under", t * 8), ("under_np", t * 8))}
            _ok(lib.gcs_score_batch_resident(lab_d.data_ptr(), planes.data_ptr(), bd.data_ptr(), maps.data_ptr(), u8, first_d.data_ptr(),
                                             iof.data_ptr(), B, t, A_MAX, h, w, n_seg, STRIDE, f["scratch"].data_ptr(), f["hist"].data_ptr(),
                                             f["counts"].data_ptr(), f["seg_max"].data_ptr(), f["area"].data_ptr(), f["perim"].data_ptr(),
                                             f["under"].data_ptr(), f["under_np"].data_ptr(), st), "gcs_score_batch_resident")
            for key, dt, wv in (("hist", np.uint32, want_t[0]), ("counts", np.int64, want_c), ("seg_max", np.int32, smax),
                                ("area", np.uint32, want_t[1]), ("perim", np.uint32, want_t[2]), ("under", np.int64, want_under[0]),
                                ("under_np", np.int64, want_under[1])):
                out["fused %s %d" % (key, u8)] = a.read(f[key], dt, np.asarray(wv).shape)
                _eq(out["fused %s %d" % (key, u8)], wv, (shape, n_seg, "gcs_score_batch_resident", u8, key))
        # region agreement on the tables the fused scorer left
        for with_max in (0, 1):
            asc = a.take(lib.gcs_region_agreement_scratch_bytes(t, n_seg, STRIDE), fill=poison, name="agreement scratch")
            sums, terms = a.take(t * 32, fill=poison, name="agreement sums"), a.take(t * 32, fill=poison, name="agreement terms")
            _ok(lib.gcs_region_agreement(f["hist"].data_ptr(), iof.data_ptr(), f["seg_max"].data_ptr() if with_max else None, t, n_seg,
                                         STRIDE, asc.data_ptr(), sums.data_ptr(), terms.data_ptr(), st), "gcs_region_agreement")
            out["sums %d" % with_max], out["terms %d" % with_max] = a.read(sums, np.uint64, (t, 4)), a.read(terms, np.float64, (t, 4))
            _eq(out["sums %d" % with_max], want_sums, (shape, n_seg, "agreement sums"))
            err = np.abs(out["terms %d" % with_max] - want_terms)
            assert (err <= 1e-11 * np.maximum(np.abs(want_terms), 1.0)).all(), (shape, n_seg, "agreement terms", float(err.max()))
        _eq(a.read(f["hist"], np.uint32, want_t[0].shape), want_t[0], (shape, "hist_dev after gcs_region_agreement (read only)"))
        again = prepared("after the last call that reads them (resident planes, counts and maps are read only)")
        for key in again:
            _eq(again[key], out[key], (shape, key, "changed by a call that only reads it"))
        return out
    _twice(torch, body, 16 << 20)


# ------------------------------------------------------------------------------------------------------------ the rest
@gpu
@pytest.mark.parametrize("nbytes", [1, 15, 16, 17, 4099])
def test_download_into_pinned_memory(torch_cuda, nbytes):
    """gcs_download into a view of exactly ``nbytes`` of a pinned HOST arena == the source bytes; both arenas intact."""
    torch, lib = torch_cuda, _lib()
    src_bytes = np.random.default_rng(nbytes).integers(1, 256, nbytes, dtype=np.uint8)
    got = []
    for poison in ar.POISONS:
        dev, host = Arena(torch, "cuda", 1 << 16), Arena(torch, "cpu", 1 << 16, pinned=True)
        src = dev.put(src_bytes, name="source")
        dst = host.take(nbytes, fill=poison, name="pinned destination")
        _ok(lib.gcs_download(src.data_ptr(), dst.data_ptr(), nbytes, _st()), "gcs_download")
        torch.cuda.synchronize()
        got.append(host.read(dst))
        _eq(got[-1], src_bytes, (nbytes, "gcs_download"))
        for a in (dev, host):
            a.check()
            a.unchanged()
    assert np.array_equal(got[0], got[1])


@gpu
def test_isqrt_counter(torch_cuda):
    """gcs_selftest_isqrt: the one uint32 it counts into is zeroed by the call."""
    torch, lib = torch_cuda, _lib()

    def body(a, poison):
        bad = a.take(4, align=4, fill=poison, name="bad_dev")
        _ok(lib.gcs_selftest_isqrt(1 << 20, bad.data_ptr(), _st()), "gcs_selftest_isqrt")
        out = {"bad": a.read(bad, np.uint32)}
        assert out["bad"].tolist() == [0]
        return out
    _twice(torch, body, 1 << 16)
