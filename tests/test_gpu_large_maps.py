"""Label-map, image, annotator-stack and canonical-tensor kernels where element indices and byte offsets pass 2^31 and 2^32. The
slab file (tests/test_gpu_large_offsets.py) closed this hole for the entry points that take a feature slab; every other device
pointer entry point promises B <= 65535 images of up to 4096 x 4096 and was never handed more than a few dozen small ones, so an
image base `b * H * W` computed in 32 bits anywhere would pass the whole suite.

Method (the slab file's): sixteen distinct base arrays (tests/large_maps.py: 161 x 241, no side a multiple of 8) replicated through
the fixed sequence idx of tests/large_offsets.py, in which any three consecutive images are three different base arrays. Every
entry point runs on the sixteen alone, that small result is held to the reference the suite already has for it, and the large run
must equal the small one through idx in every output element, every per-image count and every table row. Big arrays are built,
poisoned and compared chunk by chunk on the device (no torch operation spans 2^31 elements) and nothing is left out. The calls are
the raw C entry points (``_lib.load()`` and ``data_ptr()``s). The geometry (which image straddles which line, that the three
images around it differ, that an address short by the line reads other content) is asserted on the host in
tests/test_large_map_geometry.py.

Batches: N31 = 55 401 images (B P >= 2^31 + 2^21 pixels), N30 = 27 728, N29 = 13 891, B_GUARD = 55 346 (the largest B with
B H W < 2^31), the canonical batch 1 539 images of D = 72 (2^32 + 2^21 uint16 elements, 8.6 GB), the colour batch 36 916 images
(3 n_pixels >= 2^32 + 2^21 bytes). Lines, by array, at N31: int32 [B][H][W] - element 2^31 (= byte 2^33), bytes 2^31 and 2^32;
uint16 [T][H][W] - element 2^31 (= byte 2^32), byte 2^31; uint8 [B][H][W] - element = byte 2^31; uint8 [B][H][W][3] - bytes 2^31
and 2^32. At N30 an int32 map crosses bytes 2^31 and 2^32, at N29 byte 2^31 only (and a 64-bit array bytes 2^31 and 2^32);
neither reaches element 2^31.

COVERAGE (below) names, for every entry point of ``_lib.SIGNATURES`` and ``_lib.EXTENSIONS`` that takes a device pointer and no
feature slab, the case that runs it here or why none does; tests/test_large_map_geometry.py keeps the table complete.

NOT covered (the reasons stand in COVERAGE): gcs_download (a 4 GiB pinned host buffer is not for a shared machine); int32 maps past
element 2^32 (16 GiB a map against 24 GiB a test); gcs_boundary_counts and gcs_region_counts (one image: their kernels are the
batched entry points', run here); gcs_region_adjacency_cuts and gcs_region_tree_edges (edge tables only: the first guards every
table below 2^31 elements; the second reads what gcs_region_adjacency wrote, B E_cap 3 < 2^31 - such a table of 16 GiB, crossing its
byte lines, is left for a later case); gcs_kmeans_reduce, gcs_kmeans_finalize and gcs_kmeans_reduce_finalize (partial sums and
codebooks of a slab pass: the slab file runs them behind every pass); gcs_selftest_isqrt (one counter). The slab entry points are
the slab file's; gcs_features_unpack, gcs_features_gather and gcs_kmeans_init stay unverified above 2^31 bytes of slab (there), and
no canonical tensor here is made by gcs_features_unpack.

Seconds / GiB at the peak on an MI355X, per test (the file: 19 s with the build check and the sixteen-image references; every test
below the asserted 24 GiB): labels_widen 0.5 / 10.5; texton_gradient dir_N31 1.9 / 18.5, grad_N29 0.8 / 7.0; cue_gradient
image_cues 1.3 / 16.5, with_labels 3.1 / 22.5; region_tree_cut_in_place 0.9 / 8.5; truth_prepare 0.3 / 6.7; resident_scorer 0.1 /
15.4; boundary_counts_batch < 0.1 / 11.1; contours_and_sweep 1.2 / 16.6; label_used < 0.1 / 8.3; region_props_and_paint 0.1 / 14.3;
colour_opponent 1.2 / 8.1; connected_regions 0.2 / 16.0; merge_small_regions 0.3 / 14.1; region_nodes 0.4 / 14.1;
region_adjacency img 0.1 / 14.7, strength 1.4 / 16.7; cut_shapes 0.0 / 16.3; canonical_tensor 1.9 / 8.8; tables_at_two_to_the_thirty
0.2 / 4.6; sweeps 0.5 and 0.2 / 8.6; props_cuts_and_paint 0.2 / 16.7. Findings: no wrong result and no fault; one guard was off by
one - the scoring tables' entry points refused T * n_segments * n_truth_labels = 2^30 itself (they held it against 2^30 - 1), which
the Python layer's message and the table's own arithmetic (unsigned counts, 64-bit bases) admit: they now take it (csrc/scoring.hip,
include/gcs.h), and test_tables_at_two_to_the_thirty runs it.

Mutants of the library, each built in a scratch copy and run once against this file (failed of 24). Every one truncates without a
sign, on a load only, so every address it forms is below the right one by a multiple of 2^32 (the last: 2^31) and inside the array.
A 32-bit unsigned ELEMENT product is the identity on everything a test can hold (an int32 map passes 2^32 elements at 16 GiB), so
four of the five keep the BYTE offset in `unsigned` instead - what the compiler would form from such a product:
(1) texton_gradient.hip, the image base of the label load `blockIdx.z * H * W * 4` in `unsigned`: 1 failed, test_texton_gradient
[dir_N31], out and dir_out, from image 27 674 on (the first that starts past byte 2^32; 27 673 straddles it).
(2) region_kernels.h, cc_union_kernel's label base `blockIdx.y * P * 4` as a 32-bit product: 1 failed, test_connected_regions, from
image 27 674 on; the merge and node maps at N29 end below byte 2^32, where it is the identity.
(3) scoring.hip, boundary_maps_kernel's `q * n * 4` in `unsigned`: 1 failed, test_boundary_counts_batch, 27 675 label-map counts and
all 10 000 annotator counts.
(4) superpixel.hip, the assign pass's `b * D * hw` as a 32-bit unsigned element product: 1 failed, test_canonical_tensor, labels
and centres of image 1 538, the one image that starts past element 2^32.
(5) scoring.hip, region_reduce_kernel's `t * n_seg * stride`: in `unsigned`, as elements or as bytes, it is the identity on the
whole legal domain (at most 2^30 counters: the last table starts at byte 2^32 - 2^18), so it was not counted; with the byte offset
masked to 31 bits in its place: 1 failed, test_tables_at_two_to_the_thirty, under and under_np from map 8 192 on (byte 2^31).
Against the GPU suite as it was before this file the five ran TOGETHER in one library: 0 failed of 1 589.
"""
import functools
import time

import numpy as np
import pytest

import large_maps as lm
from large_maps import H, K_LABELS, N_BASE, P, W

gpu = pytest.mark.gpu

PEAK_BYTES = 24 << 30               # what one test may hold on the shared device
R_TG, N_TG = 2, 5                   # half-disc radius and directions (n > 4: the eight-direction chunks)
K_ADJ = 12                          # labels of the adjacency maps: at most 66 edges an image
E_CAP = 66
GCS_EINVAL = 1

NOT_YET = "not covered: "
# symbol -> the test of this file that runs it past a line, or "not covered: <why>"
COVERAGE = {
    "gcs_labels_widen": "test_labels_widen",
    "gcs_texton_gradient": "test_texton_gradient",
    "gcs_cue_gradient": "test_cue_gradient",
    "gcs_region_tree_cut": "test_region_tree_cut_in_place",
    "gcs_region_tree_contours": "test_contours_and_sweep",
    "gcs_boundary_sweep_resident": "test_contours_and_sweep",
    "gcs_label_used": "test_label_used",
    "gcs_region_props": "test_region_props_and_paint",
    "gcs_region_paint": "test_region_props_and_paint",
    "gcs_truth_prepare": "test_truth_prepare",
    "gcs_boundary_counts_resident": "test_resident_scorer",
    "gcs_region_counts_batch": "test_resident_scorer",
    "gcs_region_counts_batch_u8": "test_resident_scorer",
    "gcs_region_reduce": "test_resident_scorer",
    "gcs_score_batch_resident": "test_resident_scorer",
    "gcs_boundary_counts_batch": "test_boundary_counts_batch",
    "gcs_colour_opponent": "test_colour_opponent",
    "gcs_connected_regions": "test_connected_regions",
    "gcs_merge_small_regions": "test_merge_small_regions",
    "gcs_region_nodes": "test_region_nodes",
    "gcs_region_adjacency": "test_region_adjacency_at_its_guard",
    "gcs_cut_shapes": "test_cut_shapes_at_its_guard",
    "gcs_superpixel_segment": "test_canonical_tensor",
    "gcs_region_tree": "test_canonical_tensor",
    "gcs_boundary_counts": NOT_YET + "one image: A <= 65534 maps with (A + 1) H W < 2^31 pixels (guarded); its kernels are "
                           "gcs_boundary_counts_batch's, run here",
    "gcs_region_counts": NOT_YET + "one image (A n_seg n_truth <= 2^30): its kernel is gcs_region_counts_batch's, run here",
    "gcs_region_agreement": "test_tables_at_two_to_the_thirty",
    "gcs_region_sweep": "test_sweeps_below_their_guard",
    "gcs_region_sweep_under": "test_sweeps_below_their_guard",
    "gcs_region_props_cuts": "test_props_cuts_and_paint_below_their_guard",
    "gcs_region_adjacency_cuts": NOT_YET + "takes tables only, each guarded below 2^31 elements (n_cuts B K, B E_cap 3, the "
                                 "workspace words); the issue names no case for it",
    "gcs_region_tree_edges": NOT_YET + "takes edge tables only, those gcs_region_adjacency wrote (guarded: B E_cap 3 < 2^31, up to 16 GiB "
                             "of uint64); the issue names no case for it: unverified past byte 2^31 of vals_dev",
    "gcs_download": NOT_YET + "a 4 GiB pinned host buffer is not for a shared machine (the issue's out of scope)",
    "gcs_selftest_isqrt": NOT_YET + "one counter, no array",
    "gcs_kmeans_reduce": NOT_YET + "partial sums of a slab pass: tests/test_gpu_large_offsets.py runs it behind every pass",
    "gcs_kmeans_finalize": NOT_YET + "tables [n_sets][k][D + 1] only: n_sets <= 65535 keeps them below 2^28 elements",
    "gcs_kmeans_reduce_finalize": NOT_YET + "as gcs_kmeans_reduce and gcs_kmeans_finalize",
}
# int32 maps past element 2^32 (16 GiB a map) are not covered either: a test may hold 24 GiB.


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(autouse=True)
def peak_memory(request):
    """Every GPU test of this file: at most 24 GiB of device memory at its peak, and its time printed."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    torch = request.getfixturevalue("torch_cuda")
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("%s: %.1f s, peak %.1f GiB" % (request.node.name, time.perf_counter() - t0, peak / 2 ** 30))
    assert peak <= PEAK_BYTES, peak


class _World:
    """The sixteen base arrays on the host and on the device, the index sequences, and the small results other cases build on."""

    def __init__(self, torch):
        from gabor_color_image_segmentation_amd import _lib
        self.torch, self.lib = torch, _lib.load()
        self.lab_np, self.img_np, self.truth_np = lm.base_labels(), lm.base_images(), lm.base_truth()
        self.lab, self.img, self.truth = (torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
                                          for a in (self.lab_np, self.img_np, self.truth_np))
        self._idx, self._refs = {}, {}

    def idx(self, b):
        """(idx on the host, idx on the device) of a batch of b images."""
        if b not in self._idx:
            i = lm.batch(b)
            self._idx[b] = (i, self.torch.from_numpy(i).cuda())
        return self._idx[b]

    def st(self):
        return self.torch.cuda.current_stream().cuda_stream

    def call(self, name, *args):
        fn = getattr(self.lib, name, None)
        assert fn is not None, name + ": the library does not export it"
        rc = fn(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], self.st())
        assert rc == 0, (name, rc, self.lib.gcs_last_error())

    def refused(self, name, *args):
        rc = getattr(self.lib, name)(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], self.st())
        return rc == GCS_EINVAL

    def ref(self, key, make):
        if key not in self._refs:
            self._refs[key] = make()
        return self._refs[key]

    def dev(self, a):
        a = np.ascontiguousarray(a)
        view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
        return self.torch.from_numpy(a.view(view) if view else a).cuda()

    def masks(self):
        def make():
            import texton_gradient_ref as tg
            m = np.zeros((N_TG, 2, 2 * R_TG + 1), np.uint32)
            assert self.lib.gcs_texton_masks(R_TG, N_TG, m.ctypes.data) == 0 and np.array_equal(m, tg.masks(R_TG, N_TG))
            return self.dev(m)
        return self.ref("masks", make)

    def tree(self):
        """The region tree of the sixteen base maps on three features: (merges (16, K-1, 2), alive (16,)) on the device, the host
        copies, every image == tests/region_tree_ref.py."""
        def make():
            import region_tree_ref as rt
            torch, k, d = self.torch, K_LABELS, 3
            x_np = lm.base_canonical(d, seed=3)
            x = self.dev(x_np)
            ws = torch.empty(self.lib.gcs_region_tree_workspace_bytes(N_BASE, H, W, d, k), dtype=torch.uint8, device="cuda")
            merges = torch.full((N_BASE, k - 1, 2), 7, dtype=torch.int32, device="cuda")
            costs = torch.full((N_BASE, k - 1), 7, dtype=torch.int64, device="cuda")
            alive = torch.full((N_BASE,), -5, dtype=torch.int32, device="cuda")
            self.call("gcs_region_tree", x, self.lab, N_BASE, H, W, d, k, ws, merges, costs, alive)
            m_np, c_np, a_np = merges.cpu().numpy(), costs.cpu().numpy().view(np.uint64), alive.cpu().numpy()
            for j in range(N_BASE):
                rm, rc, ra = rt.build_tree(x_np[j], self.lab_np[j], k)
                assert int(a_np[j]) == ra and np.array_equal(m_np[j], rm) and np.array_equal(c_np[j], rc), j
            assert a_np.min() > 8
            return merges, alive, m_np, a_np
        return self.ref("tree", make)

    def contours(self):
        """U of the sixteen base maps under ``tree``: (16, H, W) int32 on the device == tests/contour_map_ref.py."""
        def make():
            import contour_map_ref as cm
            torch, k = self.torch, K_LABELS
            merges, alive, m_np, a_np = self.tree()
            ws = torch.empty(self.lib.gcs_region_tree_contours_workspace_bytes(N_BASE, k), dtype=torch.uint8, device="cuda")
            u = torch.full((N_BASE, H, W), -7, dtype=torch.int32, device="cuda")
            self.call("gcs_region_tree_contours", self.lab, merges, alive, N_BASE, H, W, k, ws, u)
            u_np = u.cpu().numpy()
            for j in range(N_BASE):
                assert np.array_equal(u_np[j], cm.contour_map(self.lab_np[j], m_np[j], int(a_np[j]))), j
            assert u_np.max() > 8
            return u, u_np
        return self.ref("contours", make)


_WORLD = []


@pytest.fixture(scope="module")
def world(torch_cuda):
    if not _WORLD:
        _WORLD.append(_World(torch_cuda))
    yield _WORLD[0]


@pytest.fixture(scope="module", autouse=True)
def _free_at_the_end():
    yield
    if _WORLD:
        torch = _WORLD[0].torch
        _WORLD.clear()
        torch.cuda.empty_cache()


_DIFFS = []


def _releasing(test):
    """The large comparisons of a test do not raise where they stand: a failure's traceback would hold the test's frame, and with
    it up to 22 GiB of device arrays, until the session ends (every later test then ran over the 24 GiB it asserts). They are
    noted (``_same``, ``_equal``), the arrays die with the test's frame, and the test fails here, behind them."""
    @functools.wraps(test)
    def wrapper(*args, **kwargs):
        del _DIFFS[:]
        test(*args, **kwargs)
        found = list(_DIFFS)
        del _DIFFS[:]
        assert not found, found
    return wrapper


def _same(w, big, small, idx_dev, what):
    bad = lm.first_difference(w.torch, big, small, idx_dev)
    if bad is not None:
        _DIFFS.append((what, "first image that differs, images that differ in its chunk:", bad))


def _equal(w, got, want, what):
    """Two small device tensors (per-image counts, gathered through idx by the caller)."""
    if not w.torch.equal(got, want):
        _DIFFS.append((what, "images that differ:", int((got != want).reshape(got.shape[0], -1).any(1).sum())))


# ------------------------------------------------------------------------------------------------------------ part 1: maps
@gpu
@_releasing
def test_labels_widen(world):
    """gcs_labels_widen at N31. In: uint8 [B][H][W], crosses element = byte 2^31. Out: int32 [B][H][W], crosses element 2^31 (byte
    2^33) and bytes 2^31, 2^32. Small == the base maps themselves."""
    w, torch = world, world.torch
    _, idx = w.idx(lm.N31)
    small8 = w.lab.to(torch.uint8)
    small = torch.full((N_BASE, H, W), -7, dtype=torch.int32, device="cuda")
    w.call("gcs_labels_widen", small8, N_BASE, H, W, small)
    assert torch.equal(small, w.lab)
    big8 = lm.replicate(torch, small8, idx)
    out = lm.filled(torch, (lm.N31, H, W), torch.int32, -7)
    w.call("gcs_labels_widen", big8, lm.N31, H, W, out)
    _same(w, out, small, idx, "gcs_labels_widen")


def _texton_ref(w):
    import texton_gradient_ref as tg
    return w.ref("texton", lambda: [np.stack(a) for a in zip(*[tg.texton_gradient(m, K_LABELS, R_TG, N_TG) for m in w.lab_np])])


@gpu
@pytest.mark.parametrize("arm", ["dir_N31", "grad_N29"])
@_releasing
def test_texton_gradient(world, arm):
    """gcs_texton_gradient. dir_N31: grad NULL, with dir_out, at N31 - labels and out int32 cross element 2^31 and bytes 2^31, 2^32
    (2^33), dir_out uint8 crosses 2^31. grad_N29: with grad and dir_out at N29 - the three int32 maps cross byte 2^31 only.
    Small == tests/texton_gradient_ref.py (joined with the edge map in the grad arm; negative G counts as 0)."""
    import texton_gradient_ref as tg
    w, torch = world, world.torch
    b = lm.N31 if arm == "dir_N31" else lm.N29
    _, idx = w.idx(b)
    want_tg, want_dir = _texton_ref(w)
    masks = w.masks()
    grad_small = grad = None
    want = want_tg
    if arm == "grad_N29":
        g_np = np.random.default_rng(29).integers(-1000, 1 << 20, (N_BASE, H, W)).astype(np.int32)
        want = np.stack([tg.joined(want_tg[j], np.maximum(g_np[j], 0)) for j in range(N_BASE)])
        grad_small = w.dev(g_np)
        grad = lm.replicate(torch, grad_small, idx)
    small = torch.full((N_BASE, H, W), -7, dtype=torch.int32, device="cuda")
    small_dir = torch.full((N_BASE, H, W), 0xA5, dtype=torch.uint8, device="cuda")
    w.call("gcs_texton_gradient", w.lab, N_BASE, H, W, K_LABELS, R_TG, N_TG, masks, grad_small, small, small_dir)
    assert np.array_equal(small.cpu().numpy(), want) and np.array_equal(small_dir.cpu().numpy(), want_dir)
    assert want.max() > 0 and len(np.unique(want_dir)) > 2
    labels = lm.replicate(torch, w.lab, idx)
    out = lm.filled(torch, (b, H, W), torch.int32, -7)
    dir_out = lm.filled(torch, (b, H, W), torch.uint8, 0xA5)
    w.call("gcs_texton_gradient", labels, b, H, W, K_LABELS, R_TG, N_TG, masks, grad, out, dir_out)
    _same(w, out, small, idx, (arm, "out"))
    _same(w, dir_out, small_dir, idx, (arm, "dir_out"))


CUE_CASES = {"image_cues": (0, 2, 1, 3), "with_labels": (3, 1, 1, 1)}
CUE_SHIFT = 5                       # 8 bins a channel


@gpu
@pytest.mark.parametrize("case", list(CUE_CASES))
@_releasing
def test_cue_gradient(world, case):
    """gcs_cue_gradient at N31. image_cues: weights (0, 2, 1, 3), labels NULL, with dir_out - img uint8 [B][H][W][3] crosses bytes
    2^31 and 2^32, out int32 element 2^31 and bytes 2^31, 2^32, dir_out 2^31. with_labels: weights (3, 1, 1, 1), dir_out dropped in
    the large run to stay below 24 GiB - labels, img and out cross their lines together. Small == tests/cue_gradient_ref.py, dir
    included."""
    import cue_gradient_ref as cg
    w, torch = world, world.torch
    weights = CUE_CASES[case]
    _, idx = w.idx(lm.N31)
    bins = 256 >> CUE_SHIFT
    assert cg.shift_of(bins) == CUE_SHIFT
    refs = [cg.cue_gradient(w.lab_np[j] if weights[0] else None, w.img_np[j], K_LABELS, bins, weights, R_TG, N_TG) for j in range(N_BASE)]
    want, want_dir = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    masks = w.masks()
    small = torch.full((N_BASE, H, W), -7, dtype=torch.int32, device="cuda")
    small_dir = torch.full((N_BASE, H, W), 0xA5, dtype=torch.uint8, device="cuda")
    args = (H, W, K_LABELS, CUE_SHIFT) + weights + (R_TG, N_TG, masks, None)
    w.call("gcs_cue_gradient", w.lab if weights[0] else None, w.img, N_BASE, *args, small, small_dir)
    assert np.array_equal(small.cpu().numpy(), want) and np.array_equal(small_dir.cpu().numpy(), want_dir) and want.max() > 0
    img = lm.replicate(torch, w.img, idx)
    labels = lm.replicate(torch, w.lab, idx) if weights[0] else None
    out = lm.filled(torch, (lm.N31, H, W), torch.int32, -7)
    dir_out = None if weights[0] else lm.filled(torch, (lm.N31, H, W), torch.uint8, 0xA5)
    w.call("gcs_cue_gradient", labels, img, lm.N31, *args, out, dir_out)
    _same(w, out, small, idx, (case, "out"))
    if dir_out is not None:
        _same(w, dir_out, small_dir, idx, (case, "dir_out"))


@gpu
@_releasing
def test_region_tree_cut_in_place(world):
    """gcs_region_tree_cut in place at N31, R = 5: the int32 map crosses element 2^31 and bytes 2^31, 2^32 as input and as
    output. Small (out of place) == tests/region_tree_ref.py's cut of the tree gcs_region_tree made (== its build_tree)."""
    import region_tree_ref as rt
    w, torch = world, world.torch
    _, idx = w.idx(lm.N31)
    k, r = K_LABELS, 5
    merges, alive, m_np, a_np = w.tree()
    small = torch.full((N_BASE, H, W), -7, dtype=torch.int32, device="cuda")
    w.call("gcs_region_tree_cut", w.lab, merges, alive, N_BASE, H, W, k, r, small)
    want = np.stack([rt.cut(w.lab_np[j], m_np[j], int(a_np[j]), r) for j in range(N_BASE)])
    assert np.array_equal(small.cpu().numpy(), want) and want.max() == r - 1
    labels = lm.replicate(torch, w.lab, idx)
    w.call("gcs_region_tree_cut", labels, merges[idx], alive[idx], lm.N31, H, W, k, r, labels)
    _same(w, labels, small, idx, "gcs_region_tree_cut in place")


def _prepare(w, truth, t, want8):
    """gcs_truth_prepare on (t, H, W) annotator maps -> (planes uint8 bytes, bd_counts int64 (t,), truth8 or None); outputs poisoned."""
    torch = w.torch
    nbytes = w.lib.gcs_bit_planes_bytes(t, H, W)
    assert nbytes == 2 * t * H * ((W + 63) // 64) * 8
    planes = lm.filled(torch, (2 * t, nbytes // (2 * t)), torch.uint8, 0xA5)
    bd = torch.full((t,), -3, dtype=torch.int64, device="cuda")
    t8 = lm.filled(torch, (t, H, W), torch.uint8, 0xA5) if want8 else None
    w.call("gcs_truth_prepare", truth, t, H, W, planes, bd, t8)
    return planes, bd, t8


def _small_prepared(w):
    """gcs_truth_prepare on the sixteen base annotator maps, every bit == scipy (tests/scoring_edge.py)."""
    def make():
        from scoring_edge import _np_planes
        planes, bd, t8 = _prepare(w, w.truth, N_BASE, True)
        wp = (W + 63) // 64
        words = planes.cpu().numpy().reshape(2, N_BASE, H, wp * 8)
        bits = np.unpackbits(words, axis=-1, bitorder="little").astype(bool)
        want = _np_planes(w.truth_np)
        assert not bits[..., W:].any() and np.array_equal(bits[..., :W], want)
        assert np.array_equal(bd.cpu().numpy(), want[0].reshape(N_BASE, -1).sum(1))
        assert np.array_equal(t8.cpu().numpy(), w.truth_np.astype(np.uint8))
        return planes, bd, t8
    return w.ref("prepared", make)


@gpu
@_releasing
def test_truth_prepare(world):
    """gcs_truth_prepare at T = N31, uint16 in and uint8 out: truth uint16 [T][H][W] crosses element 2^31 (byte 2^32) and byte
    2^31, truth8 crosses 2^31; the planes (571 MB) and counts cross nothing. Small == scipy's planes, bit for bit."""
    w, torch = world, world.torch
    t = lm.N31
    _, idx = w.idx(t)
    s_planes, s_bd, s_t8 = _small_prepared(w)
    truth = lm.replicate(torch, w.truth, idx)
    planes, bd, t8 = _prepare(w, truth, t, True)
    half = s_planes.shape[0] // 2
    _same(w, planes[:t], s_planes[:half], idx, "bd planes")
    _same(w, planes[t:], s_planes[half:], idx, "dil5 planes")
    _equal(w, bd, s_bd[idx], "bd_counts")
    _same(w, t8, s_t8, idx, "truth8")


N_SEG, N_TRUTH = K_LABELS, 10


@gpu
@_releasing
def test_resident_scorer(world):
    """At B = T = N31, one annotator map an image (that of the image's own base number): gcs_boundary_counts_resident (with
    seg_max), gcs_region_counts_batch (uint16 maps) and _u8, gcs_region_reduce on their tables, and gcs_score_batch_resident (uint8
    maps), n_segments = 48, n_truth_labels = 10 so that the tables stay small (106 MB). labels int32 crosses element 2^31 and bytes
    2^31, 2^32; the uint16 annotator stack element 2^31 and byte 2^31; the uint8 one 2^31. Small (B = T = 16) == scipy / NumPy
    (tests/scoring_edge.py); every count, table row and per-image sum of the large runs == the small ones through idx."""
    from scoring_edge import _np_counts, _np_reduce, _np_tables_batch
    w, torch = world, world.torch
    b = lm.N31
    idx_np, idx = w.idx(b)

    def run(nb, labels, truth, planes, bd, t8):
        img_of, first = torch.arange(nb, dtype=torch.int32, device="cuda"), torch.arange(nb + 1, dtype=torch.int32, device="cuda")
        new = lambda shape, dt: lm.filled(torch, shape, dt, 0x25)
        out = {}
        scratch = new((w.lib.gcs_bit_planes_bytes(nb, H, W),), torch.uint8)
        out["counts"], out["seg_max"] = new((4 * nb,), torch.int64), new((nb,), torch.int32)
        w.call("gcs_boundary_counts_resident", labels, planes, bd, img_of, nb, nb, H, W, scratch, out["counts"], out["seg_max"])
        for u8, name, maps in ((0, "gcs_region_counts_batch", truth), (1, "gcs_region_counts_batch_u8", t8)):
            hist, area, perim = new((nb, N_SEG, N_TRUTH), torch.int32), new((nb, N_SEG), torch.int32), new((nb, N_SEG), torch.int32)
            w.call(name, labels, maps, first, nb, nb, 1, H, W, N_SEG, N_TRUTH, hist, area, perim)
            out.update({"hist %d" % u8: hist, "area %d" % u8: area, "perim %d" % u8: perim})
        out["under"], out["under_np"] = new((nb,), torch.int64), new((nb,), torch.int64)
        w.call("gcs_region_reduce", out["hist 0"], out["area 0"], img_of, nb, N_SEG, N_TRUTH, out["under"], out["under_np"])
        f = {"hist": new((nb, N_SEG, N_TRUTH), torch.int32), "counts": new((4 * nb,), torch.int64), "seg_max": new((nb,), torch.int32),
             "area": new((nb, N_SEG), torch.int32), "perim": new((nb, N_SEG), torch.int32), "under": new((nb,), torch.int64),
             "under_np": new((nb,), torch.int64)}
        w.call("gcs_score_batch_resident", labels, planes, bd, t8, 1, first, img_of, nb, nb, 1, H, W, N_SEG, N_TRUTH, scratch,
               f["hist"], f["counts"], f["seg_max"], f["area"], f["perim"], f["under"], f["under_np"])
        out.update({"fused " + key: v for key, v in f.items()})
        return out

    s_planes, s_bd, s_t8 = _small_prepared(w)
    small = run(N_BASE, w.lab, w.truth, s_planes, s_bd, s_t8)
    img_of_np, first_np = np.arange(N_BASE, dtype=np.int32), np.arange(N_BASE + 1, dtype=np.int32)
    want_c = _np_counts(w.lab_np, w.truth_np, img_of_np)
    want_t = _np_tables_batch(w.lab_np, w.truth_np, first_np, N_SEG, N_TRUTH)
    want_u = _np_reduce(want_t[0], want_t[1], img_of_np)
    host = {key: v.cpu().numpy() for key, v in small.items()}
    for key in ("counts", "fused counts"):
        assert np.array_equal(host[key], want_c), key
    for key in ("seg_max", "fused seg_max"):
        assert np.array_equal(host[key], w.lab_np.reshape(N_BASE, -1).max(1)), key
    for pre in ("hist %d", "area %d", "perim %d"):
        for u8 in (0, 1):
            assert np.array_equal(host[pre % u8], want_t[("hist %d", "area %d", "perim %d").index(pre)]), pre % u8
    for i, key in enumerate(("hist", "area", "perim")):
        assert np.array_equal(host["fused " + key], want_t[i]), key
    for i, key in enumerate(("under", "under_np")):
        assert np.array_equal(host[key], want_u[i]) and np.array_equal(host["fused " + key], want_u[i]), key
    assert want_t[0].max() > 0 and want_u[0].min() > 0
    # the large run
    truth = lm.replicate(torch, w.truth, idx)
    planes, bd, t8 = _prepare(w, truth, b, True)
    labels = lm.replicate(torch, w.lab, idx)
    big = run(b, labels, truth, planes, bd, t8)
    for key, got in big.items():
        s = small[key]
        if key.endswith("counts"):                     # [b] per image, then three per annotator map
            _equal(w, got[:b], s[:N_BASE][idx], key)
            _equal(w, got[b:].view(b, 3), s[N_BASE:].view(N_BASE, 3)[idx], key)
        else:
            _same(w, got, s, idx, key)


@gpu
@_releasing
def test_boundary_counts_batch(world):
    """gcs_boundary_counts_batch at B = N31 with T = 10 000 annotator maps, those of the last T images (the entry point takes B + T <=
    65535). labels int32 crosses element 2^31 and bytes 2^31, 2^32; the scratch's uint8 planes [B + T][H][W] cross 2^31; the uint16
    annotator stack (776 MB) crosses nothing. Small (B = T = 16) == scipy (tests/scoring_edge.py)."""
    from scoring_edge import _np_counts
    w, torch = world, world.torch
    b, t = lm.N31, 10000
    assert b + t <= 65535
    idx_np, idx = w.idx(b)

    def run(nb, nt, labels, truth, img_of):
        scratch = lm.filled(torch, (w.lib.gcs_boundary_batch_scratch_bytes(nb, nt, H, W),), torch.uint8, 0xA5)
        counts = torch.full((nb + 3 * nt,), -3, dtype=torch.int64, device="cuda")
        w.call("gcs_boundary_counts_batch", labels, truth, img_of, nb, nt, H, W, scratch, counts)
        return counts

    small = run(N_BASE, N_BASE, w.lab, w.truth, torch.arange(N_BASE, dtype=torch.int32, device="cuda"))
    assert np.array_equal(small.cpu().numpy(), _np_counts(w.lab_np, w.truth_np, np.arange(N_BASE)))
    labels = lm.replicate(torch, w.lab, idx)
    truth = lm.replicate(torch, w.truth, idx[b - t:])
    got = run(b, t, labels, truth, torch.arange(b - t, b, dtype=torch.int32, device="cuda"))
    _equal(w, got[:b], small[:N_BASE][idx], "label-map counts")
    _equal(w, got[b:].view(t, 3), small[N_BASE:].view(N_BASE, 3)[idx[b - t:]], "annotator counts")


@gpu
@_releasing
def test_contours_and_sweep(world):
    """gcs_region_tree_contours at N31 (labels and the contour map, int32, cross element 2^31 and bytes 2^31, 2^32), then
    gcs_boundary_sweep_resident on that map with B = T = N31 annotator planes (571 MB, no line) and K = 48. Small == tests/
    contour_map_ref.py: the map and the three histograms of every image."""
    import contour_map_ref as cm
    w, torch = world, world.torch
    b, k = lm.N31, K_LABELS
    _, idx = w.idx(b)
    merges, alive, _, _ = w.tree()
    s_u, u_np = w.contours()
    s_planes, _, _ = _small_prepared(w)

    def sweep(nb, u, planes):
        hist = lm.filled(torch, (3 * nb, k + 1), torch.int32, 0x25)
        w.call("gcs_boundary_sweep_resident", u, planes, torch.arange(nb, dtype=torch.int32, device="cuda"), nb, nb, H, W, k, hist)
        return hist

    s_hist = sweep(N_BASE, s_u, s_planes)
    got = s_hist.cpu().numpy().view(np.uint32)
    for j in range(N_BASE):
        hm, rec, prec = cm.histograms(u_np[j], w.truth_np[j:j + 1], k)
        assert np.array_equal(got[j], hm) and np.array_equal(got[N_BASE + 2 * j], rec[0]) and np.array_equal(got[N_BASE + 2 * j + 1], prec[0]), j
    assert got[N_BASE:].max() > 0
    labels = lm.replicate(torch, w.lab, idx)
    ws = lm.filled(torch, (w.lib.gcs_region_tree_contours_workspace_bytes(b, k),), torch.uint8, 0xA5)
    u = lm.filled(torch, (b, H, W), torch.int32, -7)
    w.call("gcs_region_tree_contours", labels, merges[idx], alive[idx], b, H, W, k, ws, u)
    _same(w, u, s_u, idx, "gcs_region_tree_contours")
    del labels, ws
    truth = lm.replicate(torch, w.truth, idx)
    planes, _, _ = _prepare(w, truth, b, False)
    del truth
    hist = sweep(b, u, planes)
    _equal(w, hist[:b], s_hist[:N_BASE][idx], "rows of the maps")
    _equal(w, hist[b:].view(b, 2, k + 1), s_hist[N_BASE:].view(N_BASE, 2, k + 1)[idx], "rows of the annotator maps")


@gpu
@_releasing
def test_label_used(world):
    """gcs_label_used at N31 with K = 50 (labels 48 and 49 own no pixel): labels int32 crosses element 2^31 and bytes 2^31, 2^32;
    used_out [B][K] crosses nothing. Small == np.bincount."""
    w, torch = world, world.torch
    b, k = lm.N31, K_LABELS + 2
    _, idx = w.idx(b)
    small = torch.full((N_BASE, k), -7, dtype=torch.int32, device="cuda")
    w.call("gcs_label_used", w.lab, N_BASE, H, W, k, small)
    want = np.stack([np.bincount(m.ravel(), minlength=k) > 0 for m in w.lab_np]).astype(np.int32)
    assert np.array_equal(small.cpu().numpy(), want) and want[:, K_LABELS:].sum() == 0 and want.sum() > N_BASE * 40
    labels = lm.replicate(torch, w.lab, idx)
    used = torch.full((b, k), -7, dtype=torch.int32, device="cuda")
    w.call("gcs_label_used", labels, b, H, W, k, used)
    _same(w, used, small, idx, "gcs_label_used")


@gpu
@_releasing
def test_region_props_and_paint(world):
    """gcs_region_props (D = 0, with img) and gcs_region_paint (group NULL, G = K) at N31: labels int32 crosses element 2^31 and
    bytes 2^31, 2^32; img and rgb_out uint8 [B][H][W][3] cross bytes 2^31 and 2^32; the tables (B K C = 16 M uint64) cross nothing.
    Small == tests/region_props_ref.py (leaf_table, paint)."""
    import region_props_ref as rp
    w, torch = world, world.torch
    b, k, c = lm.N31, K_LABELS, 6
    assert b * k * c < 1 << 31
    _, idx = w.idx(b)

    def props(nb, labels, img):
        sums, bbox = lm.filled(torch, (nb, k, c), torch.int64, -3), lm.filled(torch, (nb, k, 4), torch.int32, -7)
        w.call("gcs_region_props", labels, img, None, nb, H, W, 0, k, sums, bbox)
        return sums, bbox

    def paint(nb, labels, sums):
        rgb = lm.filled(torch, (nb, H, W, 3), torch.uint8, 0xA5)
        w.call("gcs_region_paint", labels, None, sums, nb, H, W, k, k, c, k, rgb)
        return rgb

    s_sums, s_bbox = props(N_BASE, w.lab, w.img)
    s_rgb = paint(N_BASE, w.lab, s_sums)
    for j in range(N_BASE):
        want_s, want_b = rp.leaf_table(w.lab_np[j], k, img=w.img_np[j])
        assert np.array_equal(s_sums[j].cpu().numpy().view(np.uint64), want_s) and np.array_equal(s_bbox[j].cpu().numpy(), want_b), j
        assert np.array_equal(s_rgb[j].cpu().numpy(), rp.paint(w.lab_np[j], want_s)), j
    labels = lm.replicate(torch, w.lab, idx)
    img = lm.replicate(torch, w.img, idx)
    sums, bbox = props(b, labels, img)
    del img
    _same(w, sums, s_sums, idx, "sums")
    _same(w, bbox, s_bbox, idx, "bbox")
    rgb = paint(b, labels, sums)
    _same(w, rgb, s_rgb, idx, "gcs_region_paint")


@gpu
@_releasing
def test_colour_opponent(world):
    """gcs_colour_opponent on 36 916 images as ONE run of n_pixels = 1 432 377 716 pixels (3 n_pixels >= 2^32 + 2^21 bytes), gain 2,
    both pointers at an odd byte: src and out cross bytes 2^31 and 2^32. The three bytes in front of out and the bytes behind it
    keep their poison. Small (the sixteen images as one run, the same odd pointers) == tests/colour_ref.py."""
    import colour_ref as cr
    w, torch = world, world.torch
    b, gain, per = lm.N_COLOUR, 2, 3 * P
    assert 3 * b * P >= lm.LINE32 + lm.MARGIN
    _, idx = w.idx(b)

    def run(nb, fill):
        src, dst = torch.empty(nb * per + 1, dtype=torch.uint8, device="cuda"), torch.empty(nb * per + 8, dtype=torch.uint8, device="cuda")
        body = src[1:].view(nb, per)
        fill(body)
        dst[:3].fill_(0xA5)
        dst[3 + nb * per:].fill_(0xA5)
        out = dst[3:3 + nb * per].view(nb, per)
        for i in range(0, nb, lm.chunk_of(per)):
            out[i:i + lm.chunk_of(per)].fill_(0xA5)
        assert body.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
        w.call("gcs_colour_opponent", body.data_ptr(), nb * P, gain, out.data_ptr())
        assert bool((dst[:3] == 0xA5).all()) and bool((dst[3 + nb * per:] == 0xA5).all()), "a byte outside [0, 3 n_pixels) was written"
        return out

    flat = w.img.view(N_BASE, per)
    small = run(N_BASE, lambda body: body.copy_(flat)).clone()
    assert np.array_equal(small.cpu().numpy().reshape(w.img_np.shape), cr.opponent(w.img_np, gain))

    def fill(body):
        step = lm.chunk_of(per)
        for i in range(0, b, step):
            body[i:i + step] = flat[idx[i:i + step]]
    out = run(b, fill)
    _same(w, out, small, idx, "gcs_colour_opponent")


@gpu
@_releasing
def test_connected_regions(world):
    """gcs_connected_regions at N30 (N31 would need 34 GB): labels, out and the two int32 arrays of the scratch cross bytes 2^31 and
    2^32 (the scratch as a whole, 2^31 + 2^22 int32, element 2^31 too: its second array starts past it). None reaches element 2^31
    on its own. Small == spec_oracle.connected_regions."""
    from oracle import spec_oracle as so
    w, torch = world, world.torch
    b = lm.N30
    _, idx = w.idx(b)

    def run(nb, labels):
        need = w.lib.gcs_connected_scratch_bytes(nb, H, W)
        assert need == 2 * nb * P * 4
        scratch = lm.filled(torch, (2 * nb, P * 4), torch.uint8, 0xA5)
        out = lm.filled(torch, (nb, H, W), torch.int32, -7)
        w.call("gcs_connected_regions", labels, nb, H, W, scratch, out)
        return out

    small = run(N_BASE, w.lab)
    want = np.stack([so.connected_regions(m) for m in w.lab_np])
    assert np.array_equal(small.cpu().numpy(), want) and want.max() > 1000
    out = run(b, lm.replicate(torch, w.lab, idx))
    _same(w, out, small, idx, "gcs_connected_regions")


MIN_SIZE = 3


@gpu
@_releasing
def test_merge_small_regions(world):
    """gcs_merge_small_regions at N29, min_size = 3 (20 bytes of scratch a pixel: N30 would need 30 GB): labels, out and the
    scratch's three int32 arrays cross byte 2^31, its 64-bit `best` array bytes 2^31 and 2^32; the scratch as a whole (10.8 GB)
    passes bytes 2^32 and 2^33. None reaches element 2^31. Small == tests/merge_ref.py."""
    import merge_ref
    w, torch = world, world.torch
    b = lm.N29
    _, idx = w.idx(b)

    def run(nb, labels):
        need = w.lib.gcs_merge_scratch_bytes(nb, H, W, MIN_SIZE)
        assert need == nb * P * 20 + 32 * nb * 4
        scratch = lm.filled(torch, (nb, need // nb), torch.uint8, 0xA5)
        out = lm.filled(torch, (nb, H, W), torch.int32, -7)
        w.call("gcs_merge_small_regions", labels, nb, H, W, MIN_SIZE, scratch, out)
        return out

    small = run(N_BASE, w.lab)
    want = np.stack([merge_ref.merge_small_regions(m, MIN_SIZE) for m in w.lab_np])
    assert np.array_equal(small.cpu().numpy(), want)
    out = run(b, lm.replicate(torch, w.lab, idx))
    _same(w, out, small, idx, "gcs_merge_small_regions")


@gpu
@_releasing
def test_region_nodes(world):
    """gcs_region_nodes at N29, min_size = 3, k_cap = 4096 (about 20 bytes of scratch a pixel): the lines of
    test_merge_small_regions. The base maps have fewer than 4096 connected regions, so m_b = min_size and the node map is
    tests/merge_ref.py's; n_nodes and min_size_used per image through idx."""
    import merge_ref
    from oracle import spec_oracle as so
    w, torch = world, world.torch
    b, k_cap = lm.N29, 4096
    _, idx = w.idx(b)
    assert max(int(so.connected_regions(m).max()) + 1 for m in w.lab_np) <= k_cap

    def run(nb, labels):
        need = w.lib.gcs_region_nodes_scratch_bytes(nb, H, W)
        assert need > 0 and need % nb == 0
        scratch = lm.filled(torch, (nb, need // nb), torch.uint8, 0xA5)
        out = lm.filled(torch, (nb, H, W), torch.int32, -7)
        n_nodes, used = torch.full((nb,), -7, dtype=torch.int32, device="cuda"), torch.full((nb,), -7, dtype=torch.int32, device="cuda")
        w.call("gcs_region_nodes", labels, nb, H, W, MIN_SIZE, k_cap, scratch, out, n_nodes, used)
        return out, n_nodes, used

    small = run(N_BASE, w.lab)
    want = np.stack([merge_ref.merge_small_regions(m, MIN_SIZE) for m in w.lab_np])
    assert np.array_equal(small[0].cpu().numpy(), want)
    assert np.array_equal(small[1].cpu().numpy(), want.reshape(N_BASE, -1).max(1) + 1) and bool((small[2] == MIN_SIZE).all())
    big = run(b, lm.replicate(torch, w.lab, idx))
    for what, got, s in zip(("nodes", "n_nodes", "min_size_used"), big, small):
        _same(w, got, s, idx, what)


def _adjacency_labels(w):
    def make():
        lab = lm.base_labels(K_ADJ, seed=12)
        return lab, w.dev(lab)
    return w.ref("adjacency labels", make)


@gpu
@pytest.mark.parametrize("column", ["img", "strength"])
@_releasing
def test_region_adjacency_at_its_guard(world, column):
    """gcs_region_adjacency at B_GUARD = 55 346, the largest B it accepts for the shape (B H W < 2^31), on maps of 12 labels, E_cap =
    66, once with img (contrast) and once with a strength plane, so that each fits: labels int32 (and the strength plane) cross
    bytes 2^31 and 2^32, img bytes 2^31 and 2^32; no element index reaches 2^31 - the guard's point. One image more is refused,
    nothing launched. Small == tests/region_adjacency_ref.py."""
    import region_adjacency_ref as ra
    w, torch = world, world.torch
    b, k = lm.B_GUARD, K_ADJ
    assert b * P < 1 << 31 <= (b + 1) * P
    _, idx = w.idx(b)
    lab_np, lab = _adjacency_labels(w)
    plane_np = np.random.default_rng(66).integers(-500, 1 << 20, (N_BASE, H, W)).astype(np.int32)
    s_img = w.img if column == "img" else None
    s_plane = w.dev(plane_np) if column == "strength" else None

    def run(nb, labels, img, plane, expect_refusal=False):
        ws = lm.filled(torch, (w.lib.gcs_region_adjacency_workspace_bytes(nb, E_CAP),), torch.uint8, 0xA5)
        edges, vals = lm.filled(torch, (nb, E_CAP, 2), torch.int32, -7), lm.filled(torch, (nb, E_CAP, 3), torch.int64, -3)
        count = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
        args = (labels, img, plane, nb, H, W, k, E_CAP, ws, edges, vals, count)
        if expect_refusal:
            assert w.refused("gcs_region_adjacency", *args[:3], nb + 1, *args[4:])
            assert bool((count == -7).all()) and bool((edges[:4] == -7).all())
            return None
        w.call("gcs_region_adjacency", *args)
        return edges, vals, count

    small = run(N_BASE, lab, s_img, s_plane)
    for j in range(N_BASE):
        e, v = ra.leaf_graph(lab_np[j], k, img=w.img_np[j] if column == "img" else None, plane=plane_np[j] if column == "strength" else None)
        we, wv, wc = ra.table(e, v, E_CAP)
        assert int(small[2][j]) == wc > 20 and np.array_equal(small[0][j].cpu().numpy(), we), j
        assert np.array_equal(small[1][j].cpu().numpy().view(np.uint64), wv) and wv[:, 1 if column == "img" else 2].max() > 0, j
    labels = lm.replicate(torch, lab, idx)
    img = lm.replicate(torch, w.img, idx) if column == "img" else None
    plane = lm.replicate(torch, s_plane, idx) if column == "strength" else None
    big = run(b, labels, img, plane)
    for what, got, s in zip(("edges", "vals", "count"), big, small):
        _same(w, got, s, idx, (column, what))
    run(b, labels, img, plane, expect_refusal=True)


@gpu
@_releasing
def test_cut_shapes_at_its_guard(world):
    """gcs_cut_shapes at B_GUARD = 55 346 (B H W < 2^31), K = 48, cuts at R = 6 and 3: labels and contours, int32, cross bytes 2^31
    and 2^32, no element index reaches 2^31. One image more is refused, nothing launched. The contour maps are the small ones
    through idx (test_contours_and_sweep holds gcs_region_tree_contours itself). Small == tests/cut_metrics_ref.py."""
    import cut_metrics_ref as cmr
    w, torch = world, world.torch
    b, k, regions = lm.B_GUARD, K_LABELS, [6, 3]
    n = len(regions)
    _, idx = w.idx(b)
    merges, alive, m_np, a_np = w.tree()
    s_u, u_np = w.contours()
    regions_dev = w.dev(np.array(regions, np.int32))

    def run(nb, labels, u, mg, al, expect_refusal=False):
        need = w.lib.gcs_cut_shapes_workspace_bytes(nb, k, n)
        assert need > 0
        ws = lm.filled(torch, (need,), torch.uint8, 0xA5)
        area, perim = lm.filled(torch, (n, nb, k), torch.int32, -7), lm.filled(torch, (n, nb, k), torch.int32, -7)
        bd = torch.full((n, nb), -7, dtype=torch.int32, device="cuda")
        args = (labels, u, mg, al, regions_dev, nb, H, W, k, n, ws, area, perim, bd)
        if expect_refusal:
            assert w.refused("gcs_cut_shapes", *args[:5], nb + 1, *args[6:])
            assert bool((bd == -7).all())
            return None
        w.call("gcs_cut_shapes", *args)
        return area, perim, bd

    small = run(N_BASE, w.lab, s_u, merges, alive)
    for j in range(N_BASE):
        wa, wp_, wb = cmr.shapes(w.lab_np[j], u_np[j], m_np[j], int(a_np[j]), regions, k)
        assert np.array_equal(small[0][:, j].cpu().numpy().view(np.uint32), wa), j
        assert np.array_equal(small[1][:, j].cpu().numpy().view(np.uint32), wp_), j
        assert np.array_equal(small[2][:, j].cpu().numpy().view(np.uint32), wb), j
    labels, u = lm.replicate(torch, w.lab, idx), lm.replicate(torch, s_u, idx)
    mg, al = merges[idx], alive[idx]
    big = run(b, labels, u, mg, al)
    for c in range(n):
        _same(w, big[0][c], small[0][c], idx, ("area", c))
        _same(w, big[1][c], small[1][c], idx, ("perim", c))
        _equal(w, big[2][c], small[2][c][idx], ("boundary", c))
    run(b, labels, u, mg, al, expect_refusal=True)


# ------------------------------------------------------------------------------------------------------------ part 2: canonical
SP_GRID, SP_LAMBDA, SP_ITER = (5, 7), 576, 2


@gpu
@_releasing
def test_canonical_tensor(world):
    """On the canonical batch, uint16 [B][D][H][W] with B = 1 539, D = 72 (2^32 + 2^21 elements, 8.6 GB: element 2^31 = byte 2^32
    and element 2^32 = byte 2^33 inside, byte 2^31 too; the label maps, 239 MB, cross nothing), built by replication of sixteen
    base tensors over SPEC.md §3's value range - never by gcs_features_unpack: gcs_superpixel_segment (5 x 7 centres, two passes,
    with centres_out), gcs_region_tree (K = 48) and gcs_region_props (D = 72, with img: B K (6 + D) = 5.8 M). Small ==
    tests/superpixel_ref.py, tests/region_tree_ref.py, tests/region_props_ref.py."""
    import region_props_ref as rp
    import region_tree_ref as rt
    import superpixel_raw
    import superpixel_ref as sp
    w, torch = world, world.torch
    b, d, k = lm.N_CANON, lm.D_CANON, K_LABELS
    ny, nx = SP_GRID
    kk = ny * nx
    assert b * d * P >= lm.LINE32 + lm.MARGIN and b * k * (6 + d) < 1 << 31
    _, idx = w.idx(b)
    x_np = lm.base_canonical()
    s_x = w.dev(x_np)

    def run(nb, x, labels, img):
        out = {}
        need = w.lib.gcs_superpixel_workspace_bytes(nb, H, W, d, superpixel_raw.workspace_n(H, W, kk))
        assert need > 0
        ws = lm.filled(torch, (need,), torch.uint8, 0xA5)
        out["sp labels"] = lm.filled(torch, (nb, H, W), torch.int32, -7)
        out["sp centres"] = lm.filled(torch, (nb, kk, d + 2), torch.int32, -7)
        w.call("gcs_superpixel_segment", x, nb, H, W, d, ny, nx, SP_LAMBDA, SP_ITER, ws, out["sp labels"], out["sp centres"])
        ws = lm.filled(torch, (w.lib.gcs_region_tree_workspace_bytes(nb, H, W, d, k),), torch.uint8, 0xA5)
        out["merges"], out["costs"] = lm.filled(torch, (nb, k - 1, 2), torch.int32, 7), lm.filled(torch, (nb, k - 1), torch.int64, 7)
        out["alive"] = torch.full((nb,), -5, dtype=torch.int32, device="cuda")
        w.call("gcs_region_tree", x, labels, nb, H, W, d, k, ws, out["merges"], out["costs"], out["alive"])
        out["sums"], out["bbox"] = lm.filled(torch, (nb, k, 6 + d), torch.int64, -3), lm.filled(torch, (nb, k, 4), torch.int32, -7)
        w.call("gcs_region_props", labels, img, x, nb, H, W, d, k, out["sums"], out["bbox"])
        return out

    small = run(N_BASE, s_x, w.lab, w.img)
    host = {key: v.cpu().numpy() for key, v in small.items()}
    for j in range(N_BASE):
        lab_ref, cent_ref = sp.superpixels_on_grid(x_np[j], ny, nx, lam=SP_LAMBDA, n_iter=SP_ITER, return_centres=True)
        assert np.array_equal(host["sp labels"][j], lab_ref) and np.array_equal(host["sp centres"][j], cent_ref), j
        rm, rc, ra = rt.build_tree(x_np[j], w.lab_np[j], k)
        assert int(host["alive"][j]) == ra and np.array_equal(host["merges"][j], rm), j
        assert np.array_equal(host["costs"][j].view(np.uint64), rc), j
        ws_, wb_ = rp.leaf_table(w.lab_np[j], k, img=w.img_np[j], feats=x_np[j], d=d)
        assert np.array_equal(host["sums"][j].view(np.uint64), ws_) and np.array_equal(host["bbox"][j], wb_), j
    assert x_np.max() >= 32768 and len(np.unique(host["sp labels"])) == kk
    x = lm.replicate(torch, s_x, idx)
    assert x.numel() >= lm.LINE32 + lm.MARGIN
    big = run(b, x, lm.replicate(torch, w.lab, idx), lm.replicate(torch, w.img, idx))
    for key, got in big.items():
        _same(w, got, small[key], idx, key)


# ------------------------------------------------------------------------------------------------------------ part 3: tables
H3, W3 = 13, 11                     # tiny maps: the tables are what is large here
P3 = H3 * W3


def _tiny(w, k, n_truth, seed):
    """Sixteen tiny label maps in 0 .. k-1, annotator maps in 0 .. n_truth-1 and images: host arrays and device copies."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, (N_BASE, -(-H3 // 2), -(-W3 // 2))).repeat(2, axis=1).repeat(2, axis=2)[:, :H3, :W3].astype(np.int32)
    lab[:, 0, 0], lab[:, H3 - 1, W3 - 1] = 0, k - 1
    truth = rng.integers(0, n_truth, (N_BASE, -(-H3 // 3), -(-W3 // 3))).repeat(3, axis=1).repeat(3, axis=2)[:, :H3, :W3].astype(np.uint16)
    truth[:, 0, 0] = n_truth - 1
    img = rng.integers(0, 256, (N_BASE, H3, W3, 3)).astype(np.uint8)
    assert len({m.tobytes() for m in lab}) == N_BASE and len({m.tobytes() for m in truth}) == N_BASE
    lab, truth, img = (np.ascontiguousarray(a) for a in (lab, truth, img))
    return lab, truth, img, w.dev(lab), w.dev(truth), w.dev(img)


def _tiny_tree(w, lab_np, lab, k, seed):
    """gcs_region_tree of the tiny maps on three features == tests/region_tree_ref.py -> (merges, alive) device and host."""
    import region_tree_ref as rt
    torch, d = w.torch, 3
    x_np = np.random.default_rng(seed).integers(0, 46340, (N_BASE, d, H3, W3)).astype(np.uint16)
    ws = torch.empty(w.lib.gcs_region_tree_workspace_bytes(N_BASE, H3, W3, d, k), dtype=torch.uint8, device="cuda")
    merges = torch.full((N_BASE, k - 1, 2), 7, dtype=torch.int32, device="cuda")
    alive = torch.full((N_BASE,), -5, dtype=torch.int32, device="cuda")
    w.call("gcs_region_tree", w.dev(x_np), lab, N_BASE, H3, W3, d, k, ws, merges, None, alive)
    m_np, a_np = merges.cpu().numpy(), alive.cpu().numpy()
    for j in range(N_BASE):
        rm, _, ra = rt.build_tree(x_np[j], lab_np[j], k)
        assert int(a_np[j]) == ra and np.array_equal(m_np[j], rm), j
    return merges, alive, m_np, a_np


def _bits(t):
    """A float64 tensor as its bits: equality then means the same bits (the library promises them)."""
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _close(got, want, what):
    err = np.abs(got - want)
    assert (err <= 1e-11 * np.maximum(np.abs(want), 1.0)).all(), (what, float(err.max()))


@gpu
@_releasing
def test_tables_at_two_to_the_thirty(world):
    """gcs_region_counts_batch (and _u8) -> gcs_region_reduce -> gcs_region_agreement at T * n_segments * n_truth_labels = 2^30
    exactly (T = B = 16 384 maps of 13 x 11, 256 x 256 tables): the accepted side of the scoring tables' guard. hist_dev, uint32, is
    4 GiB: element 2^30 = byte 2^32 is its END (its last element ends there), byte 2^31 lies inside, rows t >= 8 192 start at or past
    it. Small (T = 16) == NumPy (tests/scoring_edge.py; the agreement of tests/test_gpu_buffer_contracts.py: integer sums exact, float
    terms within 1e-11 relative - at most 143 non-zero terms a sum); the large tables, sums and terms == the small ones through idx,
    the float terms bit for bit (the header promises the same bits for the same maps)."""
    import test_gpu_buffer_contracts as bc
    from scoring_edge import _np_reduce, _np_tables_batch
    w, torch = world, world.torch
    t, n_seg, n_truth = 1 << 14, 256, 256
    assert t * n_seg * n_truth == 1 << 30 and t * n_seg * n_truth * 4 == lm.LINE32
    _, idx = w.idx(t)
    lab_np, truth_np, _, lab, truth, _ = _tiny(w, n_seg, n_truth, seed=30)

    def run(nt, labels, maps):
        img_of, first = torch.arange(nt, dtype=torch.int32, device="cuda"), torch.arange(nt + 1, dtype=torch.int32, device="cuda")
        out = {}
        hist = lm.filled(torch, (nt, n_seg, n_truth), torch.int32, 0x25)
        area, perim = lm.filled(torch, (nt, n_seg), torch.int32, 0x25), lm.filled(torch, (nt, n_seg), torch.int32, 0x25)
        w.call("gcs_region_counts_batch_u8", labels, maps.to(torch.uint8), first, nt, nt, 1, H3, W3, n_seg, n_truth, hist, area, perim)
        out["hist u8 (its first and last rows)"] = torch.cat([hist[:64], hist[-64:]]).clone()
        for i in range(0, nt, lm.chunk_of(n_seg * n_truth)):
            hist[i:i + lm.chunk_of(n_seg * n_truth)].fill_(0x25)
        w.call("gcs_region_counts_batch", labels, maps, first, nt, nt, 1, H3, W3, n_seg, n_truth, hist, area, perim)
        out.update(hist=hist, area=area, perim=perim)
        out["under"], out["under_np"] = lm.filled(torch, (nt,), torch.int64, -3), lm.filled(torch, (nt,), torch.int64, -3)
        w.call("gcs_region_reduce", hist, area, img_of, nt, n_seg, n_truth, out["under"], out["under_np"])
        scratch = lm.filled(torch, (w.lib.gcs_region_agreement_scratch_bytes(nt, n_seg, n_truth),), torch.uint8, 0xA5)
        out["sums"], out["terms"] = lm.filled(torch, (nt, 4), torch.int64, -3), lm.filled(torch, (nt, 4), torch.float64, -3.0)
        w.call("gcs_region_agreement", hist, img_of, None, nt, n_seg, n_truth, scratch, out["sums"], out["terms"])
        return out

    small = run(N_BASE, lab, truth)
    want_t = _np_tables_batch(lab_np, truth_np, np.arange(N_BASE + 1), n_seg, n_truth)
    want_u = _np_reduce(want_t[0], want_t[1], np.arange(N_BASE))
    want_s, want_f = bc._agreement(want_t[0])
    for i, key in enumerate(("hist", "area", "perim")):
        assert np.array_equal(small[key].cpu().numpy(), want_t[i]), key
    assert np.array_equal(small["hist u8 (its first and last rows)"].cpu().numpy(), np.concatenate([want_t[0], want_t[0]])), "u8"
    assert np.array_equal(small["under"].cpu().numpy(), want_u[0]) and np.array_equal(small["under_np"].cpu().numpy(), want_u[1])
    assert np.array_equal(small["sums"].cpu().numpy().view(np.uint64), want_s)
    _close(small["terms"].cpu().numpy(), want_f, "agreement terms")
    assert (want_s[:, 0] == P3).all()
    big = run(t, lm.replicate(torch, lab, idx), lm.replicate(torch, truth, idx))
    assert big["hist"].numel() * 4 == lm.LINE32
    for key in ("hist", "area", "perim", "under", "under_np", "sums", "terms"):
        _same(w, _bits(big[key]), _bits(small[key]), idx, key)
    rows = torch.cat([idx[:64], idx[-64:]])
    _equal(w, big["hist u8 (its first and last rows)"], small["hist"][rows], "gcs_region_counts_batch_u8")


K_SWEEP, TRUTH_SWEEP, T_SWEEP = 128, 32, ((1 << 31) - 1) // (128 * 32)
REGIONS_SWEEP = [20, 5]


@gpu
@pytest.mark.parametrize("entry", ["gcs_region_sweep", "gcs_region_sweep_under"])
@_releasing
def test_sweeps_below_their_guard(world, entry):
    """gcs_region_sweep / gcs_region_sweep_under (with sums and terms) at T * K * n_truth_labels = 2 147 479 552, the largest multiple
    of K * n_truth_labels = 4096 below 2^31 (T = 524 287 maps over B = 16 trees of K = 128 leaves, 32 annotator labels, cuts at R =
    20 and 5): leaf_hist_dev, uint32, is 8.0 GiB - element 2^30 (byte 2^32) and byte 2^31 inside, just short of element 2^31 (byte
    2^33), the guard's point. Small (T = 16; the leaf tables from gcs_region_counts_batch == region_sweep_ref.leaf_table) ==
    tests/region_sweep_ref.py and tests/cut_metrics_ref.py (integer sums exact, float terms within 1e-11 relative); the large
    outputs == the small ones through idx, floats bit for bit, and so is the consumed leaf table (the table of the last cut)."""
    import cut_metrics_ref as cmr
    import region_sweep_ref as rs
    w, torch = world, world.torch
    k, n_truth, t, regions = K_SWEEP, TRUTH_SWEEP, T_SWEEP, REGIONS_SWEEP
    n = len(regions)
    assert (t + 1) * k * n_truth >= 1 << 31 > t * k * n_truth and t <= 1000000
    idx_np, idx = w.idx(t)
    lab_np, truth_np, _, lab, truth, _ = _tiny(w, k, n_truth, seed=31)
    merges, alive, m_np, a_np = _tiny_tree(w, lab_np, lab, k, seed=32)
    assert a_np.min() > regions[0]
    regions_dev = w.dev(np.array(regions, np.int32))
    leaf = torch.full((N_BASE, k, n_truth), 0x25, dtype=torch.int32, device="cuda")
    area, perim = torch.empty((N_BASE, k), dtype=torch.int32, device="cuda"), torch.empty((N_BASE, k), dtype=torch.int32, device="cuda")
    w.call("gcs_region_counts_batch", lab, truth, torch.arange(N_BASE + 1, dtype=torch.int32, device="cuda"), N_BASE, N_BASE, 1, H3, W3,
           k, n_truth, leaf, area, perim)
    for j in range(N_BASE):
        assert np.array_equal(leaf[j].cpu().numpy(), rs.leaf_table(lab_np[j], truth_np[j], k, n_truth)), j

    def run(nt, table, img_of):
        out = {"leaf": table}
        sizer = getattr(w.lib, entry + "_workspace_bytes")
        ws = lm.filled(torch, (sizer(nt, k, n_truth, n),), torch.uint8, 0xA5)
        out["sums"], out["terms"] = lm.filled(torch, (n, nt, 4), torch.int64, -3), lm.filled(torch, (n, nt, 4), torch.float64, -3.0)
        head = (table, merges, alive, img_of, regions_dev, N_BASE, nt, k, n_truth, n, ws)
        if entry == "gcs_region_sweep":
            w.call("gcs_region_sweep", *head, out["sums"], out["terms"])
        else:
            out["under"] = lm.filled(torch, (n, nt, 3), torch.int64, -3)
            w.call("gcs_region_sweep_under", *head, out["under"], out["sums"], out["terms"])
        return out

    small = run(N_BASE, leaf.clone(), torch.arange(N_BASE, dtype=torch.int32, device="cuda"))
    for j in range(N_BASE):
        ws_, wt_ = rs.sweep(lab_np[j], m_np[j], int(a_np[j]), truth_np[j:j + 1], regions, k, n_truth)
        assert np.array_equal(small["sums"][:, j].cpu().numpy().view(np.uint64), ws_[:, 0]), j
        _close(small["terms"][:, j].cpu().numpy(), wt_[:, 0], ("terms", j))
        last = rs.cut_table(rs.leaf_table(lab_np[j], truth_np[j], k, n_truth), m_np[j], cmr.tau_of(int(a_np[j]), regions[-1], k))
        assert np.array_equal(small["leaf"][j].cpu().numpy(), last), j
        if "under" in small:
            wu_ = cmr.under_counts(lab_np[j], m_np[j], int(a_np[j]), truth_np[j:j + 1], regions, k, n_truth)
            assert np.array_equal(small["under"][:, j].cpu().numpy().view(np.uint64), wu_[:, 0]), j
    table = lm.replicate(torch, leaf, idx)
    assert table.numel() == t * k * n_truth and lm.LINE32 < table.numel() * 4 < lm.LINE33
    big = run(t, table, idx.to(torch.int32))
    _same(w, big["leaf"], small["leaf"], idx, "the consumed leaf table")
    for key in [key for key in big if key != "leaf"]:
        for c in range(n):
            _same(w, _bits(big[key][c]), _bits(small[key][c]), idx, (key, c))


K_CUTS, D_CUTS, B_CUTS = 153, 207, 65535
C_CUTS = 6 + D_CUTS


@gpu
@_releasing
def test_props_cuts_and_paint_below_their_guard(world):
    """gcs_region_props_cuts and gcs_region_paint at B * K * C = 65 535 * 153 * 213 = 2 135 720 115 < 2^31 (K = 154 would pass it) on
    13 x 11 maps: the leaf table sums_dev, uint64, is 15.9 GiB - bytes 2^31, 2^32 and 2^33 and element 2^30 inside, just short of
    element 2^31 (byte 2^34). One cut at R = 3 (Rsum = 3), so that the outputs stay small. Small (B = 16; the leaf tables from
    gcs_region_props at D = 207 == region_props_ref.leaf_table) == tests/region_props_ref.py (cut_tables_by_rows, paint); the large
    group, sums and box tables and the painted pictures == the small ones through idx."""
    import region_props_ref as rp
    w, torch = world, world.torch
    b, k, c, d, regions = B_CUTS, K_CUTS, C_CUTS, D_CUTS, [3]
    assert b * k * c < 1 << 31 <= b * (k + 1) * c and b * k * c * 8 > lm.LINE33
    _, idx = w.idx(b)
    lab_np, _, img_np, lab, _, img = _tiny(w, k, 4, seed=33)
    x_np = np.random.default_rng(34).integers(0, 46340, (N_BASE, d, H3, W3)).astype(np.uint16)
    merges, alive, m_np, a_np = _tiny_tree(w, lab_np, lab, k, seed=35)
    regions_dev = w.dev(np.array(regions, np.int32))
    leaf_s, leaf_b = torch.full((N_BASE, k, c), -3, dtype=torch.int64, device="cuda"), torch.full((N_BASE, k, 4), -7, dtype=torch.int32, device="cuda")
    w.call("gcs_region_props", lab, img, w.dev(x_np), N_BASE, H3, W3, d, k, leaf_s, leaf_b)
    want_leaf = [rp.leaf_table(lab_np[j], k, img=img_np[j], feats=x_np[j], d=d) for j in range(N_BASE)]
    for j in range(N_BASE):
        assert np.array_equal(leaf_s[j].cpu().numpy().view(np.uint64), want_leaf[j][0]) and np.array_equal(leaf_b[j].cpu().numpy(), want_leaf[j][1]), j

    def run(nb, sums, bbox, mg, al, labels):
        out = {"group": lm.filled(torch, (1, nb, k), torch.int32, -7), "sums": lm.filled(torch, (nb, 3, c), torch.int64, -3),
               "bbox": lm.filled(torch, (nb, 3, 4), torch.int32, -7), "rgb": lm.filled(torch, (nb, H3, W3, 3), torch.uint8, 0xA5)}
        w.call("gcs_region_props_cuts", sums, bbox, mg, al, regions_dev, nb, H3, W3, k, c, 1, 3, out["group"], out["sums"], out["bbox"])
        w.call("gcs_region_paint", labels, None, sums, nb, H3, W3, k, k, c, k, out["rgb"])
        return out

    small = run(N_BASE, leaf_s, leaf_b, merges, alive, lab)
    for j in range(N_BASE):
        wg, ws_, wb_, _ = rp.cut_tables_by_rows(want_leaf[j][0], want_leaf[j][1], m_np[j], int(a_np[j]), regions, (H3, W3))
        assert np.array_equal(small["group"][0, j].cpu().numpy(), wg[0]), j
        assert np.array_equal(small["sums"][j].cpu().numpy().view(np.uint64), ws_) and np.array_equal(small["bbox"][j].cpu().numpy(), wb_), j
        assert np.array_equal(small["rgb"][j].cpu().numpy(), rp.paint(lab_np[j], want_leaf[j][0])), j
    assert small["rgb"].max() > 0
    sums = lm.replicate(torch, leaf_s, idx)
    assert sums.numel() == b * k * c
    big = run(b, sums, lm.replicate(torch, leaf_b, idx), merges[idx], alive[idx], lm.replicate(torch, lab, idx))
    _same(w, big["group"][0], small["group"][0], idx, "group")
    for key in ("sums", "bbox", "rgb"):
        _same(w, big[key], small[key], idx, key)
