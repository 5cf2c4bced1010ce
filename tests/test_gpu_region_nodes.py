"""gcs_region_nodes (SPEC.md §18) through the raw entry point against tests/component_tree_ref.py, bit for bit: every buffer the call
writes starts out as 0xAB bytes, 256 guard bytes lie around the scratch and the three outputs (as tests/superpixel_raw.py keeps
them), the label map is compared with what went in. Then the argument rules, with nothing written."""
import numpy as np
import pytest

import component_tree_ref as ct
from superpixel_raw import FILL, _guarded, _payload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _run(torch, labs, m, k_cap, used=True):
    """labs (B, H, W) -> (nodes int32 (B, H, W), n_nodes (B,), min_size_used (B,) or None) as host arrays."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    labs = np.ascontiguousarray(labs, dtype=np.int32)
    b, h, w = labs.shape
    src = torch.from_numpy(labs).cuda()
    need = lib.gcs_region_nodes_scratch_bytes(b, h, w)
    assert need >= 20 * b * h * w
    ws, ws_ptr = _guarded(torch, need)
    out, out_ptr = _guarded(torch, b * h * w * 4)
    cnt, cnt_ptr = _guarded(torch, b * 4)
    use, use_ptr = _guarded(torch, b * 4)
    rc = lib.gcs_region_nodes(src.data_ptr(), b, h, w, m, k_cap, ws_ptr, out_ptr, cnt_ptr, use_ptr if used else None,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(src.cpu().numpy(), labs), "the label map was written"
    _payload(ws, need, "scratch")
    nodes = _payload(out, b * h * w * 4, "nodes").view(np.int32).reshape(b, h, w).copy()
    n_nodes = _payload(cnt, b * 4, "n_nodes").view(np.int32).copy()
    use_host = _payload(use, b * 4, "min_size_used")
    if not used:
        assert (use_host == FILL).all(), "min_size_used = NULL, yet its buffer was written"
        return nodes, n_nodes, None
    return nodes, n_nodes, use_host.view(np.int32).copy()


def _check(torch, labs, m, k_cap, want_used=None):
    labs = np.asarray(labs)
    nodes, n_nodes, used = _run(torch, labs, m, k_cap)
    for i, lab in enumerate(labs):
        info = {}
        want = ct.nodes(lab, m, k_cap, info)
        assert np.array_equal(nodes[i], want), (i, int((nodes[i] != want).sum()))
        assert (int(n_nodes[i]), int(used[i])) == (info["nodes"], info["min_size"]), (i, n_nodes[i], used[i], info)
        assert n_nodes[i] <= k_cap
    if want_used is not None:
        assert used.tolist() == want_used
    again = _run(torch, labs, m, k_cap, used=False)
    assert np.array_equal(again[0], nodes) and np.array_equal(again[1], n_nodes)
    return nodes, n_nodes


def _two_pieces():
    lab = np.zeros((8, 8), np.int32)
    lab[:, 3:5] = 1                                      # label 0 lies left and right of the bar
    lab[6:, 3:5] = 2
    lab[0, 7] = 3                                        # one pixel
    return lab


def _one_pixel(h, w):
    """h x w labels of which no two 4-neighbours are equal, from four values only: every pixel is a component."""
    y, x = np.mgrid[0:h, 0:w]
    return ((y & 1) * 2 + (x & 1)).astype(np.int32)


def test_a_label_in_two_pieces_8x8(torch_cuda):
    nodes, n_nodes = _check(torch_cuda, _two_pieces()[None], 0, 4096, [0])
    assert n_nodes[0] == 5 and nodes[0, 0, 0] != nodes[0, 0, 5]
    _check(torch_cuda, _two_pieces()[None], 1, 4096, [1])


def test_one_pixel_labels_at_the_cap_and_one_row_more(torch_cuda):
    """64 x 64: C = 4096 = k_cap, no guard, every pixel a node. 65 x 64: C = 4160, the guard takes m = ceil(4160 / 4096) = 2."""
    nodes, n_nodes = _check(torch_cuda, _one_pixel(64, 64)[None], 0, 4096, [0])
    assert n_nodes[0] == 4096 and np.array_equal(nodes[0].ravel(), np.arange(4096))
    nodes, n_nodes = _check(torch_cuda, _one_pixel(65, 64)[None], 0, 4096, [2])
    assert n_nodes[0] <= 4096 and np.bincount(nodes[0].ravel()).min() >= 2


def test_the_decision_is_per_image(torch_cuda):
    """One batch: an image above the cap between two that are not (65 x 64, so 64 x 64 of one-pixel labels in a constant frame row)."""
    calm = np.zeros((65, 64), np.int32)
    calm[20:30, 10:50] = 1
    calm[22, 12] = 0                                     # a one-pixel piece of label 0: stays a node where m_b = 0
    capped = np.full((65, 64), 7, np.int32)
    capped[:64] = _one_pixel(64, 64)                     # C = 4096 + 1 > k_cap
    batch = np.stack([calm, _one_pixel(65, 64), capped, calm.T.copy().reshape(65, 64)])
    nodes, n_nodes = _check(torch_cuda, batch, 0, 4096, [0, 2, 2, 0])
    assert n_nodes[0] == 3
    _check(torch_cuda, batch, 5, 4096, [5, 5, 5, 5])
    _check(torch_cuda, batch, 1, 4096, [1, 2, 2, 1])


def test_small_cap_on_8x8(torch_cuda):
    """k_cap = 5: the guard without large maps (m_guard = ceil(64 / 5) = 13); k_cap = 6 leaves the five components alone."""
    rng = np.random.default_rng(5)
    noisy = rng.integers(0, 3, size=(8, 8)).astype(np.int32)
    _check(torch_cuda, np.stack([_two_pieces(), noisy, _one_pixel(8, 8)]), 0, 5, [0, 13, 13])
    _check(torch_cuda, np.stack([_two_pieces(), noisy]), 0, 6)
    _check(torch_cuda, np.stack([_two_pieces(), noisy]), 0, 1)                      # m_guard = 64: one node


def test_min_size_5_with_and_without_the_guard(torch_cuda):
    rng = np.random.default_rng(11)
    coarse = rng.integers(0, 4, size=(13, 10)).repeat(3, axis=0).repeat(3, axis=1)[:37, :29].astype(np.int32)
    noisy = coarse.copy()
    flip = rng.random(noisy.shape) < 0.2
    noisy[flip] = rng.integers(0, 4, size=int(flip.sum()))
    batch = np.stack([coarse, noisy])
    _check(torch_cuda, batch, 5, 4096, [5, 5])                                      # no guard: 37 * 29 < 4096
    _check(torch_cuda, batch, 5, 100, None)                                         # m_guard = ceil(1073 / 100) = 11 where C > 100
    _check(torch_cuda, batch, 5, 400, None)                                         # m_guard = 3 < 5: min_size stays
    _check(torch_cuda, batch, 40, 100, None)


def test_one_row_and_one_column(torch_cuda):
    rng = np.random.default_rng(3)
    row = rng.integers(0, 3, size=(2, 1, 301)).astype(np.int32)
    for m, k_cap in ((0, 4096), (3, 4096), (0, 50), (0, 1)):
        _check(torch_cuda, row, m, k_cap)
        _check(torch_cuda, row.reshape(2, 301, 1), m, k_cap)


def test_raw_entry_point_refuses_what_is_outside_the_domain(torch_cuda):
    """GCS_EINVAL (1) with nothing launched: every buffer keeps its bytes."""
    torch = torch_cuda
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    b, h, w = 2, 16, 16
    lab = torch.zeros((b, h, w), dtype=torch.int32, device="cuda")
    ws = torch.full((lib.gcs_region_nodes_scratch_bytes(b, h, w),), FILL, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * b * h * w * 4,), FILL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((b * 4,), FILL, dtype=torch.uint8, device="cuda")
    use = torch.full((b * 4,), FILL, dtype=torch.uint8, device="cuda")
    good = dict(lab=lab.data_ptr(), B=b, H=h, W=w, m=0, k=4096, ws=ws.data_ptr(), out=out.data_ptr(), cnt=cnt.data_ptr(),
                use=use.data_ptr())
    st = torch.cuda.current_stream().cuda_stream

    def call(a):
        return lib.gcs_region_nodes(a["lab"], a["B"], a["H"], a["W"], a["m"], a["k"], a["ws"], a["out"], a["cnt"], a["use"], st)
    for bad in (dict(lab=None), dict(ws=None), dict(out=None), dict(cnt=None), dict(B=0), dict(B=65536), dict(H=0), dict(H=4097),
                dict(W=0), dict(W=4097), dict(m=-1), dict(k=0), dict(k=4097),
                dict(out=lab.data_ptr()), dict(out=lab.data_ptr() + 4), dict(out=lab.data_ptr() + b * h * w * 4 - 4),
                dict(lab=out.data_ptr() + 4)):
        assert call(dict(good, **bad)) == 1, bad
        assert lib.gcs_last_error()
    for args in ((0, 16, 16), (65536, 16, 16), (1, 0, 16), (1, 16, 4097)):
        assert lib.gcs_region_nodes_scratch_bytes(*args) == 0
    torch.cuda.current_stream().synchronize()
    assert all(bool((t == FILL).all()) for t in (ws, out, cnt, use)) and not bool(lab.any())
    assert call(dict(good, use=None)) == 0               # min_size_used may be NULL; out right behind labels does not overlap
    torch.cuda.current_stream().synchronize()
    assert bool((use == FILL).all()) and bool((out[b * h * w * 4:] == FILL).all())
    assert out[:b * h * w * 4].view(torch.int32).any().item() is False and cnt.view(torch.int32).tolist() == [1, 1]
