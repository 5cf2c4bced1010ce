"""Raw caller of gcs_superpixel_segment for the tests (a helper, not a test module): hand-made features on a caller's grid, every
buffer the call writes starting out as 0xAB bytes, 256 guard bytes around the workspace, the labels and the centres, the feature
tensor compared with what went in. The launches sit on torch's current stream."""
import ctypes as C
import functools

import numpy as np

GUARD = 256
FILL = 0xAB


@functools.lru_cache(maxsize=None)
def workspace_n(h, w, k):
    """An ``n`` for gcs_superpixel_workspace_bytes whose own grid (gcs_superpixel_grid on the host) has at least k centres and at most
    4096: the grid with the fewest such centres, and of the n that give it the largest. The call lays the workspace out by its own K
    (include/gcs.h), so any such n is enough; the fewest centres put the guard bytes closest behind what the call uses."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    best = None
    for n in range(2, 4097):
        ny, nx = C.c_int(), C.c_int()
        assert lib.gcs_superpixel_grid(h, w, n, None, C.byref(ny), C.byref(nx)) == 0
        kk = ny.value * nx.value
        if k <= kk <= 4096 and (best is None or kk <= best[0]):
            best = (kk, n)
    assert best is not None, (h, w, k)
    return best[1]


def _guarded(torch, nbytes):
    """(whole uint8 tensor of 0xAB bytes, address of its payload): GUARD bytes, nbytes of payload, GUARD bytes."""
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + GUARD


def _payload(buf, nbytes, what):
    """The payload of a guarded buffer as host bytes, after checking that both guards still hold 0xAB."""
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all(), f"{what}: bytes in front of the buffer were written"
    assert (host[GUARD + nbytes:] == FILL).all(), f"{what}: bytes behind the buffer were written"
    return host[GUARD:GUARD + nbytes]


def run(torch, x, ny, nx, lam, n_iter, centres=True):
    """x (B, D, H, W) uint16 values -> (labels int32 (B, H, W), centres int32 (B, K, D + 2)) as host arrays. With ``centres=False`` the
    call gets centres_out = NULL and the second value is None: the centres buffer is still there, and must keep its 0xAB bytes."""
    from gabor_color_image_segmentation_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(np.asarray(x).astype(np.uint16))
    b, d, h, w = x.shape
    k = ny * nx
    xs = torch.from_numpy(x.view(np.int16)).cuda()
    need = lib.gcs_superpixel_workspace_bytes(b, h, w, d, workspace_n(h, w, k))
    assert need > 0
    lab_bytes, cen_bytes = b * h * w * 4, b * k * (d + 2) * 4
    ws, ws_ptr = _guarded(torch, need)
    lab, lab_ptr = _guarded(torch, lab_bytes)
    cen, cen_ptr = _guarded(torch, cen_bytes)
    rc = lib.gcs_superpixel_segment(xs.data_ptr(), b, h, w, d, ny, nx, lam, n_iter, ws_ptr, lab_ptr, cen_ptr if centres else None,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gcs_last_error()
    torch.cuda.current_stream().synchronize()
    assert np.array_equal(xs.cpu().numpy().view(np.uint16), x), "the feature tensor was written"
    _payload(ws, need, "workspace")
    labels = _payload(lab, lab_bytes, "labels").view(np.int32).reshape(b, h, w).copy()
    cen_host = _payload(cen, cen_bytes, "centres")
    if not centres:
        assert (cen_host == FILL).all(), "centres_out = NULL, yet the centres buffer was written"
        return labels, None
    return labels, cen_host.view(np.int32).reshape(b, k, d + 2).copy()
