"""White box of the workspace of gcs_kmeans_pass_fused (csrc/kmeans.hip: fold_rows, fused_sum_bytes, fused_cent_bytes; GcsFold in
csrc/common.h), written once for every test that looks inside it, and a plain model of what one pass does to it.

    [sum buffer 0][sum buffer 1][sum buffer 2][centroid array 0][centroid array 1][ticket: 256 bytes]

every piece a multiple of 256 bytes. A sum buffer is [n_sets][rows][k * (D + 1)] uint64: element [j * (D + 1) + e] of a row is the
sum of logical feature e over the pixels of cluster j, e == D their count. A centroid array is [n_sets][k][D] uint16. ``rows`` is 1,
except under GCS_KP_FOLD_ROWS = v (1 .. 64) with ONE global codebook: min(B * parts, v); a workgroup adds into row
(its index) % rows, and a pass reads a buffer as the total of its rows.

Pass t adds into buffer t % 3, reads buffer (t - 1) % 3 (t > 0), clears buffer (t + 1) % 3 and writes centroid array t & 1; for an
empty cluster it reads array (t - 1) & 1. The last pass adds nothing and clears the buffer it read (the ticket counts the
workgroups that are through and is 0 again afterwards)."""
import hashlib

import numpy as np

from lloyd_ref import _pass_reference
from oracle import spec_oracle as so

TICKET_BYTES = 256


def pad256(n):
    return -(-int(n) // 256) * 256


def fold_rows(b, parts, n_sets, env_rows=1):
    """Shared rows per set: ``env_rows`` = the value of GCS_KP_FOLD_ROWS the process started with (1: unset)."""
    if n_sets == b and b > 1:
        return 1
    return min(b * parts, env_rows)


def env_fold_rows():
    """GCS_KP_FOLD_ROWS as the library reads it, once per process: 1 .. 64, anything else is 1."""
    import os
    try:
        v = int(os.environ.get("GCS_KP_FOLD_ROWS", "0"))
    except ValueError:
        v = 0
    return v if 1 <= v <= 64 else 1


def sum_bytes(n_sets, rows, k, d):
    return pad256(n_sets * rows * k * (d + 1) * 8)


def cent_bytes(n_sets, k, d):
    return pad256(n_sets * k * d * 2)


def workspace_bytes(n_sets, rows, k, d):
    return 3 * sum_bytes(n_sets, rows, k, d) + 2 * cent_bytes(n_sets, k, d) + TICKET_BYTES


class Views:
    """Named views of a flat byte buffer (a NumPy uint8 array, or a torch uint8 tensor on any device: views, not copies).

    sum_raw[i] / cent_raw[i] / ticket_raw   the bytes of a piece, padding included
    sums[i]      (n_sets, rows, k, D + 1) 64-bit (NumPy: uint64; torch: int64, which has the same bits below 2^63)
    sum_pad[i], cent_pad[i]                 the padding bytes behind the piece's data
    cents[i]     (n_sets, k, D) 16-bit (NumPy: uint16; torch: int16)
    ticket       (64,) 32-bit words; the kernel uses word 0"""

    def __init__(self, buf, n_sets, rows, k, d):
        is_np = isinstance(buf, np.ndarray)
        if is_np:
            t64, t16, t32 = np.uint64, np.uint16, np.uint32
        else:
            import torch
            t64, t16, t32 = torch.int64, torch.int16, torch.int32
        sb, cb = sum_bytes(n_sets, rows, k, d), cent_bytes(n_sets, k, d)
        assert buf.ndim == 1 and buf.shape[0] == 3 * sb + 2 * cb + TICKET_BYTES, (tuple(buf.shape), 3 * sb + 2 * cb + TICKET_BYTES)
        self.n_sets, self.rows, self.k, self.d, self.sb, self.cb = n_sets, rows, k, d, sb, cb
        ns, nc = n_sets * rows * k * (d + 1) * 8, n_sets * k * d * 2
        self.sum_raw = [buf[i * sb:(i + 1) * sb] for i in range(3)]
        self.sums = [r[:ns].view(t64).reshape(n_sets, rows, k, d + 1) for r in self.sum_raw]
        self.sum_pad = [r[ns:] for r in self.sum_raw]
        self.cent_raw = [buf[3 * sb + i * cb:3 * sb + (i + 1) * cb] for i in range(2)]
        self.cents = [r[:nc].view(t16).reshape(n_sets, k, d) for r in self.cent_raw]
        self.cent_pad = [r[nc:] for r in self.cent_raw]
        self.ticket_raw = buf[3 * sb + 2 * cb:]
        self.ticket = self.ticket_raw.view(t32)


def views(buf, n_sets, rows, k, d):
    return Views(buf, n_sets, rows, k, d)


def totals(sums):
    """(n_sets, rows, k, D + 1) -> the int64 totals (n_sets, k, D + 1) a pass reads: the rows of a set added up."""
    s = np.asarray(sums)
    assert (s.view(np.int64) >= 0).all()
    return s.astype(np.int64).sum(axis=1)


def update(total, old):
    """SPEC.md §4 on folded sums (n_sets, k, D + 1) int64 and the previous centroids (n_sets, k, D): floor((2 S + n) / (2 n)) in
    Python integers, an empty cluster keeps ``old``."""
    new = np.array(old, np.int64)
    for s in range(total.shape[0]):
        for j in range(total.shape[1]):
            n = int(total[s, j, -1])
            if n:
                new[s, j] = [(2 * int(v) + n) // (2 * n) for v in total[s, j, :-1]]
    return new


_MEMO = {}


def _assigned(x, cent):
    """_pass_reference over whole images, remembered for the last few (features, centroids): a state is usually run twice, as a
    pass that is not the last and as the last one."""
    key = (x.shape, hashlib.sha1(np.ascontiguousarray(x)).digest(), cent.shape, cent.tobytes())
    if key not in _MEMO:
        if len(_MEMO) > 8:
            _MEMO.pop(next(iter(_MEMO)))
        _MEMO[key] = _pass_reference(x, cent, np.ones(x.shape[:2], bool))
    return _MEMO[key]


def expected_pass(buf, x, t, last, mode, k, rows=1):
    """The workspace after pass ``t`` of a loop, from the bytes before it (NumPy uint8, not modified), the features x (B, P, D)
    int64 and the codebook mode. -> (bytes after, the centroids (n_sets, k, D) int64 the pass wrote to ``cent``, labels (B, P)).

    The model adds a pass's sums into ROW 0 of buffer t % 3: which workgroup adds into which row is the kernel's business, so with
    rows > 1 compare ``totals`` of that buffer. Padding bytes are never touched."""
    b, _, d = x.shape
    n_sets = b if mode == "per_image" else 1
    after = buf.copy()
    v0, v1 = views(buf, n_sets, rows, k, d), views(after, n_sets, rows, k, d)
    if t == 0:
        cent = np.stack([so.kmeans_init(x[s], k) for s in range(n_sets)])
    else:
        cent = update(totals(v0.sums[(t - 1) % 3]), v0.cents[(t - 1) & 1].astype(np.int64))
    assert cent.min() >= 0 and cent.max() < 65536
    v1.cents[t & 1][...] = cent.astype(np.uint16)
    v1.sums[(t + 1) % 3][...] = 0
    lab, s, n = _assigned(x, cent)
    if last:
        if t > 0:
            assert not v0.ticket.any(), "the ticket counts from 0"
            v1.sums[(t - 1) % 3][...] = 0
            v1.ticket[...] = 0
    else:
        v1.sums[t % 3][:, 0, :, :d] += s.astype(np.uint64)
        v1.sums[t % 3][:, 0, :, d] += n.astype(np.uint64)
    return after, cent, lab


def expected_loop(buf, x, n_iter, mode, k, rows=1):
    """``n_iter`` passes chained on one workspace -> (bytes after, centroids of the last pass, its labels)."""
    cent = lab = None
    for t in range(n_iter):
        buf, cent, lab = expected_pass(buf, x, t, t == n_iter - 1, mode, k, rows)
    return buf, cent, lab


def is_as_found(buf, n_sets, rows, k, d):
    """What include/gcs.h promises after every complete loop: the three sum buffers and the ticket are zero in every byte."""
    v = views(buf, n_sets, rows, k, d)
    return not any(bool(r.any()) for r in v.sum_raw) and not bool(v.ticket_raw.any())
