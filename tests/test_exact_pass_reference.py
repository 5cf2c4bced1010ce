"""tests/lloyd_ref.py: exact_pass (float64 matrix products in torch; the reference of tests/test_gpu_nt_arm.py) == _pass_reference (int64
NumPy, so.kmeans_assign) on small crafted batches, on the CPU: values over the whole 16-bit feature range, a codebook with identical
rows and rows at equal distance from a pixel (ties go to the lowest index), row windows, one global and per-image codebooks."""
import numpy as np
import pytest

import hot_banks as hb
from lloyd_ref import _caller_codebook, _pass_reference, exact_pass, updated
from fused_workspace import update

import torch


@pytest.mark.parametrize("b,d,h,w,k", [(3, 5, 9, 14, 8), (2, 207, 7, 5, 4), (1, 72, 16, 16, 16), (4, 1, 6, 6, 4)])
def test_exact_pass_equals_the_int64_reference(b, d, h, w, k):
    rng = np.random.default_rng(b * d + k)
    x = rng.integers(0, hb.G_MAX + 1, (b, d, h, w))
    x[0, :, 0, 0], x[0, :, 0, 1] = 0, hb.G_MAX
    x[-1, :, 1:3] = 1000                                     # pixels at the same distance from the two rows made below
    flat = x.transpose(0, 2, 3, 1).reshape(b, h * w, d)                                      # (B, P, D)
    feats = torch.from_numpy(x.astype(np.uint16).view(np.int16))
    windows = [(0, h), (h // 4, h - h // 5), (h - 1, h)]
    for n_sets in {1, b}:
        book = np.stack([_caller_codebook(flat[s], k) for s in range(n_sets)])
        book[:, k - 1], book[:, k - 2] = 998, 1002           # |1000 - 998| == |1000 - 1002| in every feature: k - 2 wins
        lab, res = exact_pass(feats, book, windows)
        for (lo, hi), (sums, cnt) in zip(windows, res):
            vote = np.zeros((b, h, w), bool)
            vote[:, lo:hi] = True
            want_lab, want_sums, want_cnt = _pass_reference(flat, book, vote.reshape(b, -1))
            assert np.array_equal(lab.numpy().reshape(b, -1), want_lab)
            assert np.array_equal(sums, want_sums) and np.array_equal(cnt, want_cnt)
            assert np.array_equal(updated(sums, cnt, book), update(np.concatenate([sums, cnt[..., None]], axis=2), book))
        assert (lab.numpy()[-1, 1:3] == k - 2).all() and (cnt[:, 1] == 0).all()
