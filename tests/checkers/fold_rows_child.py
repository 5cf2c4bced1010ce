#!/usr/bin/env python3
"""Child process of tests/test_gpu_self_updating_stages.py::test_more_than_one_shared_row.

The library reads GCS_KP_FOLD_ROWS once per process, so the shared rows of the self-updating Lloyd pass (`wg % rows`, the fold loop
over the rows, the workspace that grows with them) can only be reached in a process started with it. With the value the parent
set: gcs_kmeans_fused_workspace_bytes follows rows = min(B * parts, value) for one global codebook and keeps rows = 1 for
per-image codebooks of a batch; the stage checks of tests/fused_stages.py (a written pass for every residue of the rotation, not
last and last; pass 0; a loop watched from inside) hold on 4x6 k = 8 and 2x5 k = 3 with the written sums spread over all rows;
one segment_device loop per codebook mode equals the C oracle. Prints one line `OK fold rows <value> ...`."""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def main():
    import torch
    import fused_stages as fs
    import fused_workspace as fw
    import hot_banks as hb
    from oracle import c_oracle as co

    value = int(os.environ["GCS_KP_FOLD_ROWS"])
    assert fw.env_fold_rows() == value > 1
    assert torch.cuda.is_available(), "needs a HIP device"
    b, h, w = 3, 41, 74
    imgs = hb.hot_images(b, h, w, seed=h + w)
    rows_seen = set()
    for cfg, k in (((4, 6, 13, 7), 8), ((2, 5, 11, 7), 3)):
        st = fs.stage(torch, cfg, imgs)
        lib = st.ops.lib
        n_sets, rows, _, d = st.layout("global", k)
        assert rows == min(b * st.parts, value) > 1 and st.layout("per_image", k)[1] == 1
        got = lib.gcs_kmeans_fused_workspace_bytes(b, h, w, cfg[0], cfg[1], k, 1)
        assert got == fw.workspace_bytes(1, rows, k, d), (got, rows)
        got = lib.gcs_kmeans_fused_workspace_bytes(b, h, w, cfg[0], cfg[1], k, b)
        assert got == fw.workspace_bytes(b, 1, k, d), (got, "per-image codebooks keep one row")
        one = int(lib.gcs_kmeans_parts_per_image(1, h, w))
        got = lib.gcs_kmeans_fused_workspace_bytes(1, h, w, cfg[0], cfg[1], k, 1)
        assert got == fw.workspace_bytes(1, min(one, value), k, d), (got, "one image is one global codebook")
        rows_seen.add(rows)
        assert st.x.max() >= 32768
        for t in (1, 2, 3, 4):
            for last in (False, True):
                fs.check_written_pass(st, "global", k, t, last, (cfg, value), need_inputs=k >= 6)
        for last in (False, True):
            fs.check_pass0(st, "global", k, last, (cfg, value))
        fs.check_loop(st, "global", k, 5, (cfg, value))
        fs.check_loop(st, "per_image", k, 5, (cfg, value))
        bank = hb.hot_bank(*cfg)
        seg = hb.hot_segmenter(bank, k=k, n_iter=4)
        for mode in ("global", "per_image"):
            want = co.segment_batch(imgs, bank.tapq, bank.shift, bank.n_orient, k=k, n_iter=4, mode=mode)
            got = seg.segment_device(torch.from_numpy(imgs).cuda(), mode=mode).cpu().numpy()
            assert np.array_equal(got, want), (cfg, mode, int((got != want).sum()))
            ws = seg._ws[(b, h, w, mode)]["fold"]
            assert ws is not None and fw.is_as_found(ws.cpu().numpy(), *st.layout(mode, k)), (cfg, mode)
    torch.cuda.synchronize()
    print(f"OK fold rows {value}: rows used {sorted(rows_seen)}", flush=True)


if __name__ == "__main__":
    main()
