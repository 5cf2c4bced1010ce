"""The oracle stand-in for HipOps (tests/fake_ops.py, tests/position_ops.py) extended by the stages of SPEC.md §13 and §14, each
answered by its NumPy restatement: the CPU tests of the host logic of ``Segmenter(n_superpixels=n, n_regions=R)``. Records the call
order. Never used by the product."""
import numpy as np
import torch

import region_tree_ref as rt
import superpixel_ref as sr
from position_ops import PositionOps


class RegionTreeOps(PositionOps):
    def features_unpack(self, feats, b, h, w, out=None):
        self.calls.append(("unpack", b))
        t = super().features_unpack(feats, b, h, w)
        if out is None:
            return t
        out.copy_(t)
        return out

    def superpixel_buffers(self, b, h, w, n):
        return torch.empty((b, self.bank.n_features, h, w), dtype=torch.int16), None

    def superpixels(self, canon, b, h, w, ny, nx, spatial_weight, n_iter, out, workspace, centres=None):
        self.calls.append(("superpixels", b, ny, nx))
        for i in range(b):
            x = canon[i].numpy().view(np.uint16).astype(np.int64)
            cy, cx = sr.init_positions(h, w, ny, nx)
            cent = x[:, cy, cx].T.copy()
            for t in range(n_iter):
                lab = sr.assign(x, cent, cy, cx, ny, nx, int(spatial_weight))
                if t < n_iter - 1:
                    cent, cy, cx = sr.update(x, lab, cent, cy, cx)
            out[i] = torch.from_numpy(lab.astype(np.int32))

    def region_tree_buffers(self, b, h, w, K):
        return (None, torch.zeros((b, K - 1, 2), dtype=torch.int32), torch.zeros((b, K - 1), dtype=torch.int64),
                torch.zeros((b,), dtype=torch.int32))

    def region_tree(self, canon, labels, b, h, w, K, workspace, merges, costs, alive):
        self.calls.append(("tree", b, K))
        for i in range(b):
            m, c, a = rt.build_tree(canon[i].numpy().view(np.uint16), labels[i].numpy(), K)
            merges[i] = torch.from_numpy(m)
            if costs is not None:
                costs[i] = torch.from_numpy(c.view(np.int64))
            alive[i] = a

    def region_tree_cut(self, labels, merges, alive, b, h, w, K, R, out):
        self.calls.append(("cut", b, K, R))
        res = [rt.cut(labels[i].numpy(), merges[i].numpy(), int(alive[i]), R) for i in range(b)]
        out.copy_(torch.from_numpy(np.stack(res)))

    def connected_regions(self, labels_i32, out):
        self.calls.append(("connected",))
        super().connected_regions(labels_i32, out)

    def merge_small_regions(self, labels_i32, min_size, out):
        self.calls.append(("merge", int(min_size)))
        super().merge_small_regions(labels_i32, min_size, out)
