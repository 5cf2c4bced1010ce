"""The stand-in ops of tests/region_tree_ops.py extended by the contour map of SPEC.md §15, answered by its restatement
(tests/contour_map_ref.py): the CPU tests of the host logic. Records the call order. Never used by the product."""
import numpy as np
import torch

import contour_map_ref as cm
from region_tree_ops import RegionTreeOps


class ContourMapOps(RegionTreeOps):
    def contour_buffers(self, b, K):
        self.calls.append(("contour_buffers", b, K))
        return None

    def region_tree_contours(self, labels, merges, alive, b, h, w, K, workspace, out):
        self.calls.append(("contours", b, K))
        res = [cm.contour_map(labels[i].numpy(), merges[i].numpy(), int(alive[i])) for i in range(b)]
        out.copy_(torch.from_numpy(np.stack(res)))
