"""The oracle stand-in for HipOps (tests/feature_gradient_ops.py) extended by the stages SPEC.md §23 adds behind the edge map of §22
and the leaf table of §20: the labels in use and the merges on the edge table, each answered by its NumPy restatement. Records the
call order. Never used by the product."""
import numpy as np
import torch

import boundary_tree_ref as bt
from feature_gradient_ops import FeatureGradientOps


class BoundaryTreeOps(FeatureGradientOps):
    def region_tree_edges_buffers(self, b, h, w, K, capacity=bt.E_MAX):
        stage = dict(grad=torch.zeros((b, h, w), dtype=torch.int32), adj=None, edges=torch.zeros((b, capacity, 2), dtype=torch.int32),
                     vals=torch.zeros((b, capacity, 3), dtype=torch.int64), count=torch.zeros((b,), dtype=torch.int32),
                     used=torch.zeros((b, K), dtype=torch.int32), tree=None)
        return (stage, torch.zeros((b, K - 1, 2), dtype=torch.int32), torch.zeros((b, K - 1), dtype=torch.int64),
                torch.zeros((b,), dtype=torch.int32))

    def label_used(self, labels, b, h, w, K, out):
        self.calls.append(("used", b, K))
        for i in range(b):
            out[i] = torch.from_numpy(bt.used_labels(labels[i].numpy(), K))

    def region_tree_edges(self, edges, vals, count, used, b, K, workspace, merges, costs, alive):
        self.calls.append(("tree_edges", b, K))
        for i in range(b):
            m, c, a = bt.tree_of_table(edges[i].numpy(), vals[i].numpy().view(np.uint64), int(count[i]), used[i].numpy(), K)
            merges[i] = torch.from_numpy(m)
            if costs is not None:
                costs[i] = torch.from_numpy(c.view(np.int64))
            alive[i] = a
