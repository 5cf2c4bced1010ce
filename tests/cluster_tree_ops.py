"""The oracle stand-in for HipOps (tests/region_tree_ops.py) extended by the stages SPEC.md §21 runs behind the Lloyd loop, each
answered by its NumPy restatement: the node map of §18 and the tree whose statistics come from the slab (the stand-in's "slab" is the
feature array itself). Records the call order. Never used by the product."""
import numpy as np
import torch

import component_tree_ref as ct
import region_tree_ref as rt
from region_tree_ops import RegionTreeOps


class ClusterTreeOps(RegionTreeOps):
    def labels_widen(self, labels, b, h, w, out):
        self.calls.append(("widen", str(out.dtype)))
        super().labels_widen(labels, b, h, w, out)

    def region_nodes_buffers(self, b, h, w):
        return None, torch.empty((b, h, w), dtype=torch.int32), torch.zeros((b,), dtype=torch.int32)

    def region_nodes(self, labels_i32, min_size, out, n_nodes, scratch=None, k_cap=ct.K_CAP, min_size_used=None):
        self.calls.append(("nodes", int(min_size)))
        for i, lab in enumerate(labels_i32.numpy()):
            info = {}
            out[i] = torch.from_numpy(ct.nodes(lab, int(min_size), k_cap, info))
            n_nodes[i] = info["nodes"]

    def region_tree_slab(self, feats, labels, b, h, w, K, workspace, merges, costs, alive):
        self.calls.append(("tree_slab", b, K))
        d = feats["x"].shape[2]
        for i in range(b):
            m, c, a = rt.build_tree(feats["x"][i].T.reshape(d, h, w), labels[i].numpy(), K)
            merges[i] = torch.from_numpy(m)
            if costs is not None:
                costs[i] = torch.from_numpy(c.view(np.int64))
            alive[i] = a

