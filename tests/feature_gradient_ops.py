"""The oracle stand-in for HipOps (tests/cluster_tree_ops.py) extended by the edge map of SPEC.md §22 and by what
``segment_regions(adjacency=True, gradient=True)`` runs behind it (§19's leaf table, §20's leaf graph), each answered by its NumPy
restatement (the stand-in's "slab" is the feature array itself). Records the call order. Never used by the product."""
import numpy as np
import torch

import feature_gradient_ref as fg
import region_adjacency_ref as ra
import region_props_ref as rp
from cluster_tree_ops import ClusterTreeOps


class FeatureGradientOps(ClusterTreeOps):
    def feature_gradient(self, feats, b, h, w, out):
        self.calls.append(("gradient", b))
        for i in range(b):
            out[i] = torch.from_numpy(fg.gradient(self._planes(feats, i, h, w), self.bank.n_scales, self.bank.n_orient))

    def region_props(self, labels, imgs, canon, b, h, w, K, sums, bbox):
        self.calls.append(("props", b, K))
        for i in range(b):
            s, bb = rp.leaf_table(labels[i].numpy(), K, imgs[i].numpy())
            sums[i] = torch.from_numpy(s.view(np.int64))
            bbox[i] = torch.from_numpy(bb)

    def adjacency_buffers(self, tables, capacity):
        return None

    def region_adjacency(self, labels, imgs, strength, b, h, w, K, workspace, edges, vals, count):
        self.calls.append(("adjacency", b, K, strength is not None))
        cap = int(edges.shape[1])
        for i in range(b):
            e, v = ra.leaf_graph(labels[i].numpy(), K, None if imgs is None else imgs[i].numpy(),
                                 None if strength is None else strength[i].numpy())
            eo, vo, n = ra.table(e, v, cap)
            edges[i], vals[i], count[i] = torch.from_numpy(eo), torch.from_numpy(vo.view(np.int64)), n
