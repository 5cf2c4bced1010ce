"""The oracle stand-in for HipOps with the launches of SPEC.md §28 and §29 (tests/kmeans_seed_ops.py) extended by the two launches
of SPEC.md §30, answered by their NumPy restatement (tests/label_relax_ref.py). Records the call order. Never used by the product."""
import numpy as np
import torch

import label_relax_ref as lr
from kmeans_seed_ops import KMeansSeedOps


class LabelRelaxOps(KMeansSeedOps):
    def kmeans_costs(self, feats, cent, b, h, w, k, n_sets, costs):
        self.calls.append(("costs", b, h, w, k, n_sets))
        c = cent.view(torch.int16).numpy().view(np.uint16).astype(np.int64)
        assert c.shape == (n_sets, k, self.bank.n_features) and feats["x"].shape[:2] == (b, h * w)
        assert tuple(costs.shape) == (b, k, h, w) and costs.dtype == torch.int64
        costs.copy_(torch.from_numpy(lr.cost_volume(feats["x"], c, h, w)))

    def label_relax(self, costs, beta, b, h, w, k, neighbours, sweeps, labels_in, labels_out, workspace=None, changed=None,
                    energy=None):
        self.calls.append(("relax", b, h, w, k, neighbours, sweeps, tuple(int(v) for v in beta)))
        assert tuple(costs.shape) == (b, k, h, w) and tuple(beta.shape) == (b,) and labels_in is not labels_out
        assert sweeps < 2 or workspace is not None
        lab, ch, en = lr.relax_batch(costs.numpy(), labels_in.numpy(), beta.numpy(), sweeps, neighbours)
        labels_out.copy_(torch.from_numpy(lab))
        if changed is not None:
            changed.copy_(torch.from_numpy(ch))
        if energy is not None:
            energy.copy_(torch.from_numpy(en))
