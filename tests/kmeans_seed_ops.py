"""The oracle stand-in for HipOps with the evaluate launch of SPEC.md §28 (tests/kmeans_model_ops.py) extended by the seed launch
of SPEC.md §29, answered by its NumPy restatement (tests/kmeans_seed_ref.py). Records the call order. Never used by the product."""
import numpy as np
import torch

import kmeans_seed_ref as ks
from kmeans_model_ops import KMeansModelOps


class KMeansSeedOps(KMeansModelOps):
    def kmeans_seed(self, feats, b, h, w, k, n_sets, cent, stride, trials=4, seed=0, picks=None, potential=None):
        self.calls.append(("seed", b, h, w, k, n_sets, stride, trials, seed))
        assert tuple(cent.shape) == (n_sets, k, self.bank.n_features) and feats["x"].shape[:2] == (b, h * w)
        c, q, pot = ks.seed_batch(feats["x"], h, w, k, n_sets, stride, seed, trials)
        cent.copy_(torch.from_numpy(c.astype(np.uint16).view(np.int16)))
        if picks is not None:
            picks.copy_(torch.from_numpy(q))
        if potential is not None:
            potential.copy_(torch.from_numpy(pot))
