"""The oracle stand-in for HipOps (tests/fake_ops.py) extended by the evaluate launch of SPEC.md §28, answered by its NumPy
restatement (tests/kmeans_model_ref.py). Records the call order. Never used by the product."""
import numpy as np
import torch

import kmeans_model_ref as km
from fake_ops import OracleOps


class KMeansModelOps(OracleOps):
    def kmeans_evaluate(self, feats, cent, b, h, w, k, n_sets, labels=None, best=None, second=None, stats=None):
        self.calls.append(("evaluate", b, h, w, k, n_sets, tuple(n for n, t in (("labels", labels), ("best", best),
                                                                               ("second", second), ("stats", stats)) if t is not None)))
        c = cent.view(torch.int16).numpy().view(np.uint16).astype(np.int64)
        assert c.shape == (n_sets, k, self.bank.n_features) and feats["x"].shape[:2] == (b, h * w)
        lab, bs, sc, st = km.evaluate_batch(feats["x"], c)
        for t, a in ((labels, lab), (best, bs), (second, sc)):
            if t is not None:
                t.copy_(torch.from_numpy(a.reshape(b, h, w)))
        if stats is not None:
            stats.copy_(torch.from_numpy(st))
