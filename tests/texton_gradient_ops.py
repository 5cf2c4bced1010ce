"""The oracle stand-in for HipOps (tests/feature_gradient_ops.py) extended by the texton gradient of SPEC.md §24, answered by its
NumPy restatement (tests/texton_gradient_ref.py). Records the call order. Never used by the product."""
import numpy as np
import torch

import texton_gradient_ref as tg
from feature_gradient_ops import FeatureGradientOps


class TextonGradientOps(FeatureGradientOps):
    def texton_masks(self, r, n):
        self.calls.append(("masks", r, n))
        return torch.from_numpy(tg.masks(r, n).view(np.int32))

    def texton_gradient(self, labels, b, h, w, K, r, n, grad, out, dir_out, masks=None):
        self.calls.append(("texton", b, K, r, n, grad is not None, dir_out is not None))
        table = tg.masks(r, n) if masks is None else masks.numpy().view(np.uint32)
        for i in range(b):
            t, d = tg.texton_gradient(labels[i].numpy(), K, r, n, table)
            out[i] = torch.from_numpy(t if grad is None else tg.joined(t, grad[i].numpy()))
            if dir_out is not None:
                dir_out[i] = torch.from_numpy(d)
