"""The oracle stand-in for HipOps (tests/texton_gradient_ops.py) extended by the cue gradient of SPEC.md §25, answered by its NumPy
restatement (tests/cue_gradient_ref.py). Records the call order. Never used by the product."""
import numpy as np
import torch

import cue_gradient_ref as cg
from texton_gradient_ops import TextonGradientOps


class CueGradientOps(TextonGradientOps):
    def cue_gradient(self, labels, imgs, b, h, w, K, bins, weights, r, n, grad, out, dir_out, masks=None):
        self.calls.append(("cue", b, K, bins, tuple(weights), r, n, labels is not None, imgs is not None, grad is not None,
                           dir_out is not None))
        table = cg.masks(r, n) if masks is None else masks.numpy().view(np.uint32)
        for i in range(b):
            p, d = cg.cue_gradient(None if labels is None else labels[i].numpy(), None if imgs is None else imgs[i].numpy(), K, bins,
                                   weights, r, n, table)
            out[i] = torch.from_numpy(p if grad is None else cg.joined(p, np.maximum(grad[i].numpy(), 0)))
            if dir_out is not None:
                dir_out[i] = torch.from_numpy(d)
