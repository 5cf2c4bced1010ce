"""The oracle stand-in for HipOps (tests/cue_gradient_ops.py) extended by the thin launch of SPEC.md §26, answered by its NumPy
restatement (tests/edge_thin_ref.py). Records the call order. Never used by the product."""
import numpy as np
import torch

import edge_thin_ref as et
from cue_gradient_ops import CueGradientOps


class EdgeThinOps(CueGradientOps):
    def thin_steps(self, n):
        self.calls.append(("steps", n))
        return torch.from_numpy(et.steps(n))

    def edge_thin(self, edges, dirs, b, h, w, n, out, steps=None):
        self.calls.append(("thin", b, h, w, n, steps is not None))
        table = None if steps is None else steps.numpy()
        for i in range(b):
            out[i] = torch.from_numpy(et.thin_fast(edges[i].numpy(), dirs[i].numpy(), n, table))
