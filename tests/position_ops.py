"""The oracle stand-in for HipOps (tests/fake_ops.py) extended by the steps of SPEC.md §10 - §12, each answered by its NumPy
restatement: the CPU tests of the host logic of ``Segmenter(position_weight=mu)``. Records the call order. Never used by the
product."""
import numpy as np
import torch

import colour_ref as cr
import position_ref as pr
import smooth_ref as sr
from fake_ops import OracleOps


class PositionOps(OracleOps):
    def __init__(self, bank, chroma_gain=0, smoothing=0.0):
        super().__init__(bank)
        self.chroma_gain, self.smoothing = chroma_gain, float(smoothing)

    def colour_scratch(self, b, h, w):
        return torch.empty((b, h, w, 3), dtype=torch.uint8)

    def colour_opponent(self, imgs, out):
        self.calls.append(("colour", imgs.shape[0]))
        out.copy_(torch.from_numpy(cr.opponent(imgs.numpy(), self.chroma_gain)))

    def smooth_scratch(self, b, h, w):
        return {"planes": None}

    def _planes(self, feats, i, h, w):
        d = feats["x"].shape[2]
        return feats["x"][i].T.reshape(d, h, w)

    def smooth_features(self, feats, b, h, w, scratch=None):
        self.calls.append(("smooth", b))
        d = feats["x"].shape[2]
        sm = [sr.smooth_features(self._planes(feats, i, h, w).astype(np.uint16), self.smoothing, self.bank.n_scales,
                                 self.bank.n_orient, self.bank.f_max, self.bank.ratio) for i in range(b)]
        feats["x"] = np.stack([s.reshape(d, -1).T for s in sm]).astype(np.int64)

    def position_features(self, feats, b, h, w, y0=0):
        self.calls.append(("position", b, y0))
        mu = self.bank.position_weight
        assert mu > 0 and feats["x"].shape[:2] == (b, h * w)
        d = feats["x"].shape[2]
        out = [pr.fill_slot(np.array(self._planes(feats, i, h, w)), self.bank.n_scales, self.bank.n_orient, mu, y0)
               for i in range(b)]
        feats["x"] = np.stack([p.reshape(d, -1).T for p in out]).astype(np.int64)

    def assign_accumulate(self, *a, **kw):
        self.calls.append(("assign",))
        return super().assign_accumulate(*a, **kw)

    def features_unpack(self, feats, b, h, w):
        return torch.from_numpy(np.stack([self._planes(feats, i, h, w).astype(np.uint16) for i in range(b)]).view(np.int16))

    def merge_small_regions(self, labels_i32, min_size, out):
        from merge_ref import merge_small_regions
        out.copy_(torch.from_numpy(np.stack([merge_small_regions(l, min_size) for l in labels_i32.numpy()]).astype(np.int32)))
