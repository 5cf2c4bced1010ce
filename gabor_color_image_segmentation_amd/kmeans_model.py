"""The k-means model of SPEC.md §28 as a value: codebooks with the counts and inertias they were measured at, the signature of the
feature space they live in, and the host arithmetic that finishes the integer outputs of ``gcs_kmeans_evaluate`` in float64.

A model is what ``Segmenter.fit_device`` returns and what ``predict_device`` / ``segment_device(codebook=...)`` take; it holds torch
tensors on one device and moves with ``to`` / ``cpu``. ``save`` / ``load`` keep it as an ``.npz`` with the signature as JSON."""
from __future__ import annotations

import json

import numpy as np


def mse_of(counts, inertia, n_features):
    """SPEC.md §28: sum_j inertia_j / (P_set * D) per set, float64; P_set = sum_j count_j. (n_sets, k) int64 arrays -> (n_sets,)
    float64, nan for a set without pixels."""
    total = np.asarray(inertia, np.int64).sum(axis=1).astype(np.float64)
    size = (np.asarray(counts, np.int64).sum(axis=1) * int(n_features)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return total / size


def confidence_of(best, second):
    """SPEC.md §28: (second - best) / second in float64, 0 where second = 0, delivered as float32 in [0, 1]. Torch int64 tensors
    (any device) -> float32 tensor."""
    margin = (second - best).double()
    conf = margin / second.double()
    return conf.masked_fill(second == 0, 0.0).float()


class KMeansModel:
    """``centroids`` (n_sets, k, D) uint16, ``counts`` and ``inertia`` (n_sets, k) int64 - the pixels of every cluster and the sum
    of their squared distances to its centroid on the images the model was fitted on -, and ``signature``: everything that defines
    the feature space (the bank's parameters, ``color_weight``, ``chroma_gain``, ``smoothing``, ``position_weight``) and ``k``. A
    plan takes a model only when the signature is its own. ``n_sets`` = 1: one codebook; B: one per image of the fitted batch."""

    def __init__(self, centroids, counts, inertia, signature):
        import torch
        if centroids.dtype == torch.int16:
            centroids = centroids.view(torch.uint16)
        if centroids.dtype != torch.uint16 or centroids.ndim != 3 or counts.dtype != torch.int64 or inertia.dtype != torch.int64 \
                or tuple(counts.shape) != tuple(centroids.shape[:2]) or tuple(inertia.shape) != tuple(centroids.shape[:2]):
            raise ValueError("a model holds (n_sets, k, D) uint16 centroids and (n_sets, k) int64 counts and inertias")
        self.centroids, self.counts, self.inertia = centroids.contiguous(), counts.contiguous(), inertia.contiguous()
        self.signature = dict(signature)
        if self.signature.get("k") != self.k:
            raise ValueError(f"the signature says k = {self.signature.get('k')!r}, the centroids k = {self.k}")

    n_sets = property(lambda self: int(self.centroids.shape[0]))
    k = property(lambda self: int(self.centroids.shape[1]))
    n_features = property(lambda self: int(self.centroids.shape[2]))
    device = property(lambda self: self.centroids.device)

    @property
    def mse(self):
        """(n_sets,) float64: the mean squared error per feature of the fitted pixels (``mse_of``). Reads the tensors back."""
        return mse_of(self.counts.cpu().numpy(), self.inertia.cpu().numpy(), self.n_features)

    def to(self, device):
        import torch
        if torch.device(device) == self.device:
            return self
        # (uint16 tensors move as their int16 bits: every backend copies those)
        cent = self.centroids.view(torch.int16).to(device).view(torch.uint16)
        return KMeansModel(cent, self.counts.to(device), self.inertia.to(device), self.signature)

    def cpu(self):
        return self.to("cpu")

    def save(self, path):
        """An ``.npz`` with the three arrays and the signature as JSON (sorted keys). ``path``: a file name or an open file."""
        m = self.cpu()
        np.savez(path, centroids=m.centroids.numpy(), counts=m.counts.numpy(), inertia=m.inertia.numpy(),
                 signature=np.array(json.dumps(m.signature, sort_keys=True)))

    @classmethod
    def load(cls, path):
        import torch
        with np.load(path, allow_pickle=False) as z:
            cent, counts, inertia = (np.ascontiguousarray(z[n]) for n in ("centroids", "counts", "inertia"))
            signature = json.loads(str(z["signature"]))
        if cent.dtype != np.uint16 or counts.dtype != np.int64 or inertia.dtype != np.int64:
            raise ValueError(f"{path}: not a k-means model file")
        return cls(torch.from_numpy(cent), torch.from_numpy(counts), torch.from_numpy(inertia), signature)

    def __repr__(self):
        return f"KMeansModel(n_sets={self.n_sets}, k={self.k}, D={self.n_features}, device={self.device})"
