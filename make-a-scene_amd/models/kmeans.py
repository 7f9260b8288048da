"""Codebook re-initialisation by k-means over the latent reservoir (reference models/modules.py:487-499, where it is
delegated to the third-party ``fast_pytorch_kmeans.KMeans`` -- absent from the reference tree, unpinned -- with its
defaults: random distinct data points as initial centroids, euclidean, max_iter=100, tol=1e-4, an empty cluster's
centroid becomes the zero vector).  Lloyd iterations here use the same fused nearest-codebook HIP kernel as the
forward pass for the assignment step; oracle/kmeans_oracle.py restates the algorithm for the tests.

``on_device`` (opt-in, ``MAS_KMEANS_DEVICE=1``) hands the whole fit to ``ops.kmeans_fit``: the same rule as a fixed sequence
of launches with the stop test on the device -- no host read, every sum in a fixed order."""
import os

import torch

from mas_hip import ops


def device_default() -> bool:
    """``MAS_KMEANS_DEVICE``: the default of ``on_device`` here and of ``Codebook.enable_device_reservoir(device_kmeans=None)``; off"""
    return os.environ.get("MAS_KMEANS_DEVICE", "0").strip().lower() not in ("", "0", "false", "off", "no")


@torch.no_grad()
def kmeans_fit(points: torch.Tensor, n_clusters: int, max_iter: int = 100, tol: float = 1e-4, init_idx=None,
               return_info: bool = False, on_device=None, seed=None, draw: int = 0):
    """``on_device``: None reads ``MAS_KMEANS_DEVICE`` (default off: the loop below, which reads one scalar per iteration on the host).
    On: ``ops.kmeans_fit`` -- initial rows ``init_idx``, or drawn from ``seed`` / ``draw`` by the keyed bijection (``seed`` None draws one
    from torch's CPU generator); with ``return_info`` the third value is the device int32 pair ``{iterations run, converged}``."""
    if device_default() if on_device is None else on_device:
        if init_idx is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        cent, idx, info = ops.kmeans_fit(points, n_clusters, init_idx=init_idx, seed=None if init_idx is not None else seed, draw=draw,
                                         max_iter=max_iter, tol=tol)
        return (cent, idx, info) if return_info else cent
    pts = points.detach().float().contiguous()
    m, d = pts.shape
    if init_idx is None:
        if m < n_clusters:
            raise RuntimeError(f"kmeans_fit: {m} points for {n_clusters} clusters (the library samples without replacement)")
        init_idx = torch.randperm(m, device=pts.device)[:n_clusters]
    cent = pts[init_idx].clone()
    z = pts.t().reshape(1, d, m, 1)                       # [1,D,M,1] logical == rows of pts in NHWC memory
    ones = torch.ones(m, device=pts.device)
    idx, it = None, 0
    for it in range(1, max_iter + 1):
        _, _, idx = ops.vq_lookup(z, cent, 0.0)           # nearest centroid, lowest index on ties (the VQ kernel)
        sums = torch.zeros_like(cent).index_add_(0, idx, pts)
        cnt = torch.zeros(n_clusters, device=pts.device).index_add_(0, idx, ones)
        new = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1)[:, None], torch.zeros_like(cent))
        err = (new - cent).pow(2).sum()
        cent = new
        if float(err) <= tol:
            break
    return (cent, idx, it) if return_info else cent
