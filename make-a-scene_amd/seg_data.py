"""Dataset side of the compact VQ-SEG input (CPU only).

The reference stores, per image, a panoptic label image and a human-part label image (-1 = none), a face label image (0 = none) and two
edge images, and its dataset class turns them into a dense [H, W, 159] one-hot map before augmenting and batching
(Data/dataset_preprocessor.py:54-88).  ``planes_from_arrays`` keeps them as what they are -- four uint8 planes, an ordinary [H, W, 4] image
once transposed, so that the reference's mask augmentations (nearest-neighbour resize, crop, flip) apply to it unchanged: they move whole
pixels, and the one-hot of a moved pixel is the moved one-hot.  ``collate`` stacks samples into one ``mas_hip.seglabels.SegLabels``, which
``VQBASE``, the VQ-SEG losses and ``token_data.tokenize_batch`` take in place of the dense map."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from mas_hip.seglabels import SegLabels, SegLayout

REFERENCE_LAYOUT = SegLayout(groups=(133, 20, 5), value_channels=1)


def _integers(a, name: str, lo: int, hi: int) -> np.ndarray:
    """-> int64 array; raises on non-integer values and on values outside [lo, hi] (nothing wraps into a valid label)"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"planes_from_arrays: {name} must be [H, W], got shape {a.shape}")
    if a.dtype == np.bool_:
        a = a.astype(np.int64)
    if not np.issubdtype(a.dtype, np.integer):
        if not np.issubdtype(a.dtype, np.floating) or not np.isfinite(a).all() or (a != np.rint(a)).any():
            raise ValueError(f"planes_from_arrays: {name} holds non-integer values")
    a = a.astype(np.int64)
    if a.size and (a.min() < lo or a.max() > hi):
        raise ValueError(f"planes_from_arrays: {name} holds values in [{a.min()}, {a.max()}], outside [{lo}, {hi}]")
    return a


def planes_from_arrays(seg_panoptic, edges_panoptic, seg_human, edges_human, seg_face, layout: SegLayout = REFERENCE_LAYOUT) -> torch.Tensor:
    """The arrays as the reference stores them per image -> uint8 planes [4, H, W] of ``layout`` (default: the reference's 159 channels).
    ``seg_panoptic`` in -1 .. 132 and ``seg_human`` in -1 .. 19 (-1 = none), ``seg_face`` in 0 .. 5 (0 = none); the edge plane is
    ``edges_panoptic + edges_human`` (each a non-negative integer image, the sum at most 255)."""
    if len(layout.groups) != 3 or layout.value_channels != 1:
        raise ValueError(f"planes_from_arrays: needs a layout of three groups and one value channel, got {layout}")
    pan = _integers(seg_panoptic, "seg_panoptic", -1, layout.groups[0] - 1) + 1
    hum = _integers(seg_human, "seg_human", -1, layout.groups[1] - 1) + 1
    face = _integers(seg_face, "seg_face", 0, layout.groups[2])
    edges = _integers(edges_panoptic, "edges_panoptic", 0, 255) + _integers(edges_human, "edges_human", 0, 255)
    if edges.size and edges.max() > 255:
        raise ValueError(f"planes_from_arrays: edges_panoptic + edges_human reaches {edges.max()} > 255")
    if not (pan.shape == hum.shape == face.shape == edges.shape):
        raise ValueError(f"planes_from_arrays: shapes differ: {pan.shape}, {hum.shape}, {face.shape}, {edges.shape}")
    return torch.from_numpy(np.stack([pan, hum, face, edges]).astype(np.uint8))


def collate(samples: Sequence, layout: SegLayout = REFERENCE_LAYOUT) -> SegLabels:
    """[P, H, W] uint8 planes (tensors or arrays; or ``SegLabels`` of one sample each) -> one ``SegLabels`` batch"""
    if len(samples) == 0:
        raise ValueError("collate: no samples")
    planes = []
    for s in samples:
        if isinstance(s, SegLabels):
            if s.layout != layout:
                raise ValueError(f"collate: a sample's layout {s.layout} differs from {layout}")
            planes.append(s.planes)
            continue
        t = s if isinstance(s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[0] != layout.planes:
            raise ValueError(f"collate: a sample must be uint8 [{layout.planes}, H, W], got {t.dtype} {tuple(t.shape)}")
        planes.append(t.unsqueeze(0))
    return SegLabels(torch.cat(planes, 0).contiguous(), layout)
