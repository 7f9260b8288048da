"""The VQ-SEG segmentation map as compact label planes instead of a one-hot tensor.

The reference's dataloader (Data/dataset_preprocessor.py:62-86) turns three integer label images and an edge image per sample into a dense
``[H, W, 159]`` float one-hot map: 636 bytes per pixel for 4 bytes of information.  ``SegLabels`` keeps the 4 bytes: a ``uint8`` tensor
``[B, P, H, W]`` and a ``SegLayout`` that says which channels each plane stands for.  ``VQBASE``, the VQ-SEG losses and
``token_data.tokenize_batch`` accept it wherever they accept the dense map; on the GPU the dense map is written once, in the layout the
encoder's first convolution reads (``ops.seg_expand``), and the loss derives its target in registers (``ops.seg_loss_labels``): csrc/seg_labels.hip.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

MAX_PLANES = 8            # MAS_SEG_MAX_PLANES
MAX_GROUP = 255


@dataclass(frozen=True)
class SegLayout:
    """``groups``: one uint8 label plane each; value 0 = no class, ``v`` in ``1..size`` sets channel ``base + v - 1`` to 1, anything above the
    group's size sets nothing.  Then ``value_channels`` planes whose byte IS the channel's value (the reference's edge channel:
    ``edges_panoptic + edges_human``, 0, 1 or 2).  The default is the reference's channel order: panoptic 0..132, human parts 133..152,
    face 153..157, edges 158."""
    groups: Tuple[int, ...] = (133, 20, 5)
    value_channels: int = 1

    def __post_init__(self):
        object.__setattr__(self, "groups", tuple(int(g) for g in self.groups))
        object.__setattr__(self, "value_channels", int(self.value_channels))
        if self.value_channels < 0 or not 1 <= self.planes <= MAX_PLANES:
            raise ValueError(f"SegLayout: {len(self.groups)} groups + {self.value_channels} value channels (1 .. {MAX_PLANES} planes in all)")
        if any(not 1 <= g <= MAX_GROUP for g in self.groups):
            raise ValueError(f"SegLayout: group sizes {self.groups} must be in 1 .. {MAX_GROUP}")

    @property
    def planes(self) -> int:
        return len(self.groups) + self.value_channels

    @property
    def channels(self) -> int:
        return sum(self.groups) + self.value_channels

    @property
    def bases(self) -> Tuple[int, ...]:
        """first channel of every plane"""
        out, c = [], 0
        for g in self.groups:
            out.append(c)
            c += g
        return tuple(out + [c + k for k in range(self.value_channels)])


class SegLabels:
    """``planes`` uint8 ``[B, P, H, W]`` + ``layout``: stands for the dense ``[B, C, H, W]`` map as far as the training loop touches it
    (``.to`` / ``.cuda`` / ``.pin_memory``, ``.device``, ``len``, batch indexing, the logical ``.shape``)."""

    def __init__(self, planes: torch.Tensor, layout: Optional[SegLayout] = None):
        layout = layout if layout is not None else SegLayout()
        if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or planes.dim() != 4:
            raise ValueError(f"SegLabels: planes must be a uint8 tensor [B, P, H, W], got {getattr(planes, 'dtype', type(planes))} "
                             f"{tuple(getattr(planes, 'shape', ()))}")
        if planes.shape[1] != layout.planes:
            raise ValueError(f"SegLabels: {planes.shape[1]} planes, the layout has {layout.planes}")
        self.planes = planes
        self.layout = layout

    # ---- the tensor surface train.py uses ------------------------------------------------------------------------------------
    @property
    def shape(self) -> torch.Size:
        b, _, h, w = self.planes.shape
        return torch.Size((b, self.layout.channels, h, w))

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self) -> int:
        return 4

    @property
    def device(self) -> torch.device:
        return self.planes.device

    @property
    def is_cuda(self) -> bool:
        return self.planes.is_cuda

    requires_grad = False

    def __len__(self) -> int:
        return self.planes.shape[0]

    def __getitem__(self, idx) -> "SegLabels":
        """indexing along the batch: an integer keeps the batch axis (``labels[i]`` is a batch of one)"""
        if isinstance(idx, tuple):
            raise IndexError("SegLabels: only the batch axis can be indexed")
        if isinstance(idx, int):
            if not -len(self) <= idx < len(self):
                raise IndexError(f"SegLabels: index {idx} out of range for a batch of {len(self)}")
            idx = slice(idx, idx + 1) if idx != -1 else slice(idx, None)
        return SegLabels(self.planes[idx], self.layout)

    def to(self, *args, **kwargs) -> "SegLabels":
        """moves the planes; a dtype is not taken (the planes stay uint8: ``dense(dtype=...)`` makes the float map)"""
        if any(isinstance(a, torch.dtype) for a in args) or kwargs.get("dtype") is not None:
            raise TypeError("SegLabels.to: label planes stay uint8; use dense(dtype=...) for a float map")
        return SegLabels(self.planes.to(*args, **kwargs), self.layout)

    def cuda(self, device=None, non_blocking: bool = False) -> "SegLabels":
        return SegLabels(self.planes.cuda(device, non_blocking=non_blocking), self.layout)

    def cpu(self) -> "SegLabels":
        return SegLabels(self.planes.cpu(), self.layout)

    def pin_memory(self) -> "SegLabels":
        return SegLabels(self.planes.pin_memory(), self.layout)

    def is_pinned(self) -> bool:
        return self.planes.is_pinned()

    def contiguous(self) -> "SegLabels":
        return self if self.planes.is_contiguous() else SegLabels(self.planes.contiguous(), self.layout)

    def __repr__(self) -> str:
        return f"SegLabels(shape={tuple(self.shape)}, planes={tuple(self.planes.shape)}, device={self.device}, layout={self.layout})"

    # ---- the dense map -------------------------------------------------------------------------------------------------------
    def dense(self, dtype: torch.dtype = torch.float32, memory_format: torch.memory_format = torch.contiguous_format) -> torch.Tensor:
        """the one-hot map ``[B, C, H, W]``.  CPU planes: torch ops (dataset code).  GPU planes: ``ops.seg_expand`` (csrc/seg_labels.hip)."""
        if memory_format not in (torch.contiguous_format, torch.channels_last):
            raise ValueError("SegLabels.dense: memory_format must be torch.contiguous_format or torch.channels_last")
        if self.planes.is_cuda:
            from . import ops
            return ops.seg_expand(self, dtype=dtype, channels_last=memory_format == torch.channels_last)
        lay = self.layout
        b, _, h, w = self.planes.shape
        out = torch.zeros((b, lay.channels, h, w), dtype=dtype)
        for k, (g, base) in enumerate(zip(lay.groups, lay.bases)):
            v = self.planes[:, k].long()
            ok = (v >= 1) & (v <= g)
            idx = (base + v - 1).clamp_(base, base + g - 1).unsqueeze(1)
            out.scatter_(1, idx, ok.unsqueeze(1).to(dtype))       # (a pixel without a class writes a 0 into the group's first channel)
        for k in range(lay.value_channels):
            out[:, sum(lay.groups) + k] = self.planes[:, len(lay.groups) + k].to(dtype)
        return out.contiguous(memory_format=memory_format)
