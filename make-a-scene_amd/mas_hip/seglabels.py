"""The VQ-SEG segmentation map as compact label planes instead of a one-hot tensor.

The reference's dataloader (Data/dataset_preprocessor.py:62-86) turns three integer label images and an edge image per sample into a dense
``[H, W, 159]`` float one-hot map: 636 bytes per pixel for 4 bytes of information.  ``SegLabels`` keeps the 4 bytes: a ``uint8`` tensor
``[B, P, H, W]`` and a ``SegLayout`` that says which channels each plane stands for.  ``VQBASE``, the VQ-SEG losses and
``token_data.tokenize_batch`` accept it wherever they accept the dense map; on the GPU the dense map is written once, in the layout the
encoder's first convolution reads (``ops.seg_expand``), and the loss derives its target in registers (``ops.seg_loss_labels``): csrc/seg_labels.hip.

The way back: ``SegLabels.from_logits`` reads a reconstruction's logits by the reference Visualizer's rule (log_utils.py:55-67;
on the GPU ``ops.seg_classify``, csrc/seg_classify.hip), ``SegLabels.colorize`` makes pictures of the planes, and ``SegAgreement`` holds the
counts of ``ops.seg_agreement`` from which pixel accuracy and per-class IoU are derived.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch

from . import SEG_MAX_PLANES

MAX_PLANES = SEG_MAX_PLANES   # MAS_SEG_MAX_PLANES of include/mas_hip.h
MAX_GROUP = 255
REFERENCE_THRESHOLDS = (None, None, 0.2, 0.2)     # reference log_utils.py:61-67: face and edges are gated by `sigmoid > 0.2`


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


def logit_thresholds(layout: SegLayout, thresholds=None, what: str = "seg_classify") -> Tuple[float, ...]:
    """per-plane probabilities (``None``: no gate) -> the thresholds ON THE LOGIT the rule compares with: ``tau = float32(log(t / (1 - t)))``,
    computed in double and rounded once; ``-inf`` for ``None``.  One float stands for every plane; no argument means the reference's
    ``(None, None, 0.2, 0.2)``, which only the reference layout has."""
    if thresholds is None:
        if layout != SegLayout():
            raise ValueError(f"{what}: thresholds must be given for a layout other than the reference's ({layout})")
        thresholds = REFERENCE_THRESHOLDS
    if isinstance(thresholds, (int, float)):
        thresholds = (float(thresholds),) * layout.planes
    thresholds = tuple(thresholds)
    if len(thresholds) != layout.planes:
        raise ValueError(f"{what}: {len(thresholds)} thresholds for the layout's {layout.planes} planes")
    taus = []
    for t in thresholds:
        if t is None:
            taus.append(-math.inf)
            continue
        t = float(t)
        if not 0.0 < t < 1.0:
            raise ValueError(f"{what}: a threshold is a probability in (0, 1) or None, got {t}")
        taus.append(ctypes.c_float(math.log(t / (1.0 - t))).value)
    return tuple(taus)


def _check_logits(prediction, layout: SegLayout, what: str):
    if not isinstance(prediction, torch.Tensor) or prediction.dim() != 4 or prediction.numel() == 0:
        raise ValueError(f"{what}: prediction must be a non-empty tensor [N, C, H, W], got {tuple(getattr(prediction, 'shape', ()))}")
    if prediction.shape[1] != layout.channels:
        raise ValueError(f"{what}: prediction {tuple(prediction.shape)} has {prediction.shape[1]} channels, the layout has {layout.channels}")
    if prediction.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{what}: prediction dtype {prediction.dtype} not supported (float32 / bfloat16)")


def _default_palette(planes: int) -> torch.Tensor:
    pal = torch.randint(0, 256, (planes, 256, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    pal[:, 0] = 0                                                     # label 0 (no class, value 0): black
    return pal


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

    # ---- from a reconstruction's logits, and to a picture ----------------------------------------------------------------------
    @classmethod
    def from_logits(cls, prediction: torch.Tensor, layout: Optional[SegLayout] = None, thresholds=None) -> "SegLabels":
        """VQ-SEG logits ``[B, C, H, W]`` (fp32 or bf16) -> labels by the reference Visualizer's rule (log_utils.py:55-67): per
        class plane the first channel with the largest logit, 0 where that logit is not above the plane's threshold; per value plane
        ``logit > threshold``.  GPU logits: ``ops.seg_classify`` (csrc/seg_classify.hip).  CPU logits: torch ops (dataset / tool code)."""
        layout = layout if layout is not None else SegLayout()
        if isinstance(prediction, torch.Tensor) and prediction.is_cuda:
            from . import ops
            return ops.seg_classify(prediction, layout, thresholds)
        taus = logit_thresholds(layout, thresholds, "SegLabels.from_logits")
        _check_logits(prediction, layout, "SegLabels.from_logits")
        x = prediction.detach().float()                              # (bf16 widens exactly)
        b, _, h, w = x.shape
        planes = torch.zeros((b, layout.planes, h, w), dtype=torch.uint8)
        for k, (g, base) in enumerate(zip(layout.groups, layout.bases)):
            a = x[:, base:base + g].argmax(dim=1, keepdim=True)      # the first channel among equals
            m = x[:, base:base + g].gather(1, a)
            planes[:, k] = torch.where(m > taus[k], a + 1, torch.zeros_like(a))[:, 0].to(torch.uint8)
        for k in range(len(layout.groups), layout.planes):
            planes[:, k] = (x[:, layout.bases[k]] > taus[k]).to(torch.uint8)
        return cls(planes, layout)

    def colorize(self, palette: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> uint8 ``[B, P, 3, H, W]``: one RGB picture per plane, ``palette[k, byte]`` at every pixel.  ``palette`` uint8 ``[P, 256, 3]``
        (every byte has a row: no label can index outside it); the default is seeded and maps label 0 to black.  Either device."""
        if palette is None:
            palette = _default_palette(self.layout.planes)
        if not isinstance(palette, torch.Tensor) or palette.dtype != torch.uint8 or tuple(palette.shape) != (self.layout.planes, 256, 3):
            raise ValueError(f"SegLabels.colorize: palette must be a uint8 tensor [{self.layout.planes}, 256, 3], got "
                             f"{getattr(palette, 'dtype', type(palette))} {tuple(getattr(palette, 'shape', ()))}")
        palette = palette.to(self.planes.device)
        pics = [palette[k][self.planes[:, k].long()] for k in range(self.layout.planes)]     # each [B, H, W, 3]
        return torch.stack(pics, 1).permute(0, 1, 4, 2, 3).contiguous()

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


class SegAgreement:
    """What ``ops.seg_agreement`` counts between predicted and target labels of one layout (csrc/seg_classify.hip), as ONE int64 tensor
    ``counts`` of ``3 C + P + 1`` entries on the labels' device: per channel ``inter`` / ``pred`` / ``target`` (for the class channel
    ``base + v - 1`` the pixels whose predicted byte, target byte, or both equal ``v``; for a value channel the pixels whose byte is
    ``> 0``), per plane ``agree`` (the pixels where the two planes say the same), and ``pixels``.  ``+`` / ``+=`` add counts, and
    ``ops.seg_agreement(..., out=acc)`` adds a batch in place: a validation loop accumulates without a host synchronisation.  The metrics
    are derived with torch from the counts when asked for."""

    def __init__(self, layout: SegLayout, counts: Optional[torch.Tensor] = None, device=None):
        n = 3 * layout.channels + layout.planes + 1
        if counts is None:
            counts = torch.zeros(n, dtype=torch.int64, device=device)
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or tuple(counts.shape) != (n,) or not counts.is_contiguous():
            raise ValueError(f"SegAgreement: counts must be a contiguous int64 tensor [{n}] for {layout}")
        self.layout = layout
        self.counts = counts

    def _part(self, i: int) -> torch.Tensor:
        c = self.layout.channels
        return self.counts[i * c:(i + 1) * c]

    @property
    def inter(self) -> torch.Tensor:
        return self._part(0)

    @property
    def pred(self) -> torch.Tensor:
        return self._part(1)

    @property
    def target(self) -> torch.Tensor:
        return self._part(2)

    @property
    def agree(self) -> torch.Tensor:
        c = self.layout.channels
        return self.counts[3 * c:3 * c + self.layout.planes]

    @property
    def pixels(self) -> torch.Tensor:
        return self.counts[-1]

    def _same(self, other):
        if not isinstance(other, SegAgreement) or other.layout != self.layout:
            raise ValueError("SegAgreement: counts of different layouts cannot be added")

    def __add__(self, other: "SegAgreement") -> "SegAgreement":
        self._same(other)
        return SegAgreement(self.layout, self.counts + other.counts.to(self.counts.device))

    def __iadd__(self, other: "SegAgreement") -> "SegAgreement":
        self._same(other)
        self.counts += other.counts.to(self.counts.device)
        return self

    @property
    def pixel_accuracy(self) -> torch.Tensor:
        """float64 ``[P]``: the share of pixels where the plane agrees"""
        return self.agree.double() / self.pixels.double()

    @property
    def iou(self) -> torch.Tensor:
        """float64 ``[C]``: ``inter / (pred + target - inter)``, NaN for a class in neither"""
        union = self.pred + self.target - self.inter
        return torch.where(union > 0, self.inter.double() / union.double(), torch.full_like(union, float("nan"), dtype=torch.float64))

    @property
    def miou(self) -> torch.Tensor:
        """float64 ``[P]``: the mean IoU over the classes of a plane that occur (NaN where none does)"""
        iou = self.iou
        out = []
        for g, base in zip(self.layout.groups + (1,) * self.layout.value_channels, self.layout.bases):
            out.append(torch.nanmean(iou[base:base + g]))
        return torch.stack(out)

    def __repr__(self) -> str:
        return f"SegAgreement(layout={self.layout}, device={self.counts.device})"
