"""What a VQ-IMG reconstruction is judged by: the byte rule that turns a float image into a picture, and the two holders of
what ``ops.image_agreement`` and ``ops.code_usage`` count on the GPU (csrc/img_metrics.hip).

``ImageAgreement``: per image the integer squared error of the bytes and the fp64 SSIM, from which MSE and PSNR are derived with torch when
asked for.  ``CodeUsage``: how often every code of the codebook was chosen, from which perplexity and the dead codes follow -- the numbers
the reference's reservoir / k-means re-initialisation schedule (models/modules.py:477-499) exists to keep healthy.  Both hold device
tensors and combine with ``+`` / ``+=`` without a host read, so a validation loop accumulates batches as ``SegAgreement`` does.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import IMG_MAX_CHANNELS, IMG_SSIM_WINDOW

MAX_CHANNELS = IMG_MAX_CHANNELS     # MAS_IMG_MAX_CHANNELS of include/mas_hip.h
WINDOW = IMG_SSIM_WINDOW            # MAS_IMG_SSIM_WINDOW
SIGMA = 1.5


def ssim_window() -> Tuple[float, ...]:
    """the eleven weights ``exp(-(i - 5)^2 / (2 1.5^2))`` normalised to sum 1, as Python floats (fp64): what the kernel is handed"""
    g = [math.exp(-((i - WINDOW // 2) ** 2) / (2.0 * SIGMA * SIGMA)) for i in range(WINDOW)]
    total = math.fsum(g)
    return tuple(v / total for v in g)


def byte_range(lo, hi, what: str = "image_bytes") -> Tuple[float, float]:
    """checks ``lo < hi``, both finite -> (lo, hi) as Python floats"""
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the range ({lo!r}, {hi!r}) must be two numbers") from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
        raise ValueError(f"{what}: the range [{lo}, {hi}] must be finite with lo < hi")
    return lo, hi


class ImageAgreement:
    """``sse`` int64 ``[N]`` (the squared error of the bytes, summed over C H W), ``ssim`` float64 ``[N]`` (NaN for a picture smaller than
    the 11 x 11 window) and ``elements`` int64 ``[N]`` (C H W of each image), all on one device.  ``+`` / ``+=`` concatenate along the
    batch (``torch.cat``: no host read), so batches of different sizes and picture sizes accumulate."""

    def __init__(self, sse: torch.Tensor, ssim: torch.Tensor, elements: torch.Tensor):
        for name, t, dt in (("sse", sse, torch.int64), ("ssim", ssim, torch.float64), ("elements", elements, torch.int64)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
                raise ValueError(f"ImageAgreement: {name} must be a {dt} tensor [N], got {getattr(t, 'dtype', type(t))} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
        if not (sse.shape == ssim.shape == elements.shape) or not (sse.device == ssim.device == elements.device):
            raise ValueError("ImageAgreement: sse, ssim and elements must have one length and one device")
        self.sse, self.ssim, self.elements = sse, ssim, elements

    def __len__(self) -> int:
        return self.sse.shape[0]

    @property
    def device(self) -> torch.device:
        return self.sse.device

    def _same(self, other):
        if not isinstance(other, ImageAgreement):
            raise ValueError(f"ImageAgreement: cannot add a {type(other).__name__}")

    def __add__(self, other: "ImageAgreement") -> "ImageAgreement":
        self._same(other)
        dev = self.device
        return ImageAgreement(torch.cat([self.sse, other.sse.to(dev)]), torch.cat([self.ssim, other.ssim.to(dev)]),
                              torch.cat([self.elements, other.elements.to(dev)]))

    def __iadd__(self, other: "ImageAgreement") -> "ImageAgreement":
        merged = self + other
        self.sse, self.ssim, self.elements = merged.sse, merged.ssim, merged.elements
        return self

    @property
    def mse(self) -> torch.Tensor:
        """float64 ``[N]``: sse / elements, on the 0 .. 255 scale"""
        return self.sse.double() / self.elements.double()

    @property
    def psnr(self) -> torch.Tensor:
        """float64 ``[N]``: 10 log10(255^2 / mse); ``+inf`` for identical pictures"""
        return 10.0 * torch.log10(255.0 ** 2 / self.mse)

    @property
    def mean_ssim(self) -> torch.Tensor:
        return self.ssim.mean()

    @property
    def mean_psnr(self) -> torch.Tensor:
        return self.psnr.mean()

    @property
    def pooled_psnr(self) -> torch.Tensor:
        """PSNR of the pooled error, sum sse / sum elements: finite as soon as one picture differs"""
        return 10.0 * torch.log10(255.0 ** 2 / (self.sse.sum().double() / self.elements.sum().double()))

    def __repr__(self) -> str:
        return f"ImageAgreement(images={len(self)}, device={self.device})"


class CodeUsage:
    """``counts`` int64 ``[K + 1]``: how often each of the ``K`` codes was chosen, and in ``counts[K]`` the indices outside ``[0, K)``.
    ``+`` / ``+=`` add counts, and ``ops.code_usage(..., out=acc)`` adds a batch in place."""

    def __init__(self, n_embed: int, counts: Optional[torch.Tensor] = None, device=None):
        n_embed = int(n_embed)
        if n_embed < 1:
            raise ValueError(f"CodeUsage: n_embed = {n_embed} must be positive")
        if counts is None:
            counts = torch.zeros(n_embed + 1, dtype=torch.int64, device=device)
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or tuple(counts.shape) != (n_embed + 1,) \
                or not counts.is_contiguous():
            raise ValueError(f"CodeUsage: counts must be a contiguous int64 tensor [{n_embed + 1}] for {n_embed} codes")
        self.n_embed = n_embed
        self.counts = counts

    def _same(self, other):
        if not isinstance(other, CodeUsage) or other.n_embed != self.n_embed:
            raise ValueError("CodeUsage: counts of different codebook sizes cannot be added")

    def __add__(self, other: "CodeUsage") -> "CodeUsage":
        self._same(other)
        return CodeUsage(self.n_embed, self.counts + other.counts.to(self.counts.device))

    def __iadd__(self, other: "CodeUsage") -> "CodeUsage":
        self._same(other)
        self.counts += other.counts.to(self.counts.device)
        return self

    @property
    def per_code(self) -> torch.Tensor:
        return self.counts[:self.n_embed]

    @property
    def total(self) -> torch.Tensor:
        """the indices inside ``[0, K)``"""
        return self.per_code.sum()

    @property
    def out_of_range(self) -> torch.Tensor:
        return self.counts[self.n_embed]

    @property
    def used(self) -> torch.Tensor:
        return (self.per_code > 0).sum()

    @property
    def dead(self) -> torch.Tensor:
        return self.n_embed - self.used

    @property
    def perplexity(self) -> torch.Tensor:
        """exp(-sum p ln p) over p = counts / total in fp64, with 0 ln 0 = 0: K for a uniform use of the codebook, 1 for a single code"""
        p = self.per_code.double() / self.total.double()
        return torch.exp(-torch.xlogy(p, p).sum())

    def __repr__(self) -> str:
        return f"CodeUsage(n_embed={self.n_embed}, device={self.counts.device})"
