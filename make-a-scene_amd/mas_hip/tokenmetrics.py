"""What a stage-2 run is judged by: the holder of what ``ops.token_agreement`` accumulates on the GPU
(csrc/token_readout.hip) -- per position of the token grid the fp64 sums of the negative log-likelihood and of the predictive entropy, the
number of tokens counted and the top-k hits; over all positions the histogram of the true token's rank and the number of invalid rows.

``TokenAgreement`` holds device tensors and combines with ``+`` / ``+=`` without a host read, so a validation loop accumulates batches as
``SegAgreement`` and ``CodeUsage`` do; ``dist.all_reduce`` of each of ``.tensors()`` makes it the global one.  Perplexity, bits per token,
accuracy and the per-position maps are derived with torch, in fp64, when asked for.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import TOKEN_MAX_KS, TOKEN_RANK_BINS

MAX_KS = TOKEN_MAX_KS          # MAS_TOKEN_MAX_KS of include/mas_hip.h
RANK_BINS = TOKEN_RANK_BINS    # MAS_TOKEN_RANK_BINS

_FIELDS = ("nll_sum", "entropy_sum", "count", "hits", "rank_hist", "invalid")


def check_ks(ks, what: str = "token_agreement") -> Tuple[int, ...]:
    """the top-k thresholds as a tuple of ints: 1 .. MAX_KS of them, each at least 1"""
    try:
        out = tuple(int(k) for k in ks)
        same = all(o == k for o, k in zip(out, ks))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: ks {ks!r} must be a sequence of integers") from None
    if not same or not 1 <= len(out) <= MAX_KS or any(k < 1 or k > 2 ** 31 - 1 for k in out):
        raise ValueError(f"{what}: ks {ks!r} must be 1 .. {MAX_KS} integer thresholds, each at least 1")
    return out


class TokenAgreement:
    """``nll_sum`` and ``entropy_sum`` float64 ``[L]``, ``count`` int64 ``[L]``, ``hits`` int64 ``[L, len(ks)]``, ``rank_hist`` int64
    ``[RANK_BINS]`` (bin 0: rank 0, bin b: rank in ``[2^(b-1), 2^b)``) and ``invalid`` int64 ``[1]``, all contiguous on one device, and the
    thresholds ``ks``.  ``+`` / ``+=`` add element-wise; ``ops.token_agreement(..., out=acc)`` adds a batch in place."""

    def __init__(self, positions: int, ks: Sequence[int] = (1, 5), device=None, tensors: Optional[Sequence[torch.Tensor]] = None):
        positions = int(positions)
        if positions < 1:
            raise ValueError(f"TokenAgreement: positions = {positions} must be positive")
        self.ks = check_ks(ks, "TokenAgreement")
        self.positions = positions
        shapes = ((positions,), (positions,), (positions,), (positions, len(self.ks)), (RANK_BINS,), (1,))
        dtypes = (torch.float64, torch.float64, torch.int64, torch.int64, torch.int64, torch.int64)
        if tensors is None:
            tensors = [torch.zeros(s, dtype=d, device=device) for s, d in zip(shapes, dtypes)]
        tensors = list(tensors)
        if len(tensors) != len(_FIELDS):
            raise ValueError(f"TokenAgreement: {len(_FIELDS)} tensors ({', '.join(_FIELDS)}), got {len(tensors)}")
        for name, t, s, d in zip(_FIELDS, tensors, shapes, dtypes):
            if not isinstance(t, torch.Tensor) or t.dtype != d or tuple(t.shape) != s or not t.is_contiguous():
                raise ValueError(f"TokenAgreement: {name} must be a contiguous {d} tensor {list(s)}, got {getattr(t, 'dtype', type(t))} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            if t.device != tensors[0].device:
                raise ValueError("TokenAgreement: the six tensors must be on one device")
        self.nll_sum, self.entropy_sum, self.count, self.hits, self.rank_hist, self.invalid = tensors

    def tensors(self) -> Tuple[torch.Tensor, ...]:
        """the six accumulators, in the order of the constructor: all_reduce each (SUM) and the holder is the global one"""
        return (self.nll_sum, self.entropy_sum, self.count, self.hits, self.rank_hist, self.invalid)

    @property
    def device(self) -> torch.device:
        return self.nll_sum.device

    def _same(self, other):
        if not isinstance(other, TokenAgreement):
            raise ValueError(f"TokenAgreement: cannot add a {type(other).__name__}")
        if other.ks != self.ks or other.positions != self.positions:
            raise ValueError(f"TokenAgreement: ks {self.ks} / {self.positions} positions and ks {other.ks} / {other.positions} positions "
                             "cannot be added")

    def __add__(self, other: "TokenAgreement") -> "TokenAgreement":
        self._same(other)
        return TokenAgreement(self.positions, self.ks, tensors=[a + b.to(a.device) for a, b in zip(self.tensors(), other.tensors())])

    def __iadd__(self, other: "TokenAgreement") -> "TokenAgreement":
        self._same(other)
        for a, b in zip(self.tensors(), other.tensors()):
            a += b.to(a.device)
        return self

    # ---- derived with torch, in fp64, when asked for ----------------------------------------------------------------------------
    @property
    def tokens(self) -> torch.Tensor:
        """the tokens counted (neither ignored nor invalid)"""
        return self.count.sum()

    @property
    def nll(self) -> torch.Tensor:
        """nats per token: the mean negative log-likelihood of the counted tokens (NaN when there are none)"""
        return self.nll_sum.sum() / self.tokens.double()

    @property
    def perplexity(self) -> torch.Tensor:
        return torch.exp(self.nll)

    @property
    def bits_per_token(self) -> torch.Tensor:
        return self.nll / math.log(2.0)

    @property
    def mean_entropy(self) -> torch.Tensor:
        return self.entropy_sum.sum() / self.tokens.double()

    @property
    def accuracy(self) -> torch.Tensor:
        """float64 ``[len(ks)]``: the share of counted tokens whose rank is below each threshold (top-k accuracy)"""
        return self.hits.sum(0).double() / self.tokens.double()

    @property
    def nll_by_position(self) -> torch.Tensor:
        """float64 ``[L]``; NaN where no token was counted"""
        return self.nll_sum / self.count.double()

    @property
    def entropy_by_position(self) -> torch.Tensor:
        return self.entropy_sum / self.count.double()

    @property
    def accuracy_by_position(self) -> torch.Tensor:
        """float64 ``[L]``: the accuracy at the FIRST threshold ``ks[0]`` (top-1 by default); NaN where no token was counted"""
        return self.hits[:, 0].double() / self.count.double()

    @property
    def topk_by_position(self) -> torch.Tensor:
        """float64 ``[L, len(ks)]``: ``accuracy_by_position`` for every threshold"""
        return self.hits.double() / self.count.double()[:, None]

    def grid(self, side: int, values: Optional[torch.Tensor] = None) -> torch.Tensor:
        """a per-position vector ``[L]`` (``nll_by_position`` unless given) or ``[L, n]`` map as the ``[side, side]`` (``[side, side, n]``)
        token grid, row-major as the tokens are generated; ``L`` must be ``side * side``"""
        side = int(side)
        values = self.nll_by_position if values is None else values
        if side * side != self.positions or values.shape[0] != self.positions:
            raise ValueError(f"TokenAgreement.grid: {self.positions} positions ({tuple(values.shape)} values) are not a {side} x {side} grid")
        return values.reshape(side, side, *values.shape[1:])

    def __repr__(self) -> str:
        return f"TokenAgreement(positions={self.positions}, ks={self.ks}, device={self.device})"
