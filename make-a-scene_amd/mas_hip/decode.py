"""Wrappers of the device-state decode entries (``make-a-scene_amd/csrc/decode_step.hip``; C contract in include/mas_hip.h): the kernels
of one captured token step of ``MakeAScene.generate(graph=True)``.  Every per-token value (step, cache length, temperature, guidance
scale, seed) is a device tensor the kernels read, so the calls below capture into a graph that is valid for every token."""
from __future__ import annotations

from typing import Optional

import torch

from . import ATTN_DECODE_MAX_SPLITS, ATTN_DECODE_SHARED_QT, _DT, _ptr, _require_cuda, _stream, check, lib
from .ops import _ATTN_HEAD_DIMS, _shared_layout, _shared_workspace

GREEDY, SAMPLE, FORCED = 0, 1, 2
AUTO_MAX_SPLITS = 8   # resolve_kv_splits("auto") never goes beyond: more splits measured slower
AUTO_MAX_PROMPT_SPLITS = 4   # resolve_prompt_splits("auto") likewise (shared prompt)
# Measurement only: an integer here replaces "auto" as the prompt split count of generate(num_samples=n, share_prompt=True), which has
# no argument for it (tools/sample_bench.py --prompt-splits sets it around a call and puts None back).  It is part of the graph key.
PROMPT_SPLITS_OVERRIDE = None


def resolve_kv_splits(kv_splits, rows: int, n_heads: int, n_cus: int) -> int:
    """The split count of the decode attention for ``kv_splits`` = None (1: the one-work-group kernel), an integer in
    [1, ATTN_DECODE_MAX_SPLITS] (itself) or ``"auto"``: the largest power of two n with rows * n_heads * n <= 2 * n_cus, clamped to
    [1, AUTO_MAX_SPLITS = 8] -- the rule the measured table of DESIGN 2.6 gives (rows * heads 16 ... 256 on 256 compute units: the best
    or within the run-to-run spread of the best column in every row; 16 splits lost to 8 everywhere; beyond rows * heads = 2 * n_cus,
    which nobody has measured, it is 1).  Anything else raises ValueError."""
    if kv_splits is None:
        return 1
    if isinstance(kv_splits, str):
        if kv_splits != "auto":
            raise ValueError(f"kv_splits: {kv_splits!r} is neither an integer nor 'auto'")
        if rows < 1 or n_heads < 1 or n_cus < 1:
            raise ValueError(f"kv_splits='auto': rows={rows}, n_heads={n_heads}, n_cus={n_cus} must be positive")
        n = 1
        while 2 * n <= AUTO_MAX_SPLITS and rows * n_heads * 2 * n <= 2 * n_cus:
            n *= 2
        return n
    if isinstance(kv_splits, bool) or not isinstance(kv_splits, int):
        raise ValueError(f"kv_splits: {kv_splits!r} is neither an integer nor 'auto'")
    if not 1 <= kv_splits <= ATTN_DECODE_MAX_SPLITS:
        raise ValueError(f"kv_splits: {kv_splits} outside [1, {ATTN_DECODE_MAX_SPLITS}]")
    return kv_splits


def split_workspace_floats(rows: int, n_heads: int, head_dim: int, n_split: int) -> int:
    """fp32 elements of the split decode attention's workspace: one {o[hd], m, l} state per (row, head, split)"""
    return rows * n_heads * n_split * (head_dim + 2)


def shared_workspace_floats(rows: int, heads: int, hd: int, prompt_splits: int, own_splits: int) -> int:
    """fp32 elements of the shared-prompt decode attention's workspace: one {o[hd], m, l} state per (row, head) and per key range, the
    ``prompt_splits`` ranges of the prompt block first, then the ``own_splits`` ranges of the row's own cache"""
    return rows * heads * (prompt_splits + own_splits) * (hd + 2)


def resolve_prompt_splits(value, groups: int, group: int, heads: int, n_cus: int) -> int:
    """The number of key ranges the prompt block of ``attention_decode_shared`` is split into: an integer in
    [1, ATTN_DECODE_MAX_SPLITS] (itself) or ``"auto"``: the largest power of two n <= AUTO_MAX_PROMPT_SPLITS = 4 with
    groups * ceil(group / QT) * heads * n <= n_cus -- ``resolve_kv_splits``'s rule applied to the prompt work-groups of the partial
    launch (QT = ATTN_DECODE_SHARED_QT rows of a group per work-group), with the bound and the clamp the measurement of DESIGN 2.6
    gives: at the four measured points (one prompt of 512 positions, 8 and 32 candidates, plain and guided: 32 / 64 / 128 / 256 prompt
    work-groups on 256 compute units) it picks 4 / 4 / 2 / 1 ranges, the best measured column at each.  The rule first written down
    (2 * n_cus, clamp 8: 8 / 8 / 4 / 2) lost 0.005 - 0.044 ms per token to it.  Beyond those points (other prompt lengths, more than 256
    prompt work-groups) it is unmeasured.  Anything else raises ValueError."""
    if isinstance(value, str):
        if value != "auto":
            raise ValueError(f"prompt_splits: {value!r} is neither an integer nor 'auto'")
        if groups < 1 or group < 1 or heads < 1 or n_cus < 1:
            raise ValueError(f"prompt_splits='auto': groups={groups}, group={group}, heads={heads}, n_cus={n_cus} must be positive")
        blocks = groups * (-(-group // ATTN_DECODE_SHARED_QT)) * heads
        n = 1
        while 2 * n <= AUTO_MAX_PROMPT_SPLITS and blocks * 2 * n <= n_cus:
            n *= 2
        return n
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"prompt_splits: {value!r} is neither an integer nor 'auto'")
    if not 1 <= value <= ATTN_DECODE_MAX_SPLITS:
        raise ValueError(f"prompt_splits: {value} outside [1, {ATTN_DECODE_MAX_SPLITS}]")
    return value


def attention_decode_shared_dev(qkv: torch.Tensor, prompt_k: torch.Tensor, prompt_v: torch.Tensor, k_cache: torch.Tensor,
                                v_cache: torch.Tensor, past: torch.Tensor, n_heads: int, *, group: int, prompt_splits: int = 1,
                                kv_splits: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
                                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``attention_decode_dev`` for candidates that share a prompt (``mas_attn_decode_shared_dev``): qkv [rows, 1, 3D], prompt blocks
    [rows / group, prompt_len, D] (read-only, block g serves rows g * group .. (g + 1) * group - 1), own caches [rows, cap, D] that hold
    the image positions only, ``past`` a device int32 that counts the prompt too.  Appends k / v of the new row at own cache row
    ``past - prompt_len`` and returns the context [rows, 1, D] of the query over its prompt block and its own rows 0 .. past -
    prompt_len.  ``prompt_splits`` / ``kv_splits``: key ranges of the prompt block / of the own cache (None: 1); ``workspace``: fp32, at
    least ``shared_workspace_floats(rows, n_heads, hd, prompt_splits, kv_splits)`` elements (allocated here when None)."""
    who = "attention_decode_shared_dev"
    _require_cuda(qkv, who)
    if qkv.dim() != 3 or qkv.shape[2] % 3:
        raise RuntimeError(f"{who}: qkv [rows, 1, 3D]")
    d = qkv.shape[2] // 3
    q = qkv[..., :d]
    rows, d, hd, nsp, nso = _shared_layout(who, q, prompt_k, prompt_v, k_cache, v_cache, n_heads, group, prompt_splits, kv_splits)
    if past.dtype != torch.int32 or past.device != qkv.device:
        raise RuntimeError(f"{who}: past is a device int32")
    workspace = _shared_workspace(who, workspace, shared_workspace_floats(rows, n_heads, hd, nsp, nso), qkv.device)
    if out is None:
        out = torch.empty((rows, 1, d), dtype=qkv.dtype, device=qkv.device)
    check(lib().mas_attn_decode_shared_dev(_ptr(q), _ptr(qkv[..., d:2 * d]), _ptr(qkv[..., 2 * d:]), qkv.stride(0), _ptr(prompt_k),
                                           _ptr(prompt_v), prompt_k.stride(1), prompt_k.stride(0), prompt_k.shape[1], _ptr(k_cache),
                                           _ptr(v_cache), k_cache.stride(1), k_cache.stride(0), k_cache.shape[1], _ptr(out),
                                           out.stride(0), _DT[qkv.dtype], rows, group, n_heads, hd, _ptr(past), float(hd) ** -0.5, nsp,
                                           nso, _ptr(workspace), workspace.numel(), _stream()), "attn_decode_shared_dev")
    return out


def attention_decode_dev(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, past: torch.Tensor, n_heads: int,
                         out: Optional[torch.Tensor] = None, *, kv_splits: Optional[int] = None,
                         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv [B, 1, 3D] (the new row's projection, q | k | v), caches [B, cap, D], ``past`` a device int32 (one element): appends k / v of
    the new row at cache row ``past`` and returns the context [B, 1, D] of the query over rows 0 .. past (``mas_attn_decode_dev``).
    ``kv_splits`` n > 1: the keys of every (row, head) are shared by n work-groups and merged by a second launch
    (``mas_attn_decode_split_dev``); ``workspace``: fp32, at least ``split_workspace_floats(B, n_heads, hd, n)`` elements (a capture
    passes a static one; allocated here when None)."""
    _require_cuda(qkv, "attention_decode_dev")
    b, nq, d3 = qkv.shape
    d = d3 // 3
    hd = d // n_heads
    n_split = 1 if kv_splits is None else int(kv_splits)
    if not 1 <= n_split <= ATTN_DECODE_MAX_SPLITS:
        raise RuntimeError(f"attention_decode_dev: kv_splits {kv_splits} outside [1, {ATTN_DECODE_MAX_SPLITS}]")
    if nq != 1 or qkv.dtype not in _DT or k_cache.dtype != qkv.dtype or v_cache.dtype != qkv.dtype:
        raise RuntimeError("attention_decode_dev: one new row; q / k / v and the caches share a dtype in {float32, bfloat16}")
    if k_cache.shape != v_cache.shape or k_cache.shape[0] != b or k_cache.shape[2] != d or not k_cache.is_contiguous() \
            or not v_cache.is_contiguous() or qkv.stride(2) != 1:
        raise RuntimeError(f"attention_decode_dev: caches {tuple(k_cache.shape)} must be contiguous [B, cap, {d}]")
    if hd not in _ATTN_HEAD_DIMS:
        raise RuntimeError(f"attention_decode_dev: head width {hd} not in {_ATTN_HEAD_DIMS}")
    if past.dtype != torch.int32 or past.device != qkv.device:
        raise RuntimeError("attention_decode_dev: past is a device int32")
    if out is None:
        out = torch.empty((b, 1, d), dtype=qkv.dtype, device=qkv.device)
    q = qkv[..., :d]
    if n_split > 1:
        need = split_workspace_floats(b, n_heads, hd, n_split)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.float32, device=qkv.device)
        elif workspace.dtype != torch.float32 or workspace.device != qkv.device or not workspace.is_contiguous() or workspace.numel() < need:
            raise RuntimeError(f"attention_decode_dev: the workspace is a contiguous device fp32 tensor of at least {need} elements")
        check(lib().mas_attn_decode_split_dev(_ptr(q), _ptr(qkv[..., d:2 * d]), _ptr(qkv[..., 2 * d:]), qkv.stride(0), _ptr(k_cache),
                                              _ptr(v_cache), k_cache.stride(1), k_cache.stride(0), k_cache.shape[1], _ptr(out),
                                              out.stride(0), _DT[qkv.dtype], b, n_heads, hd, _ptr(past), float(hd) ** -0.5, n_split,
                                              _ptr(workspace), workspace.numel(), _stream()), "attn_decode_split_dev")
        return out
    check(lib().mas_attn_decode_dev(_ptr(q), _ptr(qkv[..., d:2 * d]), _ptr(qkv[..., 2 * d:]), qkv.stride(0), _ptr(k_cache), _ptr(v_cache),
                                    k_cache.stride(1), k_cache.stride(0), k_cache.shape[1], _ptr(out), out.stride(0), _DT[qkv.dtype], b,
                                    n_heads, hd, _ptr(past), float(hd) ** -0.5, _stream()), "attn_decode_dev")
    return out


def decode_embed(tokens: torch.Tensor, step: torch.Tensor, img_emb: torch.Tensor, row_emb: torch.Tensor, col_emb: torch.Tensor,
                 out: torch.Tensor) -> torch.Tensor:
    """out [rows, ..., D] fp32 (rows = B, or 2B under guidance) = the embedding of tokens[r % B, step - 1] at image position step - 1
    (``mas_decode_embed``); tokens int64 [B, n*n], step a device int32."""
    _require_cuda(tokens, "decode_embed")
    b, length = tokens.shape
    d = img_emb.shape[1]
    n = row_emb.shape[0]
    if tokens.dtype != torch.int64 or tokens.stride(1) != 1 or length != n * n or step.dtype != torch.int32:
        raise RuntimeError("decode_embed: tokens int64 [B, n*n] (row-major), step int32")
    for t in (img_emb, row_emb, col_emb, out):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != d:
            raise RuntimeError("decode_embed: fp32 contiguous embedding tables and output of width D")
    rows = out.numel() // d
    check(lib().mas_decode_embed(_ptr(tokens), tokens.stride(0), _ptr(step), _ptr(img_emb), img_emb.shape[0], _ptr(row_emb),
                                 _ptr(col_emb), n, _ptr(out), b, rows, d, _stream()), "decode_embed")
    return out


def sample_tokens(logits: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, params: torch.Tensor, mode: int, *, top_k: int = 0,
                  guided: bool = False, seed: Optional[torch.Tensor] = None, forced: Optional[torch.Tensor] = None,
                  logits_out: Optional[torch.Tensor] = None, rows: Optional[int] = None, top_p: bool = False,
                  keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One token per row into tokens[r, *step] (``mas_sample_tokens``; with ``top_p`` ``mas_sample_tokens_topp``, whose params hold a
    third float, the nucleus mass: include/mas_hip.h "Top-p" -- the value lives on the device like the temperature, the flag only selects
    the entry).  logits fp32 [R, V] with R = 2B under guidance (conditional rows
    first, as ``generate`` stacks them) or B, or a single [1, V] / [2, V] row shared by ``rows`` output rows (row stride 0: the statistics
    tests).  params fp32 {temperature, cond_scale}; seed int64 {seed, offset}; forced int64 [B, L] (teacher forcing); logits_out fp32
    [B, L, V] receives the mixed row.  ``keep`` uint8 [B, L] (image prompt, ``mas_sample_tokens_prompt``): row r at step k gets
    ``forced[r, k]`` where ``keep[r, k]`` is non-zero and the GREEDY / SAMPLE token otherwise; it needs ``forced`` and the three-float
    params (top_p = 1.0: off), and is an error with FORCED, which keeps every position already."""
    if keep is not None:
        if mode not in (GREEDY, SAMPLE):
            raise RuntimeError("sample_tokens: keep goes with GREEDY or SAMPLE (FORCED keeps every position)")
        if forced is None:
            raise RuntimeError("sample_tokens: keep needs the forced tokens it keeps")
    _require_cuda(logits, "sample_tokens")
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError("sample_tokens: fp32 logits [R, V] with contiguous rows")
    nb, length = tokens.shape
    v = logits.shape[1]
    shared = rows is not None
    if tokens.dtype != torch.int64 or tokens.stride(1) != 1 or step.dtype != torch.int32 or params.dtype != torch.float32 \
            or params.numel() < (3 if top_p or keep is not None else 2) or not params.is_contiguous():
        raise RuntimeError("sample_tokens: tokens int64 [B, L], step int32, params fp32 {temperature, cond_scale} (and top_p with top_p=True)")
    if shared:
        if rows != nb or logits.shape[0] != (2 if guided else 1):
            raise RuntimeError("sample_tokens: a shared logits row (and its unconditional row) for every output row")
        ld, uoff = 0, v
    else:
        if logits.shape[0] != (2 * nb if guided else nb):
            raise RuntimeError(f"sample_tokens: {logits.shape[0]} logits rows for {nb} output rows (guided={guided})")
        ld, uoff = logits.stride(0), nb * logits.stride(0)
    if mode == SAMPLE and (seed is None or seed.dtype != torch.int64 or seed.numel() < 2):
        raise RuntimeError("sample_tokens: sampling needs the int64 {seed, offset} tensor")
    if (mode == FORCED or keep is not None) and (forced is None or forced.dtype != torch.int64 or forced.shape != tokens.shape
                                                 or forced.stride(1) != 1 or forced.device != logits.device):
        raise RuntimeError("sample_tokens: teacher forcing needs int64 tokens shaped like the output")
    if keep is not None and (keep.dtype != torch.uint8 or keep.shape != tokens.shape or keep.stride(1) != 1 or keep.device != logits.device):
        raise RuntimeError("sample_tokens: keep is a device uint8 mask shaped like the output")
    if logits_out is not None and (logits_out.dtype != torch.float32 or logits_out.shape != (nb, length, v) or not logits_out.is_contiguous()):
        raise RuntimeError("sample_tokens: logits_out fp32 contiguous [B, L, V]")
    if keep is not None:
        check(lib().mas_sample_tokens_prompt(_ptr(logits), ld, uoff, nb, v, int(guided), int(mode), int(top_k or 0), _ptr(params), _ptr(seed),
                                             _ptr(step), length, _ptr(forced), forced.stride(0), _ptr(tokens), tokens.stride(0),
                                             _ptr(logits_out), logits_out.stride(0) if logits_out is not None else 0, _ptr(keep),
                                             keep.stride(0), _stream()), "sample_tokens_prompt")
        return tokens
    entry = lib().mas_sample_tokens_topp if top_p else lib().mas_sample_tokens
    check(entry(_ptr(logits), ld, uoff, nb, v, int(guided), int(mode), int(top_k or 0), _ptr(params), _ptr(seed), _ptr(step), length,
                _ptr(forced), forced.stride(0) if forced is not None else 0, _ptr(tokens), tokens.stride(0), _ptr(logits_out),
                logits_out.stride(0) if logits_out is not None else 0, _stream()), "sample_tokens")
    return tokens


def advance(counters: torch.Tensor) -> None:
    """counters (device int32, contiguous) += 1, one thread, ordered after the step's kernels (``mas_decode_advance``)"""
    if counters.dtype != torch.int32 or not counters.is_contiguous():
        raise RuntimeError("decode advance: contiguous int32 counters")
    check(lib().mas_decode_advance(_ptr(counters), counters.numel(), _stream()), "decode_advance")
