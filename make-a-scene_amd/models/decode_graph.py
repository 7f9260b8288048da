"""``MakeAScene.generate(graph=True)``: KV-cached sampling as one captured graph replay per image token.

The eager sampler (``MakeAScene.generate``) spends ~350 launches of host time on every token.  Here the prompt is prefilled eagerly as
there, its keys / values are copied into static per-layer caches [rows, total_length, D], the first token is drawn eagerly by the
sampler kernel, and every later token k = 1 .. L-1 is one replay of a graph captured once per configuration:

    embed tokens[:, k-1] at image position k-1 (``mas_decode_embed``)
    per layer: ln_in, qkv, decode attention that appends the row at past = plen + k - 1 (``mas_attn_decode_dev``, or with
               ``generate(kv_splits=n)`` its split-key pair ``mas_attn_decode_split_dev``), out_proj,
               first sandwich LayerNorm + residual, ln_out, lin1, GELU, lin2, second sandwich LayerNorm + residual
    final LayerNorm, to_logits, sampler (``mas_sample_tokens``, or ``mas_sample_tokens_topp`` with ``generate(top_p=p)``: tokens[:, k]
               and the logits row k), step counters + 1

The modules' own forward calls build the step (the same HIP LayerNorm / GELU kernels and library GEMMs the eager decode runs on the same
row shapes), so teacher-forced logits equal the eager ones.  The step, the cache length, temperature, guidance scale, top_p and seed live
in device buffers: one capture serves every token and every call with the same key (rows, guidance, sampling mode, top_k, whether top_p
is on -- not its value --, return_logits, compute dtype, autocast state, device, decode-attention split count).  The graph reads the parameters and their bf16 shadows in place; an
entry whose pointers moved (``load_state_dict`` into new storage, ``.to()``, ``invalidate_weight_cache()``) is recaptured.

An image prompt (``generate(img_tokens=..., keep=...)``) is one more key: the step then calls ``mas_sample_tokens_prompt``, which reads the
mask and the kept tokens from the entry's static buffers (``keep`` uint8 [B, L], ``forced``), so other masks, other tokens and another
common prefix m never recapture.  With m > 0 the prefill has already run the m leading kept tokens: the caches are copied over plen + m
rows, the counters start at step m, and the host replays L - 1 - m times.

``generate(num_samples=n, share_prompt=True)`` is a configuration of its own (its key is longer: n and the prompt split count stand in
front of the split count): the entry keeps the prompt's keys / values once per group of n candidates (``pk`` / ``pv`` [groups, plen, D]),
caches of ``image_length`` rows, and the step calls ``mas_attn_decode_shared_dev`` (see ``generate_graph``).

Tokens are drawn by Gumbel-max from Philox4x32-10 (include/mas_hip.h, "Sampling"): reproducible under ``torch.manual_seed`` or a seeded
``generator``, but not the tokens ``torch.multinomial`` would draw (the eager path's)."""
import warnings

import torch

from mas_hip import decode, ops

_GEN_SEED_HIGH = 2 ** 63 - 1


def _envelope_reason(model):
    """why the graph path cannot run this model (None: it can); the eager path then runs, warned once per module and reason"""
    layers = model.transformer.layers
    attn = layers[0].attn
    hd, rem = divmod(attn.hidden_dim, attn.num_attn_heads)
    if rem or hd not in ops._ATTN_HEAD_DIMS:
        return f"head width {attn.hidden_dim}/{attn.num_attn_heads} is not one of {ops._ATTN_HEAD_DIMS}"
    for layer in layers:
        if layer.cogview_layernorm_prescale:
            return "cogview_layernorm_prescale layers"
        if layer.rudalle_relax or layer.attn.rudalle_relax:
            return "rudalle_relax layers"
        if layer.training and max(layer.attn.attn_drop.p, layer.attn.out_drop.p, layer.mlp.dropout.p) > 0:
            return "training mode with nonzero dropout"
    emb = (model.image_token_embedding, model.image_row_embeddings, model.image_col_embeddings)
    if not all(e.weight.is_cuda and e.weight.dtype == torch.float32 for e in emb):
        return "image embeddings are not fp32 tensors on a GPU"
    return None


def _param_pointers(model):
    return tuple(p.data_ptr() for p in model.parameters())


def _pointer_signature(model, bf16_autocast):
    """data_ptr of every parameter and, under bf16 autocast, of the bf16 shadow of every Linear whose forward reads one (the layer's own
    dispatch rule, ``Linear.uses_bf16_shadow``, on the device the step runs on).  Fetching the shadows is the eager path's staleness
    check: a stale shadow is recast into its own storage before anything is replayed."""
    from .transformer import Linear
    ptrs = list(_param_pointers(model))
    if bf16_autocast:
        for m in model.modules():
            if isinstance(m, Linear) and m.uses_bf16_shadow(m.weight.is_cuda):
                ptrs.append(ops._bf16_shadows.get(m.weight).data_ptr())
                ptrs.append(ops._bf16_shadows.get(m.bias).data_ptr())
    return tuple(ptrs)


class _Entry:
    """static buffers and the captured graph of one key"""

    def __init__(self, model, b, rows, guided, mode, top_k, return_logits, kv_dtype, sig, kv_splits=1, top_p=False, prompted=False,
                 num_samples=0, prompt_splits=1):
        dev = model.device
        d = model.transformer.layers[0].attn.hidden_dim
        heads = model.transformer.layers[0].attn.num_attn_heads
        # split decode attention (kv_splits > 1): one workspace for every layer -- they run one after the other on the graph's stream
        self.kv_splits = kv_splits
        self.split_ws = torch.empty(decode.split_workspace_floats(rows, heads, d // heads, kv_splits), dtype=torch.float32,
                                    device=dev) if kv_splits > 1 and not num_samples else None
        s, length = model.total_length, model.image_length
        v = model.to_logits[1].out_features
        self.b, self.rows, self.guided, self.mode, self.top_k = b, rows, guided, mode, top_k
        self.plen = model.text_length + model.seg_length
        # generate(num_samples=n): b = B * n token rows, `rows` cache rows in groups of n that share a prompt.  The prompt's keys / values
        # are stored once per group (pk / pv), the caches hold the image positions only, and the step calls the shared-prompt attention
        self.group, self.prompt_splits = num_samples, prompt_splits
        if num_samples:
            self.pk = [torch.empty((rows // num_samples, self.plen, d), dtype=kv_dtype, device=dev) for _ in model.transformer.layers]
            self.pv = [torch.empty_like(t) for t in self.pk]
            self.shared_ws = torch.empty(decode.shared_workspace_floats(rows, heads, d // heads, prompt_splits, kv_splits),
                                         dtype=torch.float32, device=dev)
            s = length
        self.kc = [torch.empty((rows, s, d), dtype=kv_dtype, device=dev) for _ in model.transformer.layers]
        self.vc = [torch.empty_like(t) for t in self.kc]
        self.x = torch.empty((rows, 1, d), dtype=torch.float32, device=dev)
        self.tokens = torch.zeros((b, length), dtype=torch.long, device=dev)
        self.forced = torch.zeros((b, length), dtype=torch.long, device=dev) if mode == decode.FORCED or prompted else None
        self.keep = torch.zeros((b, length), dtype=torch.uint8, device=dev) if prompted else None    # image prompt: the kept positions
        self.logits_out = torch.empty((b, length, v), dtype=torch.float32, device=dev) if return_logits else None
        self.top_p = top_p                                                 # which sampler entry the step calls; the value is params[2]
        self.params = torch.ones(3, dtype=torch.float32, device=dev)       # {temperature, cond_scale, top_p}
        self.seed = torch.zeros(2, dtype=torch.int64, device=dev)          # {seed, offset}
        self.ctr = torch.zeros(2, dtype=torch.int32, device=dev)           # {k, past}
        self.sig = sig
        self.graph = None

    def rewind(self, k):
        """counters for step k: the token k is sampled, the row plen + k - 1 appended"""
        self.ctr[0].fill_(k)
        self.ctr[1].fill_(self.plen + k - 1)

    def sample(self, logits):
        decode.sample_tokens(logits, self.tokens, self.ctr[0:1], self.params, self.mode, top_k=self.top_k, guided=self.guided,
                             seed=self.seed, forced=self.forced, logits_out=self.logits_out, top_p=self.top_p, keep=self.keep)
        decode.advance(self.ctr)


def _step(model, e):
    """one token: everything the graph holds.  Every call below is the module call the eager cached decode makes on the new row."""
    decode.decode_embed(e.tokens, e.ctr[0:1], model.image_token_embedding.weight, model.image_row_embeddings.weight,
                        model.image_col_embeddings.weight, e.x)
    x = e.x
    for li, layer in enumerate(model.transformer.layers):
        attn = layer.attn
        qkv = attn.qkv(layer.ln_in(x))
        if e.group:
            ctx = decode.attention_decode_shared_dev(qkv, e.pk[li], e.pv[li], e.kc[li], e.vc[li], e.ctr[1:2], attn.num_attn_heads,
                                                     group=e.group, prompt_splits=e.prompt_splits, kv_splits=e.kv_splits,
                                                     workspace=e.shared_ws)
        else:
            ctx = decode.attention_decode_dev(qkv, e.kc[li], e.vc[li], e.ctr[1:2], attn.num_attn_heads, kv_splits=e.kv_splits,
                                              workspace=e.split_ws)
        a = attn.out_drop(attn.out_proj(ctx))
        h = layer.first_ln_sandwich(a, residual=x) if layer.cogview_sandwich_layernorm else x + a
        m = layer.mlp(layer.ln_out(h))
        x = layer.second_ln_sandwich(m, residual=h) if layer.cogview_sandwich_layernorm else h + m
    e.sample(model.to_logits(model.transformer.final_ln(x))[:, 0, :].float())


def _autocast_without_cache():
    """the caller's autocast state with autocast's weight-cast cache off: nothing cast during the capture outlives it"""
    if torch.is_autocast_enabled():
        return torch.autocast("cuda", dtype=torch.get_autocast_gpu_dtype(), cache_enabled=False)
    return torch.autocast("cuda", enabled=False, cache_enabled=False)


def _capture(model, e, k=1):
    """one eager warm-up step on a side stream (settles the GEMM choices and any allocation), rewind to the step k it ran (1, or m + 1
    behind a prefilled prefix of m image tokens), capture the step on that stream"""
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=main.device)
    side.wait_stream(main)
    with torch.cuda.stream(side), _autocast_without_cache():
        _step(model, e)
        e.rewind(k)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side), _autocast_without_cache():
        _step(model, e)
    main.wait_stream(side)
    e.graph = g
    model.__dict__["_decode_graph_captures"] = model.__dict__.get("_decode_graph_captures", 0) + 1


def _replay(e, n):
    """the next n tokens (1 .. n, or m + 1 .. m + n behind a prefix): the replay calls and nothing else on the host"""
    for _ in range(n):
        e.graph.replay()


def _draw_seed(generator, device):
    """{seed, offset} for the sampler, drawn from ``generator`` (any device) or torch's default CUDA generator -- on the device when
    the generator is a CUDA one, so no host synchronisation"""
    if generator is None:
        return ops.drop_seed(device)
    s = torch.randint(0, _GEN_SEED_HIGH, (2,), dtype=torch.int64, device=generator.device, generator=generator)
    return s.to(device)


def generate_graph(model, text_tokens, seg_tokens, temperature, top_k, cond_scale, generator, img_tokens, return_logits, kv_splits=1,
                   top_p=None, keep=None, prefix=0, num_samples=None):
    """``MakeAScene.generate(..., graph=True)``; returns None outside the envelope (the caller then runs the eager path).  ``kv_splits``:
    the resolved split count of the decode attention (1: ``mas_attn_decode_dev``; n > 1: ``mas_attn_decode_split_dev``), part of the key.
    ``top_p``: None (off: ``mas_sample_tokens``) or the validated nucleus mass in (0, 1); only "on" is part of the key.
    ``keep`` / ``prefix``: the validated image-prompt mask (None: none) and the number m of leading kept positions the prefill takes;
    only "prompted" is part of the key.
    ``num_samples`` n (validated; ``prefix`` is 0 with it): n candidates per prompt that share its keys / values.  The B prompts (2B under
    guidance: conditional ones first, then the text-free ones) are prefilled once, their K / V go to per-layer prompt blocks
    [groups, plen, D], the caches [groups * n, image_length, D] hold image positions only, the prefill's last logits row is repeated n
    times per group (the sampler's Philox counter holds the row: the candidates differ from position 0 on) and the step calls
    ``mas_attn_decode_shared_dev``.  Row b * n + j of the result is candidate j of prompt b.  n and the prompt split count
    (``decode.resolve_prompt_splits("auto", ...)``) join the key in front of the split count"""
    reason = _envelope_reason(model)
    if reason is not None:
        warned = model.__dict__.setdefault("_decode_graph_warned", set())
        if reason not in warned:
            warned.add(reason)
            warnings.warn(f"MakeAScene.generate(graph=True): {reason}; sampling eagerly instead", RuntimeWarning, stacklevel=3)
        return None
    guided = cond_scale is not None
    n = int(num_samples) if num_samples is not None else 0
    groups = text_tokens.shape[0] * (2 if guided else 1)     # prompts that are prefilled
    b = text_tokens.shape[0] * max(n, 1)                     # token rows
    rows = 2 * b if guided else b                            # cache rows
    prompted = keep is not None
    mode = decode.FORCED if (img_tokens is not None and not prompted) else (decode.GREEDY if temperature == 0 else decode.SAMPLE)
    m = int(prefix) if prompted else 0
    top_k = int(top_k) if (mode == decode.SAMPLE and top_k is not None) else 0
    p_on = mode == decode.SAMPLE and top_p is not None
    autocast = torch.is_autocast_enabled()
    ac_dtype = torch.get_autocast_gpu_dtype() if autocast else None
    dev = model.device
    # the split count stays the key's last element: "prompted" goes in front of it
    key = (b, guided, mode, top_k, p_on, prompted, bool(return_logits), ops.compute_dtype(), autocast, ac_dtype, str(dev), int(kv_splits))
    p_splits = 1
    if n:                                               # a longer key: a call without num_samples never meets these entries
        attn0 = model.transformer.layers[0].attn
        p_splits = decode.resolve_prompt_splits(decode.PROMPT_SPLITS_OVERRIDE or "auto", groups, n, attn0.num_attn_heads,
                                                torch.cuda.get_device_properties(dev).multi_processor_count)
        key = key[:-1] + (n, p_splits, int(kv_splits))
    sig = _pointer_signature(model, autocast and ac_dtype == torch.bfloat16)
    graphs = model.__dict__.setdefault("_decode_graphs", {})
    params = _param_pointers(model)
    for k in [k for k, g in graphs.items() if g.sig[:len(params)] != params]:
        del graphs[k]                                   # parameters moved (.to(), new storage): every entry that read the old ones goes
    e = graphs.get(key)
    if e is not None and e.sig != sig:                  # a buffer the graph reads has moved: never replay it
        del graphs[key]
        e = None

    # ---- prefill: the eager path's (the training attention kernel over the prompt and, behind it, the m leading kept tokens) ----
    if guided:
        text_tokens = torch.cat([text_tokens, torch.zeros_like(text_tokens)], dim=0)
        seg_tokens = torch.cat([seg_tokens, seg_tokens], dim=0)
    prompt = model._prompt_embeddings(text_tokens, seg_tokens)
    bb, plen, d = prompt.shape
    for layer in model.transformer.layers:
        layer.attn.cache_capacity = plen if n else model.total_length      # shared prompt: the prefill's cache holds the prompt alone
    if m:
        prompt = torch.cat([prompt, model._prefix_embeddings(img_tokens, m, guided)], dim=1)
    hidden, cache = model.transformer(prompt, None, cache={}, use_cache=True)
    logits0 = model.to_logits(hidden[:, -1:, :])[:, 0, :].float()                  # of image position m
    prefix_logits = model._prefix_logits(hidden, plen, m, b, cond_scale) if m and return_logits else None
    kv = [(cache[i][0], cache[i][1]) for i in range(len(model.transformer.layers))]
    if e is None:
        e = _Entry(model, b, rows, guided, mode, top_k, return_logits, kv[0][0].dtype, sig, int(kv_splits), p_on, prompted, n, p_splits)
        graphs[key] = e

    # ---- per-call device state, then the static caches ----
    e.rewind(m)
    e.params[0].fill_(float(temperature) if mode == decode.SAMPLE else 1.0)
    e.params[1].fill_(float(cond_scale) if guided else 0.0)
    e.params[2].fill_(float(top_p) if p_on else 1.0)
    if mode == decode.SAMPLE:
        e.seed.copy_(_draw_seed(generator, dev))
    if mode == decode.FORCED or prompted:
        e.forced.copy_(img_tokens)
    if prompted:
        e.keep.copy_(keep)
        if m:
            e.tokens[:, :m].copy_(e.forced[:, :m])
            if prefix_logits is not None:
                e.logits_out[:, :m].copy_(prefix_logits)
    rows_filled = plen + m
    from .transformer import _kv_backing
    for li, (k, v) in enumerate(kv):
        kdst, vdst = (e.pk[li], e.pv[li]) if n else (e.kc[li], e.vc[li])
        kdst[:, :rows_filled].copy_(_kv_backing(k, bb, d)[:, :rows_filled])
        vdst[:, :rows_filled].copy_(_kv_backing(v, bb, d)[:, :rows_filled])
    if n:
        logits0 = logits0.repeat_interleave(n, dim=0)   # every candidate of a group draws position 0 from its prompt's row
    del cache, kv, hidden, prefix_logits

    # ---- token m (0 without a prefix) from the prefill (eager, the same sampler kernel), tokens m+1 .. L-1 by replay ----
    e.sample(logits0)
    if model.image_length - 1 - m > 0:
        if e.graph is None:
            _capture(model, e, m + 1)
        _replay(e, model.image_length - 1 - m)
    tokens = e.tokens.clone()
    return (tokens, e.logits_out.clone()) if return_logits else tokens
