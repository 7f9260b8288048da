"""``mas_hip.optim.Adam``: torch.optim.Adam's update (reference train.py:99-103) for fp32 CUDA parameters as ONE kernel launch per
step over all parameters of all groups that share hyper-parameters (``mas_adam_multi``).  Same arithmetic, same state layout
(``state[p] = {"step", "exp_avg", "exp_avg_sq"}``: ``state_dict()`` / ``load_state_dict()`` interchange with torch.optim.Adam), same
constructor arguments; ``amsgrad`` / ``maximize`` / ``capturable`` / ``differentiable`` are not implemented and raise.

It is a ``torch.optim.Optimizer``: the process-wide post-step hook of ``mas_hip.ops`` sees its steps, so packed weight images and
bf16 shadows are refreshed exactly as with torch's optimizers.  Parameters that are not fp32 CUDA tensors (none in the reference's
models) are updated by a plain torch expression with the same formula.

``AdamW`` is the same optimizer with decoupled weight decay (torch.optim.AdamW's update and state layout).

``max_grad_norm=m`` on either clips the gradients of ALL groups to the global L2 norm ``m`` inside the step, with
torch.nn.utils.clip_grad_norm_'s coefficient ``min(m / (norm + 1e-6), 1)``: one more read of every gradient over the same device
table (``mas_grad_sqnorm_multi``, fp64 sums), one launch for the coefficient (``mas_grad_clip_coef``), and the Adam launch multiplies
each gradient by that device scalar as it loads it (``mas_adam_multi_ex``).  Gradients are not modified, nothing is read on the host;
``opt.grad_norm`` (before clipping) and ``opt.clip_coef`` are 0-dim fp32 device tensors, valid until the next step.
``clip_grad_norm_(parameters, max_norm)`` is the standalone form for callers that keep another optimizer."""
import ctypes as C
import math

import torch

from . import AdamItem, check, lib

_RING = 4


def _table(tables, tkey, device, items):
    """The item table on the device (``tables[tkey]``: one ring of staging buffers per key).  Gradient
    tensors are usually fresh allocations every step (``zero_grad(set_to_none=True)``), so the table changes every step: it goes through a ring of pinned staging buffers with an asynchronous copy each, and the
    host only waits for the copy issued ``_RING`` steps ago -- never for the step in flight (a wait on the previous step's copy
    would serialise the host behind the whole backward: measured, +9 ms of wall time per step)."""
    arr = (AdamItem * len(items))(*items)
    raw = bytes(memoryview(arr))
    ent = tables.get(tkey)
    if ent is not None and ent["raw"] == raw:
        return ent["slots"][ent["cur"]][1]
    nbytes = len(raw)
    if ent is None or ent["cap"] < nbytes:
        cap = max(nbytes, 1 << 16)
        ent = tables[tkey] = dict(cap=cap, cur=0, raw=None, slots=[
            (torch.empty(cap, dtype=torch.uint8, pin_memory=True), torch.empty(cap, dtype=torch.uint8, device=device), torch.cuda.Event())
            for _ in range(_RING)], used=[False] * _RING)
    ent["cur"] = (ent["cur"] + 1) % _RING
    pinned, dev, ev = ent["slots"][ent["cur"]]
    if ent["used"][ent["cur"]]:
        ev.synchronize()         # the copy issued _RING table changes ago has left this staging buffer
    C.memmove(pinned.data_ptr(), raw, nbytes)
    dev[:nbytes].copy_(pinned[:nbytes], non_blocking=True)
    ev.record()
    ent["used"][ent["cur"]] = True
    ent["raw"] = raw
    return dev


def _partials(bufs, device, n):
    """``n`` doubles on ``device`` for the per-block squared norms, kept in ``bufs`` and grown on demand"""
    buf = bufs.get(device)
    if buf is None or buf.numel() < n:
        buf = bufs[device] = torch.empty(max(n, 1024), dtype=torch.float64, device=device)
    return buf


def _check_max_norm(max_norm, who):
    max_norm = float(max_norm)
    if not 0.0 < max_norm < math.inf:
        raise ValueError(f"{who}: max_norm must be positive and finite, got {max_norm}")
    return max_norm


def _one_device(grads, who):
    devices = {g.device for g in grads}
    if len(devices) > 1:
        raise NotImplementedError(f"{who}: gradients on more than one device ({sorted(map(str, devices))}) are not supported with a global norm")
    return next(iter(devices)) if devices else None


def _cpu_norm_coef(grads, max_norm):
    """the norm and the coefficient with the kernels' formulas in torch: fp64 sum of squares, fp32 norm, fp32 division, NaN kept"""
    norm = torch.stack([g.double().pow(2).sum() for g in grads]).sum().sqrt().float()
    return norm, torch.clamp(torch.full_like(norm, max_norm) / (norm + 1e-6), max=1.0)


def _norm_coef_launches(tables, out, partials, extra, max_norm, stream):
    """one mas_grad_sqnorm_multi per (table, items, blocks) into consecutive pieces of ``partials``, then ONE mas_grad_clip_coef over all
    of them and ``extra`` (a device fp64 vector or None) into ``out`` = (norm, coefficient)"""
    off = 0
    for table, n_items, blocks in tables:
        check(lib().mas_grad_sqnorm_multi(C.c_void_p(table.data_ptr()), n_items, blocks, C.c_void_p(partials.data_ptr() + 8 * off), stream),
              "grad_sqnorm_multi")
        off += blocks
    check(lib().mas_grad_clip_coef(C.c_void_p(partials.data_ptr()) if off else None, off, C.c_void_p(extra.data_ptr()) if extra is not None else None,
                                   0 if extra is None else extra.numel(), max_norm, C.c_void_p(out.data_ptr()), stream), "grad_clip_coef")


class Adam(torch.optim.Optimizer):
    _decoupled_wd = 0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, fused=None, foreach=None, max_grad_norm=None):
        name = f"mas_hip.optim.{type(self).__name__}"
        if amsgrad or maximize or capturable or differentiable:
            raise NotImplementedError(f"{name}: amsgrad / maximize / capturable / differentiable are not implemented")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError(f"{name}: invalid hyper-parameter")
        # (an attribute, not a key of `defaults`: the clip is global over all groups, and state_dict() stays torch.optim.Adam's)
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm, name)
        self.grad_norm = self.clip_coef = None      # 0-dim fp32 tensors after a clipped step
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      capturable=False, differentiable=False, fused=None, foreach=None))
        self._tables = {}            # device index -> ring of (pinned staging, device table, event) slots + the bytes of the current table
        self._clip_bufs = {}         # device -> fp64 partial sums of the norm launches
        self._clip_out = {}          # device -> (norm, coefficient) fp32

    def _table(self, tkey, device, items):
        return _table(self._tables, tkey, device, items)

    def _collect(self, group):
        """Creates missing state, advances `step`, and sorts the group's parameters that have a gradient: (device, step number) -> items
        for the kernel (parameters on different step counts take separate launches), the number of blocks per key, and the
        (parameter, state, step) triples that take the torch expression (another dtype / device / layout)."""
        by_key, first, slow = {}, {}, []
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError("mas_hip.optim.Adam does not support sparse gradients")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if st["step"].device.type != "cpu":          # a state loaded from torch.optim.Adam(fused=True / capturable=True) keeps `step` on
                st["step"] = st["step"].detach().to("cpu", torch.float32)   # the device: one sync here instead of one per step and parameter
            st["step"] += 1
            t = int(st["step"])
            if p.numel() == 0:
                continue                                 # (torch.optim.Adam accepts empty parameters: nothing to update)
            native = (p.is_cuda and p.dtype == torch.float32 and p.grad.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()
                      and st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous() and p.grad.device == p.device)
            if not native:
                slow.append((p, st, t))
                continue
            key = (p.device, t)
            it = AdamItem()
            it.p, it.g, it.m, it.v, it.n = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
            it.first_block = first.get(key, 0)
            first[key] = it.first_block + lib().mas_adam_blocks(p.numel())
            by_key.setdefault(key, []).append(it)
        return by_key, first, slow

    def _launch(self, table, n_items, blocks, hyper, t, scale, stream):
        lr, b1, b2, eps, wd = hyper
        if scale is None and not self._decoupled_wd:
            check(lib().mas_adam_multi(C.c_void_p(table.data_ptr()), n_items, blocks, lr, b1, b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t, stream),
                  "adam_multi")
        else:
            check(lib().mas_adam_multi_ex(C.c_void_p(table.data_ptr()), n_items, blocks, lr, b1, b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t,
                                          None if scale is None else C.c_void_p(scale.data_ptr()), self._decoupled_wd, stream), "adam_multi_ex")

    @staticmethod
    def _hyper(group):
        return (float(group["lr"]), *group["betas"], float(group["eps"]), float(group["weight_decay"]))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.max_grad_norm is not None:
            self._clipped_step()
            return loss
        for group in self.param_groups:
            hyper = self._hyper(group)
            by_key, first, slow = self._collect(group)
            for p, st, t in slow:
                self._torch_update(p, p.grad, st, t, *hyper)
            for (device, t), items in by_key.items():
                with torch.cuda.device(device):
                    ordinal = [k for k in by_key if k[0] == device].index((device, t))      # 0 unless parameters of the group sit on different step counts
                    table = self._table((device.index, ordinal), device, items)
                    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                    self._launch(table, len(items), first[(device, t)], hyper, t, None, stream)
        return loss

    def _clipped_step(self):
        """The tables of ALL groups first, the norm launches over them, one coefficient launch, then the Adam launches with that scalar."""
        name = f"mas_hip.optim.{type(self).__name__}"
        device = _one_device([p.grad for group in self.param_groups for p in group["params"] if p.grad is not None and p.numel()], name)
        launches, slow = [], []              # (hyper, step number, items, blocks) per kernel launch; (hyper, parameter, state, step) for torch
        for group in self.param_groups:
            hyper = self._hyper(group)
            by_key, first, sl = self._collect(group)
            launches += [(hyper, key[1], items, first[key]) for key, items in by_key.items()]
            slow += [(hyper,) + s for s in sl]
        if device is None:
            return
        if device.type != "cuda":
            self.grad_norm, self.clip_coef = _cpu_norm_coef([p.grad for _, p, _, _ in slow], self.max_grad_norm)
        else:
            with torch.cuda.device(device):
                stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                out = self._clip_out.get(device)
                if out is None:
                    out = self._clip_out[device] = torch.zeros(2, dtype=torch.float32, device=device)
                tables = [(self._table(("clip", device.index, i), device, items), len(items), blocks)
                          for i, (_, _, items, blocks) in enumerate(launches)]
                extra = torch.stack([p.grad.double().pow(2).sum() for _, p, _, _ in slow]) if slow else None
                _norm_coef_launches(tables, out, _partials(self._clip_bufs, device, sum(b for _, _, b in tables)), extra, self.max_grad_norm, stream)
                for (hyper, t, _, _), (table, n_items, blocks) in zip(launches, tables):
                    self._launch(table, n_items, blocks, hyper, t, out[1], stream)
                self.grad_norm, self.clip_coef = out[0], out[1]
        for hyper, p, st, t in slow:
            self._torch_update(p, p.grad * self.clip_coef.to(p.grad.dtype), st, t, *hyper)

    def _torch_update(self, p, g, st, t, lr, b1, b2, eps, wd):
        if wd != 0.0:
            if self._decoupled_wd:
                p.mul_(1.0 - lr * wd)
            else:
                g = g.add(p, alpha=wd)
        st["exp_avg"].lerp_(g.to(st["exp_avg"].dtype), 1.0 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
        denom = (st["exp_avg_sq"].sqrt() / math.sqrt(1.0 - b2 ** t)).add_(eps)
        p.addcdiv_(st["exp_avg"], denom, value=-lr / (1.0 - b1 ** t))


class AdamW(Adam):
    """torch.optim.AdamW's update: ``p -= lr * weight_decay * p`` ahead of the moment update, the gradient takes no ``weight_decay * p``
    term.  Everything else, ``max_grad_norm`` included, is ``Adam``; ``state_dict()`` interchanges with torch.optim.AdamW."""
    _decoupled_wd = 1

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, **kw)


_clip_tables, _clip_bufs = {}, {}        # clip_grad_norm_'s own table rings and partial sums (per device)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) for the L2 norm, on the current stream and without a host read: the norm
    launch over a device table of the fp32 gradients, the coefficient launch, and ``g *= coefficient`` in place (``mas_grad_scale_multi``).
    Returns the norm before clipping as a 0-dim fp32 tensor on the gradients' device.  Like torch's, it always multiplies (by 1 when
    the norm is within ``max_norm``); there is no ``error_if_nonfinite``, which would need the host to read the norm."""
    who = "mas_hip.optim.clip_grad_norm_"
    max_norm = _check_max_norm(max_norm, who)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None and p.grad.numel()]
    device = _one_device(grads, who)
    if device is None:
        return torch.tensor(0.0)
    if device.type != "cuda":
        norm, coef = _cpu_norm_coef(grads, max_norm)
        for g in grads:
            g.mul_(coef.to(g.dtype))
        return norm
    items, blocks, other = [], 0, []
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous():
            other.append(g)
            continue
        it = AdamItem()
        it.g, it.n, it.first_block = g.data_ptr(), g.numel(), blocks
        blocks += lib().mas_adam_blocks(g.numel())
        items.append(it)
    with torch.cuda.device(device):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        out = torch.empty(2, dtype=torch.float32, device=device)       # fresh: the returned norm stays valid across later calls
        tables = [(_table(_clip_tables, device.index, device, items), len(items), blocks)] if items else []
        extra = torch.stack([g.double().pow(2).sum() for g in other]) if other else None
        _norm_coef_launches(tables, out, _partials(_clip_bufs, device, blocks), extra, max_norm, stream)
        for table, n_items, nb in tables:
            check(lib().mas_grad_scale_multi(C.c_void_p(table.data_ptr()), n_items, nb, C.c_void_p(out.data_ptr() + 4), stream), "grad_scale_multi")
        for g in other:
            g.mul_(out[1].to(g.dtype))
    return out[0]
