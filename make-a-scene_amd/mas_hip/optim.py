"""``mas_hip.optim.Adam``: torch.optim.Adam's update (reference train.py:99-103) for fp32 CUDA parameters as ONE kernel launch per
step over all parameters of all groups that share hyper-parameters (``mas_adam_multi``).  Same arithmetic, same state layout
(``state[p] = {"step", "exp_avg", "exp_avg_sq"}``: ``state_dict()`` / ``load_state_dict()`` interchange with torch.optim.Adam), same
constructor arguments; ``amsgrad`` / ``maximize`` / ``capturable`` / ``differentiable`` are not implemented and raise (what
``capturable=True`` is asked for -- a step that a graph can capture -- is ``device_step=True`` here: see below).

It is a ``torch.optim.Optimizer``: the process-wide post-step hook of ``mas_hip.ops`` sees its steps, so packed weight images and
bf16 shadows are refreshed exactly as with torch's optimizers.  Parameters that are not fp32 CUDA tensors (none in the reference's
models) are updated by a plain torch expression with the same formula.

``AdamW`` is the same optimizer with decoupled weight decay (torch.optim.AdamW's update and state layout).

``max_grad_norm=m`` on either clips the gradients of ALL groups to the global L2 norm ``m`` inside the step, with
torch.nn.utils.clip_grad_norm_'s coefficient ``min(m / (norm + 1e-6), 1)``: one more read of every gradient over the same device
table (``mas_grad_sqnorm_multi``, fp64 sums), one launch for the coefficient (``mas_grad_clip_coef``), and the Adam launch multiplies
each gradient by that device scalar as it loads it (``mas_adam_multi_ex``).  Gradients are not modified, nothing is read on the host;
``opt.grad_norm`` (before clipping) and ``opt.clip_coef`` are 0-dim fp32 device tensors, valid until the next step.
``clip_grad_norm_(parameters, max_norm)`` is the standalone form for callers that keep another optimizer.

``ema_decay=d`` on either keeps an exponential moving average of every parameter in ``state[p]["ema"]`` (fp32, a clone of ``p`` taken
before its first update), updated in the Adam launch itself (``mas_adam_multi_ema``): ``ema = lerp(ema, p_new, 1 - d)`` at every step
that updates ``p``; a parameter without a gradient at a step keeps its average as it is.  ``ema_warmup=True`` uses
``min(d, (1 + k) / (10 + k))`` at this optimizer's ``k``-th step (computed on the host; ``k`` travels in ``state_dict()`` as
``param_groups[0]["ema_step"]``, a key torch's optimizers carry along and do not read).  ``state_dict()`` holds ``"ema"`` per parameter and
still loads into torch.optim.Adam / AdamW; a state without it (torch's, or this optimizer's without ``ema_decay``) loads here and the
average starts from the weights at the next step.  ``opt.swap_ema()`` is the context manager under which the parameters hold the averaged
weights (one ``mas_swap_multi`` launch per device, then ``ops.invalidate_weight_cache()``; the same again on exit restores both bit for
bit; storage does not move).  ``opt.ema_state_dict(module)`` is ``module.state_dict()`` with the averaged weights in place of the
parameters: the checkpoint to evaluate or sample from.  Data-parallel runs need nothing more: the average is a function of the parameters,
which are identical across ranks.

``skip_nonfinite=True`` does not apply a step whose global gradient norm is NaN or infinite: the norm launches run (with or without
``max_grad_norm``), the Adam launch reads the norm on the device and stores nothing when it is not finite, so ``p``, both moments and the
average keep their bits.  Nothing is read on the host: ``opt.grad_norm`` is set as with clipping, ``opt.step_skipped`` computes a 0-dim
bool device tensor when asked, and ``state["step"]`` advances on a skipped step too -- the bias corrections run one step ahead after a
skip.

``device_step=True`` (keyword only, off by default) keeps everything that changes from step to step on the device, so that ``step()`` can
be captured into a graph and replayed (``mas_hip.graphs.GraphedTrainStep``), and an eager step reads nothing on the host either:

* ``state[p]["step"]`` is a 0-dim fp32 device tensor -- the layout of ``torch.optim.Adam(capturable=True / fused=True)``, with which
  ``state_dict()`` interchanges -- and all of them are views into ONE fp32 vector, element 0 of which is ``ema_warmup``'s counter ``k``; one
  ``mas_adam_advance_dev`` launch behind the Adam launches adds 1 to all of them (a step skipped by ``skip_nonfinite`` advances them too).
  ``param_groups[0]["ema_step"]`` is filled from the vector in ``state_dict()`` only: one host read, never under a capture.
* the kernel (``mas_adam_multi_dev``) reads ``lr`` from a device fp32 scalar per group and forms the bias corrections from the device step
  count.  ``group["lr"]`` stays what the caller put there (a float or a 0-dim tensor: LR schedulers work unchanged);
  ``sync_hyperparameters()`` pushes changed values to the device scalars on the current stream (a no-op when nothing changed; every eager
  ``step()`` calls it; it never runs under a capture, where a copy node would rewrite the old value at every replay -- whoever replays
  calls it before).  ``betas``, ``eps`` and ``weight_decay`` are launch arguments: a change after a capture needs a new capture.
* ``init_state()`` creates the state of every parameter and every buffer a step needs (moments, average, step vector, norm buffers, the
  staging memory of a capture's tables); ``step()`` under a capture raises when something is missing instead of allocating what a replay
  would not re-create.  Tables uploaded under a capture get memory of their own that is never rewritten or freed while the optimizer lives.
* there is no torch-expression path: a parameter that is not a contiguous fp32 CUDA tensor with an fp32 gradient raises at ``step()``, and
  all parameters live on one device.
* ``load_state_dict()`` copies the loaded values INTO the existing state tensors where shapes match (storage does not move: a captured graph
  stays valid), and like ``add_param_group()`` bumps ``opt.state_generation``.

``max_grad_norm``, ``ema_decay``, ``ema_warmup``, ``skip_nonfinite``, ``swap_ema()`` and ``ema_state_dict()`` mean what they mean without it."""
import contextlib
import ctypes as C
import math

import torch

from . import AdamItem, check, lib

_RING = 4


def _table(tables, tkey, device, items, tail=b""):
    """The item table on the device (``tables[tkey]``: one ring of staging buffers per key), followed by the bytes ``tail`` (the array of
    EMA / swap pointers, one per item: the same copy and the same byte comparison cover both).  Gradient
    tensors are usually fresh allocations every step (``zero_grad(set_to_none=True)``), so the table changes every step: it goes through a ring of pinned staging buffers with an asynchronous copy each, and the
    host only waits for the copy issued ``_RING`` steps ago -- never for the step in flight (a wait on the previous step's copy
    would serialise the host behind the whole backward: measured, +9 ms of wall time per step)."""
    arr = (AdamItem * len(items))(*items)
    raw = bytes(memoryview(arr)) + tail
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


_FLT_MAX = 3.4028234663852886e38       # as max_norm: min(FLT_MAX / (norm + 1e-6), 1) is exactly 1 for every finite norm


def _check_ema_decay(d, who):
    d = float(d)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"{who}: ema_decay must be in [0, 1), got {d}")
    return d


def _ema_weight(decay):
    """``1 - decay`` as the kernel forms it: both rounded to fp32"""
    return C.c_float(1.0 - C.c_float(decay).value).value


def _pointers(ptrs):
    return bytes(memoryview((C.c_void_p * len(ptrs))(*ptrs)))


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


_ARENA_ALIGN = 256


class Adam(torch.optim.Optimizer):
    _decoupled_wd = 0
    state_generation = 0             # bumped by load_state_dict() and add_param_group(): whoever holds a captured step compares it

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, fused=None, foreach=None, max_grad_norm=None, ema_decay=None, ema_warmup=False,
                 skip_nonfinite=False, device_step=False):
        name = f"mas_hip.optim.{type(self).__name__}"
        if amsgrad or maximize or capturable or differentiable:
            raise NotImplementedError(f"{name}: amsgrad / maximize / capturable / differentiable are not implemented"
                                      + (" (a step that a graph can capture is device_step=True)" if capturable else ""))
        self.device_step = bool(device_step)        # an attribute like max_grad_norm: state_dict() stays torch.optim.Adam's
        self._dev = None                            # device_step: the step vector, the lr scalars and the launch buffers (_dev_prepare)
        self._lr_pushed = None                      # the learning rates the device scalars hold
        self._lr_staging = []                       # [pinned buffer, event of its last copy]
        self._arenas = []                           # capture-time tables: [pinned bytes, device bytes, bytes used], never rewritten or freed
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError(f"{name}: invalid hyper-parameter")
        # (an attribute, not a key of `defaults`: the clip is global over all groups, and state_dict() stays torch.optim.Adam's)
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm, name)
        self.grad_norm = self.clip_coef = None      # 0-dim fp32 tensors after a clipped (or guarded) step
        self.ema_decay = None if ema_decay is None else _check_ema_decay(ema_decay, name)     # attributes like max_grad_norm: all groups
        self.ema_warmup, self.skip_nonfinite = bool(ema_warmup), bool(skip_nonfinite)
        self._swapped = False                       # inside swap_ema()
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      capturable=False, differentiable=False, fused=None, foreach=None))
        self._tables = {}            # device index -> ring of (pinned staging, device table, event) slots + the bytes of the current table
        self._clip_bufs = {}         # device -> fp64 partial sums of the norm launches
        self._clip_out = {}          # device -> (norm, coefficient) fp32
        if self.ema_decay is not None:
            self.param_groups[0]["ema_step"] = 0     # steps taken with the average on (ema_warmup's k); saved and loaded with the groups

    def _table(self, tkey, device, items, tail=b""):
        return _table(self._tables, tkey, device, items, tail)

    def _ema_decay_now(self):
        """this step's decay (None: no average), and the step counter of ``ema_warmup`` advanced"""
        if self.ema_decay is None:
            return None
        g0 = self.param_groups[0]
        k = int(g0.get("ema_step", 0))               # (absent after loading a state saved without an average)
        g0["ema_step"] = k + 1
        return min(self.ema_decay, (1.0 + k) / (10.0 + k)) if self.ema_warmup else self.ema_decay

    @property
    def step_skipped(self):
        """0-dim bool tensor on the gradients' device: the last step's gradient norm was not finite (with ``skip_nonfinite`` that step was
        not applied).  Computed when asked; None before the first step that computes a norm."""
        return None if self.grad_norm is None else ~torch.isfinite(self.grad_norm)

    def _collect(self, group):
        """Creates missing state, advances `step`, and sorts the group's parameters that have a gradient: (device, step number) -> items
        for the kernel (parameters on different step counts take separate launches), the number of blocks per key, and the
        (parameter, state, step) triples that take the torch expression (another dtype / device / layout).  With ``ema_decay`` the state
        holds ``ema`` and the kernel's items carry its pointer as the attribute ``ema`` (0: none)."""
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
            if self.ema_decay is not None and "ema" not in st:       # with the rest of the state, or at the first step after loading a state without it
                st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
            ema = st["ema"] if self.ema_decay is not None else None
            if st["step"].device.type != "cpu":          # a state loaded from torch.optim.Adam(fused=True / capturable=True) keeps `step` on
                st["step"] = st["step"].detach().to("cpu", torch.float32)   # the device: one sync here instead of one per step and parameter
            st["step"] += 1
            t = int(st["step"])
            if p.numel() == 0:
                continue                                 # (torch.optim.Adam accepts empty parameters: nothing to update)
            native = (p.is_cuda and p.dtype == torch.float32 and p.grad.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()
                      and st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous() and p.grad.device == p.device
                      and (ema is None or (ema.dtype == torch.float32 and ema.is_contiguous() and ema.device == p.device)))
            if not native:
                slow.append((p, st, t))
                continue
            key = (p.device, t)
            it = AdamItem()
            it.p, it.g, it.m, it.v, it.n = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
            it.first_block = first.get(key, 0)
            it.ema = 0 if ema is None else ema.data_ptr()
            first[key] = it.first_block + lib().mas_adam_blocks(p.numel())
            by_key.setdefault(key, []).append(it)
        return by_key, first, slow

    def _item_table(self, tkey, device, items):
        """the device table of ``items`` with, under ``ema_decay``, the array of their EMA pointers behind it (its address: second value)"""
        if self.ema_decay is None:
            return self._table(tkey, device, items), None
        table = self._table(tkey, device, items, _pointers([it.ema for it in items]))
        return table, table.data_ptr() + C.sizeof(AdamItem) * len(items)

    def _launch(self, table, n_items, blocks, hyper, t, scale, stream, ema=None, decay=None, norm=None):
        """``ema``: device address of the EMA pointer array with this step's ``decay``; ``norm``: the device norm the guard reads"""
        lr, b1, b2, eps, wd = hyper
        if ema is not None or norm is not None:
            check(lib().mas_adam_multi_ema(C.c_void_p(table.data_ptr()), None if ema is None else C.cast(C.c_void_p(ema), C.POINTER(C.c_void_p)),
                                           n_items, blocks, lr, b1, b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t,
                                           None if scale is None else C.c_void_p(scale.data_ptr()), self._decoupled_wd,
                                           0.0 if decay is None else decay, None if norm is None else C.c_void_p(norm.data_ptr()), stream),
                  "adam_multi_ema")
        elif scale is None and not self._decoupled_wd:
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
        if self._swapped:
            raise RuntimeError(f"mas_hip.optim.{type(self).__name__}: step() inside swap_ema(): the parameters hold the averaged weights")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.device_step:
            self._step_dev()
            return loss
        decay = self._ema_decay_now()
        if self.max_grad_norm is not None or self.skip_nonfinite:
            self._clipped_step(decay)
            return loss
        for group in self.param_groups:
            hyper = self._hyper(group)
            by_key, first, slow = self._collect(group)
            for p, st, t in slow:
                self._torch_update(p, p.grad, st, t, *hyper, decay=decay)
            for (device, t), items in by_key.items():
                with torch.cuda.device(device):
                    ordinal = [k for k in by_key if k[0] == device].index((device, t))      # 0 unless parameters of the group sit on different step counts
                    table, ema = self._item_table((device.index, ordinal), device, items)
                    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                    self._launch(table, len(items), first[(device, t)], hyper, t, None, stream, ema, decay)
        return loss

    def _clipped_step(self, decay=None):
        """The tables of ALL groups first, the norm launches over them, one coefficient launch, then the Adam launches with that scalar.
        ``skip_nonfinite`` without ``max_grad_norm`` takes the same route for the norm (the coefficient launch with FLT_MAX: exactly 1
        for every finite norm) and hands the Adam launch no scale at all, so the step keeps the bits of the unclipped one."""
        max_norm = _FLT_MAX if self.max_grad_norm is None else self.max_grad_norm
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
            self.grad_norm, self.clip_coef = _cpu_norm_coef([p.grad for _, p, _, _ in slow], max_norm)
        else:
            with torch.cuda.device(device):
                stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                out = self._clip_out.get(device)
                if out is None:
                    out = self._clip_out[device] = torch.zeros(2, dtype=torch.float32, device=device)
                tables, emas = [], []
                for i, (_, _, items, blocks) in enumerate(launches):
                    table, ema = self._item_table(("clip", device.index, i), device, items)
                    tables.append((table, len(items), blocks))
                    emas.append(ema)
                extra = torch.stack([p.grad.double().pow(2).sum() for _, p, _, _ in slow]) if slow else None
                _norm_coef_launches(tables, out, _partials(self._clip_bufs, device, sum(b for _, _, b in tables)), extra, max_norm, stream)
                scale = None if self.max_grad_norm is None else out[1]
                for (hyper, t, _, _), (table, n_items, blocks), ema in zip(launches, tables, emas):
                    self._launch(table, n_items, blocks, hyper, t, scale, stream, ema, decay, out[0] if self.skip_nonfinite else None)
                self.grad_norm, self.clip_coef = out[0], out[1]
        skip = ~torch.isfinite(self.grad_norm) if self.skip_nonfinite else None
        for hyper, p, st, t in slow:
            g = p.grad if self.max_grad_norm is None else p.grad * self.clip_coef.to(p.grad.dtype)
            self._torch_update(p, g, st, t, *hyper, decay=decay, skip=skip)

    def _torch_update(self, p, g, st, t, lr, b1, b2, eps, wd, decay=None, skip=None):
        """the kernel's formulas as torch expressions.  ``decay``: this step's EMA decay; ``skip``: a 0-dim bool tensor on any device --
        where it is True the four tensors get their old bits back (a ``where`` on the device: nothing is read on the host)"""
        held = [st["exp_avg"], st["exp_avg_sq"]] + ([st["ema"]] if decay is not None else [])
        if skip is not None:
            old = [x.detach().clone() for x in [p] + held]
        if wd != 0.0:
            if self._decoupled_wd:
                p.mul_(1.0 - lr * wd)
            else:
                g = g.add(p, alpha=wd)
        st["exp_avg"].lerp_(g.to(st["exp_avg"].dtype), 1.0 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
        denom = (st["exp_avg_sq"].sqrt() / math.sqrt(1.0 - b2 ** t)).add_(eps)
        p.addcdiv_(st["exp_avg"], denom, value=-lr / (1.0 - b1 ** t))
        if decay is not None:
            st["ema"].lerp_(p.detach().to(st["ema"].dtype), _ema_weight(decay))
        if skip is not None:
            for x, o in zip([p] + held, old):
                x.copy_(torch.where(skip.to(x.device), o, x))

    # ---- device_step=True ------------------------------------------------------------------------------------------------------------
    def _who(self):
        return f"mas_hip.optim.{type(self).__name__}(device_step=True)"

    def _dev_prepare(self, create):
        """The buffers of the device path -- the vector of counters (element 0: ``ema_warmup``'s ``k``, element 1 + i: the step count of the
        i-th parameter in group order), one learning rate per group, four launch scalars per parameter, the norm launches' output and partial
        sums -- made when missing or when parameters or groups were added (the counters move over; ``create`` False, under a capture: raises)."""
        params = [p for group in self.param_groups for p in group["params"]]
        d = self._dev
        if d is not None and d["n"] == len(params) and d["n_groups"] == len(self.param_groups):
            return d
        for i, p in enumerate(params):
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"{self._who()}: parameter {i} of shape {tuple(p.shape)} ({p.dtype}, {p.device}"
                                   f"{'' if p.is_contiguous() else ', not contiguous'}) is not a contiguous fp32 CUDA tensor; this mode has no other path")
        devices = sorted({str(p.device) for p in params})
        if len(devices) != 1:
            raise NotImplementedError(f"{self._who()}: the parameters must live on one device, got {devices}")
        if not create:
            raise RuntimeError(f"{self._who()}: step() under a graph capture before init_state(): the step vector does not exist yet")
        device = params[0].device
        vec = torch.zeros(1 + len(params), dtype=torch.float32, device=device)
        if d is not None:
            vec[:1 + d["n"]].copy_(d["vec"])                 # (add_param_group appends: the slots of the old parameters stay)
        elif self.ema_decay is not None:
            vec[0] = float(self.param_groups[0].get("ema_step", 0))
        out = torch.zeros(2, dtype=torch.float32, device=device)
        self._clip_out[device] = out
        blocks = sum(lib().mas_adam_blocks(p.numel()) for p in params)
        self._dev = d = dict(n=len(params), n_groups=len(self.param_groups), device=device, vec=vec, views=[vec[1 + i] for i in range(len(params))],
                             slot={p: i for i, p in enumerate(params)}, lr=torch.zeros(len(self.param_groups), dtype=torch.float32, device=device),
                             scalars=torch.zeros(4 * len(params), dtype=torch.float32, device=device), out=out, norm=out[0], coef=out[1],
                             partials=_partials(self._clip_bufs, device, blocks), table_bytes=sum(
                                 -(-(len(g["params"]) * (C.sizeof(AdamItem) + 16)) // _ARENA_ALIGN) * _ARENA_ALIGN for g in self.param_groups))
        self._lr_pushed = None
        return d

    def _dev_state(self, p, d, create):
        """``state[p]`` with ``step`` the parameter's view into the vector and both moments (and the average) in place; a state that came from
        elsewhere (loaded before the first step, a host ``step``) is adopted: its count is copied into the view"""
        st = self.state[p]
        i = d["slot"][p]
        view = d["views"][i]
        if st.get("step") is view and "exp_avg" in st and "exp_avg_sq" in st and (self.ema_decay is None or "ema" in st):
            return st
        if not create:
            raise RuntimeError(f"{self._who()}: step() under a graph capture would create optimizer state for parameter {i} of shape "
                               f"{tuple(p.shape)}, which a replay would not re-create: call init_state() before the capture")
        if st.get("step") is not view:
            if "step" in st:
                view.copy_(torch.as_tensor(st["step"], dtype=torch.float32))
            st["step"] = view
        for key in ("exp_avg", "exp_avg_sq"):
            if key not in st:
                st[key] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if self.ema_decay is not None and "ema" not in st:
            st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
        for key in ("exp_avg", "exp_avg_sq") + (("ema",) if self.ema_decay is not None else ()):
            t = st[key]
            if not (t.dtype == torch.float32 and t.is_contiguous() and t.device == p.device and t.shape == p.shape):
                raise RuntimeError(f"{self._who()}: state `{key}` of parameter {i} of shape {tuple(p.shape)} is not a contiguous fp32 tensor on {p.device}")
        return st

    @torch.no_grad()
    def init_state(self):
        """Creates everything a step needs, for EVERY parameter (with or without a gradient now): both moments, the average, the step
        vector, the learning-rate scalars (and pushes them), the norm buffers, and staging memory for the tables of one more capture.  Call
        it before capturing ``step()``; calling it again is cheap and changes no value."""
        if not self.device_step:
            raise RuntimeError(f"mas_hip.optim.{type(self).__name__}: init_state() belongs to device_step=True")
        d = self._dev_prepare(True)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._who()}: init_state() under a graph capture")
        for group in self.param_groups:
            for p in group["params"]:
                self._dev_state(p, d, True)
        if not self._arenas or self._arenas[-1][0].numel() - self._arenas[-1][2] < d["table_bytes"]:
            cap = max(2 * d["table_bytes"], 1 << 16)
            self._arenas.append([torch.empty(cap, dtype=torch.uint8, pin_memory=True), torch.empty(cap, dtype=torch.uint8, device=d["device"]), 0])
        with torch.cuda.device(d["device"]):
            self.sync_hyperparameters()

    def sync_hyperparameters(self):
        """Pushes the groups' learning rates to the device scalars the kernel reads, on the current stream, when one of them differs from
        what was pushed last; returns whether it did.  ``group["lr"]`` may be a float or a 0-dim tensor (a CUDA tensor is read on the
        host here).  Not under a capture: a captured copy would rewrite the value of the capture at every replay."""
        if not self.device_step:
            return False
        vals = tuple(float(group["lr"]) for group in self.param_groups)
        if vals == self._lr_pushed:
            return False
        self._push_lr(vals)
        self._lr_pushed = vals
        return True

    def _push_lr(self, vals):
        """one asynchronous copy through a pinned buffer whose last copy has run (or a new one)"""
        d = self._dev_prepare(True)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._who()}: the learning rate changed under a graph capture; call sync_hyperparameters() before it")
        slot = next((s for s in self._lr_staging if s[0].numel() == len(vals) and s[1].query()), None)
        if slot is None:
            slot = [torch.empty(len(vals), dtype=torch.float32, pin_memory=True), torch.cuda.Event()]
            self._lr_staging.append(slot)
        slot[0].copy_(torch.tensor(vals, dtype=torch.float32))
        d["lr"].copy_(slot[0], non_blocking=True)
        slot[1].record()

    def _capture_table(self, raw):
        """``raw`` on the device through memory that belongs to this upload alone: the copy node a capture records reads its pinned source
        again at every replay"""
        if not self._arenas or self._arenas[-1][0].numel() - self._arenas[-1][2] < len(raw):
            raise RuntimeError(f"{self._who()}: no staging memory left for a table under a graph capture: call init_state() before every capture")
        arena = self._arenas[-1]
        pinned, dev, off = arena
        C.memmove(pinned.data_ptr() + off, raw, len(raw))
        dev[off:off + len(raw)].copy_(pinned[off:off + len(raw)], non_blocking=True)
        arena[2] = off + -(-len(raw) // _ARENA_ALIGN) * _ARENA_ALIGN
        return dev[off:off + len(raw)]

    def _step_dev(self):
        """The step with nothing read on the host: per group one mas_adam_multi_dev over the parameters that have a gradient (each with its
        own step count), the norm launches in front when clipping or guarding, the advance launch(es) behind."""
        capturing = self._capturing_now()
        d = self._dev_prepare(not capturing)
        device = d["device"]
        with torch.cuda.device(device):
            if not capturing:
                self.sync_hyperparameters()
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            launches, advance, first_item = [], [0] if self.ema_decay is not None else [], 0
            for gi, group in enumerate(self.param_groups):
                items, steps, blocks = [], [], 0
                for p in group["params"]:
                    g = p.grad
                    if g is None:
                        continue
                    if g.is_sparse:
                        raise RuntimeError("mas_hip.optim.Adam does not support sparse gradients")
                    st = self._dev_state(p, d, not capturing)
                    if not (g.dtype == torch.float32 and g.is_contiguous() and g.device == p.device and p.is_contiguous()):
                        raise RuntimeError(f"{self._who()}: the gradient of parameter {d['slot'][p]} of shape {tuple(p.shape)} ({g.dtype}, {g.device}) is "
                                           "not a contiguous fp32 tensor on the parameter's device; this mode has no other path")
                    advance.append(1 + d["slot"][p])
                    if p.numel() == 0:
                        continue
                    it = AdamItem()
                    it.p, it.g, it.m, it.v, it.n = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
                    it.first_block = blocks
                    it.ema = st["ema"].data_ptr() if self.ema_decay is not None else 0
                    blocks += lib().mas_adam_blocks(p.numel())
                    items.append(it)
                    steps.append(st["step"].data_ptr())
                if items:
                    tail = _pointers([it.ema for it in items]) + _pointers(steps)
                    if capturing:
                        arr = (AdamItem * len(items))(*items)
                        table = self._capture_table(bytes(memoryview(arr)) + tail)
                    else:
                        table = self._table(("dev", gi), device, items, tail)
                    launches.append((gi, group, table, len(items), blocks, first_item))
                    first_item += len(items)
            guard = self.max_grad_norm is not None or self.skip_nonfinite
            if guard and launches:
                _norm_coef_launches([(t, n, b) for _, _, t, n, b, _ in launches], d["out"], d["partials"], None,
                                    _FLT_MAX if self.max_grad_norm is None else self.max_grad_norm, stream)
                self.grad_norm, self.clip_coef = d["norm"], d["coef"]
            ptr = lambda a: C.cast(C.c_void_p(a), C.POINTER(C.c_void_p))
            for gi, group, table, n_items, blocks, first in launches:
                base = table.data_ptr() + C.sizeof(AdamItem) * n_items
                b1, b2 = group["betas"]
                check(lib().mas_adam_multi_dev(
                    C.c_void_p(table.data_ptr()), ptr(base) if self.ema_decay is not None else None, ptr(base + 8 * n_items), n_items, blocks,
                    C.c_void_p(d["lr"].data_ptr() + 4 * gi), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                    C.c_void_p(d["coef"].data_ptr()) if self.max_grad_norm is not None else None, self._decoupled_wd,
                    0.0 if self.ema_decay is None else self.ema_decay, C.c_void_p(d["vec"].data_ptr()) if self.ema_warmup and self.ema_decay is not None else None,
                    C.c_void_p(d["norm"].data_ptr()) if self.skip_nonfinite else None, C.c_void_p(d["scalars"].data_ptr() + 16 * first), stream),
                    "adam_multi_dev")
            advance.sort()
            k = 0
            while k < len(advance):                          # runs of neighbouring counters: one launch when every parameter has a gradient
                e = k
                while e + 1 < len(advance) and advance[e + 1] == advance[e] + 1:
                    e += 1
                check(lib().mas_adam_advance_dev(C.c_void_p(d["vec"].data_ptr() + 4 * advance[k]), e - k + 1, stream), "adam_advance_dev")
                k = e + 1

    @staticmethod
    def _capturing_now():
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self.state_generation = self.state_generation + 1

    def state_dict(self):
        """torch.optim.Optimizer.state_dict(); with ``device_step`` the ``step`` entries are copies (not views of the shared vector) and
        ``param_groups[0]["ema_step"]`` is read from the device here (one host read: not under a capture)"""
        if self.device_step and self._dev is not None and self.ema_decay is not None:
            self.param_groups[0]["ema_step"] = int(self._dev["vec"][0])
        sd = super().state_dict()
        if self.device_step:                                 # (the packed state holds the optimizer's own dicts: new ones, not new entries)
            sd["state"] = {k: {**st, "step": st["step"].clone()} if torch.is_tensor(st.get("step")) else st for k, st in sd["state"].items()}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict().  With ``device_step`` the loaded values are copied INTO the state tensors that exist
        (same shape), so their storage does not move; a parameter the loaded state does not hold starts over (zero moments and count, the
        average from the weights) in place too.  Bumps ``state_generation``."""
        self.state_generation = self.state_generation + 1
        if not self.device_step:
            return super().load_state_dict(state_dict)
        params = [p for group in self.param_groups for p in group["params"]]
        old = {p: dict(self.state[p]) for p in params if p in self.state and len(self.state[p])}
        super().load_state_dict(state_dict)
        for p, mine in old.items():
            new = dict(self.state[p]) if p in self.state else {}
            for key, t in mine.items():
                v = new.get(key)
                if v is None:                                # not in the loaded state: as at the first step
                    t.copy_(p.detach()) if key == "ema" else t.zero_()
                elif key == "step" or (torch.is_tensor(v) and v.shape == t.shape):
                    t.copy_(torch.as_tensor(v, dtype=t.dtype))
                    new[key] = t
            for key, t in mine.items():
                new.setdefault(key, t)
            self.state[p] = new
        if self._dev is not None and self.ema_decay is not None:
            self._dev["vec"][0] = float(self.param_groups[0].get("ema_step", 0))
        self._lr_pushed = None                               # (the groups are the loaded ones)

    def _ema_pairs(self):
        return [(p, self.state[p]["ema"]) for group in self.param_groups for p in group["params"] if "ema" in self.state.get(p, ())]

    @torch.no_grad()
    def _swap(self):
        """p <-> state[p]["ema"] for every parameter that has one: one mas_swap_multi launch per device, a temporary for the rest"""
        per_device = {}
        for p, e in self._ema_pairs():
            if p.numel() == 0:
                continue
            if (p.is_cuda and e.device == p.device and p.dtype == torch.float32 and e.dtype == torch.float32 and p.is_contiguous()
                    and e.is_contiguous()):
                per_device.setdefault(p.device, []).append((p, e))
            else:
                tmp = p.detach().clone()
                p.detach().copy_(e)
                e.copy_(tmp)
        for device, pairs in per_device.items():
            items, blocks = [], 0
            for p, _ in pairs:
                it = AdamItem()
                it.p, it.n, it.first_block = p.data_ptr(), p.numel(), blocks
                blocks += lib().mas_adam_blocks(p.numel())
                items.append(it)
            with torch.cuda.device(device):
                table = self._table(("swap", device.index), device, items, _pointers([e.data_ptr() for _, e in pairs]))
                other = C.cast(C.c_void_p(table.data_ptr() + C.sizeof(AdamItem) * len(items)), C.POINTER(C.c_void_p))
                check(lib().mas_swap_multi(C.c_void_p(table.data_ptr()), other, len(items), blocks,
                                           C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "swap_multi")
        from . import ops                            # (ops binds the whole library: not needed to construct or step an optimizer)
        ops.invalidate_weight_cache()

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside, the parameters hold the averaged weights and ``state[p]["ema"]`` the live ones; packed weight images and bf16 shadows
        are invalidated on entry and on exit, so every kernel sees the weights that are there.  After exit both are restored bit for
        bit.  No storage moves (captured decode graphs stay valid).  Entering twice, or ``step()`` inside, raises."""
        name = f"mas_hip.optim.{type(self).__name__}"
        if self._swapped:
            raise RuntimeError(f"{name}: swap_ema() is already active")
        if self.ema_decay is None:
            raise RuntimeError(f"{name}: swap_ema() needs ema_decay")
        self._swap()
        self._swapped = True
        try:
            yield self
        finally:
            self._swapped = False
            self._swap()

    def ema_state_dict(self, module):
        """``module.state_dict()`` with every parameter that has an average replaced by a clone of it; buffers and parameters without one
        are unchanged (the averaged weights are in the parameters themselves inside ``swap_ema()``: the result is the same)"""
        sd = module.state_dict()
        for name, p in module.named_parameters(remove_duplicate=False):
            if name in sd and "ema" in self.state.get(p, ()):
                sd[name] = (p if self._swapped else self.state[p]["ema"]).detach().clone()
        return sd


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
