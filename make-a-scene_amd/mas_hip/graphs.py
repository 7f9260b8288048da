"""``GraphedTrainStep``: a whole training call -- zero_grad, the refresh of stale weight images and bf16 shadows, forward, backward,
``optimizer.step()`` -- captured into a graph and replayed, so that a call costs the host one graph launch instead of the ~1200 kernel
launches of a stage-2 step.  Opt-in; nothing else in the package changes behaviour.

    opt  = mas_hip.optim.AdamW(model.parameters(), lr=4.5e-4, device_step=True)
    step = mas_hip.graphs.GraphedTrainStep(lambda t, s, i: model.token_loss(t, s, i), opt, (text, seg, img),
                                           amp_dtype=torch.bfloat16, modules=[model])
    for text, seg, img in loader:
        loss = step(text, seg, img)          # copies the inputs into the static ones, replays; the static 0-dim loss, no host read

One mechanism serves every step (``GraphedGanStep`` below is the VQ-IMG call on the same machinery):

* CONSTRUCTION TRAINS: ``warmup >= 1`` real training calls on ``example_inputs``, eager, on a side stream.  They settle the GEMM choices,
  every workspace and the optimizer state, tick the codebooks and count towards ``accumulate`` (``step.calls``).
* a CALL, on the host: the tick (``step.calls``, and ``Codebook.tick`` of every training codebook: its counter, and its
  re-initialisation when due -- eager, BEFORE the replay; the captured forward does not tick); a comparison of the SIGNATURE -- what a
  capture bakes in that the host can still change: every optimizer's ``state_generation``, ``betas`` / ``eps`` / ``weight_decay`` and
  clip / EMA / guard settings, the inputs' shapes and dtypes, the compute dtype, ``training`` of every module under ``modules=``, each
  codebook's phase -- with the one captured, and a lazy capture when they differ; ``sync_hyperparameters()`` (a changed learning rate
  needs no capture); the copy of the inputs into the static ones; the replay.  Afterwards the codebooks are told the rows the replay
  collected, and on a closing call the weight caches are told that the weights moved (what the optimizer's post-step hook does), so an
  eager forward, ``generate()``, ``swap_ema()`` or a checkpoint between replays sees the current weights.
* a CAPTURE executes nothing and runs no warm-up call (it changes no value); ``step.captures`` counts graphs.  It runs on the side
  stream under ``torch.autocast("cuda", amp_dtype, cache_enabled=False)`` (autocast off without ``amp_dtype``) with the convolution
  weight-gradient side stream off: one stream without branches.  The weight caches are made stale just before it, so their refresh is
  part of the graph and every replay recomputes the images from the weights of that moment; the step keeps the images alive.
* a PHASE is what a codebook's training forward does at its call counter: no collect and unquantised, collect and unquantised,
  collect + lookup.  A capture holds the graphs of the phase of that moment; a phase change is a signature change: three captures over
  a run.  ``codebooks=`` defaults to every ``Codebook`` under ``modules=``; each needs ``enable_device_reservoir()``, else this raises.
* ``accumulate=k`` > 1: the optimizer steps on calls k, 2k, ... on the sum of the k calls' gradients (unaveraged, as the reference's
  loop; the reference itself steps on calls 1, k+1, ...).  A phase then has two graphs that share the static inputs and one memory
  pool: a micro-step (forward, backward ADDING into the gradients that are there) and a closing step (the same, ``optimizer.step()``,
  the gradients zeroed in place).  The gradients are the tensors the warm-up calls left; a parameter without one keeps
  ``.grad = None`` (AdamW does not decay it) until a capture shows that it receives one -- the embedding when the lookup begins -- and
  then gets a persistent zero tensor, and the capture is taken again.
* nothing is captured before the first call (``step.captures == 0``) -- except for a step that has one phase and one graph for life
  (no codebook, ``accumulate == 1``): its capture is taken at the end of construction.
* the optimizer is ``mas_hip.optim.Adam`` / ``AdamW`` with ``device_step=True`` (step count, bias corrections, learning rate and EMA
  counter on the device); dropout needs nothing (its ``{seed, offset}`` is drawn on the device, a replay advances the generator); the
  returned loss is the replayed graph's static tensor, overwritten by the next call of that graph.
* ``nn.Embedding`` lookups of more than a few thousand indices must go through ``graphs.embedding(module, idx)`` (``MakeAScene`` does):
  ATen's backward for them reads a count on the host and faults when replayed.  Under a capture the helper sums ATen's dense backward
  over slices of the indices: the eager result up to the order of those additions, and exactly it inside ``embedding_grad_in_chunks()``.

Not supported: ``GradReducer`` / DistributedDataParallel wrappers (their collectives run on other streams; ``reducer=`` raises), inputs
that are not tensors, and a ``loss_fn`` that reads anything on the host."""
import collections
import contextlib
import warnings

import torch
import torch.nn.functional as F

from . import ops, optim

# nn.Embedding's backward cannot be captured beyond a few thousand indices: above 3072 of them ATen sorts the indices and counts the
# distinct ones with a thrust call that hands the count to the HOST (on ROCm; its fast kernel covers the smaller cases), so a capture
# bakes in whatever the host read without the kernel having run, and the replay faults.  Below, the same ATen backward is called on
# slices of at most this many indices -- the size every slice of which takes the fast kernel -- and the slices' dense results are added.
EMBEDDING_GRAD_CHUNK = 2048
_chunks_always = False


class _EmbeddingGradInChunks(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, idx):
        ctx.save_for_backward(idx)
        ctx.rows = weight.shape[0]
        return F.embedding(idx, weight)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        flat, g = idx.reshape(-1), dy.reshape(-1, dy.shape[-1])
        total = None
        for a in range(0, flat.numel(), EMBEDDING_GRAD_CHUNK):
            part = torch.ops.aten.embedding_dense_backward(g[a:a + EMBEDDING_GRAD_CHUNK], flat[a:a + EMBEDDING_GRAD_CHUNK], ctx.rows, -1, False)
            total = part if total is None else total.add_(part)
        return total, None


def embedding(module, idx):
    """``module(idx)`` for an ``nn.Embedding``, with a backward that a graph can capture at any number of indices: under a capture (or
    inside ``embedding_grad_in_chunks()``) and above ``EMBEDDING_GRAD_CHUNK`` indices the weight gradient is the sum of ATen's own dense
    backward over slices of the indices -- the eager result up to the order of the additions.  Everywhere else it IS ``module(idx)``."""
    if not (idx.is_cuda and idx.numel() > EMBEDDING_GRAD_CHUNK and torch.is_grad_enabled() and module.weight.requires_grad
            and (_chunks_always or torch.cuda.is_current_stream_capturing())):
        return module(idx)
    if module.padding_idx is not None or module.max_norm is not None or module.scale_grad_by_freq or module.sparse:
        raise NotImplementedError("mas_hip.graphs.embedding: padding_idx / max_norm / scale_grad_by_freq / sparse embeddings cannot be "
                                  f"captured above {EMBEDDING_GRAD_CHUNK} indices")
    return _EmbeddingGradInChunks.apply(module.weight, idx)


@contextlib.contextmanager
def embedding_grad_in_chunks():
    """inside, ``embedding()`` takes its capture-safe backward in eager code too: what a replayed step computes, step by step"""
    global _chunks_always
    old, _chunks_always = _chunks_always, True
    try:
        yield
    finally:
        _chunks_always = old


class GraphedTrainStep:
    def __init__(self, loss_fn, optimizer, example_inputs, *, amp_dtype=None, warmup=1, modules=(), reducer=None, codebooks=None,
                 accumulate=1):
        name = type(self).__name__
        if isinstance(accumulate, bool) or not isinstance(accumulate, int):
            raise TypeError(f"{name}: accumulate must be an integer (calls per optimizer step), got {accumulate!r}")
        if accumulate < 1:
            raise ValueError(f"{name}: accumulate must be at least 1, got {accumulate}")
        if reducer is not None:
            raise NotImplementedError(f"{name}: a gradient reducer runs collectives on other streams, which one captured stream cannot "
                                      "hold; train data-parallel runs eagerly")
        self.loss_fn, self.optimizer, self.amp_dtype = loss_fn, optimizer, amp_dtype
        for role, opt in self._roles().items():
            if not isinstance(opt, optim.Adam) or not opt.device_step:
                raise TypeError(f"{name}: {role} must be mas_hip.optim.Adam / AdamW with device_step=True (a step whose count, bias "
                                f"corrections and learning rate live on the device), got {type(opt).__name__}"
                                + ("" if not isinstance(opt, optim.Adam) else " with device_step=False"))
        if int(warmup) < 1:
            raise ValueError(f"{name}: warmup must be at least 1 (the capture needs every buffer and GEMM choice settled)")
        if isinstance(example_inputs, torch.Tensor):
            example_inputs = (example_inputs,)
        self._opts = list(self._roles().values())
        self.modules = [modules] if isinstance(modules, torch.nn.Module) else list(modules)
        self.captures = 0
        self.graph = self.loss = self._sig = self._keep = None
        if codebooks is None:                                 # (duck-typed: models imports this package, not the other way round)
            seen = []
            for mod in self.modules:
                seen += [m for m in mod.modules() if hasattr(m, "enable_device_reservoir") and not any(m is s for s in seen)]
            codebooks = seen
        self.codebooks = [codebooks] if isinstance(codebooks, torch.nn.Module) else list(codebooks)
        for cb in self.codebooks:
            if not getattr(cb, "device_reservoir", False):
                raise RuntimeError(f"{name}: a Codebook without its device reservoir cannot be captured (its reservoir is kept by CPU "
                                   "permutations and a growing tensor): call codebook.enable_device_reservoir() first")
        self.accumulate, self.calls = accumulate, 0
        self._graphs, self._cb_rows = {}, []
        self._check_inputs(example_inputs)
        self._side = torch.cuda.Stream(device=example_inputs[0].device)
        self._static = [x.detach().clone() for x in example_inputs]
        self._warm_up(int(warmup))
        if self._captures_at_construction and not self.codebooks and accumulate == 1:
            self._capture()                                   # one phase, one graph: taken now

    _captures_at_construction = True

    def _roles(self):
        """the optimizers in the order they step, by what a message calls each"""
        return {"the optimizer": self.optimizer}

    @staticmethod
    def _check_inputs(inputs):
        if not inputs or not all(isinstance(x, torch.Tensor) and x.is_cuda for x in inputs):
            raise TypeError("GraphedTrainStep: the inputs must be CUDA tensors")

    def _autocast(self):
        if self.amp_dtype is None:
            return torch.autocast("cuda", enabled=False, cache_enabled=False)
        return torch.autocast("cuda", dtype=self.amp_dtype, cache_enabled=False)

    def _signature(self, inputs):
        """everything a capture bakes in that the host can still change"""
        return (tuple((opt.state_generation,
                       tuple((tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"]), len(g["params"])) for g in opt.param_groups),
                       opt.max_grad_norm, opt.ema_decay, opt.ema_warmup, opt.skip_nonfinite) for opt in self._opts), ops.compute_dtype(),
                tuple((tuple(x.shape), x.dtype, x.device) for x in inputs),
                tuple(m.training for mod in self.modules for m in mod.modules()),
                tuple((cb.training, cb.phase()) for cb in self.codebooks))

    def _stale_for_capture(self):
        """Every derived copy of a parameter is made stale, so that its refresh gets captured.  The refresh of the packed convolution
        weights reads an item table that is uploaded from pageable memory when the set of stale images is new, which a capture cannot
        hold: the same refresh runs eagerly first (twice: the first one also takes whatever else in the process was stale, the second
        one uploads the table of this step's images alone; it changes no value, and does nothing for a model without convolutions)."""
        for _ in range(2):
            for opt in self._opts:
                ops._note_optimizer_step(opt)
            ops.refresh_stale_weight_images(self._side.device)
        for opt in self._opts:
            ops._note_optimizer_step(opt)

    @contextlib.contextmanager
    def _codebooks_in(self, mode):
        """every codebook inside its context ``mode``: ``ticked_by_caller`` (the forward leaves the tick to ``_tick``), ``dry_forward``"""
        with contextlib.ExitStack() as stack:
            for cb in self.codebooks:
                stack.enter_context(getattr(cb, mode)())
            yield

    def _tick(self):
        self.calls += 1
        for cb in self.codebooks:
            if cb.training:
                cb.tick()
        return self.calls % self.accumulate == 0            # a closing call: the optimizer steps

    def _keys(self):
        """the graphs of one phase, in capture order (what ``_step`` is handed): the closing step alone, or the micro-step and the closing step"""
        return (True,) if self.accumulate == 1 else (False, True)

    def _key(self, closing):
        """the graph this call replays"""
        return closing

    def _settle_for_capture(self):
        """eager work that a capture needs done first (on the side stream, just before the graphs are taken); changes no value"""

    def _zero_grads_in_place(self):
        """after a closing step under accumulate > 1: the gradients stay where the captured kernels add into them"""
        grads = [p.grad for opt in self._opts for g in opt.param_groups for p in g["params"] if p.grad is not None]
        if grads:
            torch._foreach_zero_(grads)

    def _step(self, closing):
        """one call.  accumulate == 1: zero_grad, forward, backward, ``optimizer.step()``; else forward and backward ADDING into the
        gradients that are there, and on a closing call ``optimizer.step()`` and the gradients zeroed in place"""
        if self.accumulate == 1:
            self.optimizer.zero_grad(set_to_none=True)
        loss = self.loss_fn(*self._static)
        loss.backward()
        if closing:
            self.optimizer.step()
            if self.accumulate > 1:
                self._zero_grads_in_place()
        return loss

    @staticmethod
    def _detached(loss):
        return loss.detach()

    def _warm_up(self, warmup):
        """``warmup`` real training calls, eager, under the conditions of the capture"""
        main = torch.cuda.current_stream(self._side.device)
        for opt in self._opts:
            opt.init_state()
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side), ops.wgrad_stream_off(), self._codebooks_in("ticked_by_caller"):
            for _ in range(warmup):
                closing = self._tick()
                with self._autocast():
                    self._step(self._key(closing))
        main.wait_stream(self._side)

    def _capture(self):
        """the graphs of the phase the codebooks are in now: one step when accumulate == 1, else a micro-step and a closing step that share
        the static inputs and one memory pool.  Executes nothing."""
        opts, k = self._opts, self.accumulate
        self.graph = self.loss = None
        self._graphs = {}                                   # (the old phase's graphs and their memory go first)
        main = torch.cuda.current_stream(self._side.device)
        params = [p for opt in opts for g in opt.param_groups for p in g["params"]]
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side), ops.wgrad_stream_off(), self._codebooks_in("ticked_by_caller"):
            if k == 1:
                for opt in opts:
                    opt.zero_grad(set_to_none=True)
            self._settle_for_capture()
            pool = None                                     # the phase's graphs share the first one's memory pool
            for key in self._keys():
                for attempt in range(2):
                    for opt in opts:
                        opt.init_state()
                    self._stale_for_capture()
                    without = [p for p in params if p.requires_grad and p.grad is None] if k > 1 else []
                    graph = torch.cuda.CUDAGraph()
                    with self._codebooks_in("dry_forward"), torch.cuda.graph(graph, pool=pool, stream=self._side), self._autocast():
                        loss = self._step(key)
                    self._cb_rows = [cb.rows_per_call() for cb in self.codebooks]
                    fresh = [p for p in without if p.grad is not None]
                    if not fresh:
                        break
                    # autograd installed a tensor of the graph's pool as these gradients (the embedding at the start of the lookup phase):
                    # they become persistent zeros that the capture, taken again, adds into
                    if attempt:
                        raise RuntimeError(f"{type(self).__name__}: gradients appeared at the second capture that the first one did not produce")
                    del graph, loss
                    for p in fresh:
                        p.grad = torch.zeros_like(p)
                self.graph, self.loss = self._graphs[key] = (graph, self._detached(loss))
                pool = graph.pool()
                self.captures += 1
        main.wait_stream(self._side)
        # the images the graphs read are kept alive here (invalidate_weight_cache() / swap_ema() drop the caches' own references); and
        # nothing ran, so none of the stamps the caches wrote inside the capture describes a refresh that happened
        self._keep = ops.weight_cache_tensors()
        ops.forget_capture_stamps()
        self._sig = self._signature(self._static)

    def _replay(self, inputs):
        closing = self._tick()                              # eager, before the replay: the counter, and a due re-initialisation
        if self._signature(inputs) != self._sig:
            if len(inputs) != len(self._static) or any(x.shape != s.shape or x.dtype != s.dtype or x.device != s.device
                                                       for x, s in zip(inputs, self._static)):
                self._graphs = {}
                self._static = [x.detach().clone() for x in inputs]
            self._capture()
        for opt in self._opts:
            opt.sync_hyperparameters()
        for s, x in zip(self._static, inputs):
            if x is not s:
                s.copy_(x, non_blocking=True)
        self.graph, self.loss = self._graphs[self._key(closing)]
        self.graph.replay()
        for cb, n in zip(self.codebooks, self._cb_rows):
            if n:
                cb.replay_collected(n)
        if closing:
            for opt in self._opts:
                ops._note_optimizer_step(opt)
        return self.loss

    def __call__(self, *inputs):
        self._check_inputs(inputs)
        return self._replay(inputs)


class GanStepOut(collections.namedtuple("GanStepOut", "loss d_loss nll_loss g_loss d_weight")):
    """what one call of ``GraphedGanStep`` returns: the graph's static 0-dim tensors, overwritten by the next call"""
    __slots__ = ()


class GraphedGanStep(GraphedTrainStep):
    """The VQ-IMG training call -- one forward, the discriminator's backward, the generator's backward with the two ``autograd.grad``
    calls of the adaptive weight, and on a closing call both Adams -- captured and replayed with ``GraphedTrainStep``'s machinery
    (warm-up on the side stream, one stream without branches, stale weight caches, signature and lazy recapture, codebook phases ticked
    eagerly before the replay, a micro-step and a closing-step graph under ``accumulate > 1``, persistent zeroed gradients).

        gopt = mas_hip.optim.Adam(model.parameters(), lr=..., betas=(0.5, 0.9), device_step=True)
        dopt = mas_hip.optim.Adam(loss.discriminator.parameters(), lr=..., betas=(0.5, 0.9), device_step=True)
        step = mas_hip.graphs.GraphedGanStep(model, loss, gopt, dopt, example_images, accumulate=8, global_step=0)
        out = step(images)          # out.loss, out.d_loss, out.nll_loss, out.g_loss, out.d_weight: static 0-dim tensors

    One call, in the order of the reference's loop (train.py:84-103): ``model(images)``; the discriminator loss on detached tensors and
    its ``backward()``; with ``requires_grad`` of the discriminator's parameters off (host flags, restored afterwards) the generator
    loss and its ``backward()``; on calls k, 2k, ... ``dopt.step()``, ``gopt.step()`` and the gradients zeroed in place.

    * ``loss`` is a ``losses.loss_img.VQLPIPSWithDiscriminator``; its tail runs with ``hip_tail`` on inside every call of this class,
      whatever the process-wide switch says: the gate ``global_step >= disc_start`` is evaluated on the device, so the gate opening needs
      no new capture.  ``step.global_step`` is the 0-dim int64 device counter the captured generator half advances by one per call;
      ``step.set_global_step(n)`` writes it (a resumed run).  Calls made at construction (``warmup``) count.
    * the signature holds both optimizers' ``state_generation``, hyperparameters and clip / EMA / guard settings, ``training`` of every
      module of ``model`` and ``loss``, and the codebook phase; ``sync_hyperparameters()`` of both runs before each replay.
    * the face term: a ``loss.face_loss`` that is a ``losses.face_loss.FaceLoss`` in evaluation mode is captured.  ``step(images,
      bbox_face)`` takes one list of boxes per image (``None``: no faces), plans them on the host and writes them into the step's
      ``mas_hip.face.FaceTable`` (``step.face_table``: ~300 bytes, one asynchronous copy, nothing read back), which the captured
      fixed-capacity node reads.  Every phase then has its graphs TWICE, keyed ``(closing, faces)``: without the term (a call without
      faces replays exactly what a step with ``face_loss=None`` replays) and with it; both are captured together and share the phase's
      pool, so batches with and without faces alternate without a capture.  ``example_bbox_face``: the boxes of the warm-up calls.
    * the object term: a ``loss.object_loss`` that is a ``losses.object_loss.ObjectLoss`` (``object_loss="lpips"``) is captured.
      ``step(images, bbox_face, bbox_obj)`` takes one list of boxes per image (``None``: no objects), plans them on the host and writes
      them into the step's ``mas_hip.objects.ObjectAtlas`` (``step.object_atlas``: ``object_atlas=`` at construction is an
      ``ObjectAtlas``, a dict of its keyword arguments, or ``None`` for its default geometry), which the captured fixed-capacity node
      reads.  The graphs are then keyed ``(closing, faces, objects)``: a call whose boxes yield no used crop replays the variant
      without the term -- exactly what a step with ``object_loss=None`` replays; all variants of a phase are captured together and
      share its pool.  (Without an object term the keys stay ``(closing, faces)``.)  Boxes that do not fit the atlas
      (``objects.AtlasOverflow``): ``on_overflow="eager"`` (the default) runs that ONE call eagerly through the same ``_step`` on the
      side stream, under the conditions of the warm-up calls, with the box lists on the list path; it counts in ``step.eager_calls``,
      warns once (``RuntimeWarning``), and leaves the graphs as they are.  ``on_overflow="raise"`` re-raises before the tick, like
      a refused face box.  ``example_bbox_obj``: the boxes of the warm-up calls.
    * refused at construction: an optimizer without ``device_step``, a codebook without its device reservoir, a ``reducer``, any
      ``object_loss`` that is not an ``ObjectLoss`` (a callable), and any other ``face_loss`` (a callable, a ``FaceLoss`` in ``train()``
      mode): their crops are cut from host box lists.  The perceptual term may be LPIPS with its HIP path on or off, any capturable
      callable, or ``None``."""

    def __init__(self, model, loss, gen_optimizer, disc_optimizer, example_images, *, amp_dtype=None, accumulate=1, global_step=0, warmup=1,
                 reducer=None, example_bbox_face=None, example_bbox_obj=None, object_atlas=None, on_overflow="eager"):
        name = type(self).__name__
        capturable = {"face_loss": self._capturable_face, "object_loss": self._capturable_object}
        for term in ("face_loss", "object_loss"):
            if getattr(loss, term, None) is not None and not capturable[term](getattr(loss, term)):
                raise NotImplementedError(f"{name}: the loss has a {term}, whose crops are cut from host box lists that a capture "
                                          f"cannot hold; build the loss with {term}=None, or train eagerly")
        if not hasattr(loss, "hip_tail") or not hasattr(loss, "discriminator"):
            raise TypeError(f"{name}: the loss must be a losses.loss_img.VQLPIPSWithDiscriminator, got {type(loss).__name__}")
        self._check_inputs((example_images,))
        # what the warm-up calls at the end of the base constructor need: they are calls like any other
        self.model, self.loss_module = model, loss
        self.gen_optimizer, self.disc_optimizer = gen_optimizer, disc_optimizer
        self.global_step = torch.full((), int(global_step), dtype=torch.int64, device=example_images.device)
        self.face_table, self._faces = None, False
        if getattr(loss, "face_loss", None) is not None:
            from . import face
            self.face_table = face.FaceTable(example_images.device)
        if on_overflow not in ("eager", "raise"):
            raise ValueError(f"{name}: on_overflow must be 'eager' or 'raise', got {on_overflow!r}")
        self.on_overflow, self.eager_calls, self._warned_overflow = on_overflow, 0, False
        self.object_atlas, self._objects, self._obj_lists = None, False, None
        if getattr(loss, "object_loss", None) is not None:
            from . import objects
            if isinstance(object_atlas, objects.ObjectAtlas):
                if object_atlas.device != example_images.device or object_atlas.n_images > example_images.shape[0]:
                    raise ValueError(f"{name}: the object atlas is on {object_atlas.device} for {object_atlas.n_images} images, the batch "
                                     f"has {example_images.shape[0]} on {example_images.device}")
                self.object_atlas = object_atlas
            else:
                self.object_atlas = objects.ObjectAtlas(example_images.device, example_images.shape[0], **(object_atlas or {}))
        self._write_faces(example_bbox_face, example_images.shape[0])
        self._write_objects(example_bbox_obj)
        super().__init__(None, gen_optimizer, (example_images,), amp_dtype=amp_dtype, warmup=warmup, modules=[model, loss], reducer=reducer,
                         accumulate=accumulate)

    _captures_at_construction = False                         # (a VQ-IMG model holds a codebook; without one the rule stays the same)

    def _roles(self):
        return {"the discriminator's optimizer": self.disc_optimizer, "the generator's optimizer": self.gen_optimizer}

    @staticmethod
    def _capturable_face(term):
        """a ``losses.face_loss.FaceLoss`` in evaluation mode: the one face term whose rows a device table can carry"""
        try:                                                  # (the loss stack imports this package, not the other way round)
            from losses.face_loss import FaceLoss
        except ImportError:
            return False
        return isinstance(term, FaceLoss) and not term.training

    @staticmethod
    def _capturable_object(term):
        """a ``losses.object_loss.ObjectLoss``: the one object term whose crops a device table (``objects.ObjectAtlas``) can carry"""
        try:
            from losses.object_loss import ObjectLoss
        except ImportError:
            return False
        return isinstance(term, ObjectLoss)

    def _write_objects(self, bbox_obj):
        """the call's boxes into the atlas (host planning, one asynchronous copy); sets which variant the call takes.  Boxes that do
        not fit: re-raised (``on_overflow="raise"``), or kept as host lists for one eager call; the atlas keeps what it held.  Without
        an object term the boxes are ignored."""
        self._objects, self._obj_lists = False, None
        if self.object_atlas is None:
            return
        from . import objects
        try:
            self._objects = self.object_atlas.write(bbox_obj) > 0
        except objects.AtlasOverflow as e:
            if self.on_overflow == "raise":
                raise
            if not self._warned_overflow:
                self._warned_overflow = True
                warnings.warn(f"{type(self).__name__}: {e}; this call runs eagerly on the list path (on_overflow='eager'; this warning "
                              "is issued once, step.eager_calls counts)", RuntimeWarning, stacklevel=3)
            self._objects, self._obj_lists = True, objects.box_lists(bbox_obj)

    def _write_faces(self, bbox_face, n_images):
        """the call's boxes into the table (host planning and checks, one asynchronous copy); sets which variant the call takes.
        Without a face term the boxes are ignored, as the loss ignores them."""
        self._faces = self.face_table is not None and self.face_table.write(bbox_face, n_images) > 0

    def _keys(self):
        variants = (False, True) if self.face_table is not None else (False,)
        keys = tuple((closing, faces) for closing in super()._keys() for faces in variants)
        if self.object_atlas is None:
            return keys
        return tuple(key + (objects,) for key in keys for objects in (False, True))

    def _key(self, closing):
        return (closing, self._faces) if self.object_atlas is None else (closing, self._faces, self._objects)

    def _settle_for_capture(self):
        """the face term alone, once, eagerly, on whatever the table holds: its weights' packed images, the BatchNorm address table and
        the convolutions' choices exist before a capture meets them (the term is frozen: no value moves)"""
        x = self._static[0]
        for term, table in ((self.loss_module.face_loss, self.face_table), (self.loss_module.object_loss, self.object_atlas)):
            if table is not None:                             # (the object term likewise: its LPIPS weights are frozen)
                rec = x.detach().clone().requires_grad_(True)
                with self._autocast():
                    term(x, rec, table).backward()

    def set_global_step(self, n):
        """writes the device counter (a resume); no capture depends on its value"""
        self.global_step.fill_(int(n))

    @staticmethod
    def _detached(out):
        return GanStepOut(*(t.detach() for t in out))

    def _step(self, key):
        closing, faces, objects = key if len(key) == 3 else key + (False,)
        model, crit, images = self.model, self.loss_module, self._static[0]
        # the object term's boxes: the atlas (what a capture holds), or the host lists of a call that did not fit it (eager only);
        # a call without a used crop runs without the term, as a loss built with object_loss=None does
        term, bbox_obj = getattr(crit, "object_loss", None), None
        if objects:
            bbox_obj = self._obj_lists if self._obj_lists is not None else self.object_atlas
        if self.accumulate == 1:
            for opt in self._opts:
                opt.zero_grad(set_to_none=True)
        disc = list(crit.discriminator.parameters())
        flags, advance = [p.requires_grad for p in disc], crit.advance_global_step
        with crit.hip_tail(True):
            rec, q_loss = model(images)
            d_loss = crit(1, self.global_step, images, rec)
            d_loss.backward()
            try:
                for p in disc:
                    p.requires_grad_(False)
                crit.advance_global_step = True
                if term is not None and not objects:
                    crit.object_loss = None
                loss, (nll_loss, _, _) = crit(0, self.global_step, images, rec, q_loss, bbox_obj=bbox_obj,
                                              bbox_face=self.face_table if faces else None, last_layer=model.decoder.model[-1])
                loss.backward()
            finally:
                if term is not None:
                    crit.object_loss = term
                crit.advance_global_step = advance
                for p, f in zip(disc, flags):
                    p.requires_grad_(f)
        terms = crit.last_terms
        if closing:
            self.disc_optimizer.step()
            self.gen_optimizer.step()
            if self.accumulate > 1:
                self._zero_grads_in_place()
        return GanStepOut(loss, d_loss, nll_loss, terms["g_loss"], terms["d_weight"])

    def _eager_call(self, images):
        """one call without a graph -- the tick, the hyperparameters, the static input and ``_step`` as a replay would run them, eagerly on
        the side stream under the conditions of ``_warm_up``.  The graphs stay valid: an eager ``optimizer.step()`` uploads tables of
        its own and bumps no ``state_generation``, and under ``accumulate > 1`` the backward adds into the persistent gradients the
        graphs add into.  The outputs are this call's own tensors, not the graphs' static ones."""
        closing = self._tick()
        for opt in self._opts:
            opt.sync_hyperparameters()
        s = self._static[0]
        if images.shape != s.shape or images.dtype != s.dtype or images.device != s.device:
            self._graphs, self._sig = {}, None                # (the next replay captures for the new shape, as it would have anyway)
            self._static = [images.detach().clone()]
        elif images is not s:
            s.copy_(images, non_blocking=True)
        main = torch.cuda.current_stream(self._side.device)
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side), ops.wgrad_stream_off(), self._codebooks_in("ticked_by_caller"), self._autocast():
            out = self._detached(self._step(self._key(closing)))
        main.wait_stream(self._side)
        self.eager_calls += 1
        return out

    def __call__(self, images, bbox_face=None, bbox_obj=None):
        self._check_inputs((images,))
        self._write_faces(bbox_face, images.shape[0])         # (before the tick: a box that is refused leaves the counters alone)
        self._write_objects(bbox_obj)
        if self._obj_lists is not None:                       # the boxes do not fit the atlas: this one call runs eagerly
            return self._eager_call(images)
        return self._replay((images,))
