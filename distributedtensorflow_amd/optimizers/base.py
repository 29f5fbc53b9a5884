"""Optimizer base: TF1-style ``minimize / compute_gradients / apply_gradients`` on flat buffers.

Reference usage: ``tf.train.AdamOptimizer(5e-4).minimize(loss,
global_step=global_step)`` (``run_mnist_distributed.py:116``), Adam 0.01
(``templates/00_mnist_replica.py:166``), Adagrad 0.01 (``templates/00_between…:34``).

MI355X design: on first use every trainable variable is re-homed into ONE flat fp32 master
buffer (views), gradients live in ONE flat fp32 buffer (views; autograd accumulates into them in
place) and each optimizer slot is one flat buffer.  The update is therefore a single fused HIP
launch over the whole model (no per-tensor launches, no multi-tensor lists), and the strategy's
gradient all-reduce operates on contiguous bucket slices of the same flat gradient buffer.

Layout: variables are placed in REVERSE creation order (backward produces gradients roughly
last-layer-first, so contiguous buckets complete in order), decayed variables first, then the
non-decayed ones (BatchNorm gamma/beta, biases) in their own tail region.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass

import torch

from ..train import global_step as gs


@dataclass
class FlatSlot:
    name: str           # TF slot suffix, e.g. "Momentum", "Adam", "Adam_1"
    buf: torch.Tensor


class FlatSpace:
    """Owns the flat master / grad / shadow buffers of a set of variables."""

    def __init__(self, variables, decay_filter=None, shadow_dtype=None, align=64):
        variables = [v for v in variables if v.requires_grad]
        if not variables:
            raise ValueError("no trainable variables")
        dev = variables[0].device
        decay_filter = decay_filter or (lambda v: True)
        decayed = [v for v in reversed(variables) if decay_filter(v)]
        plain = [v for v in reversed(variables) if not decay_filter(v)]
        self.order = decayed + plain
        self.offsets = []
        off = 0
        for v in self.order:
            self.offsets.append(off)
            off += -(-v.numel() // align) * align   # keep every view 256-B aligned
        self.n_decay = -(-sum(v.numel() for v in decayed) // 1)
        self.decay_end = self.offsets[len(decayed)] if plain else off
        self.numel = off
        self.device = dev
        self.master = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        self.shadow = (torch.zeros(off, device=dev, dtype=shadow_dtype)
                       if shadow_dtype is not None else None)
        # gradient accumulation: the held micro-batches' gradient sum, laid out as ``grad``;
        # allocated by ``Optimizer.build`` only for accumulation_steps > 1
        self.accum = None
        with torch.no_grad():
            for v, o in zip(self.order, self.offsets):
                n = v.numel()
                self.master[o:o + n].copy_(v.detach().reshape(-1).float())
                v.data = self.master[o:o + n].view(v.shape)
                v.grad = self.grad[o:o + n].view(v.shape)
                v._dtf_flat = True           # kernels may accumulate into v.grad directly
                v._dtf_grad_ready = None     # set by gradient-bucketing reducers
                if self.shadow is not None:
                    s = self.shadow[o:o + n].view(v.shape)
                    s.copy_(v.data)
                    v._dtf_shadow = s
        self.index = {id(v): i for i, v in enumerate(self.order)}

    def zero_grad(self):
        self.grad.zero_()

    def refresh_shadow(self):
        if self.shadow is not None:
            self.shadow.copy_(self.master)

    def new_slot(self, fill=0.0):
        return torch.full((self.numel,), float(fill), device=self.device, dtype=torch.float32)

    def view_of(self, buf, v):
        i = self.index[id(v)]
        o = self.offsets[i]
        return buf[o:o + v.numel()].view(v.shape)

    def regions(self):
        """[(start, end, decayed)] contiguous regions of the flat buffer."""
        out = [(0, self.decay_end, True)]
        if self.decay_end < self.numel:
            out.append((self.decay_end, self.numel, False))
        return [r for r in out if r[1] > r[0]]


def default_decay_filter(v):
    """TF official ResNet convention: L2 on everything but batch-norm variables and biases."""
    name = getattr(v, "_dtf_name", "")
    return not (re.search(r"(batch_norm|_bn/|/gamma|/beta|/bias)", name) or v.dim() <= 1)


ACCUM_BETWEEN_GRAPH = ("accumulation_steps > 1 is not available in the between-graph "
                       "parameter-server mode: the parameter-server tasks apply each pushed "
                       "gradient on arrival, so a worker has nowhere to hold micro-batches")


CLIP_BETWEEN_GRAPH = ("clip_norm is not available in the between-graph parameter-server mode: "
                      "gradient buckets leave the worker from the backward hooks before the "
                      "global norm is known")


class Optimizer:
    """Base class.  Subclasses implement ``_build_slots`` and ``_apply_native/_apply_reference``.

    ``clip_norm``: clip every step's gradient to this global L2 norm (``tf.clip_by_global_norm``
    of ``grad_scale * g``, then the update).  One deterministic norm pass over the gradient
    writes the multiplier to the device and the fused update reads it from there: no pass that
    rewrites the gradient, no host sync.  ``last_grad_norm`` (a one-element device tensor) holds
    the step's pre-clip norm.

    ``accumulation_steps=N``: N consecutive ``minimize`` calls (or ``compute_gradients`` /
    ``apply_gradients`` pairs) make ONE update.  Calls 1 .. N-1 are held micro-steps: backward
    runs, the gradient goes into ``space.accum`` (``accum = g1``, then ``accum += g``), nothing
    is communicated and nothing else moves.  Call N folds the accumulator into the gradient
    (bucket by bucket, before each bucket's collective) and updates with the gradient
    multiplier ``grad_scale() / N``: the mean over the N micro-batches of
    ``((g1 + g2) + ...) + gN``, summed in fp32 in micro-step order."""

    slot_names: tuple = ()
    # the update of each element depends only on that element's gradient / slots (a sharded
    # parameter server may then split variables between owners); LAMB's per-tensor trust ratio
    # is not elementwise
    elementwise: bool = True

    def __init__(self, learning_rate, name, weight_decay=0.0, decay_filter=None,
                 use_locking=False, clip_norm=None, variable_averages=None,
                 accumulation_steps=1):
        if type(accumulation_steps) is not int or accumulation_steps < 1:
            raise ValueError("accumulation_steps must be an int >= 1, got "
                             f"{accumulation_steps!r}")
        self.accumulation_steps = accumulation_steps
        self._accumulated = 0        # micro-batches held in space.accum
        self._accum_hold = False     # the last compute_gradients was a held micro-step
        if clip_norm is not None:
            clip_norm = float(clip_norm)
            if not clip_norm > 0.0:
                raise ValueError(f"clip_norm must be positive, got {clip_norm}")
        self.clip_norm = clip_norm
        self.last_grad_norm = None   # [1] fp32 on the device once built with clip_norm
        self._clip_rec = None        # {S: f64 | norm: f32, gmul: f32}, the norm pass's record
        self._clip_slab = None       # one fp64 partial sum per chunk of the norm pass
        self._clip_held = False      # a reducer formed this step's record: _apply keeps it
        self._lr_value = learning_rate
        self.name = name
        self.weight_decay = weight_decay
        self.decay_filter = decay_filter or default_decay_filter
        self.space: FlatSpace | None = None
        self.slots: list[FlatSlot] = []
        self.iterations = 0          # number of applied updates (TF: beta powers / global step)
        self._lr_dev = None
        self._nonfinite = None
        self._reducer = None
        self.use_locking = use_locking
        # bf16 compute shadow of the fp32 masters ("auto": on GPUs); None for fp32-compute models
        self.shadow_dtype = "auto"
        # True while a training step is being captured into a HIP graph (train/graphed.py): the
        # per-step hyper-parameters are then written by the replay wrapper, not by the step
        self._capturing = False
        # tf.train.ExponentialMovingAverage of the variables (optimizers/moving_averages.py)
        self.variable_averages = None
        self._variables_to_average = None
        # apply_gradients was given the average's ``num_updates`` object as ``global_step``: it
        # is incremented after the update, and TF's average sees the incremented value
        self._ema_bump = False
        if variable_averages is not None:
            self.set_variable_averages(variable_averages)

    # ------------------------------------------------------------------ hyper-parameters
    def learning_rate(self, step=None):
        lr = self._lr_value
        return float(lr(step if step is not None else self.iterations)) if callable(lr) else float(lr)

    def set_variable_averages(self, ema, variables_to_average=None):
        """Attach a :class:`ExponentialMovingAverage`; before ``build``.  ``variables_to_average``, if given, must be exactly the trainable variables:
        one flat buffer cannot hold a subset."""
        from .moving_averages import ExponentialMovingAverage
        if self.space is not None:
            raise ValueError("variable_averages must be attached before the optimizer is built")
        if not isinstance(ema, ExponentialMovingAverage):
            raise TypeError("variable_averages must be an ExponentialMovingAverage, got "
                            f"{type(ema).__name__}")
        ema._attach(self)
        self.variable_averages = ema
        self._variables_to_average = (None if variables_to_average is None
                                      else list(variables_to_average))

    # ------------------------------------------------------------------ build
    def build(self, variables):
        if self.space is not None:
            return self.space
        from ..parallel import strategy as _strat
        variables = list(variables)
        strat = _strat.get_strategy()
        if self.clip_norm is not None and getattr(strat, "mode", None) == "between_graph":
            raise ValueError(CLIP_BETWEEN_GRAPH)
        if self.accumulation_steps > 1 and getattr(strat, "mode", None) == "between_graph":
            raise ValueError(ACCUM_BETWEEN_GRAPH)
        ema = self.variable_averages
        if ema is not None:
            from .moving_averages import EMA_BETWEEN_GRAPH
            if getattr(strat, "mode", None) == "between_graph":
                raise ValueError(EMA_BETWEEN_GRAPH)
            if self._variables_to_average is not None and \
                    sorted(id(v) for v in self._variables_to_average) != \
                    sorted(id(v) for v in variables if v.requires_grad):
                raise ValueError("variables_to_average must be exactly the trainable variables: "
                                 "the averages are one flat buffer over all of them")
        dev = variables[0].device
        shadow = (torch.bfloat16 if dev.type == "cuda" else None) if self.shadow_dtype == "auto" \
            else self.shadow_dtype
        self.space = FlatSpace(variables, self.decay_filter, shadow)
        self.space.elementwise = self.elementwise      # read by sharding gradient reducers
        if self.accumulation_steps > 1:
            self.space.accum = torch.zeros_like(self.space.grad)
        self._build_slots()
        self._lr_dev = torch.zeros(4, device=dev, dtype=torch.float32)
        self._nonfinite = torch.zeros(1, device=dev, dtype=torch.int32)
        self._build_clip()
        self._reducer = strat.make_gradient_reducer(self.space)
        strat.broadcast_space(self.space)
        if ema is not None:
            ema._build(self)      # TF initialises a shadow with the variable's (broadcast) value
        return self.space

    def _build_slots(self):
        raise NotImplementedError

    # ------------------------------------------------------------------ TF1 API
    def compute_gradients(self, loss, var_list=None):
        if self.space is None:
            self.build(var_list)
        from .. import profiler
        if self.accumulation_steps > 1:
            # calls 1 .. N-1 of an update are held (the reducer communicates nothing); call N
            # folds the accumulator in before each bucket's collective
            self._accum_hold = self._accumulated < self.accumulation_steps - 1
            self._reducer.hold = self._accum_hold
            self._reducer.fold = not self._accum_hold
        self.space.zero_grad()
        self._reducer.begin_step()
        fn = getattr(loss, "grad_fn", None)
        if fn is not None and getattr(fn, "dtf_unit_grad_ok", False):
            fn.dtf_unit_grad = True          # backward() below seeds exactly d(loss) = 1
        with profiler.maybe_phase("backward"):
            loss.backward()
        # every deferred-work record of this step has been consumed (or never will be)
        from .. import ops
        ops.end_step()
        with profiler.maybe_phase("comm"):
            self._reducer.finish()
        if self.accumulation_steps > 1:
            if self._accum_hold:
                ops.grad_accumulate(self.space.accum, self.space.grad, self._accumulated > 0)
                self._accumulated += 1
            else:
                self._accumulated = 0        # folded into the gradient by the reducer
        return [(v.grad, v) for v in self.space.order]

    def apply_gradients(self, grads_and_vars=None, global_step=None):
        assert self.space is not None, "call build()/compute_gradients() first"
        if self._accum_hold:
            return None              # a held micro-step: the gradient is in space.accum
        self.iterations += 1
        ema = self.variable_averages
        self._ema_bump = ema is not None and global_step is not None and \
            global_step is ema.num_updates
        if getattr(self._reducer, "applies_update", False):
            # parameter-server strategies: the PS owning the variables applies the update
            step = self._reducer.apply_remote(self)
            if global_step is not None:
                if step is None:                 # colocated owners: a local synchronous step
                    gs.increment(global_step)
                elif hasattr(global_step, "assign"):
                    global_step.assign(step)     # the PS's authoritative global step
            return step
        from .. import profiler
        with profiler.maybe_phase("optimizer"):
            self._apply(self._gscale())
        if global_step is not None:
            gs.increment(global_step)
        return None

    def _gscale(self):
        """The update's gradient multiplier: the reducer's cross-replica scale, over the number
        of accumulated micro-batches (formed in doubles; the kernels take it as fp32)."""
        g = self._reducer.grad_scale()
        return g / self.accumulation_steps if self.accumulation_steps > 1 else g

    @property
    def accumulated(self):
        """Micro-batches currently held in the accumulator: 0 .. accumulation_steps - 1."""
        return self._accumulated

    def reset_accumulation(self):
        """Drop a partial accumulation: the next micro-step is the first of a whole update
        (after a restore or a cluster recovery; checkpoints do not carry the accumulator)."""
        self._accumulated = 0
        self._accum_hold = False

    def get_config(self) -> dict:
        """Serializable description (shipped to parameter-server tasks)."""
        raise NotImplementedError

    def _cfg(self, cfg):
        # only when set: the configurations of unclipped optimizers stay what they were
        if self.clip_norm is not None:
            cfg["clip_norm"] = self.clip_norm
        if self.variable_averages is not None:
            # a description only (the parameter-server tasks refuse it): it does not carry
            # ``num_updates`` and no optimizer is rebuilt from it
            cfg["variable_averages"] = self.variable_averages.get_config()
        if self.accumulation_steps > 1:
            cfg["accumulation_steps"] = self.accumulation_steps
        return cfg

    def minimize(self, loss, global_step=None, var_list=None):
        """backward -> (cross-replica reduce, overlapped) -> fused update -> global_step += 1."""
        if var_list is None:
            var_list = _infer_vars(loss)
        self.compute_gradients(loss, var_list)
        return self.apply_gradients(None, global_step)

    # ------------------------------------------------------------------ update
    def _refresh_hyper(self):
        """Write this step's hyper-parameters into the device buffers the fused kernels read
        (learning rate; Adam's lr_t; LAMB's bias corrections).  Overridden per optimizer; the
        moving average's ``1 - decay`` is written by ``_refresh_ema``, which no override has to
        remember: ``_apply`` calls it for every eager step and the graph replay wrapper before
        every replay."""
        self._lr_dev[0].fill_(self.learning_rate())

    def _refresh_ema(self):
        if self.variable_averages is not None:
            self.variable_averages._refresh(self._ema_bump)

    def _maybe_refresh_hyper(self):
        # inside a graph capture the fill would be recorded with THIS step's constant; the
        # replay wrapper refreshes the buffers before every replay instead
        if not self._capturing:
            self._refresh_hyper()

    # ------------------------------------------------------------------ global-norm clip
    def _build_clip(self):
        if self.clip_norm is None:
            return
        sp = self.space
        self._clip_rec = torch.zeros(2, device=sp.device, dtype=torch.float64)
        f32 = self._clip_rec.view(torch.float32)
        self.last_grad_norm, self._gmul = f32[2:3], f32[3:4]
        if sp.device.type == "cuda":
            from ..ops import native
            K = native.kernels()
            assert K.grad_norm_record_bytes() == 16
            self._clip_chunk = K.grad_norm_chunk()
            # any split of the space into ranges needs at most one short chunk per range more
            self._clip_slab = torch.zeros(sp.numel // self._clip_chunk + 64, device=sp.device,
                                          dtype=torch.float64)

    def _gfactor(self, gscale):
        """What the reference update multiplies g by: ``gscale``, or the record's multiplier."""
        return gscale if self.clip_norm is None else self._gmul[0]

    def _gmul_ptr(self):
        """Device address of the clip multiplier for the fused update kernels (0: use gscale)."""
        return 0 if self.clip_norm is None else self._gmul.data_ptr()

    def _grad_norm_pass(self, gscale, ranges, extra=None):
        """Form the record from S = sum of g^2 over ``ranges`` [(start, end)] plus the fp64
        sums in ``extra`` (other ranks', added in index order): norm = gscale * sqrt(S),
        gmul = gscale * clip / max(norm, clip) in fp64, rounded once to fp32; NaN for a
        non-finite S.  ``_clip_rec[0]`` is S."""
        sp, rec = self.space, self._clip_rec
        if sp.device.type == "cuda":
            from ..ops import native
            K, ch = native.kernels(), self._clip_chunk
            st = torch.cuda.current_stream().cuda_stream
            need = sum(-(-(e - s) // ch) for s, e in ranges)
            if need > self._clip_slab.numel():
                self._clip_slab = torch.zeros(need, device=sp.device, dtype=torch.float64)
            off = 0
            for s, e in ranges:
                K.grad_norm_partial(sp.grad.data_ptr() + 4 * s, e - s,
                                    self._clip_slab.data_ptr() + 8 * off, 0, st)
                off += -(-(e - s) // ch)
            K.grad_norm_finish(self._clip_slab.data_ptr(), off,
                               0 if extra is None else extra.data_ptr(),
                               0 if extra is None else extra.numel(), gscale, self.clip_norm,
                               rec.data_ptr(), st)
            return
        with torch.no_grad():
            S = torch.zeros((), dtype=torch.float64)
            for s, e in ranges:
                S = S + sp.grad[s:e].double().square().sum()
            if extra is not None:
                for x in extra.double():
                    S = S + x
            # the kernels take gscale and clip as fp32
            gs = float(torch.tensor(gscale, dtype=torch.float32))
            c = float(torch.tensor(self.clip_norm, dtype=torch.float32))
            norm = gs * S.sqrt()
            gm = gs * c / torch.clamp(norm, min=c)
            gm = torch.where(torch.isfinite(S), gm, torch.full_like(gm, float("nan")))
            rec[0] = S
            self.last_grad_norm[0] = norm.float()
            self._gmul[0] = gm.float()

    def _apply(self, gscale, rng=None, extra=None):
        """Run the update over the whole flat buffer, or only over ``rng = (start, end)`` (the
        slice a parameter-server shard owns).  With ``clip_norm`` the norm is that of the range
        plus ``extra`` (fp64 sums of squares held elsewhere), unless a reducer has already
        formed this step's record (``_clip_held``)."""
        if self.clip_norm is not None and not self._clip_held:
            self._grad_norm_pass(gscale, [rng if rng is not None else (0, self.space.numel)],
                                 extra)
        if not self._capturing:
            self._refresh_ema()      # on both devices, whatever ``_refresh_hyper`` is overridden to
        self._range = rng
        try:
            if self.space.device.type == "cuda":
                self._apply_native(gscale)
            else:
                self._apply_reference(gscale)
        finally:
            self._range = None
        ema = self.variable_averages
        if ema is not None:
            ema._update(rng)

    def _regions(self):
        regs = self.space.regions()
        rng = getattr(self, "_range", None)
        if rng is None:
            return regs
        lo, hi = rng
        return [(max(s, lo), min(e, hi), d) for s, e, d in regs if min(e, hi) > max(s, lo)]

    def synchronize_variables(self):
        """Wait for communication still writing the variables (a colocated parameter server
        gathers updated shards overlapped with the next forward); call before reading the
        master weights outside a training step (checkpoint, replica check, evaluation)."""
        if self._reducer is not None:
            self._reducer.drain()

    def gather_state(self):
        """Collective: complete every optimizer slot on every rank (a sharded parameter server
        keeps each slot slice only on its owner) -- before a checkpoint of the slots."""
        if self._reducer is not None:
            self._reducer.gather_state(self.state_tensors())

    def nonfinite_flag(self):
        return bool(self._nonfinite.item()) if self._nonfinite is not None else False

    def slot_variables(self):
        """{tf_name: tensor view} for checkpointing (e.g. 'conv2d/kernel/Adam')."""
        out = {}
        for slot in self.slots:
            for v in self.space.order:
                view = self.space.view_of(slot.buf, v)
                splits = getattr(v, "_dtf_splits", None)   # fused variables (e.g. BERT Q|K|V)
                if splits:
                    for name, s, e in splits:
                        out[f"{name}/{slot.name}"] = view[s:e]
                else:
                    out[f"{v._dtf_name}/{slot.name}"] = view
        return out

    def non_slot_variables(self):
        return {}

    def state_tensors(self):
        return [s.buf for s in self.slots]


def _infer_vars(loss):
    """Collect leaf parameters reachable from ``loss`` (TF: trainable_variables of the graph)."""
    seen, out, stack = set(), [], [loss.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if hasattr(fn, "variable"):
            out.append(fn.variable)
        for nxt, _ in fn.next_functions:
            stack.append(nxt)
    out.reverse()
    return out


def tf_adam_lr_t(lr, beta1, beta2, t):
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
