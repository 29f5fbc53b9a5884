"""``tf.train.ExponentialMovingAverage`` of the trainable variables, kept by the optimizer.

TF1 usage is ``ema = tf.train.ExponentialMovingAverage(0.9999, num_updates=global_step)`` and an
``ema.apply(tf.trainable_variables())`` op run after every ``train_op``; evaluation and export
then read the shadow variables ``<var>/ExponentialMovingAverage``.  Here the average is attached
to the optimizer,

    ema = dtf.train.ExponentialMovingAverage(0.9999, num_updates=global_step)
    opt = dtf.train.MomentumOptimizer(0.1, 0.9, variable_averages=ema)

and, because every trainable variable lives in one flat fp32 master buffer, the averages of the
whole model are one more flat buffer (one more optimizer slot) and one elementwise HIP pass per
step, run inside ``Optimizer._apply`` right after the update and over the same range:

    avg = avg - a * (avg - var),     a = 1 - decay_t

``a`` is formed on the host in fp64, rounded once to fp32 and written to the device with the
optimizer's other per-step hyper-parameters, so a captured step replays with each step's own
decay.  With ``num_updates`` the step's decay is ``min(decay, (1 + n) / (10 + n))`` where ``n`` is
the counter as TF's dependency order sees it (after this step's increment): the value read when
the hyper-parameters are refreshed, plus one when ``apply_gradients`` / ``minimize`` was given that
same object as ``global_step``.

Not averaged: BatchNorm moving statistics (they are not trainable variables; this is the
``ema.apply(tf.trainable_variables())`` recipe).  Not built: ``zero_debias``, and averages in the
between-graph parameter-server mode (the PS tasks own the update there and the workers have no
plane to pull averages over).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

EMA_BETWEEN_GRAPH = ("variable_averages is not available in the between-graph parameter-server "
                     "mode: the parameter-server tasks apply the update and the workers have no "
                     "plane to pull the averages over")


class ExponentialMovingAverage:
    def __init__(self, decay, num_updates=None, zero_debias=False,
                 name="ExponentialMovingAverage"):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError(f"decay must be in (0, 1), got {decay}")
        if zero_debias:
            raise ValueError("zero_debias is not supported")
        if num_updates is not None and not hasattr(num_updates, "value"):
            raise ValueError("num_updates must be None or a global-step object "
                             "(dtf.train.get_or_create_global_step())")
        self.decay = decay
        self.num_updates = num_updates
        self.name = name
        self.optimizer = None
        self.buf = None           # flat fp32 [space.numel], laid out as the master buffer
        self.a_dev = None         # [1] fp32 on the device: this step's 1 - decay_t
        self._bf16 = None         # swap(): bf16 cast of buf, allocated on first use
        self._swapped = False

    # ------------------------------------------------------------------ the decay schedule
    def decay_at(self, n=None) -> float:
        """The decay of the step that sees counter value ``n`` (fp64)."""
        if n is None:
            return self.decay
        n = float(n)
        return min(self.decay, (1.0 + n) / (10.0 + n))

    def a_at(self, n=None) -> np.float32:
        """``1 - decay_t``: formed in fp64, rounded once to fp32."""
        return np.float32(1.0 - self.decay_at(n))

    def get_config(self) -> dict:
        """A serializable description for ``Optimizer.get_config()``; it leaves ``num_updates``
        out, so it is not a recipe to rebuild the average from."""
        return {"decay": self.decay, "name": self.name}

    # ------------------------------------------------------------------ optimizer side
    def _attach(self, optimizer):
        if self.optimizer is not None and self.optimizer is not optimizer:
            raise ValueError("this ExponentialMovingAverage is already attached to an optimizer")
        self.optimizer = optimizer

    def _build(self, optimizer):
        """One flat buffer initialised from the (already broadcast) master, carried as one more
        slot after the optimizer's own: checkpoints, ``gather_state`` and the restore broadcast
        then cover it like any slot."""
        from .base import FlatSlot
        sp = optimizer.space
        self.buf = sp.master.detach().clone()
        self.a_dev = optimizer._lr_dev[1:2]
        optimizer.slots = list(optimizer.slots) + [FlatSlot(self.name, self.buf)]

    def _refresh(self, bump):
        n = None
        if self.num_updates is not None:
            n = int(self.num_updates.value()) + (1 if bump else 0)
        self.a_dev.fill_(float(self.a_at(n)))

    def _update(self, rng):
        from .. import ops
        sp = self.optimizer.space
        s, e = rng if rng is not None else (0, sp.numel)
        if e > s:
            ops.ema_update(self.buf[s:e], sp.master.detach()[s:e], self.a_dev)

    def _space(self):
        if self.buf is None:
            raise RuntimeError("the average exists once its optimizer is built "
                               "(variable_averages=..., then build() / minimize())")
        return self.optimizer.space

    # ------------------------------------------------------------------ accessors
    def average(self, var):
        """The fp32 average of ``var`` (a view of the flat buffer)."""
        return self._space().view_of(self.buf, var)

    def average_name(self, var):
        """``<var's name>/ExponentialMovingAverage``.  For a fused variable (BERT's Q|K|V, the
        padded vocabulary) that is the internal name, which no checkpoint holds: see
        :meth:`average_names`."""
        return f"{var._dtf_name}/{self.name}"

    def average_names(self, var):
        """The names ``var``'s average has in checkpoints: one, or one per TF variable that a
        fused variable is split into (``_dtf_splits``)."""
        splits = getattr(var, "_dtf_splits", None)
        if splits:
            return [f"{name}/{self.name}" for name, _, _ in splits]
        return [self.average_name(var)]

    def variables_to_restore(self, model=None):
        """{average name: variable (tensor, layout)}: ``Saver(ema.variables_to_restore(model))
        .restore(path)`` loads the averaged weights into the model's variables.  Fused variables
        map under their TF names and shapes; variables that have no average (BatchNorm moving
        statistics) keep their own names."""
        from ..models.layers import collect_variables
        out = {}
        for name, t, layout in collect_variables(model):
            # a fused variable's TF pieces are row slices (views) of the parameter
            base = t if isinstance(t, torch.nn.Parameter) else getattr(t, "_base", None)
            trainable = isinstance(base, torch.nn.Parameter) and base.requires_grad
            out[f"{name}/{self.name}" if trainable else name] = (t, layout)
        return out

    # ------------------------------------------------------------------ swap
    @contextlib.contextmanager
    def swap(self):
        """Inside, the model computes with the averaged weights: every variable's ``.data`` is a
        view of the average buffer (and, on the GPU, its bf16 compute shadow a view of the cast
        of that buffer).  Nothing is copied into or out of the masters; on exit the very same
        original views are put back.  Collective under a colocated parameter server, whose
        owners each hold only their part of the averages."""
        sp = self._space()
        if self._swapped:
            raise RuntimeError("ExponentialMovingAverage.swap() is already active")
        opt = self.optimizer
        opt.synchronize_variables()
        if opt._reducer is not None:
            opt._reducer.gather_state([self.buf])
        shadowed = sp.shadow is not None
        if shadowed:
            if self._bf16 is None:
                self._bf16 = torch.empty_like(sp.shadow)
            from ..ops import native
            native.kernels().cast_f32_bf16(self.buf.data_ptr(), self._bf16.data_ptr(), sp.numel,
                                           torch.cuda.current_stream().cuda_stream)
        saved = []
        self._swapped = True
        try:
            for v in sp.order:
                saved.append((v, v.data, getattr(v, "_dtf_shadow", None)))
                v.data = sp.view_of(self.buf, v)
                if shadowed:
                    v._dtf_shadow = sp.view_of(self._bf16, v)
            yield self
        finally:
            for v, data, shadow in saved:
                v.data = data
                if shadowed:
                    v._dtf_shadow = shadow
            self._swapped = False


__all__ = ["ExponentialMovingAverage", "EMA_BETWEEN_GRAPH"]
