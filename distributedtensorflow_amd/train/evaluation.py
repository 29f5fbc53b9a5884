"""Distributed evaluation: a sharded loop over a finite set of batches and a session hook that
runs it every N training steps.

    metrics = dtf.metrics.ClassificationMetrics(k=5, strategy=strategy)
    res = dtf.train.evaluate(model, test_set.single_pass(), metrics, optimizer=opt)
    # {"loss": ..., "top_1": ..., "top_k": ..., "count": ...} over every replica's shard

Every replica evaluates its own shard of the set (``DeviceArrayDataset(num_shards, shard_index)
.single_pass()`` sees every example exactly once across the replicas) and the four-number metric
state is summed over the replicas when the result is read -- so under a collective strategy
:func:`evaluate` is a collective call: every rank enters it, with as many or as few batches as its
shard holds.

An evaluation between two training steps leaves training untouched: it runs under ``no_grad`` in
``eval()`` mode (parameters, optimizer slots and BatchNorm moving statistics are only read), on
an iterator of its own, with the native ops' deferred-work records of its forward passes kept
apart from the training step's registry (``ops.records.isolated``) and released batch by batch.
"""
from __future__ import annotations

import torch

from ..ops import records
from .hooks import SessionRunHook, _gstep


def default_forward(model, batch):
    """-> (logits, labels, weights) of one batch: ``(x, y)`` batches (the CNN / MLP / ResNet
    models), or BERT's masked-LM dict batches (the model called without ``masked_lm_ids``
    returns the logits of the masked positions, a row-strided view of the padded-vocabulary
    decoder output; ``masked_lm_weights`` are optional)."""
    if isinstance(batch, dict):
        logits = model(batch["input_ids"], batch.get("segment_ids"), batch.get("input_mask"),
                       batch["masked_lm_positions"])
        return logits, batch["masked_lm_ids"], batch.get("masked_lm_weights")
    x, y = batch
    return model(x), y, None


def evaluate(model, batches, metrics, optimizer=None, strategy=None, forward=None,
             averages=None):
    """Run every batch of the finite iterable ``batches`` through ``model`` in evaluation mode,
    add it to ``metrics`` and return ``metrics.result()`` (collective under a collective
    strategy).  ``optimizer``: its pending variable communication is waited for first (a
    colocated parameter server may still be gathering updated shards).  ``forward(model, batch)
    -> (logits, labels, weights)`` replaces :func:`default_forward`.  The model's previous
    train / eval mode is restored whatever happens.  ``averages``: an
    ``ExponentialMovingAverage`` attached to the optimizer; the loop then runs inside its
    ``swap()``, on the averaged weights (collective under a colocated parameter server)."""
    if averages is not None:
        inner = getattr(optimizer, "_opt", optimizer)       # a SyncReplicasOptimizer's
        if inner is not None and averages.optimizer is not inner:
            raise ValueError("evaluate: averages= is not attached to this optimizer")
        space = getattr(averages.optimizer, "space", None)
        if space is None or {id(p) for p in model.parameters() if p.requires_grad} != \
                {id(v) for v in space.order}:
            raise ValueError("evaluate: averages= does not hold this model's variables")
        with averages.swap():
            return evaluate(model, batches, metrics, optimizer, strategy, forward)
    forward = forward or default_forward
    if optimizer is not None and getattr(optimizer, "space", None) is not None:
        optimizer.synchronize_variables()
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), records.isolated():
            for batch in batches:
                logits, labels, weights = forward(model, batch)
                metrics.update(logits, labels, weights)
                del logits
                records.end_step()
    finally:
        model.train(was_training)
    return metrics.result(strategy)


class EvalHook(SessionRunHook):
    """Evaluate every ``every_n_steps`` global steps.  ``eval_fn() -> dict`` (typically a closure
    over :func:`evaluate` with a fresh single-pass iterator and reset metrics) runs on EVERY
    replica at the same global step, because reading the result is collective; the chief writes
    ``eval/loss``, ``eval/top_1`` and ``eval/top_k`` (and ``eval/ema_loss``, ``eval/ema_top_1``,
    ``eval/ema_top_k`` where the result carries the averaged weights' figures) at that step to ``summary_writer`` (an
    ``EventFileWriter`` or a logger ``KVWriter`` such as ``TensorBoardOutputFormat``), else to the
    session's summary writer."""

    def __init__(self, eval_fn, every_n_steps, summary_writer=None):
        if not every_n_steps or int(every_n_steps) < 1:
            raise ValueError("EvalHook: every_n_steps must be a positive step count")
        self.eval_fn = eval_fn
        self.every = int(every_n_steps)
        self.writer = summary_writer
        self.last_step = None
        self.results = []            # [(global step, result dict)] on every replica

    def after_create_session(self, session, coord=None):
        self.last_step = _gstep(session)

    def after_run(self, run_context, run_values):
        session = run_context.session
        step = _gstep(session)
        # a step-count trigger: synchronous replicas share the global step, so they all fire
        if self.last_step is None:
            self.last_step = 0
        if step < self.last_step + self.every:
            return
        self.last_step = step
        res = self.eval_fn()
        self.results.append((step, res))
        if not getattr(session, "is_chief", True):
            return
        vals = {f"eval/{k}": res[k] for k in ("loss", "top_1", "top_k", "ema_loss", "ema_top_1",
                                              "ema_top_k") if k in res}
        w = self.writer if self.writer is not None else getattr(session, "summary_writer", None)
        if w is None:
            return
        if hasattr(w, "add_scalars"):
            w.add_scalars(vals, step)
        else:
            w.writekvs(vals, step)


__all__ = ["evaluate", "default_forward", "EvalHook"]
