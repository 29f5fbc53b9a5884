"""Streaming evaluation metrics (``dtf.metrics``): loss, top-1 and top-k accuracy accumulated on
the device, reduced over the replicas of a strategy only when the result is read.

    m = dtf.metrics.ClassificationMetrics(k=5, strategy=strategy)
    for x, y in batches:
        m.update(model(x), y)            # device work only: no .item(), no .cpu(), no sync
    m.result()                           # {"loss", "top_1", "top_k", "count"}; collective

The state is four fp64 numbers ``[sum w, sum w loss, sum w [rank < 1], sum w [rank < k]]`` with
``rank`` the stable descending rank of the label (:func:`distributedtensorflow_amd.ops.eval_rows`:
among tied logits the lower index ranks first, so top-1 is ``argmax == label``; stricter than
TF's ``in_top_k``).  On the GPU a batch is two kernel launches (``eval_rows`` reads the logits
once, ``metrics_accumulate`` adds the batch in a fixed order without atomics: two runs give a
bit-identical state); on CPU tensors the same class runs on the reference op and torch fp64.
"""
from __future__ import annotations

import torch

from .. import ops


class EmptyMetricsError(RuntimeError):
    """``result()`` of a metric that has seen no example of non-zero weight."""


class ClassificationMetrics:
    def __init__(self, k=5, strategy=None):
        if int(k) < 1:
            raise ValueError("ClassificationMetrics: k must be at least 1")
        self.k = int(k)
        self.strategy = strategy
        self._state = None

    @property
    def state(self):
        """The device-resident fp64 state (None before the first update)."""
        return self._state

    def update(self, logits, labels, weights=None):
        """Add a batch.  ``logits`` [..., V] (rows may be strided), integer ``labels`` (a label
        outside ``[0, V)`` marks an ignored row), optional per-row ``weights`` (BERT's
        ``masked_lm_weights``; weight 0 drops the row)."""
        with torch.no_grad():
            if logits.dim() != 2:
                logits = logits.reshape(-1, logits.shape[-1])
            if self._state is None:
                self._state = torch.zeros(4, dtype=torch.float64, device=logits.device)
            elif self._state.device != logits.device:
                raise ValueError(f"metrics state on {self._state.device}, batch on {logits.device}")
            rows, rank = ops.eval_rows(logits, labels)
            if weights is not None:
                weights = weights.reshape(-1)
                if weights.numel() != rank.numel():
                    raise ValueError(f"{weights.numel()} weights for {rank.numel()} rows")
            if ops._use_native(logits):
                ops._native().metrics_accumulate(self._state, rows, rank, weights, self.k)
            else:
                w = (rank >= 0).double()
                if weights is not None:
                    w = w * weights.to(w.device).double()
                keep = w != 0
                loss = torch.where(keep, rows.double(), torch.zeros_like(w))
                self._state += torch.stack([w.sum(), (w * loss).sum(), (w * (rank < 1)).sum(),
                                            (w * (rank < self.k)).sum()])
        return self

    def result(self, strategy=None):
        """{"loss", "top_1", "top_k", "count"} as Python floats.  Under a collective strategy
        this is a collective call (one SUM all-reduce of the four fp64 values): every replica
        must enter it.  The only place the host reads the state."""
        strategy = strategy if strategy is not None else self.strategy
        collective = strategy is not None and bool(getattr(strategy, "collective", False))
        if self._state is None:
            if not collective:
                raise EmptyMetricsError("metrics result() before any update()")
            total = torch.zeros(4, dtype=torch.float64, device=strategy.device)
        else:
            total = self._state.clone()
        if collective:
            strategy.all_reduce_(total)
        count, loss, top1, topk = total.tolist()
        if count == 0:
            raise EmptyMetricsError("metrics result() over zero examples (every row ignored or "
                                    "of weight 0)")
        return {"loss": loss / count, "top_1": top1 / count, "top_k": topk / count,
                "count": count}

    def reset(self):
        if self._state is not None:
            self._state.zero_()
        return self


__all__ = ["ClassificationMetrics", "EmptyMetricsError"]
