"""HBM-resident token sets with fused on-device masked-LM example creation.

A tokenised pre-training corpus fits the device whole (English Wikipedia + BooksCorpus is about
3.3 G tokens: 6.6 GB as uint16, of 288 GB of HBM3E), so it is uploaded once and every BERT batch
is ONE kernel (``ops.mlm_mask_tokens``): gather, input mask and segment ids, the choice of the
positions to predict and the 80 / 10 / 10 replacement.  That is dynamic masking -- a fresh mask
each time an example is seen -- with no host pipeline and no per-step copy: the only per-step
host work is drawing one 32-bit seed, which reaches the kernel by value.

On disk a set is one array per split in one directory (:func:`load_token_arrays`):

    {split}_tokens.npy   uint16 or int32 [N, S], S <= 512   (memory-mapped, never copied whole)
    meta.json            optional: vocab_size, pad_id, cls_id, sep_id, mask_id
    continuation.npy     optional: uint8 or bool [vocab_size], 1 at the continuation pieces of the
                         vocabulary (``##...``); whole-word masking reads it
                         (:func:`wordpiece_continuation` makes it from a vocab.txt)

A row is one packed example, ``[CLS] a ... [SEP] b ... [SEP] pad ...``; segment ids and the input
mask are derived from it, so nothing else is stored.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .device import DeviceArrayDataset, upload_sharded

META_KEYS = ("vocab_size", "pad_id", "cls_id", "sep_id", "mask_id")


class TokenMasking:
    """The settings of the masking rule (``ops.reference.mlm_mask_tokens``): the vocabulary and
    its special ids (BERT's uncased WordPiece defaults), the masking probability ``prob`` and
    ``random_low``, the smallest id a random replacement may take.  ``prob_q16`` is
    ``round(prob * 65536)``, the form the integer rule uses."""

    def __init__(self, vocab_size=30522, pad_id=0, cls_id=101, sep_id=102, mask_id=103, prob=0.15,
                 random_low=0):
        self.vocab_size, self.random_low = int(vocab_size), int(random_low)
        self.pad_id, self.cls_id, self.sep_id, self.mask_id = (int(pad_id), int(cls_id),
                                                               int(sep_id), int(mask_id))
        self.prob = float(prob)
        if self.vocab_size < 1:
            raise ValueError(f"TokenMasking: vocab_size {vocab_size}")
        for name in ("pad_id", "cls_id", "sep_id", "mask_id", "random_low"):
            if not 0 <= getattr(self, name) < self.vocab_size:
                raise ValueError(f"TokenMasking: {name} {getattr(self, name)} outside the "
                                 f"vocabulary of {self.vocab_size}")
        if not 0.0 <= self.prob <= 1.0:
            raise ValueError(f"TokenMasking: prob {prob} outside [0, 1]")
        self.prob_q16 = int(round(self.prob * 65536))

    def replace(self, **kw):
        """A copy with some settings changed."""
        cur = {k: getattr(self, k) for k in META_KEYS + ("prob", "random_low")}
        cur.update(kw)
        return TokenMasking(**cur)

    def __repr__(self):
        return "TokenMasking({})".format(", ".join(
            f"{k}={getattr(self, k)}" for k in META_KEYS + ("prob", "random_low")))


def load_token_arrays(data_dir, split, masking=None):
    """-> (tokens, masking): ``{split}_tokens.npy`` (uint16 or int32 [N, S], memory-mapped) and
    the :class:`TokenMasking` it is read under -- ``masking`` (default: BERT's) with the settings
    of an optional ``meta.json`` laid over it.  Raises ValueError on a wrong dtype or rank, a
    negative id, an id ``>= vocab_size``, or an unknown meta.json key."""
    masking = masking or TokenMasking()
    mpath = os.path.join(data_dir, "meta.json")
    if os.path.exists(mpath):
        with open(mpath) as f:
            meta = json.load(f)
        unknown = sorted(set(meta) - set(META_KEYS)) if isinstance(meta, dict) else ["<not a map>"]
        if unknown:
            raise ValueError(f"{mpath}: unknown settings {unknown}; expected some of {META_KEYS}")
        masking = masking.replace(**meta)
    path = os.path.join(data_dir, f"{split}_tokens.npy")
    tokens = np.load(path, mmap_mode="r")
    if tokens.dtype not in (np.uint16, np.int32):
        raise ValueError(f"{path}: dtype {tokens.dtype}, expected uint16 or int32")
    if tokens.ndim != 2 or tokens.shape[1] < 1:
        raise ValueError(f"{path}: shape {tokens.shape}, expected [N, S]")
    if tokens.dtype == np.uint16 and masking.vocab_size > 65536:
        raise ValueError(f"{path}: uint16 tokens cannot hold a vocabulary of {masking.vocab_size}")
    step = max(1, (64 << 20) // (tokens.shape[1] * tokens.dtype.itemsize))
    for s in range(0, len(tokens), step):                 # bounded working set over the map
        part = tokens[s:s + step]
        lo, hi = int(part.min()), int(part.max())
        if lo < 0:
            raise ValueError(f"{path}: negative id {lo}")
        if hi >= masking.vocab_size:
            raise ValueError(f"{path}: id {hi} >= vocab_size {masking.vocab_size}")
    return tokens, masking


def wordpiece_continuation(vocab):
    """The whole-word table of a WordPiece vocabulary -> np.uint8 [len(vocab)], 1 where the piece
    starts with ``##``.  ``vocab``: the path of a vocab.txt (one piece per line, line k is id k)
    or a sequence of pieces."""
    if isinstance(vocab, (str, os.PathLike)):
        with open(vocab, encoding="utf-8") as f:
            vocab = [line.rstrip("\r\n") for line in f]
    return np.fromiter((p.startswith("##") for p in vocab), dtype=np.uint8, count=len(vocab))


def check_continuation(table, masking, where="continuation"):
    """-> ``table`` as contiguous np.uint8 [vocab_size]; ValueError unless it is uint8 or bool of
    that shape, holds 0 / 1 only and leaves pad_id, cls_id, sep_id and mask_id unflagged."""
    table = np.asarray(table)
    if table.dtype not in (np.uint8, np.bool_):
        raise ValueError(f"{where}: dtype {table.dtype}, expected uint8 or bool")
    if table.shape != (masking.vocab_size,):
        raise ValueError(f"{where}: shape {table.shape}, expected [{masking.vocab_size}] "
                         "(vocab_size)")
    table = np.ascontiguousarray(table.view(np.uint8))
    if table.max() > 1:
        raise ValueError(f"{where}: a value above 1")
    for name in ("pad_id", "cls_id", "sep_id", "mask_id"):
        if table[getattr(masking, name)]:
            raise ValueError(f"{where}: {name} {getattr(masking, name)} is flagged as a "
                             "continuation piece")
    return table


def load_continuation(data_dir, masking):
    """-> ``DIR/continuation.npy`` as np.uint8 [vocab_size], checked against ``masking`` (the one
    :func:`load_token_arrays` returned).  FileNotFoundError names a missing file."""
    path = os.path.join(data_dir, "continuation.npy")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: no such file (whole-word masking needs the table of "
                                "continuation pieces)")
    return check_continuation(np.load(path), masking, path)


def causal_lm_targets(input_ids, input_mask):
    """Next-token targets of a left-to-right language model -> ``(labels, weights)``, int64 and
    fp32 ``[B, S]``: ``labels[b, j] = input_ids[b, j + 1]`` and ``weights[b, j] =
    float(input_mask[b, j + 1])`` for ``j < S - 1``; the last position has nothing to predict
    (label 0, weight 0.0).  A pure function of its arguments."""
    labels = torch.zeros_like(input_ids, dtype=torch.int64)
    weights = torch.zeros(input_ids.shape, dtype=torch.float32, device=input_ids.device)
    labels[:, :-1] = input_ids[:, 1:]
    weights[:, :-1] = input_mask[:, 1:].to(torch.float32)
    return labels, weights


OBJECTIVES = ("mlm", "causal")


class DeviceTokenDataset(DeviceArrayDataset):
    """A :class:`DeviceArrayDataset` of token rows whose batches are masked-LM examples made on
    the device by one kernel; a batch is the dict :class:`SyntheticMLM` yields plus
    ``masked_lm_weights``.  Example order, epochs, sharding and the shuffle generator are the
    parent's.  ``__next__`` draws one 32-bit seed per batch from a CPU generator of its own
    (``mask_seed``), so an example gets a fresh mask each time it is seen and the same seeds give
    the same batches on the CPU and on the GPU.  ``single_pass()`` uses the fixed ``eval_seed``
    and touches no generator: the rule keys on the GLOBAL example number (``shard_index +
    k * num_shards`` for local row k), so evaluation masks depend on (``eval_seed``, example)
    alone -- not on the batch size, the sharding or how often evaluation runs -- and an evaluation
    between two steps leaves training bit-identical.

    ``tokens``: uint16 or int32 [N, S] (numpy, possibly memory-mapped); 16-bit sets are held as
    their int16 reinterpretation and read unsigned.  Upload: chunked and shard-strided
    (:func:`upload_sharded`).

    ``continuation`` (uint8 or bool [vocab_size], 1 at the ``##`` pieces) turns on whole-word
    masking, for training batches and ``single_pass()`` alike: the table is checked here,
    uploaded once and handed to every call of the kernel.

    ``objective="causal"`` yields left-to-right language-model batches instead: the gathered
    rows (read unsigned) as int64 ``input_ids``, ``input_mask = ids != pad_id``, all-zero
    ``segment_ids``, ``masked_lm_positions = None`` (the model's head then scores every position)
    and ``masked_lm_ids`` / ``masked_lm_weights`` ``[B, S]`` from :func:`causal_lm_targets`.
    Nothing is masked: no masking kernel runs, no seed is drawn (``mask_seed``, ``eval_seed``
    and ``max_predictions`` are unused), ``continuation`` is refused, and ``single_pass()`` is
    the same batches in order.  A batch is a handful of elementwise launches, not a fused
    kernel."""

    def __init__(self, tokens, batch_size, device, masking=None, max_predictions=20,
                 shuffle=False, seed=0, mask_seed=0, eval_seed=0, num_shards=1, shard_index=0,
                 drop_remainder=True, chunk_bytes=256 << 20, continuation=None, objective="mlm"):
        device = torch.device(device)
        masking = masking or TokenMasking()
        if objective not in OBJECTIVES:
            raise ValueError(f"DeviceTokenDataset: objective {objective!r}, expected one of "
                             f"{OBJECTIVES}")
        if objective == "causal" and continuation is not None:
            raise ValueError("DeviceTokenDataset: continuation (whole-word masking) has no "
                             "meaning with objective='causal', which masks nothing")
        self.objective = objective
        if tokens.dtype not in (np.uint16, np.int32) or tokens.ndim != 2:
            raise ValueError("DeviceTokenDataset: tokens must be uint16 or int32 [N, S]")
        if not 0 <= shard_index < num_shards:
            raise ValueError(f"DeviceTokenDataset: shard {shard_index} of {num_shards}")
        if not 0 <= int(eval_seed) < (1 << 32):
            raise ValueError("DeviceTokenDataset: eval_seed must be in [0, 2^32)")
        if continuation is not None:
            continuation = check_continuation(continuation, masking, "DeviceTokenDataset: "
                                              "continuation")
        self.tokens = upload_sharded(tokens, device, num_shards, shard_index, int(chunk_bytes),
                                     view=np.int16 if tokens.dtype == np.uint16 else None)
        self.n = len(self.tokens)
        self.batch_size = batch_size
        self.device = device
        self.masking = masking
        self.max_predictions = int(max_predictions)
        self.num_shards, self.shard_index = int(num_shards), int(shard_index)
        self.shuffle = shuffle
        self.drop_remainder = drop_remainder
        self._gen = torch.Generator(device=device)
        self._gen.manual_seed(seed)
        self._order = None
        self._pos = 0
        self.epoch = 0
        if self.n < batch_size:
            raise ValueError(f"dataset of {self.n} examples < batch size {batch_size}")
        self._mask_gen = torch.Generator(device="cpu")
        self._mask_gen.manual_seed(mask_seed)
        self.eval_seed = int(eval_seed)
        from ..ops.reference import _mlm_check, _mlm_continuation_check
        if objective == "causal":
            # nothing is masked: max_predictions plays no part, only the storage must hold the ids
            if self.tokens.dim() != 2 or self.tokens.shape[1] < 1:
                raise ValueError("DeviceTokenDataset: tokens must be [N, S] with S >= 1")
            if self.tokens.element_size() == 2 and masking.vocab_size > 65536:
                raise ValueError(f"DeviceTokenDataset: vocab_size {masking.vocab_size} does not "
                                 "fit 16-bit token storage")
            self.continuation = None
            return
        rule = _mlm_check(self.tokens, torch.zeros(0, dtype=torch.int64, device=device), 0,
                          self.max_predictions, masking)[3]  # validates S, P and the ids now
        self.continuation = None
        if continuation is not None:
            self.continuation = torch.from_numpy(continuation).to(device)
            _mlm_continuation_check(self.continuation, self.tokens, rule)

    @property
    def seq_len(self):
        return self.tokens.shape[1]

    def single_pass(self, batch_size=None):
        """This shard's examples in order, once, the remainder batch included, masked under
        ``eval_seed``.  Touches neither generator nor the training position."""
        bs = int(batch_size or self.batch_size)
        for pos in range(0, self.n, bs):
            idx = torch.arange(pos, min(pos + bs, self.n), device=self.device)
            yield self._gather(idx, seed=self.eval_seed)

    def _gather_causal(self, idx):
        store = self.tokens
        ids = store.index_select(0, idx).long() & ((1 << (8 * store.element_size())) - 1)
        real = (ids != self.masking.pad_id).long()
        labels, weights = causal_lm_targets(ids, real)
        return {"input_ids": ids, "segment_ids": torch.zeros_like(ids), "input_mask": real,
                "masked_lm_positions": None, "masked_lm_ids": labels,
                "masked_lm_weights": weights}

    def _gather(self, idx, seed=None):
        from .. import ops
        if self.objective == "causal":
            return self._gather_causal(idx)
        if seed is None:                                  # a training batch: a fresh seed
            seed = int(torch.randint(0, 1 << 32, (1,), generator=self._mask_gen,
                                     dtype=torch.int64, device="cpu"))
        return ops.mlm_mask_tokens(self.tokens, idx.contiguous(), seed, self.max_predictions,
                                   self.masking, example_stride=self.num_shards,
                                   example_offset=self.shard_index,
                                   continuation=self.continuation)
