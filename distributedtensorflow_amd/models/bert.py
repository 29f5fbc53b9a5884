"""BERT (google-research/bert ``modeling.py`` architecture) for masked-LM pre-training.

North-star BASELINE.json config 5 ("BERT-base MLM MultiWorkerMirroredStrategy, MFMA GEMM path +
fused LAMB"); the reference itself has no sequence models, so semantics and
variable names follow google-research/bert so TF checkpoints line up:
``bert/embeddings/word_embeddings``, ``bert/encoder/layer_0/attention/self/query/kernel``,
``cls/predictions/transform/dense/kernel``, ``cls/predictions/output_bias`` ...

MI355X layout choices:
  * activations are token-major bf16 ``[B*S, 768]`` matrices end to end (no [B,H,S,D]
    transposes): Q/K/V come from ONE fused ``768 -> 2304`` GEMM whose output the MFMA attention
    kernel reads in place; its fp32 master ``[2304, 768]`` is exported to checkpoints as the
    three TF variables ``query|key|value`` (row slices, ``_dtf_splits``);
  * every GEMM runs on our persistent MFMA GEMM (csrc/kernels/gemm.hip gemm_pp2) and every
    weight gradient on our TN weight-gradient kernel, and everything around them is fused into
    our kernels: bias+GELU, bias+dropout+residual+LayerNorm, embedding gather+sum+LN+dropout,
    flash attention with in-kernel dropout, weighted MLM cross-entropy;
  * the MLM decoder is tied to the word embeddings (one fp32 master whose bf16 shadow feeds both
    the gather and the logits GEMM).  Its vocabulary is padded to a multiple of 64 (30522 ->
    30528 rows) so the decoder's forward, data gradient and weight gradient fit our GEMM tiles:
    the padding rows of the table and of the output bias are zero, never gathered, get an exact
    zero gradient (the loss leaves their logits out of the softmax), so training is exactly the
    unpadded model; checkpoints and SavedModels carry the TF shapes ``[30522, 768]`` /
    ``[30522]`` (row slices, ``_dtf_splits``).
"""
from __future__ import annotations

import dataclasses
import os

import torch
import torch.nn as nn

from .. import ops
from .layers import Layer, _tag, truncated_normal_


# BERT's dense layers take ops.dense(impl="library"): the bias rides in the GEMM epilogue or in
# the fused consumer kernel, and the GEMMs run on our persistent MFMA GEMM (ops/native.py _Dense;
# hipBLASLt only for shapes outside its tiles, none in BERT-base).  "native" selects the
# tf.layers.dense form (bias + ReLU epilogue, separate bias-gradient pass) instead.
BERT_GEMM = os.environ.get("DTF_BERT_GEMM", "library")
# the tied decoder's vocabulary rows are padded to a multiple of this (GEMM tile / 16-B rows)
VOCAB_ALIGN = 64


def padded_vocab(v: int) -> int:
    return -(-v // VOCAB_ALIGN) * VOCAB_ALIGN
# FFN: bias + GELU + second GEMM as one op whose data gradient carries the GELU derivative in our
# GEMM's epilogue (A/B knob)
FUSE_GELU_DGRAD = os.environ.get("DTF_BERT_FUSE_GELU_DGRAD", "1") == "1"
# the skinny-M weight-streaming kernel (ops.dense(impl="skinny")) serves up to this many rows; a
# decode or extend call with more keeps the default GEMMs even under gemm="skinny"
SKINNY_MAX_ROWS = 64
# ... and a GEMM wider than SKINNY_WIDE outputs only up to this many rows.  Measured
# (tools/dense_bench.py, profiles/SKINNY.md): the 30528 x 768 vocabulary GEMM takes 21.1 us
# against 22.2 at 32 rows, but 22.0 against 21.7 at 33, 26.0 against 20.9 at 48 and 31.3 against
# 21.5 at 64 (every further row tile re-reads x from L2 for each of the 1908 column tiles); the
# layer GEMMs, up to 3072 wide, win at all of 1 to 64 rows.  Widths in between: not measured.
SKINNY_MAX_ROWS_WIDE = 32
SKINNY_WIDE = 3072


_SKINNY_GEMMS = ("skinny", "skinny_ln", "skinny_w8", "skinny_ln_w8")


def _skinny(gemm, rows, width=0):
    """The route of a GEMM with ``width`` outputs in a decode / extend call over ``rows`` rows
    -> (impl, w8): impl is "skinny", or "skinny_ln" (the skinny kernel with the layers' LayerNorms
    deferred into it), when ``gemm`` asks for it and the rows fit, else None (today's path on the
    bf16 shadow); w8: ``gemm`` is "skinny_w8" / "skinny_ln_w8" and the GEMM takes the FP8 pair of
    :meth:`BertForPreTraining.quantize_weights` in place of the shadow.  The SKINNY_MAX_ROWS_WIDE
    rule holds for the pairs too (21.1 us at 32 rows, 20.6 at 33 against the default route's 20.4
    to 20.8: no clearer a crossing than for bf16, profiles/SKINNY_W8.md).
    Decided on the host from the shapes."""
    if gemm not in (None, "default") + _SKINNY_GEMMS:
        raise ValueError(f"gemm must be None, 'default' or one of {_SKINNY_GEMMS}, got {gemm!r}")
    most = SKINNY_MAX_ROWS_WIDE if width > SKINNY_WIDE else SKINNY_MAX_ROWS
    if gemm not in _SKINNY_GEMMS or rows > most:
        return None, False
    w8 = gemm.endswith("_w8")
    return (gemm[:-3] if w8 else gemm), w8


def _wt(p, w8):
    """The weight a GEMM takes: the parameter (its bf16 shadow), or its FP8 pair."""
    return p._dtf_w8 if w8 else p


# Under gemm="skinny_ln" the hidden state between layers is a pair (t, ln): ln = (gamma, beta,
# eps) of the LayerNorm that t still lacks, None when t is already normalised.
def _deferred(x):
    return x if isinstance(x, tuple) else (x, None)


def _normalised(x):
    """The tensor a pair stands for (one LayerNorm launch), for a consumer off the skinny path."""
    if not isinstance(x, tuple):
        return x
    return x[0] if x[1] is None else ops.layer_norm(x[0], *x[1])


@dataclasses.dataclass
class BertConfig:
    vocab_size: int = 30522
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    hidden_act: str = "gelu"
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    initializer_range: float = 0.02
    layer_norm_eps: float = 1e-12
    # left-to-right attention (query i sees key j iff j <= i) in every layer: the same post-LN
    # blocks, variables, padded vocabulary and head as a causal language model (GPT-1's block).
    # Called with masked_lm_positions=None, so the head scores every position.
    causal: bool = False

    @staticmethod
    def base(**kw):
        return BertConfig(**kw)

    @staticmethod
    def large(**kw):
        d = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                 intermediate_size=4096)
        d.update(kw)
        return BertConfig(**d)


def _param(shape, name, std=None, layout=None, fill=None):
    p = nn.Parameter(torch.empty(*shape))
    if fill is not None:
        p.data.fill_(fill)
    else:
        truncated_normal_(p.data, std)
    return _tag(p, name, layout)


class _Dense(nn.Module):
    """y = x @ W^T (hipBLASLt) with the bias applied by the fused consumer kernel."""

    def __init__(self, n_in, n_out, name, std):
        super().__init__()
        self.kernel = _param((n_out, n_in), f"{name}/kernel", std, "OI")
        self.bias = _param((n_out,), f"{name}/bias", fill=0.0)

    def gemm(self, x, impl=None, w8=False):
        return ops.dense(x, _wt(self.kernel, w8), None, impl=impl or BERT_GEMM)


class _LayerNorm(nn.Module):
    def __init__(self, n, name):
        super().__init__()
        self.gamma = _param((n,), f"{name}/gamma", fill=1.0)
        self.beta = _param((n,), f"{name}/beta", fill=0.0)


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig, idx: int):
        super().__init__()
        H, std = cfg.hidden_size, cfg.initializer_range
        pre = f"bert/encoder/layer_{idx}"
        self.cfg = cfg
        # fused Q|K|V projection; checkpoint names split back into query / key / value
        self.qkv_kernel = _param((3 * H, H), f"{pre}/attention/self/qkv/kernel", std, "OI")
        self.qkv_kernel._dtf_splits = [
            (f"{pre}/attention/self/{n}/kernel", i * H, (i + 1) * H) for i, n in
            enumerate(("query", "key", "value"))]
        self.qkv_bias = _param((3 * H,), f"{pre}/attention/self/qkv/bias", fill=0.0)
        self.qkv_bias._dtf_splits = [
            (f"{pre}/attention/self/{n}/bias", i * H, (i + 1) * H) for i, n in
            enumerate(("query", "key", "value"))]
        self.attn_out = _Dense(H, H, f"{pre}/attention/output/dense", std)
        self.attn_ln = _LayerNorm(H, f"{pre}/attention/output/LayerNorm")
        self.inter = _Dense(H, cfg.intermediate_size, f"{pre}/intermediate/dense", std)
        self.out = _Dense(cfg.intermediate_size, H, f"{pre}/output/dense", std)
        self.out_ln = _LayerNorm(H, f"{pre}/output/LayerNorm")

    def forward(self, x, mask, B, S, cache=None):
        """``cache``: a ``(k, v)`` pair of [B, heads, C, 64] tensors that receives this layer's
        keys and values of positions 0 .. S-1 (the prefill of incremental decoding); an FP8
        cache's ``(k, v, k_scale, v_scale)``."""
        cfg = self.cfg
        qkv = ops.dense(x, self.qkv_kernel, self.qkv_bias, impl=BERT_GEMM)
        if cache is not None:
            ops.kv_cache_fill(qkv, cache[0], cache[1], B, S, cfg.num_attention_heads, *cache[2:])
        ctx = ops.attention_qkv(qkv, mask, B, S, cfg.num_attention_heads,
                                cfg.attention_probs_dropout_prob, self.training,
                                causal=cfg.causal)
        return self._after_attention(x, ctx)

    def decode(self, x, k_cache, v_cache, pos, max_len=None, k_scale=None, v_scale=None,
               gemm=None):
        """One new token per sequence (x [B, H]) at positions ``pos`` against this layer's cache,
        which takes the token's key and value in place (``k_scale`` / ``v_scale``: an FP8 cache's
        row scales).  ``gemm="skinny"``: the QKV and output projections and the FFN run on the
        weight-streaming kernel when B <= 64.  ``gemm="skinny_ln"``: also the two LayerNorms, deferred
        into those GEMMs (five launches); x may then be a ``(t, ln)`` pair and the result is one."""
        impl, w8 = _skinny(gemm, _deferred(x)[0].shape[0])
        qkv, x = self._qkv(x, impl, w8)
        ctx = ops.attention_decode(qkv, k_cache, v_cache, pos, self.cfg.num_attention_heads,
                                   max_len=max_len, k_scale=k_scale, v_scale=v_scale)
        return self._after_attention(x, ctx, impl, w8)

    def extend(self, x, k_cache, v_cache, pos, n_new, T, max_len=None, k_scale=None,
               v_scale=None, gemm=None):
        """T new tokens per sequence (x [B*T, H]), the first ``n_new[b]`` of them real, at
        positions ``pos[b] ..`` against this layer's cache, which takes their keys and values in
        place (``ops.attention_append``).  ``gemm="skinny"`` / ``"skinny_ln"``: as :meth:`decode`,
        when B*T <= 64."""
        impl, w8 = _skinny(gemm, _deferred(x)[0].shape[0])
        qkv, x = self._qkv(x, impl, w8)
        ctx = ops.attention_append(qkv, k_cache, v_cache, pos, self.cfg.num_attention_heads,
                                   n_new=n_new, max_len=max_len, k_scale=k_scale,
                                   v_scale=v_scale)
        return self._after_attention(x, ctx, impl, w8)

    def _qkv(self, x, impl, w8=False):
        """The QKV projection of a decode / extend call -> (qkv, x as the rest of the layer takes
        it: the ``(t, ln)`` pair under "skinny_ln", whose LayerNorm the GEMM applies on load)."""
        if impl == "skinny_ln":
            t, ln = x = _deferred(x)
            return ops.dense(t, _wt(self.qkv_kernel, w8), self.qkv_bias, impl="skinny",
                             pre_ln=ln), x
        x = _normalised(x)
        return ops.dense(x, _wt(self.qkv_kernel, w8), self.qkv_bias, impl=impl or BERT_GEMM), x

    def _after_attention_ln(self, t, ln, ctx, w8=False):
        """The rest of the layer with both LayerNorms deferred: the output projection stores
        t1 = ctx W^T + b + LN(t) and the FFN pair t2 = ffn(LN(t1)) + b + LN(t1), un-normalised; a
        decode / extend step has no dropout.  -> (t2, its LayerNorm)."""
        eps = self.cfg.layer_norm_eps
        t1 = ops.dense(ctx, _wt(self.attn_out.kernel, w8), self.attn_out.bias, impl="skinny",
                       residual=t, residual_ln=ln)
        ln1 = (self.attn_ln.gamma, self.attn_ln.beta, eps)
        t2 = ops.dense_gelu_dense(t1, _wt(self.inter.kernel, w8), self.inter.bias,
                                  _wt(self.out.kernel, w8), impl="skinny", pre_ln=ln1,
                                  b2=self.out.bias, residual=t1, residual_ln=ln1)
        return t2, (self.out_ln.gamma, self.out_ln.beta, eps)

    def _after_attention(self, x, ctx, impl=None, w8=False):
        if impl == "skinny_ln":
            return self._after_attention_ln(*x, ctx, w8)
        cfg = self.cfg
        a = self.attn_out.gemm(ctx, impl, w8)
        # x feeds the QKV dense above and the residual here: its two gradients are summed by
        # that dense's dgrad GEMM (beta = 1), not by a separate add
        x = ops.bias_dropout_add_layer_norm(a, self.attn_out.bias, x, self.attn_ln.gamma,
                                            self.attn_ln.beta, cfg.hidden_dropout_prob,
                                            self.training, cfg.layer_norm_eps,
                                            residual_to_dense=True)
        if impl == "skinny":
            # a decode step's FFN: two launches of the skinny-M kernel, bias + GELU in the first
            o = ops.dense_gelu_dense(x, _wt(self.inter.kernel, w8), self.inter.bias,
                                     _wt(self.out.kernel, w8), impl=impl)
        elif FUSE_GELU_DGRAD and BERT_GEMM == "library":
            # the whole FFN as one op: the first GEMM applies bias + GELU in its epilogue (our
            # MFMA GEMM); the backward forms d(pre-activation) in one GEMM pass with the GELU
            # derivative in the epilogue (ops.native.dense_gelu_dense / _BiasGeluDense)
            o = ops.dense_gelu_dense(x, self.inter.kernel, self.inter.bias, self.out.kernel)
        else:
            h = ops.bias_gelu(self.inter.gemm(x), self.inter.bias)
            o = self.out.gemm(h)
        return ops.bias_dropout_add_layer_norm(o, self.out.bias, x, self.out_ln.gamma,
                                               self.out_ln.beta, cfg.hidden_dropout_prob,
                                               self.training, cfg.layer_norm_eps,
                                               residual_to_dense=True)


class BertForPreTraining(Layer):
    """BERT encoder + masked-LM head (the NSP head of the original is omitted: config 5 is MLM)."""

    def __init__(self, cfg: BertConfig | None = None):
        super().__init__()
        cfg = cfg or BertConfig()
        self.cfg = cfg
        H, std = cfg.hidden_size, cfg.initializer_range
        if H % cfg.num_attention_heads or H // cfg.num_attention_heads != 64:
            raise ValueError("attention kernels are built for head_dim 64")
        V, Vp = cfg.vocab_size, padded_vocab(cfg.vocab_size)
        self.word_embeddings = _param((Vp, H), "bert/embeddings/word_embeddings", std)
        self.token_type_embeddings = _param((cfg.type_vocab_size, H),
                                            "bert/embeddings/token_type_embeddings", std)
        self.position_embeddings = _param((cfg.max_position_embeddings, H),
                                          "bert/embeddings/position_embeddings", std)
        self.emb_ln = _LayerNorm(H, "bert/embeddings/LayerNorm")
        self.layers = nn.ModuleList(BertLayer(cfg, i) for i in range(cfg.num_hidden_layers))
        self.mlm_transform = _Dense(H, H, "cls/predictions/transform/dense", std)
        self.mlm_ln = _LayerNorm(H, "cls/predictions/transform/LayerNorm")
        self.mlm_bias = _param((Vp,), "cls/predictions/output_bias", fill=0.0)
        if Vp != V:
            with torch.no_grad():
                self.word_embeddings[V:].zero_()
            # checkpoints / SavedModels carry the TF shapes (the first V rows)
            self.word_embeddings._dtf_splits = [("bert/embeddings/word_embeddings", 0, V)]
            self.mlm_bias._dtf_splits = [("cls/predictions/output_bias", 0, V)]

    def num_params_tf(self) -> int:
        """Parameters of the TF model (the padding rows of the tied vocabulary excluded)."""
        return sum(t.numel() for _, t, _ in self.variables_tf())

    def variables_tf(self):
        for p in self.parameters():
            if hasattr(p, "_dtf_name"):
                splits = getattr(p, "_dtf_splits", None)
                if splits:
                    for name, s, e in splits:
                        yield name, p[s:e], p._dtf_layout
                else:
                    yield p._dtf_name, p, p._dtf_layout

    def encode(self, input_ids, token_type_ids=None, attention_mask=None, cache=None):
        """-> ([B*S, H] final hidden states, additive key mask).  ``cache``: a :class:`KVCache`
        that every layer fills with its keys and values."""
        cfg = self.cfg
        B, S = input_ids.shape
        dtype = torch.bfloat16 if input_ids.is_cuda else torch.float32
        x = ops.embedding_layer_norm(input_ids, token_type_ids, self.word_embeddings,
                                     self.position_embeddings, self.token_type_embeddings,
                                     self.emb_ln.gamma, self.emb_ln.beta, cfg.hidden_dropout_prob,
                                     self.training, cfg.layer_norm_eps, dtype=dtype)
        mask = None
        if attention_mask is not None:
            mask = (1.0 - attention_mask.float()) * -10000.0
        for i, layer in enumerate(self.layers):
            if cache is None:
                x = layer(x, mask, B, S)
            else:
                x = layer(x, mask, B, S, cache=cache.layer(i))
        return x, mask

    def forward(self, input_ids, token_type_ids=None, attention_mask=None,
                masked_lm_positions=None, masked_lm_ids=None, masked_lm_weights=None):
        """Returns the MLM loss (sum(w * nll) / sum(w)) when labels are given, else logits of the
        masked positions ``[B*P, vocab]``."""
        cfg = self.cfg
        B, S = input_ids.shape
        x, _ = self.encode(input_ids, token_type_ids, attention_mask)
        if masked_lm_positions is None:
            masked_lm_positions = torch.arange(S, device=x.device).expand(B, S)
        flat = (masked_lm_positions + torch.arange(B, device=x.device).unsqueeze(1) * S).reshape(-1)
        h = x.index_select(0, flat)                                      # [B*P, H] gather
        logits = self._head(h)
        V = cfg.vocab_size
        if masked_lm_ids is None:
            return logits if logits.shape[-1] == V else logits[:, :V]
        return ops.mlm_loss(logits, masked_lm_ids, masked_lm_weights, vocab=V)

    def _head(self, h, gemm=None):
        """Hidden rows [N, H] -> logits over the padded vocabulary [N, Vp] (the padding logits
        are exactly 0).  ``gemm="skinny"``: the transform and vocabulary GEMMs on the
        weight-streaming kernel when N <= 64 (the vocabulary GEMM: N <= 32, see
        SKINNY_MAX_ROWS_WIDE).  ``gemm="skinny_ln"``: h may be a ``(t, ln)`` pair, whose LayerNorm
        the transform GEMM then applies on load; the vocabulary GEMM is the "skinny" one (its 1908
        blocks would each recompute the statistics)."""
        impl, w8 = _skinny(gemm, _deferred(h)[0].shape[0])
        if impl == "skinny_ln":
            t, ln = _deferred(h)
            h = ops.dense(t, _wt(self.mlm_transform.kernel, w8), None, impl="skinny", pre_ln=ln)
        else:
            h = self.mlm_transform.gemm(_normalised(h), impl, w8)
        h = ops.bias_gelu(h, self.mlm_transform.bias)
        h = ops.bias_dropout_add_layer_norm(h, None, None, self.mlm_ln.gamma, self.mlm_ln.beta,
                                            0.0, self.training, self.cfg.layer_norm_eps)
        impl, w8 = _skinny(gemm, h.shape[0], self.word_embeddings.shape[0])
        return ops.dense(h, _wt(self.word_embeddings, w8), self.mlm_bias,
                         impl="skinny" if impl else BERT_GEMM)

    # ------------------------------------------------------------------------- generation
    def _w8_params(self):
        """The matrices the decode path's GEMMs read: every layer's four, the head's transform
        and the tied vocabulary projection."""
        for layer in self.layers:
            yield from (layer.qkv_kernel, layer.attn_out.kernel, layer.inter.kernel,
                        layer.out.kernel)
        yield from (self.mlm_transform.kernel, self.word_embeddings)

    @torch.no_grad()
    def quantize_weights(self):
        """Build the FP8 pairs (``ops.weight_quantize_fp8``) of the decode path's matrices from
        their current values, for ``gemm="skinny_w8"`` / ``"skinny_ln_w8"``.  They are kept on the
        parameters next to the fp32 masters, which the embedding lookup and every other path
        keep using; call it again after the weights change or move."""
        for p in self._w8_params():
            p._dtf_w8 = ops.weight_quantize_fp8(p)
        return self

    def _check_w8(self, gemm):
        if gemm in ("skinny_w8", "skinny_ln_w8") and any(
                getattr(p, "_dtf_w8", None) is None for p in self._w8_params()):
            raise ValueError(f"gemm={gemm!r} needs the FP8 weights: call quantize_weights() first")

    def _check_prompts(self, input_ids, prompt_lens):
        if not self.cfg.causal:
            raise ValueError("incremental decoding needs a causal model (BertConfig(causal=True))")
        B, Sp = input_ids.shape
        lens = torch.as_tensor(prompt_lens).reshape(-1).cpu()
        if lens.numel() != B or int(lens.min()) < 1 or int(lens.max()) > Sp:
            raise ValueError(f"prompt_lens must hold {B} lengths in [1, {Sp}]")
        return lens

    @torch.no_grad()
    def prefill(self, input_ids, prompt_lens, cache, _padded=False, chunk=None, gemm=None):
        """The causal forward over the right-padded prompts [B, Sp] (``prompt_lens``: CPU lengths
        in [1, Sp]): fills every layer of ``cache``, sets ``cache.pos = prompt_lens`` and returns
        the logits of each row's last real position, [B, vocab_size].

        ``chunk=T``: the prompt goes through :meth:`extend` in ``ceil(Sp / T)`` pieces from an
        empty cache instead, piece c with ``n_new = clamp(prompt_lens - c T, 0, T)``: activation
        memory is that of T tokens per row and Sp needs no padding to a multiple of 64.  ``gemm``
        goes to those :meth:`extend` calls; the one-shot forward does not take it."""
        lens = self._check_prompts(input_ids, prompt_lens)
        B, Sp = input_ids.shape
        if B != cache.batch or Sp > cache.capacity:
            raise ValueError(f"cache is for batch {cache.batch}, capacity {cache.capacity}")
        if chunk is not None:
            self._check_w8(gemm)
            T = int(chunk)
            if T < 1:
                raise ValueError("chunk must be at least 1")
            cache.reset()
            piece_of = ((lens - 1) // T).to(input_ids.device).view(B, 1)
            logits = None
            for c in range(-(-Sp // T)):
                part = self.extend(input_ids[:, c * T:(c + 1) * T].contiguous(), cache,
                                   (lens - c * T).clamp(0, min(T, Sp - c * T)), _padded=_padded,
                                   gemm=gemm)
                logits = part if logits is None else torch.where(piece_of == c, part, logits)
            return logits
        dev = input_ids.device
        lens_d = lens.to(dev)
        am = (torch.arange(Sp, device=dev).unsqueeze(0) < lens_d.unsqueeze(1)).long()
        x, _ = self.encode(input_ids, None, am, cache=cache)
        cache.pos.copy_(lens_d)
        cache.max_len = int(lens.max())
        last = torch.arange(B, device=dev) * Sp + lens_d.long() - 1
        logits = self._head(x.index_select(0, last))
        return logits if _padded else logits[:, :self.cfg.vocab_size]

    @torch.no_grad()
    def decode_step(self, ids_new, cache, _padded=False, gemm=None):
        """One token per sequence (``ids_new`` [B]) at positions ``cache.pos``: every layer runs
        at B rows with ``ops.attention_decode`` against its cache, ``cache.pos`` advances by one
        on the device.  -> logits [B, vocab_size].  Nothing here reads the device.

        ``gemm="skinny"``: every GEMM of the step (four per layer and the head's two) runs on the
        weight-streaming kernel of ``ops.dense(impl="skinny")`` when B <= 64; None or "default"
        and larger batches keep the persistent GEMM.  ``gemm="skinny_ln"``: the same GEMMs with
        every layer's two LayerNorms deferred into them (``ops.dense(pre_ln=, residual_ln=)``): five
        launches a layer instead of seven, the last layer's LayerNorm applied by the head's
        transform GEMM; the same row limits.  ``"skinny_w8"`` / ``"skinny_ln_w8"``: those two
        with the FP8 weight pairs of :meth:`quantize_weights` (a ValueError before it was called)
        in place of the bf16 shadows: half the weight bytes a step streams, and the step computes
        with exactly the dequantised matrices."""
        cfg = self.cfg
        if not cfg.causal:
            raise ValueError("incremental decoding needs a causal model (BertConfig(causal=True))")
        self._check_w8(gemm)
        dtype = cache.act_dtype
        # the embedding kernel indexes positions by row % S: form word[id] + pos[p] + type[0] as
        # it does (tables rounded to the activation dtype, summed in fp32, rounded once)
        p = cache.pos.long().clamp(max=cfg.max_position_embeddings - 1)
        s = (self.word_embeddings[ids_new.reshape(-1)].to(dtype).float()
             + self.position_embeddings[p].to(dtype).float()
             + self.token_type_embeddings[0].to(dtype).float()).to(dtype)
        x = ops.bias_dropout_add_layer_norm(s, None, None, self.emb_ln.gamma, self.emb_ln.beta,
                                            0.0, False, cfg.layer_norm_eps)
        cache.max_len = min(cache.max_len + 1, cache.capacity)
        for i, layer in enumerate(self.layers):
            x = layer.decode(x, cache.k[i], cache.v[i], cache.pos, cache.max_len,
                             *cache.layer(i)[2:], gemm=gemm)
        cache.pos.add_(1)
        logits = self._head(x, gemm)
        return logits if _padded else logits[:, :cfg.vocab_size]

    @torch.no_grad()
    def extend(self, ids_new, cache, n_new=None, all_logits=False, _padded=False, gemm=None):
        """T new tokens per sequence (``ids_new`` [B, T], the first ``n_new[b]`` of row b real;
        ``n_new``: CPU lengths in [0, T], default T everywhere) at positions ``cache.pos[b] ..``:
        every layer runs at B*T rows with ``ops.attention_append`` against its cache and
        ``cache.pos`` advances by ``n_new`` on the device.  -> the logits of each row's last new
        token [B, vocab_size], or of all T positions [B, T, vocab_size] with ``all_logits``.

        A row with ``n_new == 0`` and, with ``all_logits``, the positions at or past ``n_new[b]``
        return logits that callers must not use.  The capacity is checked on the host against
        ``cache.max_len``, the host's bound on ``cache.pos`` (``cache.reset()`` and ``prefill``
        set it); nothing here reads the device.  ``gemm="skinny"``: as :meth:`decode_step`, for
        the layers when B*T <= 64 and for the head when its rows are."""
        cfg = self.cfg
        if not cfg.causal:
            raise ValueError("incremental decoding needs a causal model (BertConfig(causal=True))")
        self._check_w8(gemm)
        B, T = ids_new.shape
        n = torch.full((B,), T) if n_new is None else torch.as_tensor(n_new).reshape(-1).cpu()
        if B != cache.batch or n.numel() != B or int(n.min()) < 0 or int(n.max()) > T:
            raise ValueError(f"n_new must hold {cache.batch} lengths in [0, {T}]")
        if cache.max_len + int(n.max()) > cache.capacity:
            raise ValueError(f"{cache.max_len} cached + {int(n.max())} new tokens exceed the "
                             f"capacity {cache.capacity}")
        dev, dtype = ids_new.device, cache.act_dtype
        n_d = n.to(dev, torch.int32)
        # word[id] + pos[p] + type[0] as decode_step forms it, p = cache.pos[b] + i
        p = (cache.pos.long().view(B, 1) + torch.arange(T, device=dev).view(1, T)).reshape(-1)
        p = p.clamp(max=cfg.max_position_embeddings - 1)
        s = (self.word_embeddings[ids_new.reshape(-1)].to(dtype).float()
             + self.position_embeddings[p].to(dtype).float()
             + self.token_type_embeddings[0].to(dtype).float()).to(dtype)
        x = ops.bias_dropout_add_layer_norm(s, None, None, self.emb_ln.gamma, self.emb_ln.beta,
                                            0.0, False, cfg.layer_norm_eps)
        launch_len = max(T, min(cache.max_len + T, cache.capacity))
        for i, layer in enumerate(self.layers):
            x = layer.extend(x, cache.k[i], cache.v[i], cache.pos, n_d, T, launch_len,
                             *cache.layer(i)[2:], gemm=gemm)
        cache.pos.add_(n_d)
        cache.max_len = min(cache.max_len + int(n.max()), cache.capacity)
        if not all_logits:
            last = torch.arange(B, device=dev) * T + (n_d.long() - 1).clamp(min=0)
            t, ln = _deferred(x)                      # a row-wise LayerNorm commutes with the pick
            x = t.index_select(0, last) if ln is None else (t.index_select(0, last), ln)
        logits = self._head(x, gemm)
        logits = logits if _padded else logits[:, :cfg.vocab_size]
        return logits.view(B, T, -1) if all_logits else logits

    def generate(self, input_ids, prompt_lens, max_new_tokens, temperature=0.0, top_k=0,
                 eos_id=None, generator=None, top_p=1.0, seed=None, return_logprobs=False,
                 prefill_chunk=None, kv_dtype=None, decode_gemm=None):
        """Continue the right-padded prompts [B, Sp] by ``max_new_tokens`` tokens -> int64
        [B, max_new_tokens].  Greedy at ``temperature == 0``; otherwise softmax sampling of
        ``logits / temperature`` over the ``top_k`` largest (all when 0) with ``generator``.  A row
        that has produced ``eos_id`` keeps producing it.  ``prompt_lens`` are CPU lengths: the one
        host check (capacity) is made from them before the loop, which never reads the device.

        With an int ``seed`` every pick is one ``ops.sample_tokens`` call on the padded logits
        (greedy included), counted by ``cache.pos``: the tokens are a function of the seed,
        ``top_p`` (nucleus) filtering is available and ``return_logprobs=True`` also returns the
        log-probability of every picked token, fp32 [B, max_new_tokens] (of the sampled token, also
        where ``eos_id`` replaced it).  ``generator`` is not used then.

        ``prefill_chunk=T`` feeds the prompt through ``prefill(chunk=T)``, T tokens at a time.
        ``kv_dtype="fp8"`` keeps the keys and values in an FP8 cache (:class:`KVCache`).
        ``decode_gemm="skinny"`` runs the GEMMs of every decode step, and of a chunked prefill's
        pieces of at most 64 rows, on the weight-streaming kernel (:meth:`decode_step`),
        ``"skinny_ln"`` also defers the layers' LayerNorms into it; ``"skinny_w8"`` /
        ``"skinny_ln_w8"`` run them on FP8 weights, quantised here from the current weights
        (:meth:`quantize_weights`) before the loop; None or "default" is the persistent GEMM."""
        lens = self._check_prompts(input_ids, prompt_lens)
        if _skinny(decode_gemm, 1)[1]:
            self.quantize_weights()
        if seed is None and (top_p != 1.0 or return_logprobs):
            raise ValueError("top_p and return_logprobs need the seeded path: pass seed=")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        need = int(lens.max()) + max_new_tokens
        if need > self.cfg.max_position_embeddings:
            raise ValueError(f"prompt + max_new_tokens = {need} exceeds the capacity "
                             f"{self.cfg.max_position_embeddings}")
        dev = input_ids.device
        cache = KVCache(self.cfg, input_ids.shape[0], need, dev,
                        torch.bfloat16 if input_ids.is_cuda else torch.float32,
                        min_rows=input_ids.shape[1], kv_dtype=kv_dtype)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                out = torch.empty(input_ids.shape[0], max_new_tokens, dtype=torch.int64,
                                  device=dev)
                done = torch.zeros(input_ids.shape[0], dtype=torch.bool, device=dev)
                fused = seed is not None
                lps = torch.empty(out.shape, dtype=torch.float32, device=dev) if fused else None
                if prefill_chunk is None:
                    logits = self.prefill(input_ids, lens, cache, _padded=fused)
                else:
                    logits = self.prefill(input_ids, lens, cache, _padded=fused,
                                          chunk=prefill_chunk, gemm=decode_gemm)
                for t in range(max_new_tokens):
                    if fused:
                        tok, lps[:, t] = ops.sample_tokens(logits, seed, cache.pos, temperature,
                                                           top_k, top_p, self.cfg.vocab_size)
                    else:
                        tok = _pick(logits, temperature, top_k, generator)
                    if eos_id is not None:
                        tok = torch.where(done, torch.full_like(tok, eos_id), tok)
                        done = done | (tok == eos_id)
                    out[:, t] = tok
                    if t + 1 < max_new_tokens:
                        logits = self.decode_step(tok, cache, _padded=fused, gemm=decode_gemm)
        finally:
            self.train(was_training)
        return (out, lps) if return_logprobs else out


def _pick(logits, temperature, top_k, generator):
    """The next token of every row: argmax, or a sample of softmax(logits / temperature) over the
    ``top_k`` largest logits."""
    if temperature <= 0:
        return logits.argmax(-1)
    x = logits.float() / temperature
    if top_k > 0:
        vals, idx = x.topk(min(top_k, x.shape[-1]), dim=-1)
        choice = torch.multinomial(torch.softmax(vals, -1), 1, generator=generator)
        return idx.gather(1, choice).squeeze(1)
    return torch.multinomial(torch.softmax(x, -1), 1, generator=generator).squeeze(1)


class KVCache:
    """The keys and values of every layer for incremental decoding: ``k`` / ``v``
    [L, B, heads, C, 64] (one (batch, head)'s keys are contiguous 128-B rows, the layout the decode
    kernel streams) and ``pos`` int32 [B] on the device, the row each sequence's next token takes.
    ``capacity`` is rounded up to a multiple of 64.  ``max_len`` is the host's upper bound on
    ``pos + 1``; it only sizes launches.

    ``kv_dtype`` (default ``dtype``): ``torch.float8_e4m3fn`` or ``"fp8"`` stores ``k`` / ``v`` as
    e4m3 bytes, 64-B rows, with ``k_scale`` / ``v_scale`` fp32 [L, B, heads, C], one power-of-two
    scale per row (``ops.reference.kv_quantize_rows``): 68 bytes per cached row instead of 128.
    ``act_dtype`` is ``dtype``, what the model computes in."""

    def __init__(self, cfg: BertConfig, batch, capacity, device, dtype=torch.bfloat16,
                 min_rows=0, kv_dtype=None):
        # min_rows: storage for a prefill whose padding runs past the capacity
        C = -(-max(int(capacity), int(min_rows)) // 64) * 64
        if capacity < 1 or capacity > cfg.max_position_embeddings:
            raise ValueError(f"capacity {capacity} outside [1, max_position_embeddings = "
                             f"{cfg.max_position_embeddings}]")
        shape = (cfg.num_hidden_layers, batch, cfg.num_attention_heads, C, 64)
        if kv_dtype in (None, "bf16") or kv_dtype == dtype:
            kv_dtype = dtype
        elif kv_dtype == "fp8":
            kv_dtype = torch.float8_e4m3fn
        if kv_dtype not in (dtype, torch.float8_e4m3fn):
            raise ValueError(f"kv_dtype {kv_dtype} is neither the activation dtype nor fp8")
        self.act_dtype = dtype
        self.k = torch.zeros(shape, device=device, dtype=kv_dtype)
        self.v = torch.zeros(shape, device=device, dtype=kv_dtype)
        self.k_scale = self.v_scale = None
        if kv_dtype == torch.float8_e4m3fn:
            self.k_scale = torch.zeros(shape[:4], device=device, dtype=torch.float32)
            self.v_scale = torch.zeros(shape[:4], device=device, dtype=torch.float32)
        self.pos = torch.zeros(batch, device=device, dtype=torch.int32)
        self.batch, self.capacity, self.max_len = batch, C, C

    def layer(self, i):
        """Layer i's ``(k, v)``, an FP8 cache's ``(k, v, k_scale, v_scale)``."""
        if self.k_scale is None:
            return self.k[i], self.v[i]
        return self.k[i], self.v[i], self.k_scale[i], self.v_scale[i]

    def reset(self):
        """An empty cache: ``pos = 0`` on the device and ``max_len = 0`` (the stored keys and
        values stay; nothing reads rows at or past ``pos``)."""
        self.pos.zero_()
        self.max_len = 0


def bert_base(**kw) -> BertForPreTraining:
    return BertForPreTraining(BertConfig.base(**kw))


def bert_large(**kw) -> BertForPreTraining:
    return BertForPreTraining(BertConfig.large(**kw))


def mlm_flops_per_token(cfg: BertConfig, seq_len: int, max_predictions: int) -> float:
    """Training FLOPs per input token (fwd + bwd = 3x fwd) for MFU accounting."""
    H, L, I = cfg.hidden_size, cfg.num_hidden_layers, cfg.intermediate_size
    gemm = 2 * (3 * H * H + H * H + 2 * H * I) * L
    attn = 2 * 2 * seq_len * H * L
    head = 2 * (H * H + H * cfg.vocab_size) * max_predictions / seq_len
    return 3.0 * (gemm + attn + head)


def causal_lm_flops_per_token(cfg: BertConfig, seq_len: int) -> float:
    """Training FLOPs per input token of a causal model (fwd + bwd = 3x fwd): the head decodes
    every position and half the attention products are counted (the visible triangle; the
    kernels do (n + 1) / (2 n) of them at n = seq_len / 64 tiles, the diagonal tiles whole)."""
    H, L, I = cfg.hidden_size, cfg.num_hidden_layers, cfg.intermediate_size
    gemm = 2 * (3 * H * H + H * H + 2 * H * I) * L
    attn = 2 * 2 * seq_len * H * L / 2
    head = 2 * (H * H + H * cfg.vocab_size)
    return 3.0 * (gemm + attn + head)


__all__ = ["BertConfig", "BertForPreTraining", "BertLayer", "KVCache", "bert_base", "bert_large",
           "causal_lm_flops_per_token", "mlm_flops_per_token"]
