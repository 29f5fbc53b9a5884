"""PyTorch reference implementations of every op in :mod:`distributedtensorflow_amd.ops`.

These are the *oracles* the HIP kernels are tested against and the CPU execution path
(``OneDeviceStrategy("/cpu:0")``, BASELINE config 1).  All image tensors are NHWC
(TF ``channels_last``, the tf.layers default used by the reference CNN,
``run_mnist_distributed.py:50-69``).  Filters are stored ``[K, R, S, C]`` (output channel
major, reduction axis contiguous) which is the layout the MFMA implicit-GEMM kernels consume;
the checkpoint layer converts to TF's ``HWIO`` on save/load.

Math follows the TF1 kernels the reference calls:
  * ``sparse_softmax_cross_entropy`` = mean over the batch (``run_mnist_distributed.py:113``);
  * batch-norm uses biased batch variance for normalisation and the Bessel-corrected
    variance for the moving average (TF ``FusedBatchNorm`` training semantics).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv_out_size(h, r, stride, pad_lo, pad_hi):
    return (h + pad_lo + pad_hi - r) // stride + 1


def resolve_padding(padding, h, w, r, s, stride):
    """Return (pad_top, pad_bottom, pad_left, pad_right) for TF-style or explicit padding."""
    sh, sw = _pair(stride)
    if isinstance(padding, str):
        p = padding.upper()
        if p == "VALID":
            return 0, 0, 0, 0
        if p == "SAME":
            oh = -(-h // sh)
            ow = -(-w // sw)
            th = max((oh - 1) * sh + r - h, 0)
            tw = max((ow - 1) * sw + s - w, 0)
            return th // 2, th - th // 2, tw // 2, tw - tw // 2
        raise ValueError(f"unknown padding {padding!r}")
    ph, pw = _pair(padding)
    return ph, ph, pw, pw


def conv2d(x, w, stride=1, padding=0, bias=None):
    """x: [N,H,W,C]; w: [K,R,S,C] -> y: [N,P,Q,K]."""
    n, h, wd, c = x.shape
    k, r, s, c2 = w.shape
    assert c == c2, (x.shape, w.shape)
    pt, pb, pl, pr = resolve_padding(padding, h, wd, r, s, stride)
    xn = x.permute(0, 3, 1, 2)
    if (pt, pl) != (pb, pr):
        xn = F.pad(xn, (pl, pr, pt, pb))
        pad = 0
    else:
        pad = (pt, pl)
    y = F.conv2d(xn, w.to(x.dtype).permute(0, 3, 1, 2), bias, _pair(stride), pad)
    return y.permute(0, 2, 3, 1)


def batch_norm(x, gamma, beta, running_mean=None, running_var=None, training=True,
               momentum=0.997, eps=1e-5, relu=False, residual=None):
    """Fused BN (+ residual add) (+ ReLU) over the channel (last) axis of an NHWC tensor.

    ``momentum`` is TF's *decay*: moving = moving * momentum + batch * (1 - momentum).
    """
    c = x.shape[-1]
    xf = x.float().reshape(-1, c)
    if training:
        mean = xf.mean(0)
        var = xf.var(0, unbiased=False)
        if running_mean is not None:
            n = xf.shape[0]
            with torch.no_grad():
                running_mean.mul_(momentum).add_(mean.detach() * (1 - momentum))
                unb = var.detach() * (n / max(n - 1, 1))
                running_var.mul_(momentum).add_(unb * (1 - momentum))
    else:
        mean, var = running_mean, running_var
    y = (xf - mean) * torch.rsqrt(var + eps) * gamma.float() + beta.float()
    if residual is not None:
        y = y + residual.float().reshape(-1, c)
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype).reshape(x.shape)


def relu(x):
    return torch.relu(x)


def max_pool2d(x, kernel=2, stride=2, padding=0):
    kh, kw = _pair(kernel)
    n, h, w, c = x.shape
    pt, pb, pl, pr = resolve_padding(padding, h, w, kh, kw, stride)
    xn = x.permute(0, 3, 1, 2)
    if (pt, pl) != (pb, pr):
        xn = F.pad(xn, (pl, pr, pt, pb), value=float("-inf"))
        pad = 0
    else:
        pad = (pt, pl)
    y = F.max_pool2d(xn, (kh, kw), _pair(stride), pad)
    return y.permute(0, 2, 3, 1)


def global_avg_pool(x):
    """[N,H,W,C] -> [N,C] (mean over H, W; computed in fp32)."""
    return x.float().mean(dim=(1, 2)).to(x.dtype)


def deferred_ln_check(pre_ln, residual, residual_ln, gelu=False, relu=False, bias=True):
    """The argument rules of a dense layer with a deferred LayerNorm, one check for both backends.
    ``pre_ln`` / ``residual_ln``: ``(gamma, beta, eps)`` of the LayerNorm that the input / the
    residual still lacks; a call normalises at most one matrix."""
    for ln in (pre_ln, residual_ln):
        if ln is not None and (not isinstance(ln, (tuple, list)) or len(ln) != 3):
            raise ValueError("dense: pre_ln / residual_ln are (gamma, beta, eps) tuples")
    if pre_ln is not None and residual_ln is not None:
        raise ValueError("dense: pre_ln and residual_ln cannot both be set: a call normalises "
                         "one matrix")
    if residual_ln is not None and residual is None:
        raise ValueError("dense: residual_ln needs the residual it normalises")
    if residual is not None and (gelu or relu):
        raise ValueError("dense: a residual combines with the bias epilogue only, not with an "
                         "activation")
    if residual is not None and not bias:
        raise ValueError("dense: the residual epilogue needs a bias")


def dense(x, w, b=None, relu=False, pre_ln=None, residual=None, residual_ln=None):
    """x: [M, in]; w: [out, in] (GEMM 'NT' layout); b: [out].  Deferred LayerNorm (the rule of the
    skinny-M kernel): ``pre_ln`` -> the input is ``layer_norm(x, *pre_ln)``, rounded to x's dtype;
    ``residual`` [M, out] (``residual_ln``: ``layer_norm`` of it, rounded likewise) is added to
    the fp32 sum after the bias, so the result rounds once."""
    if pre_ln is None and residual is None and residual_ln is None:
        y = F.linear(x, w.to(x.dtype), None if b is None else b.to(x.dtype))
        return torch.relu(y) if relu else y
    deferred_ln_check(pre_ln, residual, residual_ln, relu=relu, bias=b is not None)
    if pre_ln is not None:
        x = layer_norm(x, *pre_ln)
    if residual is None:
        return dense(x, w, b, relu)
    if residual.shape != x.shape[:-1] + w.shape[:1]:
        raise ValueError(f"dense: residual {tuple(residual.shape)} does not match the output")
    if residual_ln is not None:
        residual = layer_norm(residual, *residual_ln)
    y = F.linear(x.float(), w.to(x.dtype).float(), b.float()) + residual.float()
    return y.to(x.dtype)


def sparse_softmax_cross_entropy(logits, labels, label_smoothing=0.0):
    """Mean over batch of -log softmax(logits)[label] (TF default reduction); with
    ``label_smoothing`` e the target row is (1-e) onehot + e/V (TF's and torch's definition)."""
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError("label_smoothing must be in [0, 1]")
    return F.cross_entropy(logits.float(), labels.long(), label_smoothing=float(label_smoothing))


def mixed_softmax_cross_entropy(logits, labels_a, labels_b, lam, label_smoothing=0.0):
    """The two-label loss of Mixup / CutMix: the mean over the batch of the cross-entropy against
    ``lam onehot(a) + (1 - lam) onehot(b)``, smoothed as ``sparse_softmax_cross_entropy``.
    ``lam``: fp32 [B] in [0, 1], the weight of ``labels_a``; ``1 - lam`` is formed in fp32."""
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError("label_smoothing must be in [0, 1]")
    _mixed_xent_check(logits, labels_a, labels_b, lam)
    if lam.numel() and (float(lam.min()) < 0.0 or float(lam.max()) > 1.0):
        raise ValueError("mixed_softmax_cross_entropy: lam outside [0, 1]")
    e, x = float(label_smoothing), logits.float()
    xa = x.gather(1, labels_a.long().unsqueeze(1)).squeeze(1)
    xb = x.gather(1, labels_b.long().unsqueeze(1)).squeeze(1)
    rows = torch.logsumexp(x, 1) - (1.0 - e) * (lam * xa + (1.0 - lam) * xb)
    if e:
        rows = rows - (e / x.shape[1]) * x.sum(1)
    return rows.mean()


def _mixed_xent_check(logits, labels_a, labels_b, lam):
    """Shared argument validation of ``mixed_softmax_cross_entropy`` (both backends)."""
    if logits.dim() != 2:
        raise ValueError("logits must be [B, V]")
    B = logits.shape[0]
    if tuple(labels_a.shape) != (B,) or tuple(labels_b.shape) != (B,):
        raise ValueError("mixed_softmax_cross_entropy: labels_a and labels_b must be [B]")
    if lam.dtype != torch.float32 or tuple(lam.shape) != (B,):
        raise ValueError("mixed_softmax_cross_entropy: lam must be fp32 [B]")
    for t in (labels_a, labels_b, lam):
        if t.device != logits.device:
            raise ValueError("mixed_softmax_cross_entropy: every argument lives on the logits' "
                             "device")


def softmax_cross_entropy_clipped_sum(logits, onehot):
    """The MLP template's loss: -sum(y * log(clip(softmax(logits), 1e-10, 1)))
    (``templates/00_mnist_replica.py:162-164``)."""
    p = torch.softmax(logits.float(), dim=-1).clamp(1e-10, 1.0)
    return -(onehot.float() * torch.log(p)).sum()


def layer_norm(x, gamma, beta, eps=1e-12):
    return F.layer_norm(x.float(), (x.shape[-1],), gamma.float(), beta.float(), eps).to(x.dtype)


def gelu(x):
    return F.gelu(x.float(), approximate="tanh").to(x.dtype)


def _causal_select(s):
    """Scores [..., S, S] with every key above the query's own position selected to -inf."""
    S = s.shape[-1]
    vis = torch.ones(S, S, dtype=torch.bool, device=s.device).tril()
    return torch.where(vis, s, torch.full_like(s, float("-inf")))


def attention(q, k, v, mask=None, scale=None, causal=False):
    """q,k,v: [B, H, S, D] -> [B, H, S, D].  mask: additive [B,1,1,S] or None.  ``causal``:
    query i sees key j iff j <= i."""
    d = q.shape[-1]
    scale = scale if scale is not None else d ** -0.5
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if mask is not None:
        s = s + mask.float()
    if causal:
        s = _causal_select(s)
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, v.float()).to(q.dtype)


def dropout(x, p, training=True):
    return F.dropout(x, p, training)


# ----------------------------------------------------------------------------- transformer ops
# Bit-exact twins of csrc/kernels/nlp.hip (same hash-based dropout masks), used as the CPU path
# and as the oracle of the GPU numerics tests.

_M32 = 0xFFFFFFFF


def _fmix32(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def drop_threshold(p):
    import numpy as np
    if p <= 0:
        return 0
    t = float(np.float32(p)) * 4294967296.0
    return 4294967295 if t >= 4294967295.0 else int(t)


def keep_mask(seed, idx, p):
    """keep(idx) of the kernels: fmix32(idx * 0x9E3779B1 + seed) >= p * 2^32 (uint32 math)."""
    idx = idx.to(torch.int64) & _M32
    h = _fmix32((idx * 0x9E3779B1 + int(seed)) & _M32)
    return h >= drop_threshold(p)


def sample_uniform(seed, counter):
    """The draw of ``sample_tokens``: row b of the int32 ``counter`` [B] gets
    ``u = (fmix32(fmix32(b * 0x9E3779B1 + seed) + counter[b]) >> 8) * 2^-24`` (uint32 math), fp64."""
    b = torch.arange(counter.numel(), device=counter.device, dtype=torch.int64)
    h = _fmix32((b * 0x9E3779B1 + int(seed)) & _M32)
    h = _fmix32((h + (counter.to(torch.int64) & _M32)) & _M32)
    return (h >> 8).double() * 2.0 ** -24


def _drop(x, p, seed, idx):
    if p <= 0:
        return x
    return torch.where(keep_mask(seed, idx, p), x / (1.0 - float(torch.tensor(p, dtype=torch.float32))), torch.zeros_like(x))


def _rows_cols_idx(M, H, device):
    return torch.arange(M * H, device=device, dtype=torch.int64).view(M, H)


def _next_seed(p):
    return int(torch.randint(0, 2 ** 31 - 1, (1,), device="cpu").item()) if p > 0 else 0


def _round_st(t, dtype):
    """Round the forward value to ``dtype`` (what the kernels store) while the gradient passes
    through in full precision (the kernels accumulate gradients in fp32)."""
    if dtype == t.dtype:
        return t
    return t + (t.to(dtype).to(t.dtype) - t).detach()


def _ln(s, gamma, beta, eps):
    mean = s.mean(-1, keepdim=True)
    var = s.var(-1, unbiased=False, keepdim=True)
    return (s - mean) * torch.rsqrt(var + eps) * gamma.float() + beta.float()


def bias_dropout_add_layer_norm(a, bias, residual, gamma, beta, p=0.0, training=True, eps=1e-12,
                                seed=None):
    p = p if training else 0.0
    H = a.shape[-1]
    s = a.float().reshape(-1, H)
    if bias is not None:
        s = s + bias.float()
    if p > 0:
        seed = _next_seed(p) if seed is None else seed
        s = _drop(s, p, seed, _rows_cols_idx(s.shape[0], H, s.device))
    if residual is not None:
        s = s + residual.float().reshape(-1, H)
    s = _round_st(s, a.dtype)
    return _ln(s, gamma, beta, eps).to(a.dtype).view(a.shape)


def embedding_layer_norm(ids, token_type_ids, word, pos, typ, gamma, beta, p=0.0, training=True,
                         eps=1e-12, seed=None, dtype=None):
    p = p if training else 0.0
    B, S = ids.shape
    H = word.shape[1]
    dtype = dtype or word.dtype
    tt = token_type_ids if token_type_ids is not None else torch.zeros_like(ids)
    w32, p32, t32 = (_round_st(t.float(), dtype) for t in (word, pos, typ))
    s = (w32[ids] + p32[:S].unsqueeze(0) + t32[tt]).reshape(B * S, H)
    s = _round_st(s, dtype)
    y = _ln(s, gamma, beta, eps)
    if p > 0:
        seed = _next_seed(p) if seed is None else seed
        y = _drop(y, p, seed, _rows_cols_idx(B * S, H, y.device))
    return y.to(dtype)


def bias_gelu(a, bias=None):
    x = a.float() + (bias.float() if bias is not None else 0.0)
    return F.gelu(x, approximate="tanh").to(a.dtype)


def attention_qkv(qkv, mask, batch, seq_len, heads, p=0.0, training=True, scale=None, seed=None,
                  causal=False):
    """qkv [B*S, 3*H*D] (all q heads | all k heads | all v heads) -> [B*S, H*D].  ``causal``:
    query i sees key j iff j <= i (a lower-triangular select before the softmax; the dropout
    indices stay those of the full [B, H, S, S] space)."""
    p = p if training else 0.0
    B, S, Hh = batch, seq_len, heads
    D = qkv.shape[-1] // (3 * Hh)
    scale = D ** -0.5 if scale is None else scale
    x = qkv.float().view(B, S, 3, Hh, D)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))     # [B, H, S, D]
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s + mask.float().view(B, 1, 1, S)
    if causal:
        s = _causal_select(s)
    prob = torch.softmax(s, dim=-1)
    if p > 0:
        seed = _next_seed(p) if seed is None else seed
        idx = torch.arange(B * Hh * S * S, device=qkv.device, dtype=torch.int64).view(B, Hh, S, S)
        prob = _drop(prob, p, seed, idx)
    o = torch.matmul(prob, v)                                         # [B, H, S, D]
    return o.permute(0, 2, 1, 3).reshape(B * S, Hh * D).to(qkv.dtype)


F8 = torch.float8_e4m3fn


def kv_quantize_rows(x):
    """THE rule of the FP8 key / value cache (the kernels of csrc/kernels/kv_f8.h reproduce it bit
    for bit): rows ``x`` [..., 64] of finite values -> (e4m3 bytes [..., 64], fp32 scales [...]).

    With ``a = max |x_i| = f 2^k``, f in [0.5, 1): ``e = k - 9`` if ``f <= 0.875`` (448 =
    0.875 * 2^9, the largest e4m3 value) else ``k - 8``, clamped to [-100, 120]; ``a == 0`` gives
    ``e = 0``.  The scale is ``2^e`` and byte i is ``x_i 2^-e`` rounded to nearest even: by
    construction ``|x_i 2^-e| <= 448``, nothing saturates."""
    xf = x.detach().float()
    a = xf.abs().amax(-1)
    f, k = torch.frexp(a)
    e = torch.where(f <= 0.875, k - 9, k - 8)
    e = torch.where(a == 0, torch.zeros_like(e), e).clamp(-100, 120)
    one = torch.ones_like(a)
    return (xf * torch.ldexp(one, -e).unsqueeze(-1)).to(F8), torch.ldexp(one, e)


def kv_dequantize(q, scale, dtype=torch.float32):
    """``float(byte) * scale``: exact in fp32 (a power of two times 4 significant bits) and, with
    the clamp on the exponent, a normal bf16."""
    return (q.float() * scale.unsqueeze(-1)).to(dtype)


def weight_quantize_fp8(w):
    """An [N, K] weight (K % 64 == 0) -> the FP8 pair ``(q, scale)`` of the skinny-M dense kernel:
    :func:`kv_quantize_rows` on every 64-k unit of the bf16-ROUNDED weight (what the bf16 path
    consumes), ``q`` float8_e4m3fn [N, K] and ``scale`` fp32 [N, K / 64]."""
    if w.dim() != 2 or w.shape[1] % 64 or not w.shape[1]:
        raise ValueError(f"weight_quantize_fp8 takes an [N, K] weight with K % 64 == 0, got "
                         f"{tuple(w.shape)}")
    N, K = w.shape
    q, scale = kv_quantize_rows(w.detach().to(torch.bfloat16).reshape(N, K // 64, 64))
    return q.view(N, K), scale


def is_weight_pair(w):
    return isinstance(w, (tuple, list))


def check_weight_pair(w):
    """The one rule of an FP8 weight pair, for both backends -> (q, scale)."""
    if len(w) != 2 or not all(isinstance(t, torch.Tensor) for t in w):
        raise ValueError("dense: an FP8 weight is the pair (q, scale) of weight_quantize_fp8")
    q, scale = w
    if q.dtype != F8 or q.dim() != 2 or q.shape[1] % 64 or not q.is_contiguous():
        raise ValueError(f"dense: q must be a contiguous float8_e4m3fn [N, K] with K % 64 == 0, "
                         f"got {q.dtype} {tuple(q.shape)}, strides {tuple(q.stride())}")
    if (scale.dtype != torch.float32 or tuple(scale.shape) != (q.shape[0], q.shape[1] // 64)
            or not scale.is_contiguous() or scale.device != q.device):
        raise ValueError(f"dense: scale must be a contiguous fp32 "
                         f"{[q.shape[0], q.shape[1] // 64]} on q's device, got {scale.dtype} "
                         f"{tuple(scale.shape)}")
    return q, scale


def weight_dequantize(w, dtype=torch.float32):
    """The matrix an FP8 weight pair stands for, exactly (see :func:`kv_dequantize`)."""
    q, scale = check_weight_pair(w)
    N, K = q.shape
    return kv_dequantize(q.view(N, K // 64, 64), scale, dtype).view(N, K)


def check_kv_dtypes(name, qkv, k_cache, v_cache, k_scale, v_scale):
    """The one rule for the cache's data type, shared by the three cache ops and both backends ->
    True for an FP8 cache.  ``float8_e4m3fn`` caches need both fp32 [B, heads, C] scales; any
    other cache shares ``qkv``'s dtype and takes none."""
    if k_cache.dtype != v_cache.dtype:
        raise ValueError("k_cache and v_cache must share one dtype")
    if k_cache.dtype != F8:
        if k_scale is not None or v_scale is not None:
            raise ValueError("k_scale / v_scale go with float8_e4m3fn caches only")
        if qkv.dtype != k_cache.dtype:
            raise ValueError(f"{name} and the caches must share one dtype")
        return False
    if k_scale is None or v_scale is None:
        raise ValueError("float8_e4m3fn caches need k_scale and v_scale")
    for t in (k_scale, v_scale):
        if (t.dtype != torch.float32 or t.shape != k_cache.shape[:3] or not t.is_contiguous()
                or t.device != k_cache.device):
            raise ValueError(f"k_scale / v_scale must be contiguous fp32 "
                             f"{list(k_cache.shape[:3])} on the caches' device")
    return True


def _f8_call(qkv, k_cache, v_cache, k_scale, v_scale, run):
    """An FP8-cache op of the reference: ``run(qkv', k, v)`` is the bf16-cache op on the
    DEQUANTISED caches, fed the new rows as the cache will hold them (quantised and dequantised),
    and -> the cache rows it wrote as a bool [B, C].  Those rows' bytes and scales go back into
    the FP8 caches; nothing else is touched."""
    B, H, C, D = k_cache.shape
    x = qkv.detach().reshape(B, -1, 3, H, D)
    packed = [kv_quantize_rows(x[:, :, i]) for i in (1, 2)]           # bytes / scale [B, T, H(, D)]
    x = torch.stack([x[:, :, 0]] + [kv_dequantize(q, s, qkv.dtype) for q, s in packed], 2)
    k, v = (kv_dequantize(c, s, qkv.dtype) for c, s in ((k_cache, k_scale), (v_cache, v_scale)))
    out, b_idx, rows, t_idx = run(x.reshape(qkv.shape), k, v)
    for (q, s), cache, scale in zip(packed, (k_cache, v_cache), (k_scale, v_scale)):
        cache.view(torch.uint8)[b_idx, :, rows] = q.view(torch.uint8)[b_idx, t_idx]
        scale[b_idx, :, rows] = s[b_idx, t_idx]
    return out


def check_decode_args(qkv_new, k_cache, v_cache, pos, heads, max_len, splits, k_scale=None,
                      v_scale=None):
    """The shape / dtype conditions of ``attention_decode``, shared by both backends ->
    (B, capacity, max_len)."""
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[3] != 64:
        raise ValueError("k_cache and v_cache must both be [B, heads, capacity, 64]")
    B, H, C, D = k_cache.shape
    if H != heads:
        raise ValueError(f"caches hold {H} heads, not {heads}")
    if qkv_new.dim() != 2 or tuple(qkv_new.shape) != (B, 3 * H * D):
        raise ValueError(f"qkv_new must be [{B}, {3 * H * D}], got {tuple(qkv_new.shape)}")
    if C < 64 or C % 64:
        raise ValueError("cache capacity must be a multiple of 64, at least 64")
    if pos.dtype != torch.int32 or tuple(pos.shape) != (B,):
        raise ValueError(f"pos must be int32 [{B}]")
    check_kv_dtypes("qkv_new", qkv_new, k_cache, v_cache, k_scale, v_scale)
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("the caches must be contiguous")
    max_len = C if max_len is None else int(max_len)
    if not 1 <= max_len <= C:
        raise ValueError("max_len must lie in [1, capacity]")
    if splits < 0 or splits > -(-max_len // 64):
        raise ValueError(f"splits {splits} exceeds the {-(-max_len // 64)} tiles of max_len")
    return B, C, max_len


def check_fill_args(qkv, k_cache, v_cache, batch, seq_len, heads, k_scale=None, v_scale=None):
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[3] != 64:
        raise ValueError("k_cache and v_cache must both be [B, heads, capacity, 64]")
    B, H, C, D = k_cache.shape
    if (B, H) != (batch, heads):
        raise ValueError(f"caches are for batch {B}, {H} heads")
    if qkv.dim() != 2 or tuple(qkv.shape) != (batch * seq_len, 3 * H * D):
        raise ValueError(f"qkv must be [{batch * seq_len}, {3 * H * D}], got {tuple(qkv.shape)}")
    if C < 64 or C % 64 or not 1 <= seq_len <= C:
        raise ValueError("capacity must be a multiple of 64 and 1 <= seq_len <= capacity")
    check_kv_dtypes("qkv", qkv, k_cache, v_cache, k_scale, v_scale)
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("the caches must be contiguous")


def no_grad_op(name, *tensors):
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(f"{name} is a no-grad op: call it under torch.no_grad()")


def kv_cache_fill(qkv, k_cache, v_cache, batch, seq_len, heads, k_scale=None, v_scale=None):
    """The K and V thirds of a prefill qkv [B*S, 3*H*64] into rows 0 .. S-1 of the [B, H, C, 64]
    caches (in place; rows >= S untouched).  FP8 caches take ``kv_quantize_rows`` of them."""
    no_grad_op("kv_cache_fill", qkv, k_cache, v_cache)
    check_fill_args(qkv, k_cache, v_cache, batch, seq_len, heads, k_scale, v_scale)
    x = qkv.detach().view(batch, seq_len, 3, heads, 64)
    if k_cache.dtype == F8:
        for i, cache, scale in ((1, k_cache, k_scale), (2, v_cache, v_scale)):
            q, s = kv_quantize_rows(x[:, :, i].permute(0, 2, 1, 3))
            cache.view(torch.uint8)[:, :, :seq_len] = q.view(torch.uint8)
            scale[:, :, :seq_len] = s
        return
    k_cache[:, :, :seq_len] = x[:, :, 1].permute(0, 2, 1, 3)
    v_cache[:, :, :seq_len] = x[:, :, 2].permute(0, 2, 1, 3)


def attention_decode(qkv_new, k_cache, v_cache, pos, heads, scale=None, max_len=None, splits=0,
                     k_scale=None, v_scale=None):
    """One new query per sequence against the caches: the new K / V rows go to row ``pos[b]``
    (clamped to the cache), the query attends keys 0 .. pos[b].  fp32 math on the stored values;
    ``max_len`` and ``splits`` only size the native launch.  With FP8 caches the new rows are
    quantised (``kv_quantize_rows``) and this is the same attention on the dequantised caches."""
    no_grad_op("attention_decode", qkv_new, k_cache, v_cache)
    B, C, _ = check_decode_args(qkv_new, k_cache, v_cache, pos, heads, max_len, splits, k_scale,
                                v_scale)
    scale = 64 ** -0.5 if scale is None else scale
    if k_cache.dtype == F8:
        def run(x, k, v):
            b = torch.arange(B, device=pos.device)
            return (attention_decode(x, k, v, pos, heads, scale), b, pos.long().clamp(0, C - 1),
                    torch.zeros_like(b))
        return _f8_call(qkv_new, k_cache, v_cache, k_scale, v_scale, run)
    x = qkv_new.detach().view(B, 3, heads, 64)
    p = pos.long().clamp(0, C - 1)
    rows = torch.arange(B, device=pos.device)
    k_cache[rows, :, p] = x[:, 1]
    v_cache[rows, :, p] = x[:, 2]
    s = torch.einsum("bhd,bhkd->bhk", x[:, 0].float(), k_cache.float()) * scale
    vis = torch.arange(C, device=pos.device).view(1, 1, C) <= p.view(B, 1, 1)
    prob = torch.softmax(torch.where(vis, s, torch.full_like(s, float("-inf"))), dim=-1)
    # select, not multiply: unwritten cache rows may hold anything
    v = torch.where(vis.unsqueeze(-1), v_cache.float(), torch.zeros((), device=pos.device))
    return torch.einsum("bhk,bhkd->bhd", prob, v).reshape(B, heads * 64).to(qkv_new.dtype)


def check_append_args(qkv_new, k_cache, v_cache, pos, heads, n_new, max_len, splits,
                      k_scale=None, v_scale=None):
    """The shape / dtype conditions of ``attention_append``, shared by both backends ->
    (B, T, capacity, max_len)."""
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[3] != 64:
        raise ValueError("k_cache and v_cache must both be [B, heads, capacity, 64]")
    B, H, C, D = k_cache.shape
    if H != heads:
        raise ValueError(f"caches hold {H} heads, not {heads}")
    if (qkv_new.dim() != 2 or qkv_new.shape[1] != 3 * H * D or qkv_new.shape[0] < B
            or qkv_new.shape[0] % B):
        raise ValueError(f"qkv_new must be [{B} * T, {3 * H * D}], got {tuple(qkv_new.shape)}")
    T = qkv_new.shape[0] // B
    if C < 64 or C % 64:
        raise ValueError("cache capacity must be a multiple of 64, at least 64")
    for name, t in (("pos", pos), ("n_new", n_new)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (B,)
                              or t.device != qkv_new.device):
            raise ValueError(f"{name} must be int32 [{B}] on qkv_new's device")
    check_kv_dtypes("qkv_new", qkv_new, k_cache, v_cache, k_scale, v_scale)
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("the caches must be contiguous")
    max_len = C if max_len is None else int(max_len)
    if not T <= max_len <= C:
        raise ValueError(f"max_len must lie in [T = {T}, capacity = {C}]")
    if splits < 0 or splits > -(-max_len // 64):
        raise ValueError(f"splits {splits} exceeds the {-(-max_len // 64)} tiles of max_len")
    return B, T, C, max_len


def attention_append(qkv_new, k_cache, v_cache, pos, heads, n_new=None, scale=None, max_len=None,
                     splits=0, k_scale=None, v_scale=None):
    """T new tokens per sequence against the caches.  Per row b, with p0 = clamp(pos[b], 0, C) and
    n = clamp(n_new[b] (default T), 0, min(T, C - p0)): the K / V of new tokens 0 .. n-1 go to
    cache rows p0 .. p0+n-1, query i < n attends keys 0 .. p0+i, output rows i >= n are zero.
    fp32 math on the stored values; ``max_len`` and ``splits`` only size the native launch.  With
    FP8 caches the new rows are quantised (``kv_quantize_rows``) and this is the same attention on
    the dequantised caches."""
    no_grad_op("attention_append", qkv_new, k_cache, v_cache)
    B, T, C, _ = check_append_args(qkv_new, k_cache, v_cache, pos, heads, n_new, max_len, splits,
                                   k_scale, v_scale)
    scale = 64 ** -0.5 if scale is None else scale
    dev = qkv_new.device
    if k_cache.dtype == F8:
        def run(x, k, v):
            p0 = pos.long().clamp(0, C)
            n = (torch.full_like(p0, T) if n_new is None else n_new.long()).clamp(min=0)
            n = torch.minimum(n, (C - p0).clamp(max=T))
            b_idx, t_idx = (torch.arange(T, device=dev).view(1, T) < n.view(B, 1)).nonzero(
                as_tuple=True)
            return (attention_append(x, k, v, pos, heads, n_new, scale), b_idx,
                    p0[b_idx] + t_idx, t_idx)
        return _f8_call(qkv_new, k_cache, v_cache, k_scale, v_scale, run)
    x = qkv_new.detach().view(B, T, 3, heads, 64)
    p0 = pos.long().clamp(0, C)
    n = (torch.full_like(p0, T) if n_new is None else n_new.long()).clamp(min=0)
    n = torch.minimum(n, (C - p0).clamp(max=T))
    i = torch.arange(T, device=dev)
    live = i.view(1, T) < n.view(B, 1)                                   # [B, T]
    b_idx, t_idx = live.nonzero(as_tuple=True)
    rows = p0[b_idx] + t_idx
    k_cache[b_idx, :, rows] = x[b_idx, t_idx, 1]
    v_cache[b_idx, :, rows] = x[b_idx, t_idx, 2]
    s = torch.einsum("bthd,bhkd->bhtk", x[:, :, 0].float(), k_cache.float()) * scale
    last = (p0.view(B, 1) + i.view(1, T)).view(B, 1, T, 1)
    vis = (torch.arange(C, device=dev).view(1, 1, 1, C) <= last) & live.view(B, 1, T, 1)
    # select, not multiply: hidden scores and unwritten cache rows may hold anything
    s = torch.where(vis, s, torch.full_like(s, float("-inf")))
    e = torch.where(vis, torch.exp(s - s.amax(-1, keepdim=True).clamp_min(-3e38)),
                    torch.zeros_like(s))
    prob = e / e.sum(-1, keepdim=True).clamp_min(1e-30)                  # a dead row: all zeros
    keys = (torch.arange(C, device=dev).view(1, C) < (p0 + n).view(B, 1)).view(B, 1, C, 1)
    v = torch.where(keys, v_cache.float(), torch.zeros((), device=dev))
    out = torch.einsum("bhtk,bhkd->bthd", prob, v)
    return out.reshape(B * T, heads * 64).to(qkv_new.dtype)


def check_sample_args(logits, seed, counter, temperature, top_k, top_p, vocab):
    """The argument conditions of ``sample_tokens``, shared by both backends -> (B, vocab)."""
    if logits.dim() != 2:
        raise ValueError("logits must be [B, ld]")
    B, ld = logits.shape
    V = ld if vocab is None else int(vocab)
    if not 0 < V <= ld:
        raise ValueError(f"vocab {V} outside (0, {ld}]")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p {top_p} outside (0, 1]")
    if top_k < 0:
        raise ValueError(f"top_k {top_k} is negative")
    if temperature < 0:
        raise ValueError(f"temperature {temperature} is negative")
    if not 0 <= int(seed) < 2 ** 31:
        raise ValueError(f"seed {seed} outside [0, 2^31)")
    if (not torch.is_tensor(counter) or counter.dtype != torch.int32
            or tuple(counter.shape) != (B,) or counter.device != logits.device):
        raise ValueError(f"counter must be int32 [{B}] on the logits' device")
    return B, V


def sample_details(logits, seed, counter, temperature=1.0, top_k=0, top_p=1.0, vocab=None,
                   math=torch.float32):
    """``sample_tokens`` with its intermediate quantities, in ``math`` precision on the logits
    rounded to bf16 (the values the device stores) -> dict: ``tokens`` [B], ``logprob`` [B],
    ``keep`` [B, V] (the final candidate set) and, when not greedy, ``keep_k`` [B, V] (what top-k
    kept) and per row ``Z`` (final mass),
    ``target`` (u Z), ``cdf_lo`` / ``cdf_hi`` (the running mass before / at the token), ``need``
    (top_p times the mass top-k kept), ``s_at`` / ``s_above`` (the upper mass at the top-p
    threshold key and at the next key above it; ``s_above`` is 0 at the largest key).

    The rule: 16-bit keys of the bf16 bits (negatives flipped, others with the sign bit set) carry
    the order; top-k keeps ``key >= k-th largest key``; top-p then keeps ``key >= t``, t the largest
    key whose upper mass ``sum{m : key >= t}`` reaches ``fp32(top_p)`` times the kept mass, with
    ``m = exp(z - zmax)``, ``z = x / temperature``; the token is the lowest kept index whose running
    mass in index order exceeds ``u Z``; ``logprob = z_tok - zmax - log Z``.  ``temperature == 0``:
    the lowest index of the largest key, its log-softmax over all classes at temperature 1."""
    B, V = check_sample_args(logits, seed, counter, temperature, top_k, top_p, vocab)
    xb = logits.detach()[:, :V].to(torch.bfloat16).contiguous()
    bits = xb.view(torch.int16).to(torch.int64) & 0xFFFF
    key = torch.where(bits >= 0x8000, ~bits & 0xFFFF, bits | 0x8000)
    x = xb.to(math)
    idx = torch.arange(V, device=x.device)
    if temperature == 0:
        top = key == key.max(1, keepdim=True).values
        tok = torch.where(top, idx, V).min(1).values
        lp = torch.log_softmax(x, 1).gather(1, tok.unsqueeze(1)).squeeze(1)
        return {"tokens": tok, "logprob": lp, "keep": torch.ones_like(top)}
    z = x / temperature
    zmax = z.max(1, keepdim=True).values
    m = torch.exp(z - zmax)
    u = sample_uniform(seed, counter).to(math)
    p32 = float(torch.tensor(top_p, dtype=torch.float32))
    out = {k: [] for k in ("tokens", "logprob", "keep", "keep_k", "Z", "target", "cdf_lo", "cdf_hi", "need",
                           "s_at", "s_above")}
    for b in range(B):
        k, mb = key[b], m[b]
        keep = torch.ones(V, dtype=torch.bool, device=x.device)
        if 0 < top_k < V:
            keep = k >= torch.topk(k, top_k).values[-1]
        need = p32 * (mb * keep).sum()
        out["keep_k"].append(keep)
        s_at, s_above = need / p32, torch.zeros((), dtype=math, device=x.device)
        if top_p < 1.0:
            uk, inv = torch.unique(k[keep], return_inverse=True)
            mass = torch.zeros(uk.numel(), dtype=math, device=x.device).index_add_(0, inv, mb[keep])
            upper = mass.flip(0).cumsum(0).flip(0)
            j = int(torch.nonzero(upper >= need).max())
            keep = keep & (k >= uk[j])
            s_at = upper[j]
            if j + 1 < uk.numel():
                s_above = upper[j + 1]
        mk = mb * keep
        cum = mk.cumsum(0)
        Z = cum[-1]
        hit = keep & (cum > u[b] * Z)
        tok = torch.where(hit, idx, V).min() if bool(hit.any()) else idx[keep].max()
        for name, v in (("tokens", tok), ("logprob", z[b, tok] - zmax[b, 0] - torch.log(Z)),
                        ("keep", keep), ("Z", Z), ("target", u[b] * Z), ("cdf_hi", cum[tok]),
                        ("cdf_lo", cum[tok] - mk[tok]), ("need", need), ("s_at", s_at),
                        ("s_above", s_above)):
            out[name].append(v)
    return {name: torch.stack(v) for name, v in out.items()}


def sample_tokens(logits, seed, counter, temperature=1.0, top_k=0, top_p=1.0, vocab=None):
    """One token per logits row -> (tokens int64 [B], logprob fp32 [B]); see ``sample_details``."""
    no_grad_op("sample_tokens", logits)
    d = sample_details(logits, seed, counter, temperature, top_k, top_p, vocab)
    return d["tokens"], d["logprob"].float()


def mlm_loss(logits, labels, weights=None, vocab=None):
    """sum_i w_i * nll_i / sum_i w_i  (google-research/bert run_pretraining.py).  ``vocab``: the
    class count when the logits rows are padded past it (columns from ``vocab`` on are ignored)."""
    if vocab is not None and vocab != logits.shape[-1]:
        logits = logits[..., :vocab]
    nll = F.cross_entropy(logits.float(), labels.reshape(-1).long(), reduction="none")
    if weights is None:
        return nll.mean()
    w = weights.reshape(-1).float()
    return (w * nll).sum() / w.sum().clamp_min(1e-5)


def eval_rows(logits, labels, vocab=None, loss_dtype=torch.float32):
    """Per-row evaluation loss and rank of the label: the oracle of the ``eval_rows`` kernel.

    ``loss_rows[i] = logsumexp(x_i) - x_i[label_i]`` in fp64 on the stored values (unsmoothed),
    returned as ``loss_dtype``; ``rank[i]`` (int32) is the stable descending rank of the label,

        rank = #{j : x_j > x_label} + #{j < label : x_j == x_label}

    so the label is in the top k iff ``rank < k``, ties included: among equal logits the lower
    index ranks first, which for k = 1 is ``torch.argmax``'s rule.  This is stricter than TF's
    ``in_top_k``, which counts strictly greater logits only and so admits every member of a tie
    at the k boundary.  ``vocab``: the class count when the rows are padded past it (columns from
    ``vocab`` on are not classes, whatever they hold).  A label outside ``[0, vocab)`` marks an
    ignored row (rank -1, loss 0); a NaN label logit is a miss (rank = vocab)."""
    if logits.dim() != 2:
        raise ValueError("logits must be [N, V]")
    N, ld = logits.shape
    V = ld if vocab is None else int(vocab)
    if not 0 < V <= ld:
        raise ValueError(f"eval_rows: vocab {vocab} outside the logits width {ld}")
    lab = labels.reshape(-1).long()
    if lab.numel() != N:
        raise ValueError(f"eval_rows: {lab.numel()} labels for {N} rows")
    loss = torch.zeros(N, dtype=torch.float64, device=logits.device)
    rank = torch.full((N,), -1, dtype=torch.int32, device=logits.device)
    cols = torch.arange(V, device=logits.device)
    step = max(1, (1 << 22) // V)                      # bounds the fp64 working set
    for r0 in range(0, N, step):
        x = logits[r0:r0 + step, :V].double()
        lb = lab[r0:r0 + step]
        ok = (lb >= 0) & (lb < V)
        xl = x.gather(1, lb.clamp(0, V - 1).unsqueeze(1))
        gt = (x > xl).sum(1)
        eq = ((x == xl) & (cols.unsqueeze(0) < lb.unsqueeze(1))).sum(1)
        rk = torch.where(torch.isnan(xl.squeeze(1)), torch.full_like(gt, V), gt + eq)
        rank[r0:r0 + step] = torch.where(ok, rk, torch.full_like(rk, -1)).to(torch.int32)
        ls = torch.logsumexp(x, 1) - xl.squeeze(1)
        loss[r0:r0 + step] = torch.where(ok, ls, torch.zeros_like(ls))
    return loss.to(loss_dtype), rank


def _augment_check(images, idx, boxes, flip, lut, out_hw, fill, mix=None):
    """Shared argument validation of ``augment_images`` and, with ``mix`` = (partner, lam_q,
    cut), of ``augment_mix_images`` (both backends) -> (B, Ho, Wo)."""
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] not in (1, 3):
        raise ValueError("augment_images: images must be uint8 [N, Hs, Ws, C] with C in {1, 3}")
    if not images.is_contiguous() or images.shape[0] < 1:
        raise ValueError("augment_images: images must be contiguous and non-empty")
    C = images.shape[3]
    Ho, Wo = (int(v) for v in out_hw)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"augment_images: output size {out_hw}")
    B = idx.numel()
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError("augment_images: idx must be int64 [B]")
    if boxes.dtype != torch.int32 or tuple(boxes.shape) != (B, 4):
        raise ValueError("augment_images: boxes must be int32 [B, 4] = (y0, x0, h, w)")
    if flip.dtype != torch.uint8 or tuple(flip.shape) != (B,):
        raise ValueError("augment_images: flip must be uint8 [B]")
    if tuple(lut.shape) != (C, 256) or lut.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("augment_images: lut must be bf16 / fp32 [C, 256]")
    if not 0 <= int(fill) <= 255:
        raise ValueError("augment_images: fill must be one byte")
    for t in (idx, boxes, flip, lut):
        if t.device != images.device:
            raise ValueError("augment_images: every argument lives on the images' device")
    if mix is not None:
        partner, lam_q, cut = mix
        if partner.dtype != torch.int32 or tuple(partner.shape) != (B,):
            raise ValueError("augment_mix_images: partner must be int32 [B]")
        if lam_q.dtype != torch.int32 or tuple(lam_q.shape) != (B,):
            raise ValueError("augment_mix_images: lam_q must be int32 [B]")
        if cut.dtype != torch.int32 or tuple(cut.shape) != (B, 4):
            raise ValueError("augment_mix_images: cut must be int32 [B, 4] = (oy0, ox0, h, w)")
        for t in mix:
            if t.device != images.device:
                raise ValueError("augment_mix_images: every argument lives on the images' device")
    return B, Ho, Wo


def _augment_axis(o, O, side):
    """Source position of output coordinates ``o`` [B, O] over box sides ``side`` [B] (int64):
    half-pixel centres with 8 fractional bits -> (i0, i1, f), each [B, O]."""
    side = side.unsqueeze(1)
    pos = torch.div((2 * o + 1) * side * 256, 2 * O, rounding_mode="floor") - 128
    pos = torch.minimum(pos.clamp(min=0), (side - 1) * 256)
    i0 = pos >> 8
    return i0, torch.minimum(i0 + 1, side - 1), pos & 255


def augment_images(images, idx, boxes, flip, lut, out_hw, fill=0):
    """Crop + bilinear resize + flip + per-channel normalisation of a gathered batch, in integer
    arithmetic: the oracle of the ``augment_images`` kernel (csrc/kernels/augment.hip) and the
    CPU path; both produce the same bits.

    ``images`` u8 [N, Hs, Ws, C]; ``idx`` int64 [B]; ``boxes`` int32 [B, 4] = (y0, x0, h, w) in
    source pixels, h, w >= 1, possibly reaching outside the image; ``flip`` u8 [B]; ``lut``
    [C, 256] in the output dtype.  Output [B, Ho, Wo, C].  For output pixel (b, oy, ox):

        ox' = Wo - 1 - ox if flip[b] else ox
        per axis: pos = floor((2 o + 1) * side * 256 / (2 O)) - 128 in [0, (side - 1) * 256],
                  i0 = pos >> 8, f = pos & 255, i1 = min(i0 + 1, side - 1)
        taps (y0 + iy, x0 + ix); a tap outside the image reads ``fill``
        v = ((256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11) + 32768) >> 16
        out = lut[c][v]

    i.e. TF's ``resize_bilinear(half_pixel_centers=True)`` without antialiasing, weights
    quantised to 1/256; a box of the output's size is an exact copy through the table."""
    _augment_check(images, idx, boxes, flip, lut, out_hw, fill)
    v = _augment_v(images, idx, boxes, flip, out_hw, fill)
    return lut[torch.arange(images.shape[3], device=images.device).view(1, 1, 1, -1), v.long()]


def _augment_v(images, idx, boxes, flip, out_hw, fill):
    """The resampled 8-bit value ``v`` of the rule of ``augment_images`` -> int32
    [B, Ho, Wo, C] (checked arguments)."""
    B, (Ho, Wo) = idx.numel(), (int(v) for v in out_hw)
    N, Hs, Ws, C = images.shape
    dev = images.device
    if B and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise ValueError("augment_images: index outside the image set")
    bx = boxes.long()
    y0, x0, bh, bw = bx[:, 0:1], bx[:, 1:2], bx[:, 2], bx[:, 3]
    oy = torch.arange(Ho, device=dev).unsqueeze(0).expand(B, Ho)
    ox = torch.arange(Wo, device=dev).unsqueeze(0).expand(B, Wo)
    ox = torch.where(flip.bool().unsqueeze(1), Wo - 1 - ox, ox)
    iy0, iy1, fy = _augment_axis(oy, Ho, bh)
    ix0, ix1, fx = _augment_axis(ox, Wo, bw)
    n = idx.view(B, 1, 1)

    def tap(iy, ix):
        ty, tx = (y0 + iy).unsqueeze(2), (x0 + ix).unsqueeze(1)           # [B, Ho, 1], [B, 1, Wo]
        ok = (ty >= 0) & (ty < Hs) & (tx >= 0) & (tx < Ws)
        p = images[n, ty.clamp(0, Hs - 1), tx.clamp(0, Ws - 1)]           # [B, Ho, Wo, C]
        return torch.where(ok.unsqueeze(3), p, p.new_tensor(int(fill))).to(torch.int32)

    fy = fy.to(torch.int32).view(B, Ho, 1, 1)
    fx = fx.to(torch.int32).view(B, 1, Wo, 1)
    top = (256 - fx) * tap(iy0, ix0) + fx * tap(iy0, ix1)
    bot = (256 - fx) * tap(iy1, ix0) + fx * tap(iy1, ix1)
    return ((256 - fy) * top + fy * bot + 32768) >> 16


def augment_mix_images(images, idx, boxes, flip, lut, out_hw, partner, lam_q, cut, fill=0):
    """``augment_images`` with row b mixed with row ``p = partner[b]`` of the same batch (Mixup /
    CutMix), in the 8-bit pixel domain: the oracle of the ``augment_mix_images`` kernel and the
    CPU path; both produce the same bits.

    ``partner`` int32 [B]; ``lam_q`` int32 [B], the weight of row b in 1/65536; ``cut`` int32
    [B, 4] = (oy0, ox0, h, w) in output pixels, clipped to the output, h <= 0 or w <= 0: no box.
    With vA the ``v`` of ``augment_images`` for row b and vB the one for row p (p's own index,
    box and flip) at the same output pixel, and q = clamp(lam_q[b], 0, 65536):

        v = vB if oy0 <= oy < oy0 + h and ox0 <= ox < ox0 + w
            else (q vA + (65536 - q) vB + 32768) >> 16
        out = lut[c][v]

    The table is affine and the weights sum to 1, so this is the mix of the normalised images at
    the precision of the source.  q = 65536 without a box is ``augment_images`` to the bit, q = 0
    the partner's row; a row that is its own partner is unmixed.  A partner outside [0, B)
    raises here (the kernel, which cannot, leaves the row unmixed)."""
    B, Ho, Wo = _augment_check(images, idx, boxes, flip, lut, out_hw, fill,
                               (partner, lam_q, cut))
    dev = images.device
    if B and (int(partner.min()) < 0 or int(partner.max()) >= B):
        raise ValueError("augment_mix_images: partner outside the batch")
    va = _augment_v(images, idx, boxes, flip, out_hw, fill)
    vb = va[partner.long()]                   # row p at the same output pixel
    q = lam_q.clamp(0, 65536).view(B, 1, 1, 1)
    c = cut.long()
    oy = torch.arange(Ho, device=dev).view(1, Ho, 1)
    ox = torch.arange(Wo, device=dev).view(1, 1, Wo)
    y0, x0, h, w = (c[:, i].view(B, 1, 1) for i in range(4))
    inside = (oy >= y0) & (oy < y0 + h) & (ox >= x0) & (ox < x0 + w) & (h > 0) & (w > 0)
    v = torch.where(inside.unsqueeze(3), vb, (q * va + (65536 - q) * vb + 32768) >> 16)
    return lut[torch.arange(images.shape[3], device=dev).view(1, 1, 1, -1), v.long()]


RAND_MAX_SIDE = 1024          # the kernel's axis tables hold every output row and column
RAND_MAX_LAYERS = 4
RAND_IDENTITY = (65536, 0, 0, 0, 65536, 0)
# pointwise op codes of augment_rand_images and the inclusive range of each one's parameter
RAND_NONE, RAND_INVERT, RAND_SOLARIZE, RAND_SOLARIZE_ADD, RAND_POSTERIZE, RAND_BRIGHTNESS, \
    RAND_COLOR = range(7)
RAND_PARAM_RANGE = {RAND_SOLARIZE: (0, 256), RAND_SOLARIZE_ADD: (0, 128), RAND_POSTERIZE: (0, 255),
                    RAND_BRIGHTNESS: (0, 1 << 18), RAND_COLOR: (0, 1 << 18)}


def _augment_rand_check(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, partner, lam_q,
                        cut, fill, ra_fill):
    """Shared argument validation of ``augment_rand_images`` (both backends) -> (B, Ho, Wo, L)."""
    mix = (partner, lam_q, cut)
    if any(t is None for t in mix) and not all(t is None for t in mix):
        raise ValueError("augment_rand_images: partner, lam_q and cut are all given or all None")
    B, Ho, Wo = _augment_check(images, idx, boxes, flip, lut, out_hw, fill,
                               None if partner is None else mix)
    if Ho > RAND_MAX_SIDE or Wo > RAND_MAX_SIDE:
        raise ValueError(f"augment_rand_images: output sides are at most {RAND_MAX_SIDE}")
    if aff.dtype != torch.int32 or tuple(aff.shape) != (B, 6):
        raise ValueError("augment_rand_images: aff must be int32 [B, 6] = (a, b, c, d, e, f)")
    if pops.dtype != torch.int32 or pops.dim() != 2 or pops.shape[0] != B:
        raise ValueError("augment_rand_images: pops must be int32 [B, L]")
    L = pops.shape[1]
    if not 1 <= L <= RAND_MAX_LAYERS:
        raise ValueError(f"augment_rand_images: {L} layers outside [1, {RAND_MAX_LAYERS}]")
    if ppar.dtype != torch.int32 or tuple(ppar.shape) != (B, L):
        raise ValueError("augment_rand_images: ppar must be int32 [B, L]")
    for t in (aff, pops, ppar):
        if t.device != images.device:
            raise ValueError("augment_rand_images: every argument lives on the images' device")
        if not t.is_contiguous():
            raise ValueError("augment_rand_images: aff, pops and ppar must be contiguous")
    if not 0 <= int(ra_fill) <= 255:
        raise ValueError("augment_rand_images: ra_fill must be one byte")
    return B, Ho, Wo, L


def _augment_rand_v(images, idx, boxes, flip, out_hw, aff, pops, ppar, fill, ra_fill):
    """Steps 1 and 2 of the rule of ``augment_rand_images`` (the map and the pointwise chain) ->
    int32 [B, Ho, Wo, C] (checked arguments)."""
    B, (Ho, Wo) = idx.numel(), (int(v) for v in out_hw)
    C, dev = images.shape[3], images.device
    virt = _augment_v(images, idx, boxes, flip, out_hw, fill)
    a, b, c, d, e, f = (aff[:, i].long().view(B, 1, 1) for i in range(6))
    X = 2 * torch.arange(Wo, device=dev).view(1, 1, Wo) + 1
    Y = 2 * torch.arange(Ho, device=dev).view(1, Ho, 1) + 1
    u = (a * X + b * Y + 2 * c) >> 17
    v = (d * X + e * Y + 2 * f) >> 17
    inside = (u >= 0) & (u < Wo) & (v >= 0) & (v < Ho)
    rows = torch.arange(B, device=dev).view(B, 1, 1)
    x = virt[rows, v.clamp(0, Ho - 1), u.clamp(0, Wo - 1)]               # [B, Ho, Wo, C]
    x = torch.where(inside.unsqueeze(3), x, x.new_tensor(int(ra_fill)))
    for k in range(pops.shape[1]):
        code = pops[:, k].view(B, 1, 1, 1)
        m = ppar[:, k].view(B, 1, 1, 1)
        y = torch.where(code == RAND_INVERT, 255 - x, x)
        y = torch.where(code == RAND_SOLARIZE, torch.where(x < m, x, 255 - x), y)
        y = torch.where(code == RAND_SOLARIZE_ADD,
                        torch.where(x < 128, (x + m).clamp(max=255), x), y)
        y = torch.where(code == RAND_POSTERIZE, x & m, y)
        y = torch.where(code == RAND_BRIGHTNESS, ((x * m) >> 16).clamp(0, 255), y)
        if C == 3:
            g = (19595 * x[..., 0:1] + 38470 * x[..., 1:2] + 7471 * x[..., 2:3] + 32768) >> 16
            y = torch.where(code == RAND_COLOR, ((65536 * g + m * (x - g)) >> 16).clamp(0, 255), y)
        x = y
    return x


def augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, partner=None,
                        lam_q=None, cut=None, fill=0, ra_fill=128):
    """``augment_images`` / ``augment_mix_images`` with RandAugment: per row an output -> input
    affine map and a chain of pointwise ops, in integer arithmetic: the oracle of the
    ``augment_rand_images`` kernel and the CPU path; both produce the same bits.

    ``aff`` int32 [B, 6] = (a, b, c, d, e, f) in Q16; ``pops`` / ``ppar`` int32 [B, L], the op
    codes and their parameters, 1 <= L <= 4.  Let V_b(v, u) be the ``v`` of ``augment_images``
    for row b at output pixel (oy = v, ox = u) (the row's virtual image).  For output pixel
    (b, oy, ox):

        U = a (2 ox + 1) + b (2 oy + 1) + 2 c,  W = d (2 ox + 1) + e (2 oy + 1) + 2 f    (int64)
        u = U >> 17, v = W >> 17          (floor: PIL's nearest-neighbour affine transform on
                                           pixel centres; (65536, 0, 0, 0, 65536, 0) is u = ox,
                                           v = oy)
        x_c = V_b(v, u)[c] if 0 <= u < Wo and 0 <= v < Ho else ra_fill
        for k = 0 .. L - 1, with m = ppar[b, k] and code pops[b, k]:
            0 none         x
            1 Invert       255 - x
            2 Solarize     x if x < m else 255 - x                      m in [0, 256]
            3 SolarizeAdd  min(255, x + m) if x < 128 else x            m in [0, 128]
            4 Posterize    x & m                                        m a byte mask
            5 Brightness   clamp((x m) >> 16, 0, 255)                   m = factor in Q16 <= 2^18
            6 Color        C = 3: g = (19595 x_0 + 38470 x_1 + 7471 x_2 + 32768) >> 16 (PIL's L),
                           x_c = clamp((65536 g + m (x_c - g)) >> 16, 0, 255); C = 1: x
        with a partner: the mix of ``augment_mix_images`` of this value for row b and for row
        p = partner[b] (p's own index, box, flip, aff, pops and ppar) at the same output pixel
        out = lut[c][value]

    The identity map with all-zero ``pops`` is ``augment_images`` (with a partner
    ``augment_mix_images``) to the bit.  A code outside 0..6 or a parameter outside its range
    raises here (the kernel treats an unknown code as none and clamps the parameters)."""
    B, Ho, Wo, L = _augment_rand_check(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar,
                                       partner, lam_q, cut, fill, ra_fill)
    dev = images.device
    if B and (int(pops.min()) < 0 or int(pops.max()) > RAND_COLOR):
        raise ValueError("augment_rand_images: op code outside 0..6")
    for code, (lo, hi) in RAND_PARAM_RANGE.items():
        m = ppar[pops == code]
        if m.numel() and (int(m.min()) < lo or int(m.max()) > hi):
            raise ValueError(f"augment_rand_images: parameter of op {code} outside [{lo}, {hi}]")
    if partner is not None and B and (int(partner.min()) < 0 or int(partner.max()) >= B):
        raise ValueError("augment_rand_images: partner outside the batch")
    v = _augment_rand_v(images, idx, boxes, flip, out_hw, aff, pops, ppar, fill, ra_fill)
    if partner is not None:
        va, vb = v, v[partner.long()]             # row p at the same output pixel
        q = lam_q.clamp(0, 65536).view(B, 1, 1, 1)
        c = cut.long()
        oy = torch.arange(Ho, device=dev).view(1, Ho, 1)
        ox = torch.arange(Wo, device=dev).view(1, 1, Wo)
        y0, x0, h, w = (c[:, i].view(B, 1, 1) for i in range(4))
        inside = (oy >= y0) & (oy < y0 + h) & (ox >= x0) & (ox < x0 + w) & (h > 0) & (w > 0)
        v = torch.where(inside.unsqueeze(3), vb, (q * va + (65536 - q) * vb + 32768) >> 16)
    return lut[torch.arange(images.shape[3], device=dev).view(1, 1, 1, -1), v.long()]


MLM_MAX_SEQ = 512


def _mlm_check(tokens, idx, seed, max_predictions, masking):
    """Shared argument validation of ``mlm_mask_tokens`` (both backends) -> (B, S, P, rule) with
    ``rule = [vocab_size, pad_id, cls_id, sep_id, mask_id, random_low, prob_q16]``."""
    if tokens.dim() != 2 or tokens.dtype not in (torch.uint16, torch.int16, torch.int32):
        raise ValueError("mlm_mask_tokens: tokens must be [N, S], 16-bit or int32 storage")
    if not tokens.is_contiguous() or tokens.shape[0] < 1:
        raise ValueError("mlm_mask_tokens: tokens must be contiguous and non-empty")
    S, P = tokens.shape[1], int(max_predictions)
    if not 1 <= S <= MLM_MAX_SEQ:
        raise ValueError(f"mlm_mask_tokens: sequence length {S} outside [1, {MLM_MAX_SEQ}]")
    if not 1 <= P <= S:
        raise ValueError(f"mlm_mask_tokens: max_predictions {P} outside [1, {S}]")
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError("mlm_mask_tokens: idx must be int64 [B]")
    if idx.device != tokens.device:
        raise ValueError("mlm_mask_tokens: idx lives on the tokens' device")
    if not 0 <= int(seed) < (1 << 32):
        raise ValueError("mlm_mask_tokens: seed must be in [0, 2^32)")
    V = int(masking.vocab_size)
    if V < 1 or V > (1 << 31) or (tokens.element_size() == 2 and V > 65536):
        raise ValueError(f"mlm_mask_tokens: vocab_size {V} does not fit the token storage")
    for name in ("pad_id", "cls_id", "sep_id", "mask_id", "random_low"):
        if not 0 <= int(getattr(masking, name)) < V:
            raise ValueError(f"mlm_mask_tokens: {name} outside the vocabulary")
    q = int(masking.prob_q16)
    if not 0 <= q <= 65536:
        raise ValueError("mlm_mask_tokens: prob must be in [0, 1]")
    rule = [V, int(masking.pad_id), int(masking.cls_id), int(masking.sep_id),
            int(masking.mask_id), int(masking.random_low), q]
    return idx.numel(), S, P, rule


def _mlm_continuation_check(continuation, tokens, rule):
    """Shared validation of the whole-word table (both backends): uint8 or bool ``[vocab_size]``,
    contiguous, on the tokens' device, values 0 / 1, the four special ids not flagged.  The two
    value checks read the table, which on a GPU waits for the device; they run once per table
    (and again after an in-place write to it) and are remembered on the tensor, so a training
    step does not wait."""
    V, pad, cls, sep, mask_id = rule[:5]
    if not isinstance(continuation, torch.Tensor) or \
            continuation.dtype not in (torch.uint8, torch.bool):
        raise ValueError("mlm_mask_tokens: continuation must be a uint8 or bool tensor")
    if continuation.dim() != 1 or continuation.shape[0] != V:
        raise ValueError(f"mlm_mask_tokens: continuation of shape {tuple(continuation.shape)}, "
                         f"expected [{V}] (vocab_size)")
    if not continuation.is_contiguous() or continuation.device != tokens.device:
        raise ValueError("mlm_mask_tokens: continuation must be contiguous and on the tokens' "
                         "device")
    seen = (continuation._version, continuation.data_ptr(), pad, cls, sep, mask_id)
    if getattr(continuation, "_mlm_checked", None) == seen:
        return
    table = continuation.view(torch.uint8)
    if int(table.max()) > 1:
        raise ValueError("mlm_mask_tokens: continuation holds a value above 1")
    special = torch.tensor([pad, cls, sep, mask_id], device=table.device)
    if int(table[special].max()) != 0:
        raise ValueError("mlm_mask_tokens: continuation flags one of pad_id, cls_id, sep_id, "
                         "mask_id")
    continuation._mlm_checked = seen


def _mlm_select_words(t, cand, key, T, continuation, V):
    """The whole-word choice of ``mlm_mask_tokens`` -> (selected positions [B, S], T' [B])."""
    B, S = t.shape
    dev = t.device
    j = torch.arange(S, device=dev).unsqueeze(0)
    table = continuation.view(torch.uint8)
    piece = cand & (t < V) & (table[t.clamp(max=V - 1)] != 0)
    after = torch.cat([torch.zeros(B, 1, dtype=torch.bool, device=dev), cand[:, :-1]], 1)
    start = cand & ~(piece & after)
    nw = start.sum(1)
    # words are numbered in position order; column S collects what belongs to none
    word = torch.where(cand, start.cumsum(1) - 1, torch.full_like(t, S))
    length = torch.zeros(B, S + 1, dtype=torch.int64, device=dev)
    length.scatter_add_(1, word, torch.ones_like(t))
    pair = torch.full((B, S + 1), 1 << 62, dtype=torch.int64, device=dev)
    pair.scatter_(1, torch.where(start, word, torch.full_like(t, S)), key * 1024 + j)
    order = pair[:, :S].argsort(1)                        # the words in visiting order
    length = length[:, :S].gather(1, order)
    taken = torch.zeros_like(nw)
    fits = torch.zeros(B, S, dtype=torch.bool, device=dev)
    for k in range(int(nw.max()) if B else 0):            # the greedy fill, rank by rank
        ok = (k < nw) & (taken < T) & (taken + length[:, k] <= T)
        taken = taken + torch.where(ok, length[:, k], torch.zeros_like(taken))
        fits[:, k] = ok
    chosen = torch.zeros(B, S + 1, dtype=torch.bool, device=dev)
    chosen.scatter_(1, order, fits)
    chosen[:, S] = False
    return chosen.gather(1, word), taken


def mlm_mask_tokens(tokens, idx, seed, max_predictions, masking, example_stride=1,
                    example_offset=0, continuation=None):
    """Masked-LM example creation for a gathered batch of token rows, in integer arithmetic: the
    oracle of the ``mlm_mask_tokens`` kernel (csrc/kernels/mlm_mask.hip) and the CPU path; both
    produce the same bits.

    ``tokens`` [N, S] (uint16 / int16 / int32 storage, read unsigned); ``idx`` int64 [B];
    ``seed`` in [0, 2^32); ``masking`` a :class:`data.TokenMasking`.  -> dict of ``input_ids``,
    ``segment_ids``, ``input_mask`` (int64 [B, S]), ``masked_lm_positions``, ``masked_lm_ids``
    (int64 [B, P]) and ``masked_lm_weights`` (fp32 [B, P]).  Row b reads example ``idx[b]`` and
    keys its hashes on the example number ``n = example_offset + idx[b] * example_stride`` (a
    shard of a set passes its global numbers).  All hashes are uint32, ``t[j]`` the stored token:

        row_seed = fmix32(lo32(n) * 0x9E3779B1 + seed) ^ hi32(n)
        key[j]   = fmix32(j * 0x9E3779B1 + row_seed)
        input_mask[j]  = t[j] != pad_id
        segment_ids[j] = input_mask[j] and j > (index of the first sep_id); no sep_id: all 0
        candidates: t[j] not in {pad_id, cls_id, sep_id}; nc of them
        T = 0 if nc == 0 else min(P, nc, max(1, (nc * prob_q16 + 32768) >> 16))
        selected: the T candidates with the smallest (key[j], j), listed in ascending j:
            slot s < T: positions = j, ids = t[j], weights = 1;  slots s >= T: 0, 0, 0.0
        at a selected j: h2 = fmix32(key[j] + 0x85EBCA6B), d = ((h2 & 0xFFFF) * 10) >> 16
            d < 8: mask_id;  d == 8: t[j];
            d == 9: random_low + ((fmix32(h2 + 0x9E3779B1) * (vocab_size - random_low)) >> 32)
        every other position copies t[j]

    An ``idx[b]`` outside [0, N) yields an all-pad row with weights 0.

    Whole-word masking: ``continuation`` is a uint8 / bool table [vocab_size] with 1 at the
    continuation pieces of the vocabulary (WordPiece's ``##...``; pad_id, cls_id, sep_id and
    mask_id must be 0; an id past the table is no continuation).  Everything above holds but
    the choice of the selected positions, which becomes create_pretraining_data.py's
    ``--do_whole_word_mask``:

        candidate j starts a word iff continuation[t[j]] == 0, or j == 0, or j - 1 is no
            candidate; otherwise it belongs to the word of the nearest start below it
        words are visited in ascending (key[start], start); taken = 0; for each word:
            stop if taken >= T;  skip the word if taken + len(word) > T;
            else select every token of the word and add len(word) to taken
        T' = taken (<= T; 0 when every word is longer than T); T == nc selects everything
        the selected positions are listed in ascending j in the slots s < T'; slots s >= T' hold
            0, 0, 0.0; each selected token draws its own 80 / 10 / 10 from its own key[j]

    An all-zero table is the token rule to the bit.  Two differences from the script: the budget
    is formed from ``nc`` as above (not from the row's length), and a continuation piece that does
    not directly follow a candidate starts a word of its own (the script would glue it to the
    last word across a ``[SEP]``; well-formed WordPiece rows hold no such piece)."""
    B, S, P, rule = _mlm_check(tokens, idx, seed, max_predictions, masking)
    if continuation is not None:
        _mlm_continuation_check(continuation, tokens, rule)
    V, pad, cls, sep, mask_id, low, q = rule
    N, dev = tokens.shape[0], tokens.device
    store = tokens.view(torch.int16) if tokens.dtype == torch.uint16 else tokens
    ok = (idx >= 0) & (idx < N)
    t = store.index_select(0, idx.clamp(0, N - 1)).long() & ((1 << (8 * store.element_size())) - 1)
    t = torch.where(ok.unsqueeze(1), t, torch.full_like(t, pad))
    n = idx * int(example_stride) + int(example_offset)                 # wraps like uint64
    row_seed = _fmix32(((n & _M32) * 0x9E3779B1 + int(seed)) & _M32) ^ ((n >> 32) & _M32)
    j = torch.arange(S, device=dev).unsqueeze(0)
    key = _fmix32((j * 0x9E3779B1 + row_seed.unsqueeze(1)) & _M32)       # [B, S]

    real = t != pad
    is_sep = t == sep
    first = torch.where(is_sep.any(1), torch.argmax(is_sep.to(torch.uint8), 1),
                        torch.full_like(idx, S))
    segment = real & (j > first.unsqueeze(1))
    cand = real & (t != cls) & (t != sep)
    nc = cand.sum(1)
    T = torch.minimum(torch.clamp((nc * q + 32768) >> 16, min=1), nc).clamp(max=P)
    if continuation is None:
        # (key, j) pairs as one integer; no candidate ranks below nc, so none is ever selected
        pair = torch.where(cand, key * 1024 + j, torch.full_like(key, 1 << 62))
        rank = torch.empty_like(pair)
        rank.scatter_(1, pair.argsort(1), j.expand(B, S).contiguous())
        sel = cand & (rank < T.unsqueeze(1))
    else:
        sel, T = _mlm_select_words(t, cand, key, T, continuation, V)

    h2 = _fmix32((key + 0x85EBCA6B) & _M32)
    d = ((h2 & 0xFFFF) * 10) >> 16
    rnd = low + ((_fmix32((h2 + 0x9E3779B1) & _M32) * (V - low)) >> 32)
    new = torch.where(d < 8, torch.full_like(t, mask_id), torch.where(d == 8, t, rnd))
    input_ids = torch.where(sel, new, t)

    # slot of a selected position: the selected positions below it; the rest land in a spare column
    slot = torch.where(sel, sel.cumsum(1) - 1, torch.full_like(t, P))
    positions = torch.zeros(B, P + 1, dtype=torch.int64, device=dev)
    positions.scatter_(1, slot, j.expand(B, S).contiguous())
    ids = torch.zeros(B, P + 1, dtype=torch.int64, device=dev).scatter_(1, slot, t)
    weights = (torch.arange(P, device=dev).unsqueeze(0) < T.unsqueeze(1)).float()
    return {"input_ids": input_ids, "segment_ids": segment.long(), "input_mask": real.long(),
            "masked_lm_positions": positions[:, :P].contiguous(),
            "masked_lm_ids": ids[:, :P].contiguous(), "masked_lm_weights": weights}


def space_to_depth_operands(x, w, stride, pad, want_x=True):
    """Rewrite a strided conv (the ResNet stem: 7x7 / 2, pad 3, C = 3) as a stride-1 VALID conv
    on the space-to-depth input.  Output pixel p reads padded input rows s*p + r, r < R; with
    r = s*i + a that is row p + i of the s2d image at sub-row a, so

        x' [N, P + R' - 1, Q + S' - 1, s*s*C']  (C' = C zero-padded so s*s*C' % 8 == 0)
        w' [K, R', S', s*s*C']                  (R' = ceil(R / s), taps past R are zero)

    compute exactly the original conv.  For the stem: 16 taps x 16 channels = K 256 of which
    147 are real (vs 49 taps x 8 padded channels = 392), and whole 32-B tap rows per pixel.
    Both rewrites are differentiable torch views/pads (w' keeps autograd back to the master).
    ``want_x=False`` skips x' (returned as None) for callers with a native layout kernel."""
    n, h, wd, c = x.shape
    K, R, S, C = w.shape
    s = stride
    P = (h + 2 * pad - R) // s + 1
    Q = (wd + 2 * pad - S) // s + 1
    Rp, Sp = -(-R // s), -(-S // s)
    cp = c
    while (s * s * cp) % 8:
        cp += 1
    Hn, Wn = s * (P + Rp - 1), s * (Q + Sp - 1)
    wp = torch.nn.functional.pad(w, (0, cp - C, 0, s * Sp - S, 0, s * Rp - R))
    ws = wp.view(K, Rp, s, Sp, s, cp).permute(0, 1, 3, 2, 4, 5).reshape(K, Rp, Sp, s * s * cp)
    if not want_x:
        return None, ws
    xp = torch.nn.functional.pad(x, (0, cp - c, pad, Wn - wd - pad, pad, Hn - h - pad))
    xs = xp.view(n, Hn // s, s, Wn // s, s, cp).permute(0, 1, 3, 2, 4, 5).reshape(
        n, Hn // s, Wn // s, s * s * cp)
    return xs.contiguous(), ws


def ema_update(avg, var, a_dev):
    """tf.train.ExponentialMovingAverage's update in place, in fp32 and in the kernel's operation
    order: ``avg = avg - a * (avg - var)`` with ``a = 1 - decay`` the one-element fp32 tensor
    ``a_dev``.  ``avg == var`` is a bit-exact fixed point."""
    with torch.no_grad():
        avg.sub_(a_dev.reshape(()) * (avg - var))
    return avg


def grad_accumulate(dst, src, add):
    """Gradient accumulation's pass in place: ``dst = src``, or ``dst = dst + src`` (one fp32 add
    per element) when ``add``."""
    with torch.no_grad():
        if add:
            dst.add_(src)
        else:
            dst.copy_(src)
    return dst
