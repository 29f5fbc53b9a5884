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


def dense(x, w, b=None, relu=False):
    """x: [M, in]; w: [out, in] (GEMM 'NT' layout); b: [out]."""
    y = F.linear(x, w.to(x.dtype), None if b is None else b.to(x.dtype))
    return torch.relu(y) if relu else y


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
