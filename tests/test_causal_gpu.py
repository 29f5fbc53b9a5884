"""Causal flash attention on the device: the CAUSAL instantiations of attn_fwd_kernel,
attn_bwd_dq_kernel and attn_bwd_dkv_kernel, the op, the causal BERT and the causal token batches.

Query q sees key k iff k <= q, on top of the additive key mask.  The kernels skip every 64-key
tile above the diagonal and select the hidden scores of the diagonal tile to -inf (forward) or
their p to an exact 0 (backward).  The checks:

  1. out, lse, delta and the three thirds of dqkv against fp64 with the per-element bounds of
     tests/test_nlp_kernels_gpu.py (same gamma terms: a causal row sums fewer terms, so they stay
     upper bounds; the score magnitude that enters them is taken over the visible keys only,
     which is tighter).  The oracle reads the stored bf16 O and fp32 lse, as there.
  2. the last row (it sees every key, in the same order) is bit-identical to the non-causal call;
  3. the <8,128> and <4,64> shapes are bit-identical to each other;
  4. a change at positions >= j leaves rows < j bit-identical;
  5. NaN planted in the tiles that must be skipped never reaches the rows that skip them (a
     kernel that loads such a tile and only masks it turns 0 * NaN into NaN);
  6. causal with a keep buffer or column partials raises, and the op asks for neither;
  7. the op and a tiny causal BERT against the reference path, and a captured step;
  8. the causal token batches on the device against their CPU twin.
"""
import copy
import math

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.ops import reference as R
from test_nlp_kernels_gpu import (AD, ALLOW, BF16, INTR, LN2, LOG2E, SENT, U16, U32, _attn_idx,
                                  _attn_inputs, _attn_switches, _dev, _gen, _heads, _inv_keep,
                                  _K, _keep, _measure, _p, _ratio, _rows, _run_attn, _scores,
                                  _split_qkv, _st, assert_within, gamma)


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# (S, wide): one diagonal tile; one 128-key chunk with the wave-level skip; three 64-key chunks
# with the block-level skip and the diagonal in every position; two 128-key chunks
PATHS = [(64, 1), (128, 1), (128, 0), (192, 1), (256, 1), (256, 0)]
B, H, SCALE = 2, 3, AD ** -0.5


def _vis(S):
    return torch.ones(S, S, dtype=torch.bool).tril()


def causal_fwd_oracle(qkv, mask, B, S, H, scale, p, seed):
    """attn_fwd_oracle with the [S, S] -inf select above the diagonal."""
    q, k, v = _split_qkv(qkv, B, S, H)
    s2, smag = _scores(q, k, mask, B, S, scale)
    vis = _vis(S)
    s2 = torch.where(vis, s2, torch.full_like(s2, float("-inf")))
    smag = torch.where(vis, smag, torch.zeros_like(smag))
    smax = smag.max(-1, keepdim=True).values
    m = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    keep = _keep(seed, _attn_idx(B, H, S), p)
    Pd = torch.where(keep, P * _inv_keep(p), torch.zeros_like(P))
    out, mag = Pd @ v, Pd @ v.abs()
    rel32 = gamma(S + 8) + 2 * LN2 * gamma(70) * smax + 2 * INTR
    lse = (m + torch.log2(l))[..., 0]
    lunit = U32 * (m.abs() + torch.log2(l))[..., 0]
    lb = gamma(70) * smax[..., 0] + gamma(S) / LN2 + ALLOW["lse"] * lunit
    return {"out": (_rows(out, B, S, H), _rows((2 * U16 + rel32) * mag, B, S, H)),
            "lse": (lse.reshape(-1), lb.reshape(-1)), "lse_unit": lunit.reshape(-1)}


def causal_fwd_emulate(qkv, mask, B, S, H, scale, p, seed, strict=False):
    """fp32 arithmetic with bf16 where the kernel rounds.  ``strict``: the diagonal shifted by one
    (k < q; row 0 keeps key 0 so that it stays finite) -- the bound must reject it."""
    x = qkv.float().view(B, S, 3, H, AD)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s2 = q @ k.transpose(-1, -2) * c
    if mask is not None:
        s2 = s2 + (mask.float() * torch.tensor(LOG2E, dtype=torch.float32)).view(B, 1, 1, S)
    vis = _vis(S)
    if strict:
        vis = torch.ones(S, S, dtype=torch.bool).tril(-1)
        vis[0, 0] = True
    s2 = torch.where(vis, s2, torch.full_like(s2, float("-inf")))
    e = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    keep = _keep(seed, _attn_idx(B, H, S), p)
    ik = torch.tensor(_inv_keep(p), dtype=torch.float32)
    pd = torch.where(keep, e * ik, torch.zeros_like(e)).to(BF16).float()
    return _rows((pd @ v) * (1.0 / l), B, S, H).to(BF16)


def causal_bwd_oracle(qkv, mask, dO, O, lse, B, S, H, scale, p, seed):
    """attn_bwd_oracle with the same select: fp64 backward of what the kernels read."""
    q, k, v = _split_qkv(qkv, B, S, H)
    s2, smag = _scores(q, k, mask, B, S, scale)
    s2 = torch.where(_vis(S), s2, torch.full_like(s2, float("-inf")))
    L = lse.double().view(B, H, S, 1)
    P = torch.exp2(s2 - L)
    dOh, Oh = _heads(dO, B, S, H), _heads(O, B, S, H)
    delta = (Oh * dOh).sum(-1, keepdim=True)
    dmag = (Oh * dOh).abs().sum(-1, keepdim=True)
    keep = _keep(seed, _attn_idx(B, H, S), p)
    ik = _inv_keep(p)
    zero = torch.zeros_like(P)
    Pd = torch.where(keep, P * ik, zero)
    dPd = torch.where(keep, dOh @ v.transpose(-1, -2) * ik, zero)
    dPm = torch.where(keep, dOh.abs() @ v.abs().transpose(-1, -2) * ik, zero)
    dS, dSm = P * (dPd - delta), P * (dPm + dmag)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    live = P > 0                       # a hidden or masked key: P exactly 0 on both sides
    relP = LN2 * gamma(72) * float((smag + L.abs())[live].max()) + INTR
    T = lambda t: t.transpose(-1, -2)
    dV, mV = T(Pd) @ dOh, T(Pd) @ dOh.abs()
    dK, mK, mK2 = sc * T(dS) @ q, sc * T(dS.abs()) @ q.abs(), sc * T(dSm) @ q.abs()
    dQ, mQ, mQ2 = sc * dS @ k, sc * dS.abs() @ k.abs(), sc * dSm @ k.abs()
    r2 = gamma(S + 72) + relP + 2 * U32
    ref = torch.cat([_rows(t, B, S, H) for t in (dQ, dK, dV)], 1)
    bnd = torch.cat([_rows(t, B, S, H) for t in
                     (2 * U16 * mQ + r2 * mQ2, 2 * U16 * mK + r2 * mK2,
                      (2 * U16 + gamma(S + 4) + relP) * mV)], 1)
    return {"dqkv": (ref, bnd), "delta": (delta.reshape(-1), gamma(66) * dmag.reshape(-1))}


def _run_causal(qkv, mask, dO, B, S, H, scale, p, seed):
    """Causal attn_fwd then attn_bwd on the GPU -> dict of CPU tensors."""
    K = _K()
    qd, md, dod = _dev(qkv), _dev(mask), _dev(dO)
    out = torch.full((B * S, H * AD), SENT, device="cuda", dtype=BF16)
    lse = torch.full((B * H * S,), SENT, device="cuda")
    K.attn_fwd(qd.data_ptr(), _p(md), out.data_ptr(), lse.data_ptr(), B, S, H, float(scale),
               float(p), seed, _st(), 0, causal=1)
    dqkv = torch.full_like(qd, SENT)
    delta = torch.full_like(lse, SENT)
    K.attn_bwd(qd.data_ptr(), _p(md), out.data_ptr(), dod.data_ptr(), lse.data_ptr(),
               delta.data_ptr(), dqkv.data_ptr(), B, S, H, float(scale), float(p), seed, _st(),
               0, 0, causal=1)
    torch.cuda.synchronize()
    return {"out": out.cpu(), "lse": lse.cpu(), "dqkv": dqkv.cpu(), "delta": delta.cpu()}


def _tok(S, lo, hi):
    """Row indices of tokens lo..hi-1 of every batch entry in the [B*S, ...] layout."""
    return (torch.arange(B).view(B, 1) * S + torch.arange(lo, hi).view(1, -1)).reshape(-1)


def _lse_rows(t, S, lo, hi):
    return t.view(B, H, S)[:, :, lo:hi]


# ----------------------------------------------------------------------------- 1. fp64 bounds
@pytest.mark.gpu
@pytest.mark.parametrize("S,wide", PATHS)
def test_causal_attention_bound(S, wide):
    _attn_switches(wide, 1, 1)
    try:
        for p, seed in ((0.0, 0), (0.1, 977 + S)):
            for masked in (False, True):
                g = _gen(S * 10 + int(p * 10) + masked + 5)
                qkv, dO, mask = _attn_inputs(B, S, H, g, masked)
                r = _run_causal(qkv, mask, dO, B, S, H, SCALE, p, seed)
                tag = f"causal attention S={S} wide={wide} p={p} mask={masked}"
                of = causal_fwd_oracle(qkv, mask, B, S, H, SCALE, p, seed)
                _measure("lse", r["lse"], of["lse"][0], of["lse_unit"])
                print(f"MEASURE out/bound {_ratio(r['out'], *of['out']):.4f}")
                assert_within(r["out"], *of["out"], f"{tag} out")
                assert_within(r["lse"], *of["lse"], f"{tag} lse")
                ob = causal_bwd_oracle(qkv, mask, dO, r["out"], r["lse"], B, S, H, SCALE, p, seed)
                _measure("delta/bound", r["delta"], *ob["delta"])
                assert_within(r["delta"], *ob["delta"], f"{tag} delta")
                ref, bnd = ob["dqkv"]
                for i, name in enumerate(("dQ", "dK", "dV")):
                    sl = slice(i * H * AD, (i + 1) * H * AD)
                    print(f"MEASURE {name}/bound "
                          f"{_ratio(r['dqkv'][:, sl], ref[:, sl], bnd[:, sl]):.4f}")
                    assert_within(r["dqkv"][:, sl], ref[:, sl], bnd[:, sl], f"{tag} {name}")
    finally:
        _attn_switches(1, 1, 1)


def test_causal_bound_accepts_emulation_and_rejects_shifted_diagonal():
    """CPU self-check of the oracle: the fp32 / bf16 emulation of the causal forward lies inside
    the bound; the same emulation with the diagonal shifted by one (k < q) lies outside."""
    S = 192
    qkv, _, mask = _attn_inputs(B, S, H, _gen(8), masked=True)
    for p, seed in ((0.0, 0), (0.1, 31)):
        o = causal_fwd_oracle(qkv, mask, B, S, H, SCALE, p, seed)
        out = causal_fwd_emulate(qkv, mask, B, S, H, SCALE, p, seed)
        print(f"emulation / bound p={p}: {_ratio(out, *o['out']):.3f}")
        assert_within(out, *o["out"], f"emulated causal forward p={p}")
        with pytest.raises(AssertionError, match="outside the bound"):
            assert_within(causal_fwd_emulate(qkv, mask, B, S, H, SCALE, p, seed, strict=True),
                          *o["out"])


# ----------------------------------------------------------------------------- 2. last row
@pytest.mark.gpu
@pytest.mark.parametrize("S,wide", PATHS)
def test_causal_last_row_is_the_non_causal_row(S, wide):
    """Query S - 1 sees every key and the key order is unchanged: out, lse and dQ of that row
    are the non-causal kernels' bits (the split ones)."""
    _attn_switches(wide, 0, 1)
    try:
        for p, seed in ((0.0, 0), (0.1, 55 + S)):
            qkv, dO, mask = _attn_inputs(B, S, H, _gen(S + 3), masked=True)
            c = _run_causal(qkv, mask, dO, B, S, H, SCALE, p, seed)
            n = _run_attn(qkv, mask, dO, B, S, H, SCALE, p, seed)
            rows = _tok(S, S - 1, S)
            assert torch.equal(c["out"][rows], n["out"][rows]), (S, wide, p)
            assert torch.equal(_lse_rows(c["lse"], S, S - 1, S), _lse_rows(n["lse"], S, S - 1, S))
            assert torch.equal(c["dqkv"][rows, :H * AD], n["dqkv"][rows, :H * AD]), (S, wide, p)
            # and a row that does not see every key differs: the comparison can fail
            assert not torch.equal(c["out"][_tok(S, 0, 1)], n["out"][_tok(S, 0, 1)])
    finally:
        _attn_switches(1, 1, 1)


# ----------------------------------------------------------------------------- 3. shapes agree
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_causal_wide_and_narrow_shapes_bit_identical(p):
    S = 256
    qkv, dO, mask = _attn_inputs(B, S, H, _gen(12), masked=True)
    res = []
    try:
        for wide in (1, 0):
            _attn_switches(wide, 1, 1)
            res.append(_run_causal(qkv, mask, dO, B, S, H, SCALE, p, 808))
    finally:
        _attn_switches(1, 1, 1)
    for name in ("out", "lse", "delta", "dqkv"):
        assert torch.equal(res[0][name], res[1][name]), name


# ----------------------------------------------------------------------------- 4. no look-ahead
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_causal_no_look_ahead_bit_for_bit(p):
    S, j = 192, 70
    g = _gen(21)
    qkv, dO, mask = _attn_inputs(B, S, H, g, masked=False)
    other, _, _ = _attn_inputs(B, S, H, g, masked=False)
    late = _tok(S, j, S)
    qkv2 = qkv.clone()
    qkv2[late] = other[late]
    assert not torch.equal(qkv2, qkv)
    a = _run_causal(qkv, mask, dO, B, S, H, SCALE, p, 99)
    b = _run_causal(qkv2, mask, dO, B, S, H, SCALE, p, 99)
    early = _tok(S, 0, j)
    assert torch.equal(a["out"][early], b["out"][early])
    assert torch.equal(_lse_rows(a["lse"], S, 0, j), _lse_rows(b["lse"], S, 0, j))
    assert torch.equal(a["dqkv"][early, :H * AD], b["dqkv"][early, :H * AD])
    assert not torch.equal(a["out"][late], b["out"][late])


# ----------------------------------------------------------------------------- 5. skipped tiles
@pytest.mark.gpu
@pytest.mark.parametrize("S,wide,t", [(192, 0, 64), (192, 0, 128), (256, 1, 64), (256, 1, 128),
                                      (128, 1, 64)])
def test_causal_skipped_tiles_are_not_used(S, wide, t):
    """NaN in the tiles above the diagonal (ordinary values, read by nobody): a kernel that loads
    such a tile and merely masks it gives 0 * NaN = NaN in its PV / dV / dK / dQ products."""
    nan = float("nan")
    HD = H * AD
    _attn_switches(wide, 1, 1)
    try:
        qkv, dO, mask = _attn_inputs(B, S, H, _gen(S + t), masked=False)
        clean = _run_causal(qkv, mask, dO, B, S, H, SCALE, 0.1, 4)
        lo, hi = _tok(S, 0, t), _tok(S, t, S)
        # (a) K and V of rows >= t
        bad = qkv.clone()
        bad[hi, HD:] = nan
        r = _run_causal(bad, mask, dO, B, S, H, SCALE, 0.1, 4)
        for got, ref, name in ((r["out"][lo], clean["out"][lo], "out"),
                               (_lse_rows(r["lse"], S, 0, t), _lse_rows(clean["lse"], S, 0, t),
                                "lse"),
                               (r["dqkv"][lo, :HD], clean["dqkv"][lo, :HD], "dQ")):
            assert bool(torch.isfinite(got.float()).all()), f"(a) {name} S={S} t={t}"
            assert torch.equal(got, ref), f"(a) {name} S={S} t={t}"
        # (b) Q and dO of rows < t
        bad = qkv.clone()
        bad[lo, :HD] = nan
        dbad = dO.clone()
        dbad[lo] = nan
        r = _run_causal(bad, mask, dbad, B, S, H, SCALE, 0.1, 4)
        for i, name in ((1, "dK"), (2, "dV")):
            got, ref = r["dqkv"][hi, i * HD:(i + 1) * HD], clean["dqkv"][hi, i * HD:(i + 1) * HD]
            assert bool(torch.isfinite(got.float()).all()), f"(b) {name} S={S} t={t}"
            assert torch.equal(got, ref), f"(b) {name} S={S} t={t}"
    finally:
        _attn_switches(1, 1, 1)


# ----------------------------------------------------------------------------- 6. refusals
@pytest.mark.gpu
def test_causal_refuses_keep_buffer_and_column_partials():
    K = _K()
    S, p = 128, 0.1
    qkv, dO, _ = _attn_inputs(B, S, H, _gen(2), masked=False)
    qd, dod = _dev(qkv), _dev(dO)
    out = torch.zeros(B * S, H * AD, device="cuda", dtype=BF16)
    lse = torch.zeros(B * H * S, device="cuda")
    nk = K.attn_keep_words(B, S, H, p)
    assert nk > 0                                   # the non-causal call would take the buffer
    keep = torch.zeros(nk, device="cuda", dtype=torch.int32)
    part = torch.zeros(B, 3 * H * AD, device="cuda")
    with pytest.raises(RuntimeError, match="causal"):
        K.attn_fwd(qd.data_ptr(), 0, out.data_ptr(), lse.data_ptr(), B, S, H, SCALE, p, 1, _st(),
                   keep.data_ptr(), causal=1)
    K.attn_fwd(qd.data_ptr(), 0, out.data_ptr(), lse.data_ptr(), B, S, H, SCALE, p, 1, _st(), 0,
               causal=1)
    dqkv, delta = torch.zeros_like(qd), torch.zeros_like(lse)
    args = (qd.data_ptr(), 0, out.data_ptr(), dod.data_ptr(), lse.data_ptr(), delta.data_ptr(),
            dqkv.data_ptr(), B, S, H, SCALE, p, 1, _st())
    with pytest.raises(RuntimeError, match="causal"):
        K.attn_bwd(*args, part.data_ptr(), 0, causal=1)
    with pytest.raises(RuntimeError, match="causal"):
        K.attn_bwd(*args, 0, keep.data_ptr(), causal=1)
    torch.cuda.synchronize()


class _Ctx:
    def save_for_backward(self, *t):
        self.saved_tensors = t


@pytest.mark.gpu
def test_causal_op_asks_for_no_keep_bits_and_leaves_no_column_partials(monkeypatch):
    """At S == 128 with dropout the non-causal op takes the keep buffer and the fused backward's
    column partials; the causal op consults neither switch and its dqkv carries no partials."""
    from distributedtensorflow_amd.ops import native_nlp
    S, p = 128, 0.1
    qkv, dO, _ = _attn_inputs(B, S, H, _gen(3), masked=False)
    qd, dod = _dev(qkv), _dev(dO)
    ctx = _Ctx()
    native_nlp._AttentionQKV.forward(ctx, qd, None, B, S, H, p, SCALE, False)
    assert ctx.keep is not None
    dq = native_nlp._AttentionQKV.backward(ctx, dod)[0]
    assert hasattr(dq, "_dtf_colsum_part")          # the control: the attribute can be there

    def trap(*a):
        raise AssertionError("the causal op consulted a fused-backward switch")

    monkeypatch.setattr(native_nlp._K, "attn_keep_words", trap)
    monkeypatch.setattr(native_nlp._K, "attn_bwd_fused", trap)
    ctx = _Ctx()
    native_nlp._AttentionQKV.forward(ctx, qd, None, B, S, H, p, SCALE, True)
    assert ctx.keep is None
    res = native_nlp._AttentionQKV.backward(ctx, dod)
    torch.cuda.synchronize()
    assert not hasattr(res[0], "_dtf_colsum_part")
    assert len(res) == 8 and all(r is None for r in res[1:])


# ----------------------------------------------------------------------------- 7. op and model
def _grads_of(fn, inputs, dy):
    y = fn()
    return y.detach().float(), [g.detach().float() for g in torch.autograd.grad(y, inputs, dy)]


@pytest.mark.gpu
@pytest.mark.parametrize("B_,S,H_,p,masked", [(2, 128, 3, 0.1, True), (2, 192, 2, 0.0, False),
                                              (3, 256, 2, 0.1, True)])
def test_causal_op_matches_reference(B_, S, H_, p, masked):
    """ops.attention_qkv(causal=True) against reference.attention_qkv, at the tolerances
    tests/test_nlp.py::test_attention_gpu uses for the non-causal op."""
    torch.manual_seed(0)
    qkv32 = torch.randn(B_ * S, 3 * H_ * AD)
    mask = torch.zeros(B_, S)
    if masked:
        mask[0, S - 37:] = -10000.0
    dy = torch.randn(B_ * S, H_ * AD)
    x = qkv32.to("cuda", BF16).requires_grad_(True)
    torch.manual_seed(11)
    y, (dx,) = _grads_of(lambda: ops.attention_qkv(x, mask.cuda() if masked else None, B_, S, H_,
                                                   p, True, causal=True), [x], dy.cuda().to(BF16))
    x_ = qkv32.to(BF16).float().requires_grad_(True)
    torch.manual_seed(11)
    y_, (dx_,) = _grads_of(lambda: R.attention_qkv(x_, mask if masked else None, B_, S, H_, p,
                                                   True, causal=True), [x_], dy.to(BF16).float())
    torch.testing.assert_close(y.cpu(), y_, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(dx.cpu(), dx_, atol=5e-2, rtol=5e-2)


@pytest.mark.gpu
def test_causal_op_qkv_api():
    """ops.attention(q, k, v, causal=True) on the device against the reference."""
    torch.manual_seed(1)
    q, k, v = (torch.randn(2, 2, 64, AD).to(BF16) for _ in range(3))
    got = ops.attention(q.cuda(), k.cuda(), v.cuda(), causal=True)
    want = R.attention(q.float(), k.float(), v.float(), causal=True)
    torch.testing.assert_close(got.float().cpu(), want, atol=2e-2, rtol=2e-2)


TINY = dict(vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
            intermediate_size=512, max_position_embeddings=128, hidden_dropout_prob=0.0,
            attention_probs_dropout_prob=0.0)


def _lm_batch(Bn=4, S=64, V=1000, seed=0):
    from distributedtensorflow_amd.data import causal_lm_targets
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (Bn, S), generator=g)
    am = torch.ones(Bn, S, dtype=torch.int64)
    am[1, S - 9:] = 0
    ids = ids * am
    lab, w = causal_lm_targets(ids, am)
    return ids, am, lab, w


@pytest.mark.gpu
def test_causal_bert_tiny_gpu_matches_cpu():
    """The loss within the 5 % that tests/test_nlp.py allows the non-causal tiny model between
    the two backends, and three variable gradients within 5 % of their largest element (the same
    relative budget: bf16 activations end to end against the fp32 reference path)."""
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    torch.manual_seed(0)
    cfg = BertConfig(**TINY, causal=True)
    m_cpu = BertForPreTraining(cfg)
    m_gpu = BertForPreTraining(cfg)
    m_gpu.load_state_dict(m_cpu.state_dict())
    m_gpu.cuda()
    ids, am, lab, w = _lm_batch()

    def pick(m):
        return [m.layers[0].qkv_kernel, m.layers[0].qkv_bias, m.mlm_transform.kernel]

    ref = m_cpu(ids, torch.zeros_like(ids), am, None, lab, w)
    gref = torch.autograd.grad(ref, pick(m_cpu))
    with OneDeviceStrategy("cuda").scope():
        loss = m_gpu(ids.cuda(), torch.zeros_like(ids).cuda(), am.cuda(), None, lab.cuda(),
                     w.cuda())
        ggpu = torch.autograd.grad(loss, pick(m_gpu))
    assert abs(loss.item() - ref.item()) < 0.05 * abs(ref.item())
    for a, b in zip(ggpu, gref):
        err = (a.float().cpu() - b).abs().max().item()
        print(f"MEASURE grad err / max {err / b.abs().max().item():.4f}")
        assert err <= 0.05 * b.abs().max().item()


@pytest.mark.gpu
def test_causal_bert_no_look_ahead_on_the_device():
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    ids, _, _, _ = _lm_batch(Bn=2)
    j, S = 21, ids.shape[1]
    ids2 = ids.clone()
    ids2[:, j:] = (ids2[:, j:] + 17) % 1000
    res = {}
    for causal in (True, False):
        torch.manual_seed(2)
        m = BertForPreTraining(BertConfig(**TINY, causal=causal)).cuda().eval()
        with torch.no_grad():
            a = m(ids.cuda()).view(2, S, -1)
            b = m(ids2.cuda()).view(2, S, -1)
        res[causal] = torch.equal(a[:, :j], b[:, :j])
        assert not torch.equal(a[:, j:], b[:, j:])
    assert res[True] and not res[False]


@pytest.mark.gpu
def test_causal_step_captured_as_a_graph_matches_eager():
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    from distributedtensorflow_amd.optimizers import LAMBOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import GraphedTrainStep
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = BertForPreTraining(BertConfig(**TINY, causal=True))
    batches = [[t.cuda() for t in _lm_batch(seed=s)] for s in range(4)]
    res = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        with OneDeviceStrategy("/gpu:0").scope():
            opt = LAMBOptimizer(1e-3)
            opt.build(list(model.parameters()))

        def step(ids, am, lab, w):
            loss = model(ids, torch.zeros_like(ids), am, None, lab, w)
            opt.minimize(loss)
            return loss

        losses = []
        if graphed:
            fn = GraphedTrainStep(step, opt, [t.clone() for t in batches[0]], warmup=2)
            for b in batches[1:]:
                losses.append(fn(*b).clone())
        else:
            for _ in range(2):
                step(*batches[0])
            for b in batches[1:]:
                losses.append(step(*b).detach().clone())
        torch.cuda.synchronize()
        res.append((torch.stack(losses), opt.space.master.clone()))
    assert torch.equal(res[0][0], res[1][0]), (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


# ----------------------------------------------------------------------------- 8. dataset
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
def test_causal_token_batches_on_the_device_match_the_cpu(dtype):
    from distributedtensorflow_amd.data import DeviceTokenDataset, TokenMasking
    rng = np.random.default_rng(5)
    V = 60000 if dtype == np.uint16 else 100000
    N, S = 37, 64
    tok = rng.integers(1, V, (N, S)).astype(dtype)
    for i in range(N):
        tok[i, S - int(rng.integers(0, 20)):] = 0 if i % 3 else tok[i, S - 1]
    tok[3, 5] = V - 1
    masking = TokenMasking(vocab_size=V)
    kw = dict(masking=masking, seed=9, num_shards=2, shard_index=1, objective="causal")
    a = DeviceTokenDataset(tok, 4, "cpu", **kw)
    b = DeviceTokenDataset(tok, 4, "cuda", chunk_bytes=3 * S * tok.itemsize, **kw)

    def same(x, y):
        assert x.keys() == y.keys()
        for k in x:
            if x[k] is None:
                assert y[k] is None
            else:
                assert y[k].is_cuda and x[k].dtype == y[k].dtype
                assert torch.equal(x[k], y[k].cpu()), k

    for _ in range(6):                                           # over an epoch boundary
        same(next(a), next(b))
    pa, pb = list(a.single_pass()), list(b.single_pass())
    assert len(pa) == len(pb) == 5
    for x, y in zip(pa, pb):
        same(x, y)
    y = pb[0]
    assert y["masked_lm_positions"] is None and y["input_ids"].dtype == torch.int64
    assert int(y["input_ids"].max()) < V and int(y["input_ids"].min()) >= 0
    assert int(torch.cat([x["input_ids"] for x in pb]).max()) > 32767
    assert math.isclose(float(y["masked_lm_weights"].sum()),
                        float((y["input_ids"][:, 1:] != 0).sum()))
