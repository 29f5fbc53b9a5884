"""The FP8 (e4m3) KV cache on the reference path: the quantise / dequantise rule at its edges, the
three cache ops against the bf16-cache reference on the dequantised cache, the argument check,
KVCache(kv_dtype="fp8") and generate(kv_dtype="fp8")."""
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.models import KVCache, bert
from distributedtensorflow_amd.ops import reference as R
from test_append import CASES
from test_decode import LENS, TINY

B, H, C = 2, 3, 256
F8 = torch.float8_e4m3fn
i32 = lambda v: torch.tensor(v, dtype=torch.int32)


def _row(*head):
    """A 64-element row: ``head`` then zeros."""
    x = torch.zeros(64)
    x[:len(head)] = torch.tensor(head)
    return x


# (row, exponent of the scale, the first bytes as floats): 448 * 2^j fills the format at e = j;
# the next bf16 above it (f = 0.87890625 > 0.875) moves to e = j + 1; f = 0.875 exactly stays;
# 17 -> 16, 19 -> 20 and 18 +- ties to even at e = 0 (max 256 = 0.5 * 2^9); 2^-9 is the smallest
# subnormal, 1.5 * 2^-10 rounds up to it and 2^-10 ties to zero; the clamp below (k - 9 = -113)
# and the largest bf16, which reaches e = 120 (no finite input goes past it)
RULE = [(_row(), 0, [0.0]),
        (_row(448.0 * 4, -3.0 * 4), 2, [448.0, -3.0]),
        (_row(450.0 * 4, 3.0 * 4), 3, [224.0, 1.5]),
        (_row(0.875 * 2.0 ** -20, -2.0 ** -21), -29, [448.0, -256.0]),
        (_row(256.0, 17.0, 19.0, 18.0, -22.0), 0, [256.0, 16.0, 20.0, 18.0, -22.0]),
        (_row(256.0, 2.0 ** -9, 1.5 * 2.0 ** -10, 2.0 ** -10, 2.0 ** -6), 0,
         [256.0, 2.0 ** -9, 2.0 ** -9, 0.0, 2.0 ** -6]),
        (_row(2.0 ** -105, 2.0 ** -108, 2.0 ** -120), -100, [2.0 ** -5, 2.0 ** -8, 0.0]),
        (_row(1.9921875 * 2.0 ** 127, 2.0 ** 121), 120, [256.0, 2.0])]


@pytest.mark.parametrize("row,e,head", RULE)
def test_quantize_rule_at_its_edges(row, e, head):
    q, s = R.kv_quantize_rows(row.to(torch.bfloat16))
    assert q.dtype == F8 and float(s) == 2.0 ** e
    assert q.float()[:len(head)].tolist() == head and bool((q.float()[len(head):] == 0).all())
    d32, d16 = R.kv_dequantize(q, s), R.kv_dequantize(q, s, torch.bfloat16)
    assert torch.equal(d32, q.float().double().mul(2.0 ** e).float())
    assert torch.equal(d16.float(), d32)


def _caches(pos, g):
    """-> k bytes, k scales, v bytes, v scales: rows < pos[b] real, the rest 0x7F and NaN."""
    out = []
    for _ in range(2):
        q, s = R.kv_quantize_rows(torch.randn(B, H, C, 64, generator=g))
        real = (torch.arange(C).view(1, 1, C) < torch.tensor(pos).view(B, 1, 1)).expand(B, H, C)
        q.view(torch.uint8)[~real] = 0x7F
        s[~real] = float("nan")
        out += [q, s]
    return out


def _same(a, b):
    bits = lambda t: t.view(torch.uint8 if t.dtype == F8 else torch.int32)
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("T,pos,n_new", [(0, (5, 200), None)] + CASES[1:])
def test_fp8_ops_are_the_reference_on_the_dequantised_cache(T, pos, n_new):
    """T = 0: attention_decode.  The new rows enter as their dequantised values; the cache takes
    their bytes and scales and nothing else changes."""
    g = torch.Generator().manual_seed(T)
    kq, ks, vq, vs = _caches(pos, g)
    new = torch.randn(B * max(T, 1), 3, H, 64, generator=g)
    knew, vnew = (R.kv_quantize_rows(new[:, i]) for i in (1, 2))
    deq = new.clone()
    deq[:, 1], deq[:, 2] = R.kv_dequantize(*knew), R.kv_dequantize(*vnew)
    kd, vd = R.kv_dequantize(kq, ks), R.kv_dequantize(vq, vs)
    flat = lambda t: t.reshape(t.shape[0], -1)
    if T == 0:
        want = ops.attention_decode(flat(deq), kd, vd, i32(pos), H)
        got = ops.attention_decode(flat(new), kq, vq, i32(pos), H, k_scale=ks, v_scale=vs)
    else:
        want = ops.attention_append(flat(deq), kd, vd, i32(pos), H, n_new=i32(n_new))
        got = ops.attention_append(flat(new), kq, vq, i32(pos), H, n_new=i32(n_new), k_scale=ks,
                                   v_scale=vs)
    assert torch.equal(got, want)
    # the caches dequantise to the bf16-cache op's caches; unwritten rows are bit-unchanged
    for q, s, d in ((kq, ks, kd), (vq, vs, vd)):
        assert _same(R.kv_dequantize(q, s), d)
        live = ~torch.isnan(s)
        assert bool((q.view(torch.uint8)[~live] == 0x7F).all())
        assert [int(n) for n in live[:, 0].sum(-1)] == [p + (n if T else 1) for p, n in
                                                        zip(pos, n_new or (1, 1))]


@pytest.mark.parametrize("S", [1, 100])
def test_fp8_fill_is_the_rule(S):
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(B * S, 3 * H * 64, generator=g)
    kq, ks, vq, vs = _caches((0, 0), g)
    before = [t.clone() for t in (kq, ks, vq, vs)]
    ops.kv_cache_fill(qkv, kq, vq, B, S, H, k_scale=ks, v_scale=vs)
    x = qkv.view(B, S, 3, H, 64)
    for i, q, s, (q0, s0) in ((1, kq, ks, before[:2]), (2, vq, vs, before[2:])):
        wq, wsc = R.kv_quantize_rows(x[:, :, i].permute(0, 2, 1, 3))
        assert _same(q[:, :, :S], wq) and _same(s[:, :, :S], wsc)
        assert _same(q[:, :, S:], q0[:, :, S:]) and _same(s[:, :, S:], s0[:, :, S:])


def test_the_argument_check():
    g = torch.Generator().manual_seed(0)
    kq, ks, vq, vs = _caches((5, 9), g)
    new, pos = torch.randn(B, 3 * H * 64), i32((5, 9))
    kf, vf = torch.zeros(B, H, C, 64), torch.zeros(B, H, C, 64)
    for kw, k, v in ((dict(), kq, vq), (dict(k_scale=ks), kq, vq),
                     (dict(k_scale=ks, v_scale=vs), kf, vf),
                     (dict(k_scale=ks, v_scale=vs), kq, vf),
                     (dict(k_scale=ks, v_scale=vs[:, :, :64]), kq, vq),
                     (dict(k_scale=ks.double(), v_scale=vs), kq, vq)):
        with pytest.raises(ValueError, match="scale|dtype"):
            ops.attention_decode(new, k, v, pos, H, **kw)
        with pytest.raises(ValueError, match="scale|dtype"):
            ops.attention_append(new, k, v, pos, H, **kw)
        with pytest.raises(ValueError, match="scale|dtype"):
            ops.kv_cache_fill(new, k, v, B, 1, H, **kw)


def test_fp8_kvcache_and_generate():
    torch.manual_seed(0)
    m = bert.BertForPreTraining(bert.BertConfig(**TINY, causal=True)).eval()
    L, heads = TINY["num_hidden_layers"], TINY["num_attention_heads"]
    for kv in ("fp8", F8):
        cache = KVCache(m.cfg, 2, 100, "cpu", torch.float32, kv_dtype=kv)
        assert cache.k.dtype == cache.v.dtype == F8 and cache.act_dtype == torch.float32
        assert cache.k.shape == (L, 2, heads, 128, 64) and cache.k_scale.dtype == torch.float32
        assert cache.k_scale.shape == cache.v_scale.shape == (L, 2, heads, 128)
    plain = KVCache(m.cfg, 2, 100, "cpu", torch.float32)
    assert plain.k.dtype == plain.act_dtype and plain.k_scale is None and len(plain.layer(0)) == 2
    with pytest.raises(ValueError, match="kv_dtype"):
        KVCache(m.cfg, 2, 100, "cpu", torch.float32, kv_dtype=torch.float16)
    ids = torch.randint(1, TINY["vocab_size"], (2, 64), generator=torch.Generator().manual_seed(1))
    a, b = (m.generate(ids, LENS, 6, kv_dtype="fp8") for _ in range(2))
    assert torch.equal(a, b) and a.shape == (2, 6)
    assert torch.equal(m.generate(ids, LENS, 6, kv_dtype="fp8", prefill_chunk=16), a)
