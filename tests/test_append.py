"""Append attention on the reference path: ops.attention_append and the model's extend,
prefill(chunk=) and generate(prefill_chunk=)."""
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.models import KVCache, bert
from test_decode import LENS, TINY

B, H, C = 2, 3, 256
# (T, pos, n_new): see tests/test_append_gpu.py for what each catches
CASES = [(1, (5, 200), (1, 1)), (5, (63, 250), (5, 5)), (16, (0, 48), (16, 16)),
         (64, (0, 100), (64, 37)), (80, (10, 176), (80, 0))]


@pytest.mark.parametrize("T,pos,n_new", [CASES[1], CASES[3], CASES[4]])
def test_attention_append_is_rows_of_the_causal_forward(T, pos, n_new):
    g = torch.Generator().manual_seed(T)
    new = torch.randn(B, T, 3, H, 64, generator=g)
    old = torch.randn(B, C, 3, H, 64, generator=g)             # the tokens already cached
    kc = torch.full((B, H, C, 64), float("nan"))
    vc = kc.clone()
    for b in range(B):
        kc[b, :, :pos[b]] = old[b, :pos[b], 1].permute(1, 0, 2)
        vc[b, :, :pos[b]] = old[b, :pos[b], 2].permute(1, 0, 2)
    k0, v0 = kc.clone(), vc.clone()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    out = ops.attention_append(new.view(B * T, -1), kc, vc, i32(pos), H, n_new=i32(n_new))
    out = out.view(B, T, -1)
    for b in range(B):
        p0, n = pos[b], n_new[b]
        seq = torch.cat([old[b, :p0], new[b, :n]]).reshape(p0 + n, -1)
        full = ops.attention_qkv(seq, None, 1, p0 + n, H, causal=True)
        torch.testing.assert_close(out[b, :n], full[p0:], atol=1e-5, rtol=1e-5)
        assert bool((out[b, n:] == 0).all())
        # rows p0 .. p0+n-1 written, every other row as it was (NaN rows compare as bits)
        for got, was, i in ((kc, k0, 1), (vc, v0, 2)):
            assert torch.equal(got[b, :, p0:p0 + n], new[b, :n, i].permute(1, 0, 2))
            was[b, :, p0:p0 + n] = got[b, :, p0:p0 + n]
            assert torch.equal(got[b].view(torch.int32), was[b].view(torch.int32))


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    m = bert.BertForPreTraining(bert.BertConfig(**TINY, causal=True)).eval()
    ids = torch.randint(1, TINY["vocab_size"], (2, 128), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        full = m(ids).view(2, 128, -1)
    return m, ids, full


def test_chunked_prefill_and_extend_match_the_full_forward(tiny):
    m, ids, full = tiny
    rows = torch.arange(2)
    cache = KVCache(m.cfg, 2, 128, "cpu", torch.float32)
    logits = m.prefill(ids[:, :64].contiguous(), LENS, cache, chunk=16)
    torch.testing.assert_close(logits, full[rows, LENS - 1], atol=1e-4, rtol=1e-4)
    assert torch.equal(cache.pos, LENS.int()) and cache.max_len == 64
    at = LENS.view(2, 1) + torch.arange(8).view(1, 8)
    more = m.extend(ids[rows.view(2, 1), at], cache, all_logits=True)
    torch.testing.assert_close(more, full[rows.view(2, 1), at], atol=1e-4, rtol=1e-4)
    assert torch.equal(cache.pos, (LENS + 8).int())
    # ragged n_new: the last new token's logits; generate takes the chunked prefill
    last = m.extend(ids[rows.view(2, 1), at + 8], cache, n_new=[3, 8])
    torch.testing.assert_close(last, full[rows, LENS + 8 + torch.tensor([2, 7])],
                               atol=1e-4, rtol=1e-4)
    prompt = ids[:, :64].contiguous()
    assert torch.equal(m.generate(prompt, LENS, 4, prefill_chunk=16), m.generate(prompt, LENS, 4))


def test_extend_refusals(tiny):
    m, ids, _ = tiny
    cache = KVCache(m.cfg, 2, 128, "cpu", torch.float32)
    m.prefill(ids[:, :64].contiguous(), LENS, cache, chunk=24)         # 64 = 24 + 24 + 16
    for bad in ([9, 1], [-1, 1], [1]):
        with pytest.raises(ValueError, match="n_new"):
            m.extend(ids[:, :8].contiguous(), cache, n_new=bad)
    with pytest.raises(ValueError, match="capacity"):
        m.extend(ids[:, :65].contiguous(), cache)
    mlm = bert.BertForPreTraining(bert.BertConfig(**TINY))
    with pytest.raises(ValueError, match="causal"):
        mlm.extend(ids[:, :8], cache)
    with pytest.raises(ValueError, match="causal"):
        mlm.prefill(ids[:, :64].contiguous(), LENS, cache, chunk=16)
    with pytest.raises(ValueError, match="max_len"):
        ops.attention_append(torch.zeros(2 * 80, 3 * 2 * 64), cache.k[0, :, :, :64].contiguous(),
                             cache.v[0, :, :, :64].contiguous(), cache.pos, 2)
