"""Incremental decoding on the device: attn_decode_kernel / attn_decode_combine_kernel /
kv_cache_fill_kernel (csrc/kernels/attn_decode.hip), the ops and the KV-cache methods of the model.

The kernel check is per element against fp64 on the stored bf16 values with the forward bound of
tests/test_nlp_kernels_gpu.py and ONE bf16 rounding instead of two (p stays fp32):
``(U16 + rel32) (P @ |v|)``, ``rel32 = gamma(len + 8) + 2 LN2 gamma(70) smax + 2 INTR``, smax over
the visible keys.  Every cache row past pos[b] holds garbage, NaN bit patterns among it.

Measured on an MI355X: see profiles/DECODE.md.
"""
import copy

import pytest
import torch

from distributedtensorflow_amd import ops
from test_nlp_kernels_gpu import (AD, BF16, INTR, LN2, SENT, U16, _attn_inputs, _dev, _gen, _K,
                                  _ratio, _scores, _split_qkv, _st, assert_within, gamma)


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    """This module leaves odd-sized cached blocks behind; test_resnet_gpu compares
    ``max_memory_allocated`` between steps to within 4 MB, so they are released when it is done
    (as in tests/test_conv_kernels_gpu.py)."""
    yield
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


B, H, C, SCALE = 2, 3, 256, AD ** -0.5
# a single key, a full first tile; one key in the second tile; a ragged middle, the last slot;
# very unequal rows (waves and splits of row 0 without a key)
POS = [(0, 63), (64, 127), (130, 255), (5, 200)]


def _case(pos, seed):
    """-> (qkv_new [B, 3*H*64], k / v caches [B, H, C, 64] with rows < pos real and the rest
    garbage, the expected caches after the call, (out64, bound))."""
    qkv, _, _ = _attn_inputs(B, C, H, _gen(seed), masked=False)       # a C-token sequence
    p = torch.tensor(pos)
    new = qkv.view(B, C, -1)[torch.arange(B), p].contiguous()
    q, k, v = _split_qkv(qkv, B, C, H)                                # fp64 [B, H, C, 64]
    vis = (torch.arange(C).view(1, C) <= p.view(B, 1)).view(B, 1, 1, C)
    s2, smag = _scores(q[torch.arange(B), :, p].unsqueeze(2), k, None, B, C, SCALE)  # [B,H,1,C]
    s2 = torch.where(vis, s2, torch.full_like(s2, float("-inf")))
    smax = torch.where(vis, smag, torch.zeros_like(smag)).max(-1, keepdim=True).values
    P = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
    P = P / P.sum(-1, keepdim=True)
    glen = torch.tensor([gamma(n + 1 + 8) for n in pos], dtype=torch.float64).view(B, 1, 1, 1)
    rel32 = glen + 2 * LN2 * gamma(70) * smax + 2 * INTR
    flat = lambda t: t[:, :, 0].reshape(B, H * AD)
    oracle = (flat(P @ v), flat((U16 + rel32) * (P @ v.abs())))
    # garbage: the guard value, every third element a NaN bit pattern
    junk = torch.full((B, H, C, AD), SENT).to(BF16)
    junk.view(-1)[::3] = float("nan")
    caches, after = [], []
    for t in (k, v):
        real = t.to(BF16)
        before = torch.where((torch.arange(C).view(1, C) < p.view(B, 1)).view(B, 1, C, 1), real,
                             junk)
        caches.append(before.contiguous())
        after.append(torch.where(vis.view(B, 1, C, 1), real, junk).contiguous())
    return new, caches, after, oracle


def _run(new, caches, pos, splits, max_len=C):
    K = _K()
    kc, vc, nd = _dev(caches[0]), _dev(caches[1]), _dev(new)
    pd = _dev(torch.tensor(pos, dtype=torch.int32))
    out = torch.full((B, H * AD), SENT, device="cuda", dtype=BF16)
    ws = torch.full((max(1, K.attn_decode_ws_floats(B, H, splits)),), float("nan"), device="cuda")
    K.attn_decode(nd.data_ptr(), pd.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                  ws.data_ptr(), B, H, C, max_len, splits, SCALE, _st())
    torch.cuda.synchronize()
    return out.cpu(), kc.cpu(), vc.cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ----------------------------------------------------------------------------- 1. fp64 bound
@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("pos", POS)
def test_attn_decode_bound(pos, splits):
    new, caches, after, (ref, bnd) = _case(pos, 100 + pos[0])
    out, kc, vc = _run(new, caches, pos, splits)
    print(f"MEASURE decode out/bound pos={pos} splits={splits} {_ratio(out, ref, bnd):.4f}")
    assert_within(out, ref, bnd, f"attn_decode pos={pos} splits={splits}")   # finite, too
    # rows pos[b] are the new K and V bit for bit, every other element is bit-unchanged
    assert _same_bits(kc, after[0]) and _same_bits(vc, after[1])


# ----------------------------------------------------------------------------- 2. determinism
@pytest.mark.gpu
def test_attn_decode_is_deterministic_and_splits_agree():
    pos = (130, 255)
    new, caches, _, (ref, bnd) = _case(pos, 7)
    outs = {}
    for splits in (1, 2, 4):
        a, b = (_run(new, caches, pos, splits)[0] for _ in range(2))
        assert _same_bits(a, b), splits
        outs[splits] = a
    for splits in (2, 4):
        assert_within(outs[splits], outs[1].double(), 2 * bnd, f"splits {splits} against 1")


# ----------------------------------------------------------------------------- 3. prefill copy
@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 192])
def test_kv_cache_fill_bit_exact(S):
    qkv, _, _ = _attn_inputs(B, S, H, _gen(S), masked=False)
    junk = torch.full((B, H, C, AD), SENT).to(BF16)
    junk.view(-1)[::3] = float("nan")
    kc, vc = _dev(junk), _dev(junk)
    ops.kv_cache_fill(_dev(qkv), kc, vc, B, S, H)
    x = qkv.view(B, S, 3, H, AD)
    for got, i in ((kc, 1), (vc, 2)):
        want = junk.clone()
        want[:, :, :S] = x[:, :, i].permute(0, 2, 1, 3)
        assert _same_bits(got.cpu(), want), i


# ----------------------------------------------------------------------------- 4. refusals
@pytest.mark.gpu
def test_attn_decode_refusals():
    K = _K()
    new, caches, _, _ = _case((5, 200), 1)
    nd, kc, vc = _dev(new), _dev(caches[0]), _dev(caches[1])
    pos = torch.tensor([5, 90], dtype=torch.int32, device="cuda")
    out = torch.zeros(B, H * AD, device="cuda", dtype=BF16)
    ws = torch.zeros(K.attn_decode_ws_floats(B, H, 4), device="cuda")
    call = lambda cap, max_len, splits: K.attn_decode(
        nd.data_ptr(), pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
        ws.data_ptr(), B, H, cap, max_len, splits, SCALE, _st())
    with pytest.raises(RuntimeError, match="multiple of 64"):
        call(96, 96, 1)
    with pytest.raises(RuntimeError, match="splits"):
        call(C, 128, 3)                                    # max_len has two tiles
    call(C, 128, 2)
    with pytest.raises(ValueError, match="qkv_new"):
        ops.attention_decode(nd[:, :-64].contiguous(), kc, vc, pos, H)
    with pytest.raises(ValueError, match="splits"):
        ops.attention_decode(nd, kc, vc, pos, H, max_len=128, splits=3)
    assert K.attn_decode_splits(8, 12, 64) == 1 and K.attn_decode_splits(8, 12, 2048) > 1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 5. the model
# hidden 256 / 4 heads: the LayerNorm kernels the model runs take H % 256 == 0
TINY = dict(vocab_size=256, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
            intermediate_size=512, max_position_embeddings=128, causal=True)


@pytest.mark.gpu
def test_prefill_and_decode_steps_match_the_full_forward_on_the_device():
    """Teacher-forced prefill + 8 decode steps against the rows of the full causal forward over
    the 128-padded sequence.  Both are bf16 computations of the fp32 reference model with
    independent roundings of the same size, so their difference is bounded by twice the bf16
    forward's own distance to the fp32 CPU result at the same positions."""
    from distributedtensorflow_amd.models import KVCache
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    cpu = BertForPreTraining(BertConfig(**TINY)).eval()
    gpu = copy.deepcopy(cpu).cuda().eval()
    lens, steps, rows = torch.tensor([5, 64]), 8, torch.arange(2)
    prompt = torch.randint(1, 256, (2, 64), generator=_gen(3))
    prompt = prompt * (torch.arange(64).view(1, 64) < lens.view(2, 1))
    gen = gpu.generate(prompt.cuda(), lens, steps + 1).cpu()          # the sequence fed below
    seq = torch.zeros(2, 128, dtype=torch.int64)
    seq[:, :64] = prompt
    for b in range(2):
        seq[b, lens[b]:lens[b] + steps + 1] = gen[b]
    at = lens.view(2, 1) - 1 + torch.arange(steps + 1).view(1, -1)   # positions compared
    with torch.no_grad():
        ref32 = cpu(seq).view(2, 128, -1)[rows.view(2, 1), at]
        full = gpu(seq.cuda()).view(2, 128, -1)[rows.view(2, 1), at.cuda()].float().cpu()
    cache = KVCache(gpu.cfg, 2, 128, "cuda")
    logits = [gpu.prefill(prompt.cuda(), lens, cache)]
    for t in range(steps):
        logits.append(gpu.decode_step(gen[:, t].cuda(), cache))
    got = torch.stack(logits, 1).float().cpu()                        # [2, steps + 1, V]
    assert torch.equal(cache.pos.cpu(), (lens + steps).int())
    tol = 2 * float((full - ref32).abs().max())
    err = float((got - full).abs().max())
    print(f"MEASURE decode-vs-forward / tolerance {err / tol:.4f} (tolerance {tol:.4f})")
    assert err <= tol
    # greedy generate is the argmax of these logits; a row that produced eos_id keeps it
    assert torch.equal(got.argmax(-1), gen)
    eos = int(gen[0, 0])
    stopped = gpu.generate(prompt.cuda(), lens, 4, eos_id=eos).cpu()
    assert stopped[0].tolist() == [eos] * 4
