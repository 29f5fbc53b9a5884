"""Append attention on the device: kv_cache_append_kernel / attn_append_kernel /
attn_append_combine_kernel (csrc/kernels/attn_append.hip), the op and the model's extend,
prefill(chunk=) and generate(prefill_chunk=).

The kernel check is per element against fp64 on the stored bf16 values with attn_fwd_oracle's
bound (P rounded to bf16 for the MFMA, the output rounded once) applied to this mask:
``(2 U16 + rel32) (P @ |v|)``, ``rel32 = gamma(len + 8) + 2 LN2 gamma(70) smax + 2 INTR``,
``len = p0 + i + 1``, smax over the visible keys.  Every cache row at or past pos[b] starts as
garbage, NaN bit patterns among it.

| T  | pos       | n_new    | what it catches                                                     |
| 1  | (5, 200)  | (1, 1)   | the decode shape; a wave share without keys                         |
| 5  | (63, 250) | (5, 5)   | T % 16 != 0; diagonal across the 63/64 boundary; last cache row 254 |
| 16 | (0, 48)   | (16, 16) | empty cache; p0 + n landing exactly on a tile edge                  |
| 64 | (0, 100)  | (64, 37) | four query tiles; the causal forward for row 0; diagonal across key |
|    |           |          | 128; zero rows i >= 37                                              |
| 80 | (10, 176) | (80, 0)  | second query block; p0 + n = 256 = C; a row with n = 0              |

Measured on an MI355X: see profiles/APPEND.md.
"""
import copy
import functools

import pytest
import torch

from distributedtensorflow_amd import ops
from test_append import CASES
from test_decode_gpu import TINY
from test_nlp_kernels_gpu import (AD, BF16, INTR, LN2, SENT, U16, _attn_inputs, _dev, _gen, _K,
                                  _ratio, _rows, _scores, _split_qkv, _st, assert_within, gamma)


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield                                    # as tests/test_decode_gpu.py
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


B, H, C, SCALE = 2, 3, 256, AD ** -0.5


@functools.lru_cache(maxsize=None)
def _case(T, pos, n_new):
    """-> (qkv_new [B*T, 3*H*64], k / v caches [B, H, C, 64] with rows < pos real and the rest
    garbage, the expected caches after the call, (out64, bound) [B*T, H*64], live [B*T])."""
    old, _, _ = _attn_inputs(B, C, H, _gen(T), masked=False)          # the tokens cached so far
    new, _, _ = _attn_inputs(B, T, H, _gen(1000 + T), masked=False)
    p0, n = torch.tensor(pos).view(B, 1), torch.tensor(n_new).view(B, 1)
    _, ko, vo = _split_qkv(old, B, C, H)                              # fp64 [B, H, C, 64]
    q, kn, vn = _split_qkv(new, B, T, H)                              # fp64 [B, H, T, 64]
    row = torch.arange(C).view(1, C)
    fresh = ((row >= p0) & (row < p0 + n)).view(B, 1, C, 1)
    src = (row - p0).clamp(0, T - 1).view(B, 1, C, 1).expand(B, H, C, AD)
    k = torch.where(fresh, kn.gather(2, src), ko)                     # rows >= p0 + n: hidden
    v = torch.where(fresh, vn.gather(2, src), vo)
    i = torch.arange(T).view(1, T)
    live = i < n                                                      # [B, T]
    vis = ((row.view(1, 1, C) <= (p0 + i).view(B, T, 1)) & live.view(B, T, 1)).view(B, 1, T, C)
    s2, smag = _scores(q, k, None, B, C, SCALE)                       # [B, H, T, C]
    s2 = torch.where(vis, s2, torch.full_like(s2, float("-inf")))
    smax = torch.where(vis, smag, torch.zeros_like(smag)).max(-1, keepdim=True).values
    P = torch.where(vis, torch.exp2(s2 - s2.max(-1, keepdim=True).values.clamp_min(-1e300)),
                    torch.zeros_like(s2))
    P = P / P.sum(-1, keepdim=True).clamp_min(1e-300)                 # a dead row: all zeros
    glen = torch.tensor([[gamma(p + t + 1 + 8) for t in range(T)] for p in pos],
                        dtype=torch.float64).view(B, 1, T, 1)
    rel32 = glen + 2 * LN2 * gamma(70) * smax + 2 * INTR
    oracle = (_rows(P @ v, B, T, H), _rows((2 * U16 + rel32) * (P @ v.abs()), B, T, H))
    junk = torch.full((B, H, C, AD), SENT).to(BF16)                   # the guard value, every
    junk.view(-1)[::3] = float("nan")                                 # third a NaN bit pattern
    caches, after = [], []
    for t in (k, v):
        caches.append(torch.where((row < p0).view(B, 1, C, 1), t.to(BF16), junk).contiguous())
        after.append(torch.where((row < p0 + n).view(B, 1, C, 1), t.to(BF16), junk).contiguous())
    return new, caches, after, oracle, live.reshape(-1)


def _run(T, pos, n_new, splits, max_len=C):
    K = _K()
    new, caches = _case(T, pos, n_new)[:2]
    kc, vc, nd = _dev(caches[0]), _dev(caches[1]), _dev(new)
    pd, nn = (_dev(torch.tensor(v, dtype=torch.int32)) for v in (pos, n_new))
    out = torch.full((B * T, H * AD), SENT, device="cuda", dtype=BF16)
    ws = torch.full((max(1, K.attn_append_ws_floats(B, H, T, splits)),), float("nan"), device="cuda")
    K.attn_append(nd.data_ptr(), pd.data_ptr(), nn.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                  out.data_ptr(), ws.data_ptr(), B, T, H, C, max_len, splits, SCALE, _st())
    torch.cuda.synchronize()
    return out.cpu(), kc.cpu(), vc.cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ----------------------------------------------------------------------------- 1. fp64 bound
@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("T,pos,n_new", CASES)
def test_attn_append_bound(T, pos, n_new, splits):
    _, _, after, (ref, bnd), live = _case(T, pos, n_new)
    out, kc, vc = _run(T, pos, n_new, splits)
    print(f"MEASURE append out/bound T={T} pos={pos} splits={splits} {_ratio(out, ref, bnd):.4f}")
    assert_within(out, ref, bnd, f"attn_append T={T} pos={pos} splits={splits}")   # finite, too
    assert bool((out[~live] == 0).all())
    # rows p0 .. p0+n-1 are the new K and V bit for bit, every other element is bit-unchanged
    assert _same_bits(kc, after[0]) and _same_bits(vc, after[1])


# ----------------------------------------------------------------------------- 2. determinism
@pytest.mark.gpu
def test_attn_append_is_deterministic_and_splits_agree():
    case = CASES[3]
    bnd = _case(*case)[3][1]
    outs = {}
    for splits in (1, 2, 4):
        a, b = (_run(*case, splits)[0] for _ in range(2))
        assert _same_bits(a, b), splits
        outs[splits] = a
    for splits in (2, 4):
        assert_within(outs[splits], outs[1].double(), 2 * bnd, f"splits {splits} against 1")


# ----------------------------------------------------------------------------- 3. refusals
@pytest.mark.gpu
def test_attn_append_refusals():
    K = _K()
    T, pos, n_new = CASES[2]
    new, caches = _case(T, pos, n_new)[:2]
    nd, kc, vc = _dev(new), _dev(caches[0]), _dev(caches[1])
    pd = torch.tensor(pos, dtype=torch.int32, device="cuda")
    out = torch.zeros(B * T, H * AD, device="cuda", dtype=BF16)
    ws = torch.zeros(K.attn_append_ws_floats(B, H, T, 4), device="cuda")

    def call(cap=C, max_len=C, splits=1, t=T, q=nd.data_ptr(), w=ws.data_ptr()):
        K.attn_append(q, pd.data_ptr(), 0, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), w, B, t,
                      H, cap, max_len, splits, SCALE, _st())

    for kw, msg in ((dict(q=0), "null"), (dict(cap=96, max_len=96), "multiple of 64"),
                    (dict(t=0), "T >= 1"), (dict(max_len=T - 1), "max_len"),
                    (dict(max_len=C + 64), "max_len"), (dict(max_len=128, splits=3), "splits"),
                    (dict(splits=2, w=0), "workspace")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    call(max_len=128, splits=2)
    with pytest.raises(ValueError, match="qkv_new"):
        ops.attention_append(nd[:, :-64].contiguous(), kc, vc, pd, H)
    with pytest.raises(ValueError, match="splits"):
        ops.attention_append(nd, kc, vc, pd, H, max_len=128, splits=3)
    with pytest.raises(ValueError, match="n_new"):
        ops.attention_append(nd, kc, vc, pd, H, n_new=pd.long())
    assert K.attn_append_splits(8, 12, 16, 64) == 1 and K.attn_append_splits(1, 12, 16, 2048) > 1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 4. the model
@pytest.mark.gpu
def test_chunked_prefill_and_extend_match_the_full_forward_on_the_device():
    """prefill(chunk=16) + one extend of 8 teacher-forced tokens against the rows of the full
    causal forward over the 128-padded sequence.  The tolerance is that of
    tests/test_decode_gpu.py, for its reason: both are bf16 computations of the fp32 model with
    independent roundings of the same size, so they differ by at most twice the bf16 forward's
    own distance to the fp32 CPU result at the same positions."""
    from distributedtensorflow_amd.models import KVCache
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    cpu = BertForPreTraining(BertConfig(**TINY)).eval()
    gpu = copy.deepcopy(cpu).cuda().eval()
    lens, steps, rows = torch.tensor([5, 64]), 8, torch.arange(2).view(2, 1)
    prompt = torch.randint(1, 256, (2, 64), generator=_gen(3))
    prompt = prompt * (torch.arange(64).view(1, 64) < lens.view(2, 1))
    gen = gpu.generate(prompt.cuda(), lens, steps + 1, prefill_chunk=16).cpu()
    seq = torch.zeros(2, 128, dtype=torch.int64)
    seq[:, :64] = prompt
    for b in range(2):
        seq[b, lens[b]:lens[b] + steps + 1] = gen[b]
    at = lens.view(2, 1) - 1 + torch.arange(steps + 1).view(1, -1)   # positions compared
    with torch.no_grad():
        ref32 = cpu(seq).view(2, 128, -1)[rows, at]
        full = gpu(seq.cuda()).view(2, 128, -1)[rows.cuda(), at.cuda()].float().cpu()
    cache = KVCache(gpu.cfg, 2, 128, "cuda")
    first = gpu.prefill(prompt.cuda(), lens, cache, chunk=16)
    more = gpu.extend(gen[:, :steps].cuda(), cache, all_logits=True)
    got = torch.cat([first.unsqueeze(1), more], 1).float().cpu()      # [2, steps + 1, V]
    assert torch.equal(cache.pos.cpu(), (lens + steps).int())
    tol = 2 * float((full - ref32).abs().max())
    err = float((got - full).abs().max())
    print(f"MEASURE append-vs-forward / tolerance {err / tol:.4f} (tolerance {tol:.4f})")
    assert err <= tol
    assert torch.equal(got.argmax(-1), gen)
