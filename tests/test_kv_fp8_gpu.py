"""The FP8 (e4m3) KV cache on the device: kv_cache_fill_f8_kernel / attn_decode_f8_kernel
(csrc/kernels/attn_f8.hip), kv_cache_append_f8_kernel / attn_append_kernel<QT, F8 = true>
(csrc/kernels/attn_append.hip), the ops and the model.

The cache bytes and scales must equal ``ops.reference.kv_quantize_rows`` bit for bit.  Because
dequantising is exact, the attention kernels compute the bf16 kernels' function of the DEQUANTISED
cache: the oracle is fp64 attention over it and the bounds are those of tests/test_decode_gpu.py
(one bf16 rounding: ``u = U16``) and tests/test_append_gpu.py (P rounded for the MFMA too:
``u = 2 U16``), ``(u + rel32) (P @ |v|)`` with their ``rel32``.  Every cache row the call may not
read holds 0x7F bytes (NaN) and a NaN scale.  Measured on an MI355X: see profiles/KV_FP8.md.
"""
import copy
import functools

import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.ops import reference as R
from test_append import CASES
from test_decode_gpu import POS, TINY
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


B, H, SCALE = 2, 3, AD ** -0.5
F8 = torch.float8_e4m3fn


def _junk(C):
    """An unwritten fp8 cache and its scales: 0x7F bytes, NaN scales."""
    return (torch.full((B, H, C, AD), 0x7F, dtype=torch.uint8).view(F8),
            torch.full((B, H, C), float("nan")))


def _same(a, b):
    bits = lambda t: t.cpu().view(torch.uint8 if t.dtype == F8 else torch.int32)
    return torch.equal(bits(a), bits(b))


# append: uneven pos / n_new, a row with n = 0, a row that ends at C = 128, n clamped by C
@pytest.mark.gpu
@pytest.mark.parametrize("T,pos,n_new", [(0, S, None) for S in (1, 63, 64, 100)]
                         + [(16, (3, 112), (0, 16)), (5, (60, 100), (5, 3)),
                            (40, (7, 120), (33, 40))])
def test_fill_and_append_copy_are_the_rule_bit_for_bit(T, pos, n_new):
    """T = 0: kv_cache_fill of S = pos tokens.  Against the reference backend's caches, which
    tests/test_kv_fp8.py holds to the rule: written and unwritten bytes and scales, bit for bit."""
    C = 128
    qkv, _, _ = _attn_inputs(B, T or pos, H, _gen(T + sum(pos) if T else pos), masked=False)
    qkv[::7] *= 2.0 ** -20                                            # rows of another magnitude
    qkv[-1] = 0                                                       # an all-zero row
    want, got = [t for t in _junk(C) + _junk(C)], [_dev(t) for t in _junk(C) + _junk(C)]
    for dev, (kq, ks, vq, vs) in (("cpu", want), ("cuda", got)):
        x = qkv.to(dev)
        if T == 0:
            ops.kv_cache_fill(x, kq, vq, B, pos, H, k_scale=ks, v_scale=vs)
        else:
            i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
            ops.attention_append(x, kq, vq, i32(pos), H, n_new=i32(n_new), k_scale=ks, v_scale=vs)
    written = int((~torch.isnan(want[1])).sum())
    assert written == H * (B * pos if T == 0 else sum(min(n, C - p) for p, n in zip(pos, n_new)))
    for g, w in zip(got, want):
        assert _same(g, w)


@functools.lru_cache(maxsize=None)
def _case(T, pos, n_new, u):
    """tests/test_append_gpu.py's case (T = 1, n_new = 1: tests/test_decode_gpu.py's) on an FP8
    cache -> (qkv_new, caches (k bytes, k scale, v bytes, v scale) before and after the call,
    (out64, bound) [B*T, H*64] over the dequantised cache, live [B*T])."""
    C = 256
    old, _, _ = _attn_inputs(B, C, H, _gen(T), masked=False)
    new, _, _ = _attn_inputs(B, T, H, _gen(1000 + T), masked=False)
    p0, n = torch.tensor(pos).view(B, 1), torch.tensor(n_new).view(B, 1)
    _, ko, vo = _split_qkv(old, B, C, H)
    q, kn, vn = _split_qkv(new, B, T, H)
    row = torch.arange(C).view(1, C)
    fresh = ((row >= p0) & (row < p0 + n)).view(B, 1, C, 1)
    src = (row - p0).clamp(0, T - 1).view(B, 1, C, 1).expand(B, H, C, AD)
    packed = [R.kv_quantize_rows(torch.where(fresh, tn.gather(2, src), to).to(BF16))
              for tn, to in ((kn, ko), (vn, vo))]
    k, v = (R.kv_dequantize(b, s).double() for b, s in packed)        # what the kernels must see
    i = torch.arange(T).view(1, T)
    live = i < n
    vis = ((row.view(1, 1, C) <= (p0 + i).view(B, T, 1)) & live.view(B, T, 1)).view(B, 1, T, C)
    s2, smag = _scores(q, k, None, B, C, SCALE)
    s2 = torch.where(vis, s2, torch.full_like(s2, float("-inf")))
    smax = torch.where(vis, smag, torch.zeros_like(smag)).max(-1, keepdim=True).values
    P = torch.where(vis, torch.exp2(s2 - s2.max(-1, keepdim=True).values.clamp_min(-1e300)),
                    torch.zeros_like(s2))
    P = P / P.sum(-1, keepdim=True).clamp_min(1e-300)
    glen = torch.tensor([[gamma(p + t + 1 + 8) for t in range(T)] for p in pos],
                        dtype=torch.float64).view(B, 1, T, 1)
    rel32 = glen + 2 * LN2 * gamma(70) * smax + 2 * INTR
    oracle = (_rows(P @ v, B, T, H), _rows((u + rel32) * (P @ v.abs()), B, T, H))
    before, after = [], []
    for (b, s), (jb, js) in zip(packed, (_junk(C), _junk(C))):
        for upto, dst in ((p0, before), (p0 + n, after)):
            keep = (row < upto).view(B, 1, C)
            dst += [torch.where(keep.unsqueeze(-1), b.view(torch.uint8),
                                jb.view(torch.uint8)).view(F8), torch.where(keep, s, js)]
    return new, before, after, oracle, live.reshape(-1)


def _run(decode, T, pos, n_new, splits, u):
    K = _K()
    new, before = _case(T, pos, n_new, u)[:2]
    kq, ks, vq, vs = (_dev(t) for t in before)
    nd = _dev(new)
    pd, nn = (_dev(torch.tensor(t, dtype=torch.int32)) for t in (pos, n_new))
    out = torch.full((B * T, H * AD), SENT, device="cuda", dtype=BF16)
    nws = (K.attn_decode_ws_floats(B, H, splits) if decode
           else K.attn_append_ws_floats(B, H, T, splits))
    ws = torch.full((max(1, nws),), float("nan"), device="cuda")
    ptr = [t.data_ptr() for t in (kq, vq, ks, vs, out, ws)]
    if decode:
        K.attn_decode_f8(nd.data_ptr(), pd.data_ptr(), *ptr, B, H, 256, 256, splits, SCALE, _st())
    else:
        K.attn_append_f8(nd.data_ptr(), pd.data_ptr(), nn.data_ptr(), *ptr, B, T, H, 256, 256,
                         splits, SCALE, _st())
    torch.cuda.synchronize()
    return out.cpu(), [kq, ks, vq, vs]


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("name,T,pos,n_new", [("decode", 1, p, (1, 1)) for p in POS]
                         + [("append", *c) for c in CASES])
def test_fp8_attention_bound(name, T, pos, n_new, splits):
    decode = name == "decode"
    u = U16 if decode else 2 * U16
    _, _, after, (ref, bnd), live = _case(T, pos, n_new, u)
    out, caches = _run(decode, T, pos, n_new, splits, u)
    print(f"MEASURE fp8 {name} out/bound T={T} pos={pos} splits={splits} "
          f"{_ratio(out, ref, bnd):.4f}")
    assert_within(out, ref, bnd, f"fp8 {name} T={T} pos={pos} splits={splits}")
    assert bool((out[~live] == 0).all())
    # the new rows hold the rule's bytes and scales, everything else is bit-unchanged
    for got, want in zip(caches, after):
        assert _same(got, want)
    assert _same(_run(decode, T, pos, n_new, splits, u)[0], out)       # the same bits twice


@pytest.mark.gpu
def test_fp8_cache_model_matches_the_reference_backend():
    """Prefill, 8 teacher-forced decode steps and one extend with an FP8 cache, on the device
    against the CPU reference backend.  The tolerance is the rule of tests/test_decode_gpu.py:
    twice the bf16 forward's own distance to the fp32 CPU result at the same positions.  The
    backends quantise keys that differ by the bf16 roundings: the differing bytes are counted."""
    from distributedtensorflow_amd.models import KVCache
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    cpu = BertForPreTraining(BertConfig(**TINY)).eval()
    gpu = copy.deepcopy(cpu).cuda().eval()
    lens, steps, ext, rows = torch.tensor([5, 64]), 8, 4, torch.arange(2).view(2, 1)
    seq = torch.randint(1, 256, (2, 128), generator=_gen(3))
    prompt = seq[:, :64] * (torch.arange(64).view(1, 64) < lens.view(2, 1))
    forced = seq[:, 64:64 + steps + ext].clone()
    for b in range(2):
        seq[b, lens[b]:lens[b] + steps + ext] = forced[b]
    at = lens.view(2, 1) - 1 + torch.arange(steps + ext + 1).view(1, -1)
    with torch.no_grad():
        ref32 = cpu(seq).view(2, 128, -1)[rows, at]
        full = gpu(seq.cuda()).view(2, 128, -1)[rows.cuda(), at.cuda()].float().cpu()
    got = []
    for m, dev, dtype in ((gpu, "cuda", BF16), (cpu, "cpu", torch.float32)):
        cache = KVCache(m.cfg, 2, 128, dev, dtype, kv_dtype="fp8")
        logits = [m.prefill(prompt.to(dev), lens, cache).unsqueeze(1)]
        logits += [m.decode_step(forced[:, t].to(dev), cache).unsqueeze(1) for t in range(steps)]
        logits.append(m.extend(forced[:, steps:].to(dev), cache, all_logits=True))
        assert torch.equal(cache.pos.cpu(), (lens + steps + ext).int())
        got.append((torch.cat(logits, 1).float().cpu(), cache))
    (a, ca), (b, cb) = got
    held = (torch.arange(128).view(1, 128) < (lens + steps + ext).view(2, 1)).view(1, 2, 1, 128, 1)
    diff = ((ca.k.cpu().view(torch.uint8) != cb.k.view(torch.uint8)) & held).sum()
    tol = 2 * float((full - ref32).abs().max())
    err = float((a - b).abs().max())
    total = int(held.sum()) * ca.k.shape[0] * ca.k.shape[2] * 64
    print(f"MEASURE fp8 model device-vs-reference / tolerance {err / tol:.4f} (tolerance "
          f"{tol:.4f}); {int(diff)} of {total} cached K bytes differ")
    assert err <= tol
