"""The skinny-M dense kernel on FP8 weights (csrc/kernels/dense_skinny_f8.hip) on the device: the
quantiser bit for bit, the GEMM per element against fp64 on the DEQUANTISED matrix (exact in bf16,
so the bounds of tests/test_skinny_dense_gpu.py and tests/test_skinny_ln_gpu.py apply unchanged),
bit-reproducible, never reading past M, its refusals, and decode steps of the model.  Named to
sort after tests/test_resnet_gpu.py (see tests/test_skinny_model_gpu.py).

Measured on an MI355X: see profiles/SKINNY_W8.md."""
import copy
import functools

import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.ops import reference
from fp64_util import BF16, SENT, U16, assert_within, gamma, measure
from test_decode_gpu import TINY
from test_nlp_kernels_gpu import _K, _gen, _st, gelu_fwd_bound
from test_skinny_dense_gpu import _data, _release_cached_blocks          # noqa: F401 (fixture)
from test_skinny_ln_gpu import EPS, _ref64, data                          # noqa: F401 (fixture)


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(16, 64), (80, 256)])
def test_quantiser_is_the_rule_bit_for_bit(N, K):
    w = torch.randn(N, K, generator=_gen(7)).to(BF16)
    w[0, :64] = 0                                          # an all-zero unit: e = 0
    w[1, :64] = w[1, :64].clamp(-1, 1)
    w[1, 5] = 7.0                                          # largest magnitude 0.875 * 2^3: e = k - 9
    w[2, :64] = w[2, :64].clamp(-1, 1)
    w[2, 9] = -7.03125                                     # one bf16 ulp above it: e = k - 8
    w[3, :64] = (w[3, :64].float().clamp(-1, 1) * 2.0 ** -120).to(BF16)   # the exponent clamps
    w[4, :64] = (w[4, :64].float() * 2.0 ** 100).to(BF16)
    want_q, want_s = reference.weight_quantize_fp8(w)
    q, s = ops.weight_quantize_fp8(w.cuda())
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert torch.equal(q.cpu().view(torch.int8), want_q.view(torch.int8))
    assert torch.equal(s.cpu(), want_s)
    assert float(want_s[3, 0]) == 2.0 ** -100 and float(want_s[1, 0]) * 2 == float(want_s[2, 0])


# 64: one unit, three waves idle; 256: one unit per wave; 2304: 9 units per wave with one split,
# a full load-ahead batch (8 units at up to 32 rows, two of 4 above) and a one-unit tail batch
KS = (64, 256, 2304)


@functools.lru_cache(maxsize=None)
def _oracle(K):
    """The weights of tests/test_skinny_dense_gpu.py with every (row, unit) times 2^r, r in
    [-12, 12], quantised by the rule -> (q, scale, fp64 x Wq^T, fp64 |x| |Wq|^T) for 64 rows and
    80 outputs: a wrong scale index or k permutation misses by orders of magnitude."""
    x, w, _ = _data()
    r = torch.randint(-12, 13, (80, K // 64, 1), generator=_gen(13))
    ws = (w[:80, :K].float().view(80, K // 64, 64) * torch.exp2(r.float())).view(80, K).to(BF16)
    pair = reference.weight_quantize_fp8(ws)
    x64, w64 = x[:, :K].double(), reference.weight_dequantize(pair).double()
    return pair[0], pair[1], x64 @ w64.t(), x64.abs() @ w64.abs().t()


def _launch(xd, q, s, bd, epi, splits):
    (M, K), N = xd.shape, q.shape[0]
    n = splits or _K().dense_skinny_splits(M, N, K)
    ws = torch.full((max(1, n * M * N),), float("nan"), device="cuda")
    y = torch.full((M, N), SENT, device="cuda", dtype=BF16)
    _K().dense_skinny_w8(xd.data_ptr(), q.data_ptr(), s.data_ptr(), bd.data_ptr(), y.data_ptr(),
                         ws.data_ptr(), M, N, K, xd.stride(0), epi, splits, _st())
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", (1, 16, 17, 64))
def test_dense_skinny_w8_bound(M, K):
    """The bound of test_dense_skinny_bound, unchanged, against fp64 on the dequantised matrix."""
    x, _, b = _data()
    q, s, dot, mag = _oracle(K)
    xd, bd = x[:M, :K].contiguous().cuda(), b.cuda()
    worst = 0.0
    for N in (16, 80):
        qd, sd = q[:N].contiguous().cuda(), s[:N].contiguous().cuda()
        z = dot[:M, :N] + b[:N].double()
        e32 = gamma(K + 8) * (mag[:M, :N] + b[:N].double().abs())
        gref, gbnd = gelu_fwd_bound(z)
        want = {0: (dot[:M, :N], U16 * (dot[:M, :N].abs() + e32) + e32),
                1: (z, U16 * (z.abs() + e32) + e32),
                2: (gref, gbnd + 1.13 * (1 + U16) * e32)}
        for epi, (ref, bnd) in want.items():
            for splits in (0, 1, K // 64):
                y = _launch(xd, qd, sd, bd, epi, splits).cpu()
                tag = f"dense_skinny_w8 M={M} N={N} K={K} epi={epi} splits={splits}"
                worst = max(worst, measure(tag, y, ref, bnd))
                assert_within(y, ref, bnd, tag)
    print(f"MEASURE dense_skinny_w8 worst M={M} K={K} {worst:.4f}")


def _ln_case(data, M, rows=None):
    """Device operands of the (N, K) = (80, 256) deferred-LayerNorm case -> (CPU operands with the
    dequantised weight, x, the pair, bias, residual, ln_k, ln_n); ``rows``: x and the residual are
    the head of ``rows``-row allocations whose other rows are NaN."""
    x, res, w, b, gm, bt = data
    N, K = 80, 256
    x, res, b = x[:M, :K].contiguous(), res[:M, :N].contiguous(), b[:N]
    pair = reference.weight_quantize_fp8(w[:N, :K])
    wq = reference.weight_dequantize(pair, BF16)
    xd = torch.full((rows or M, K), float("nan"), device="cuda", dtype=BF16)[:M]
    resd = torch.full((rows or M, N), float("nan"), device="cuda", dtype=BF16)[:M]
    xd.copy_(x)
    resd.copy_(res)
    ln_k, ln_n = ((gm[:n].cuda(), bt[:n].cuda(), EPS) for n in (K, N))
    return (x, res, wq, b, gm, bt), xd, tuple(t.cuda() for t in pair), b.cuda(), resd, ln_k, ln_n


@pytest.mark.gpu
@pytest.mark.parametrize("M", (1, 17))
def test_deferred_ln_on_fp8_weights_bound(data, M):
    """The bound of tests/test_skinny_ln_gpu.py; gamma and beta vary along k, so a gamma / beta
    index that does not follow the kernel's k permutation fails."""
    from distributedtensorflow_amd.ops import native
    cpu, xd, pair, bd, resd, ln_k, ln_n = _ln_case(data, M)
    kws = {"pre_ln": dict(pre_ln=ln_k), "pre_ln_gelu": dict(pre_ln=ln_k, gelu=True),
           "residual": dict(residual=resd), "residual_ln": dict(residual=resd, residual_ln=ln_n)}
    worst = 0.0
    for mode, kw in kws.items():
        ref, bnd = _ref64(*cpu, mode)
        for splits in (1, 4):
            with torch.no_grad():
                y = native._dense_skinny(xd, pair, bd, splits=splits, **kw).cpu()
            tag = f"dense_skinny_ln_w8 M={M} {mode} splits={splits}"
            worst = max(worst, measure(tag, y, ref, bnd))
            assert_within(y, ref, bnd, tag)
    print(f"MEASURE dense_skinny_ln_w8 worst M={M} {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["plain", "ln"])
def test_same_bits_twice_and_never_reads_past_m(data, family):
    from distributedtensorflow_amd.ops import native
    outs = []
    for rows in (None, None, 32):                 # twice tight, then NaN in rows 17 to 31
        _, xd, pair, bd, resd, ln_k, _ = _ln_case(data, 17, rows)
        kw = dict(gelu=True) if family == "plain" else dict(pre_ln=ln_k, residual=resd)
        with torch.no_grad():
            outs.append(native._dense_skinny(xd, pair, bd, splits=4, **kw))
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))
    assert bool(torch.isfinite(outs[2].float()).all())


def _tiny(device):
    """The tiny causal BERT with an embedding table that FP8 holds exactly (the tied table is also
    the lookup's, which keeps the master: both arms below must look up the same rows)."""
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    model = BertForPreTraining(BertConfig(**TINY)).eval()
    with torch.no_grad():
        for p in model.parameters():                           # LayerNorms that are not the identity
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        model.word_embeddings.copy_(reference.weight_dequantize(
            reference.weight_quantize_fp8(model.word_embeddings)))
    return model.to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["impl_none", "impl_library", "scale_shape", "scale_dtype",
                                  "q_strided", "never_quantized"])
def test_refusals(case):
    x = torch.zeros(8, 128, device="cuda", dtype=BF16)
    q, s = ops.weight_quantize_fp8(torch.randn(16, 128, device="cuda"))
    with torch.no_grad(), pytest.raises(ValueError):
        if case == "never_quantized":
            from distributedtensorflow_amd.models import KVCache
            model = _tiny("cuda")
            model.decode_step(torch.zeros(2, dtype=torch.int64, device="cuda"),
                              KVCache(model.cfg, 2, 64, "cuda"), gemm="skinny_w8")
        pair = {"scale_shape": (q, s[:, :1].contiguous()), "scale_dtype": (q, s.double()),
                "q_strided": (q.t().contiguous().t(), s)}.get(case, (q, s))
        ops.dense(x, pair, None, impl={"impl_none": None, "impl_library": "library"}.get(
            case, "skinny"))


@pytest.mark.gpu
def test_decode_steps_on_fp8_weights_match_the_steps_on_the_dequantised_weights():
    """4 teacher-forced steps: gemm="skinny_w8" / "skinny_ln_w8" against "skinny" / "skinny_ln" on
    a copy whose quantised matrices hold their dequantised values, same cache contents.  Both arms
    see exactly the same weights, so this isolates the kernel from the quantisation error; the
    tolerance is that of tests/test_skinny_model_gpu.py."""
    from distributedtensorflow_amd.models import KVCache
    cpu = _tiny("cpu")
    gpu = copy.deepcopy(cpu).cuda().quantize_weights()
    twin = copy.deepcopy(gpu)
    with torch.no_grad():
        for p, p2 in zip(gpu._w8_params(), twin._w8_params()):
            p2.copy_(reference.weight_dequantize(p._dtf_w8))
    lens, steps = torch.tensor([5, 64]), 4
    prompt = torch.randint(1, 256, (2, 64), generator=_gen(3))
    prompt = prompt * (torch.arange(64).view(1, 64) < lens.view(2, 1))
    gen = gpu.generate(prompt.cuda(), lens, steps).cpu()
    seq = torch.zeros(2, 128, dtype=torch.int64)
    seq[:, :64] = prompt
    for r in range(2):
        seq[r, lens[r]:lens[r] + steps] = gen[r]
    at = lens.view(2, 1) + torch.arange(steps).view(1, -1)
    with torch.no_grad():
        diff = (gpu(seq.cuda()).float().cpu() - cpu(seq)).view(2, 128, -1)
        tol = 2 * float(diff[torch.arange(2).view(2, 1), at].abs().max())
    cache = KVCache(gpu.cfg, 2, 128, "cuda")
    gpu.prefill(prompt.cuda(), lens, cache)
    err, qerr = {"skinny": 0.0, "skinny_ln": 0.0}, 0.0
    for t in range(steps):
        tok = gen[:, t].cuda()
        for g in err:
            got = gpu.decode_step(tok, copy.deepcopy(cache), gemm=g + "_w8")
            ref = twin.decode_step(tok, copy.deepcopy(cache), gemm=g)
            err[g] = max(err[g], float((got.float() - ref.float()).abs().max()))
        ref = gpu.decode_step(tok, cache, gemm="skinny")
        qerr = max(qerr, float((got.float() - ref.float()).abs().max()))
    print(f"MEASURE w8-vs-dequantised decode / tolerance skinny {err['skinny'] / tol:.4f} "
          f"skinny_ln {err['skinny_ln'] / tol:.4f} (tolerance {tol:.4f}); the quantisation error "
          f"itself, w8 against bf16 logits: {qerr:.4f}")
    assert max(err.values()) <= tol
    out = gpu.generate(prompt.cuda(), lens, steps, decode_gemm="skinny_ln_w8", seed=1,
                       kv_dtype="fp8")
    assert out.shape == (2, steps) and int(out.min()) >= 0 and int(out.max()) < gpu.cfg.vocab_size
