"""The deferred LayerNorm of the skinny-M dense kernel (csrc/kernels/dense_skinny.hip,
dense_skinny_ln_kernel) on the device: per element against fp64, rows past M, and a decode step of
the model.  Named to sort after tests/test_resnet_gpu.py (see tests/test_skinny_model_gpu.py).

Bound.  The reference is fp64 on the stored bf16 inputs with the LayerNorm in fp64, NOT rounded.
With a = LN(x) (pre_ln) or x, z = a W^T + b (+ r, r = res or LN(res)):
  E = gamma(K + 8) (|a| |W|^T + |b| + |r|)      the fp32 sums, as tests/test_skinny_dense_gpu.py
    + 2^-8 (|LN(x)| |W|^T)                      pre_ln: a full bf16 spacing per operand element
                                                covers its rounding and fp32-against-fp64 statistics
    + 2^-8 |LN(res)|                            residual_ln: the same for the rounded residual
  bias epilogue:  U16 (|z| + E) + E;   bias + GELU:  gelu_fwd_bound(z) + 1.13 (1 + U16) E.
Measured on an MI355X: see profiles/SKINNY_LN.md.
"""
import copy

import pytest
import torch

from fp64_util import BF16, U16, assert_within, gamma, measure
from test_decode_gpu import TINY
from test_nlp_kernels_gpu import _gen, gelu_fwd_bound

EPS = 1e-12


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def data():
    """x / res [64, 768], W [768, 768] (bf16 values), b, gamma, beta [768], made once."""
    g = _gen(23)
    x, res = (torch.randn(64, 768, generator=g).to(BF16) for _ in range(2))
    w = (0.05 * torch.randn(768, 768, generator=g)).to(BF16)
    b, bt = torch.randn(768, generator=g), torch.randn(768, generator=g)
    return x, res, w, b, 1 + 0.2 * torch.randn(768, generator=g), bt


def _ref64(x, res, w, b, gm, bt, mode):
    """fp64 (reference, bound of the module docstring) of one mode on CPU operands."""
    def ln(t):
        d = t.double() - t.double().mean(1, keepdim=True)
        n = t.shape[1]
        return d / (d.pow(2).mean(1, keepdim=True) + EPS).sqrt() * gm[:n].double() + bt[:n].double()
    K, pre = x.shape[1], mode.startswith("pre_ln")
    a, w64 = ln(x) if pre else x.double(), w.double()
    mag = a.abs() @ w64.abs().t()
    z, e = a @ w64.t() + b.double(), gamma(K + 8) * (mag + b.double().abs())
    if pre:
        e = e + U16 * mag
    if "residual" in mode:
        r = ln(res) if mode == "residual_ln" else res.double()
        z = z + r
        e = e + gamma(K + 8) * r.abs() + (U16 * r.abs() if mode == "residual_ln" else 0)
    if mode == "pre_ln_gelu":
        ref, bnd = gelu_fwd_bound(z)
        return ref, bnd + 1.13 * (1 + U16) * e
    return z, U16 * (z.abs() + e) + e


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,offset", [(M, N, K, False) for M in (1, 16, 17, 64)
                                          for N, K in ((16, 64), (80, 256), (768, 768))]
                         + [(17, 80, 256, True)])
def test_deferred_ln_bound(data, M, N, K, offset):
    """Every mode and K split against fp64.  ``offset``: the live rows are 64 + N(0, 1) (a
    one-pass variance E[x^2] - mean^2 cancels there) at the head of 32-row allocations whose other
    rows are NaN (a row-tile select after the normalisation lets them through)."""
    from distributedtensorflow_amd.ops import native
    x, res, w, b, gm, bt = data
    x, res, w, b = x[:M, :K].contiguous(), res[:M, :N].contiguous(), w[:N, :K].contiguous(), b[:N]
    if offset:
        x, res = (64 + x.float()).to(BF16), (64 + res.float()).to(BF16)
    xd = torch.full((32 if offset else M, K), float("nan"), device="cuda", dtype=BF16)[:M]
    resd = torch.full((32 if offset else M, N), float("nan"), device="cuda", dtype=BF16)[:M]
    xd.copy_(x)
    resd.copy_(res)
    wd, bd = w.cuda(), b.cuda()
    ln_k, ln_n = ((gm[:n].cuda(), bt[:n].cuda(), EPS) for n in (K, N))
    kws = {"pre_ln": dict(pre_ln=ln_k), "pre_ln_gelu": dict(pre_ln=ln_k, gelu=True),
           "residual": dict(residual=resd), "residual_ln": dict(residual=resd, residual_ln=ln_n),
           "pre_ln_residual": dict(pre_ln=ln_k, residual=resd)}
    worst = 0.0
    for mode, kw in kws.items():
        ref, bnd = _ref64(x, res, w, b, gm, bt, mode)
        for splits in sorted({1, K // 64}):
            with torch.no_grad():
                y = native._dense_skinny(xd, wd, bd, splits=splits, **kw).cpu()
            tag = f"dense_skinny_ln M={M} N={N} K={K} offset={offset} {mode} splits={splits}"
            worst = max(worst, measure(tag, y, ref, bnd))
            assert_within(y, ref, bnd, tag)
    print(f"MEASURE dense_skinny_ln worst M={M} K={K} offset={offset} {worst:.4f}")

@pytest.mark.gpu
def test_decode_steps_with_deferred_layer_norms_match_the_default_steps():
    """As tests/test_skinny_model_gpu.py with gemm="skinny_ln": the tolerance is twice the bf16
    forward's own distance to the fp32 CPU result."""
    from distributedtensorflow_amd.models import KVCache
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    cpu = BertForPreTraining(BertConfig(**TINY)).eval()
    with torch.no_grad():                                  # LayerNorms that are not the identity
        for p in cpu.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    gpu = copy.deepcopy(cpu).cuda().eval()
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
    err = 0.0
    for t in range(steps):
        twin = copy.deepcopy(cache)
        ref = gpu.decode_step(gen[:, t].cuda(), cache)
        got = gpu.decode_step(gen[:, t].cuda(), twin, gemm="skinny_ln")
        assert got.shape == ref.shape
        err = max(err, float((got.float() - ref.float()).abs().max()))
    print(f"MEASURE skinny_ln-vs-default decode / tolerance {err / tol:.4f} (tolerance {tol:.4f})")
    assert err <= tol
    ids = torch.randint(1, 256, (2, 16), generator=_gen(4)).cuda()
    assert gpu.extend(ids, cache, gemm="skinny_ln").shape == (2, 256)
    out = gpu.generate(prompt.cuda(), lens, steps, decode_gemm="skinny_ln", prefill_chunk=16)
    assert out.shape == (2, steps)
