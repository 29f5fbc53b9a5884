"""The skinny-M dense kernel (csrc/kernels/dense_skinny.hip) on the device: per element against
fp64, bit-reproducible, never reading past M, and its refusals (a decode step of the model:
tests/test_skinny_model_gpu.py).

Bound.  fp64_util has no form for a K-long fp32 dot product, so, with z = x W^T + b in fp64 on the
stored bf16 x and W:  E32 = gamma(K + 8) (|x| |W|^T + |b|) covers the fp32 accumulation in any
order (K products, the wave and split merges, the bias add), and the result rounds once to bf16:
  epilogues none / bias:  U16 (|z| + E32) + E32
  bias + GELU:            gelu_fwd_bound(z) of tests/test_nlp_kernels_gpu.py (the evaluation of
                          gelu_f and its one rounding) + 1.13 (1 + U16) E32 (|gelu'| <= 1.13).
Measured on an MI355X: see profiles/SKINNY.md.
"""
import functools

import pytest
import torch

from distributedtensorflow_amd import ops
from fp64_util import BF16, SENT, U16, assert_within, gamma, measure
from test_nlp_kernels_gpu import _K, _gen, _st, gelu_fwd_bound


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    """This module leaves odd-sized cached blocks behind; test_resnet_gpu compares
    ``max_memory_allocated`` between steps to within a few MB, so they are released when it is
    done (as in tests/test_decode_gpu.py)."""
    yield
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


MS, NS = (1, 15, 16, 17, 64), (16, 80, 768)
# 64: one unit, three waves of a block get none; 256: one unit per wave; 3072: the FFN's K
KS = (64, 256, 3072)


@functools.lru_cache(maxsize=None)
def _data():
    """x [64, 3072], W [768, 3072] (bf16 values) and b [768], made once; every case is a corner."""
    g = _gen(11)
    x = torch.randn(64, 3072, generator=g).to(BF16)
    w = (0.05 * torch.randn(768, 3072, generator=g)).to(BF16)
    b = torch.randn(768, generator=g)
    return x, w, b


@functools.lru_cache(maxsize=None)
def _oracle(K):
    """fp64 (x W^T, |x| |W|^T) over the first K columns, for all 64 rows and 768 outputs."""
    x, w, _ = _data()
    x64, w64 = x[:, :K].double(), w[:, :K].double()
    return x64 @ w64.t(), x64.abs() @ w64.abs().t()


def _launch(xd, wd, bd, epi, splits, ldx=None):
    """The binding on device tensors xd [M, K] (row stride ldx), wd [N, K], bd [N] -> y [M, N]."""
    K_ = _K()
    (M, K), N = xd.shape, wd.shape[0]
    n = splits or K_.dense_skinny_splits(M, N, K)
    ws = torch.full((max(1, n * M * N),), float("nan"), device="cuda")
    y = torch.full((M, N), SENT, device="cuda", dtype=BF16)
    K_.dense_skinny(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), ws.data_ptr(), M,
                    N, K, ldx or xd.stride(0), epi, splits, _st())
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_dense_skinny_bound(M, K):
    x, w, b = _data()
    dot, mag = _oracle(K)
    xd, bd = x[:M, :K].contiguous().cuda(), b.cuda()
    worst = 0.0
    for N in NS:
        wd = w[:N, :K].contiguous().cuda()
        z = dot[:M, :N] + b[:N].double()
        e32 = gamma(K + 8) * (mag[:M, :N] + b[:N].double().abs())
        gref, gbnd = gelu_fwd_bound(z)
        want = {0: (dot[:M, :N], U16 * (dot[:M, :N].abs() + e32) + e32),
                1: (z, U16 * (z.abs() + e32) + e32),
                2: (gref, gbnd + 1.13 * (1 + U16) * e32)}
        for epi, (ref, bnd) in want.items():
            for splits in (0, 1, K // 64):
                y = _launch(xd, wd, bd, epi, splits).cpu()
                tag = f"dense_skinny M={M} N={N} K={K} epi={epi} splits={splits}"
                worst = max(worst, measure(tag, y, ref, bnd))
                assert_within(y, ref, bnd, tag)
    print(f"MEASURE dense_skinny worst M={M} K={K} {worst:.4f}")


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [0, 1, 4])
def test_dense_skinny_same_bits_twice_and_never_reads_past_m(splits):
    x, w, b = _data()
    M, N, K = 17, 80, 256
    wd, bd = w[:N, :K].contiguous().cuda(), b.cuda()
    tight = x[:M, :K].contiguous().cuda()
    a, a2 = (_launch(tight, wd, bd, 2, splits) for _ in range(2))
    assert torch.equal(a.view(torch.int16), a2.view(torch.int16))
    # the same rows as the head of a 64-row buffer whose other rows are NaN
    big = torch.full((64, K), float("nan"), device="cuda", dtype=BF16)
    big[:M] = tight
    c = _launch(big[:M], wd, bd, 2, splits)
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))
    assert bool(torch.isfinite(c.float()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,pad", [(65, 16, 64, 0), (8, 24, 64, 0), (8, 16, 96, 0),
                                       (8, 16, 64, 4)],
                         ids=["M65", "N24", "K96", "row_stride"])
def test_dense_skinny_refusals(M, N, K, pad):
    g = _gen(5)
    x = torch.randn(M, K + pad, generator=g).to(BF16).cuda()[:, :K]
    w = torch.randn(N, K, generator=g).cuda()
    b = torch.zeros(N, device="cuda")
    with pytest.raises(ValueError, match="skinny"):
        ops.dense(x, w, b, impl="skinny")
    with pytest.raises(ValueError, match="skinny"):
        ops.dense_gelu_dense(x, w, b, torch.zeros(16, N, device="cuda"), impl="skinny")
    with pytest.raises(RuntimeError, match="dense_skinny"):
        _launch(x, w.to(BF16), b, 1, 1, ldx=K + pad)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_dense_skinny_op_refuses_grad_and_bad_splits():
    x = torch.zeros(8, 64, device="cuda", dtype=BF16)
    w = torch.zeros(16, 64, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="forward-only"):
        ops.dense(x, w, None, impl="skinny")
    with torch.no_grad():
        assert ops.dense(x, w, None, impl="skinny").shape == (8, 16)
    with pytest.raises(RuntimeError, match="splits"):
        _launch(x, w.detach().to(BF16), torch.zeros(16, device="cuda"), 0, 2)   # K has one unit
    torch.cuda.synchronize()
