"""sample_kernel (csrc/kernels/sample.hip) against ``reference.sample_details`` in fp64 on the
stored bf16 logits: tokens must be EQUAL, log-probabilities within a bound derived from the
kernel's stated summation order (u = ``U32``).  A mass ``exp2((x - xmax) c)`` has three roundings in
its exponent and v_exp_f32: ``gamma(3) |ln m| + INTR`` relatively.  Every sum is a chain of at most
``n = R + 23`` additions (R = 8 ceil(chunks / 1024) elements of a thread, 6 wave levels, 16 wave
totals, offset + running sum), so a sum S over a set with ``E = sum m (gamma(3) |ln m| + INTR)`` is
off by ``rel = E / S + gamma(n) (1 + E / S) + 2 u`` of S (2 u: the products top_p S and u Z).
``((x_tok - xmax) c - log2 Z) ln 2`` adds the roundings of its own operations and v_log_f32:
``2 gamma(3) (|ln m_tok| + |ln Z|) + rel / (1 - rel) + INTR (1 + |ln Z|)``.
Equality is a fair demand only where the fp64 decisions have the margin ``rel``: the upper mass at
the top-p threshold key and at the key above it against top_p S, and u Z against the running mass
before and at the token.  Every case ASSERTS that before it looks at the kernel.
"""
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.ops import reference
from test_decode_gpu import TINY
from test_nlp_kernels_gpu import BF16, INTR, U32, _gen, gamma


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield                                    # as tests/test_decode_gpu.py
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


SEED = 14
COUNTER = torch.tensor([5, 64, 1000], dtype=torch.int32)
SHAPES = [(70, 128), (1000, 1024), (30522, 30528)]
CASES = [(V, ld, k, p, T, "randn") for V, ld in SHAPES for k in (0, 1, 5, V)
         for p in (1.0, 0.9, 0.05) for T in (1.0, 0.7)]
CASES += [(V, ld, 0, 1.0, 0.0, rows) for V, ld in SHAPES for rows in ("randn", "equal")]
CASES += [(1000, 1024, k, p, 0.7, rows) for rows in ("equal", "ninf", "negative", "tie")
          for k in (0, 1, 5, 1000) for p in (1.0, 0.9, 0.05)]
# the 65536-key instantiation (129 KB of LDS)
CASES += [(40000, 40000, 5, 0.9, 0.7, "randn"), (65530, 65536, 0, 0.05, 1.0, "randn"),
          (65530, 65536, 0, 1.0, 0.0, "randn")]


def _logits(V, ld, rows):
    """bf16 [3, ld]; the padding columns hold exact zeros, as the head writes them."""
    x = torch.zeros(3, ld)
    x[:, :V] = 3.0 * torch.randn(3, V, generator=_gen(V + len(rows)))
    if rows == "equal":
        x[:, :V] = -1.25
    elif rows == "ninf":
        x[:, V // 10:V // 2] = float("-inf")
    elif rows == "negative":
        x[:, :V] = -x[:, :V].abs() - 0.5
    elif rows == "tie":                      # places 4 .. 11 share one value
        x[:, :V] = x[:, :V].clamp(max=6.0)
        x[:, 3:V:V // 7] = 7.0
        x[:, 1], x[:, V - 1], x[:, V // 2] = 9.0, 8.5, 8.0
    return x.to(BF16)


def _oracle(x, V, top_k, top_p, T):
    """-> (reference details in fp64, rel of the final set, rel of the top-k set, logprob bound)."""
    d = reference.sample_details(x, SEED, COUNTER, T, top_k, top_p, V, math=torch.float64)
    z = x[:, :V].double() / (T or 1.0)
    lnm = z.max(1, keepdim=True).values - z                          # |ln m|, +inf at -inf
    m = torch.exp(-lnm)
    e = torch.where(m > 0, m * (gamma(3) * lnm + INTR), torch.zeros_like(m))
    n = 8 * -(-(-(-V // 8)) // 1024) + 23

    def rel(keep):
        r = (e * keep).sum(1) / (m * keep).sum(1)
        return r + gamma(n) * (1 + r) + 2 * U32

    if T == 0:
        Z, lnm_tok = m.sum(1), torch.zeros(3, dtype=torch.float64)
        rel_z = rel_k = rel(torch.ones_like(m))
    else:
        Z, lnm_tok = d["Z"], lnm.gather(1, d["tokens"].unsqueeze(1)).squeeze(1)
        rel_z, rel_k = rel(d["keep"]), rel(d["keep_k"])
    lnz = Z.log().abs()
    bound = 2 * gamma(3) * (lnm_tok + lnz) + rel_z / (1 - rel_z) + INTR * (1 + lnz)
    return d, rel_z, rel_k, bound


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld,top_k,top_p,T,rows", CASES)
def test_sample_tokens_match_fp64(V, ld, top_k, top_p, T, rows):
    x = _logits(V, ld, rows)
    d, rel_z, rel_k, bound = _oracle(x, V, top_k, top_p, T)
    if T > 0:                                # the precondition of token equality
        kept = d["need"] / float(torch.tensor(top_p, dtype=torch.float32))
        assert bool(((d["s_at"] - d["need"]).abs() > rel_k * kept).all() or top_p == 1.0)
        assert bool(((d["s_above"] - d["need"]).abs() > rel_k * kept).all() or top_p == 1.0)
        assert bool((d["cdf_hi"] - d["target"] > rel_z * d["Z"]).all())
        assert bool(((d["target"] - d["cdf_lo"] > rel_z * d["Z"]) | (d["cdf_lo"] == 0)).all())
    tok, lp = ops.sample_tokens(x.cuda(), SEED, COUNTER.cuda(), T, top_k, top_p, V)
    assert torch.equal(tok.cpu(), d["tokens"]), (tok.cpu(), d["tokens"])
    ratio = float(((lp.cpu().double() - d["logprob"]).abs() / bound).max())
    print(f"MEASURE sample logprob/bound V={V} k={top_k} p={top_p} T={T} {rows} {ratio:.4f}")
    assert ratio <= 1.0 and bool(torch.isfinite(lp).all())


@pytest.mark.gpu
def test_sample_reads_nothing_from_the_device_and_repeats_its_bits():
    x, c = _logits(30522, 30528, "randn").cuda(), COUNTER.cuda()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = ops.sample_tokens(x, SEED, c, 0.7, 50, 0.9, 30522)
        b = ops.sample_tokens(x, SEED, c, 0.7, 50, 0.9, 30522)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    with pytest.raises(ValueError, match="exceeds"):
        ops.sample_tokens(torch.zeros(1, 65544, device="cuda", dtype=BF16), 0, c[:1])


@pytest.mark.gpu
def test_seeded_generate_repeats_itself_on_the_device():
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    gpu = BertForPreTraining(BertConfig(**TINY)).cuda().eval()
    lens = torch.tensor([5, 64])
    prompt = torch.randint(1, 256, (2, 64), generator=_gen(3))
    prompt = (prompt * (torch.arange(64).view(1, 64) < lens.view(2, 1))).cuda()
    run = lambda: gpu.generate(prompt, lens, 8, temperature=0.8, top_k=50, top_p=0.9, seed=7,  # noqa: E731
                               return_logprobs=True)
    (a, la), (b, lb) = run(), run()
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert int(a.max()) < 256 and bool(torch.isfinite(la).all())
