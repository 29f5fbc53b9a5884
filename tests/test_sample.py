"""ops.sample_tokens on the reference path and the seeded path of BertForPreTraining.generate."""
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.models import KVCache, bert
from distributedtensorflow_amd.ops import reference

from test_decode import LENS, TINY
from test_mlm_data import M32, fmix32          # the Python-int hash


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


@pytest.mark.parametrize("seed,counter", [(0, (0, 0, 0)), (7, (5, 64, 2 ** 31 - 1)),
                                          (2 ** 31 - 1, (1, 2, 3))])
def test_sample_uniform_is_the_counter_hash(seed, counter):
    want = [(fmix32((fmix32((b * 0x9E3779B1 + seed) & M32) + c) & M32) >> 8) / 2 ** 24
            for b, c in enumerate(counter)]
    got = reference.sample_uniform(seed, _i32(*counter))
    assert got.tolist() == want and all(0 <= u < 1 for u in want)


@pytest.mark.parametrize("kw", [dict(top_k=1), dict(temperature=0.0)])
def test_top_1_and_greedy_give_the_lowest_index_maximum(kw):
    x = torch.tensor([[0.5, 2.0, -1.0, 1.0, 0.0, 0.0], [-3.0, -3.0, -4.0, -3.0, 9.0, 9.0]])
    tok, lp = ops.sample_tokens(x, 3, _i32(0, 1), vocab=4, **kw)
    assert tok.dtype == torch.int64 and lp.dtype == torch.float32
    if "top_k" in kw:                      # row 1: the ties with the first place are kept
        assert int(tok[0]) == 1 and int(tok[1]) in (0, 1, 3)
        torch.testing.assert_close(lp, torch.tensor([1.0, 1 / 3]).log())
    else:
        assert tok.tolist() == [1, 0]
        torch.testing.assert_close(lp, torch.log_softmax(x[:, :4], 1)[[0, 1], [1, 0]])


@pytest.mark.parametrize("top_k,top_p", [(0, 0.6), (4, 1.0), (4, 0.5), (3, 0.9)])
def test_kept_set_matches_a_brute_force_sort_on_a_row_with_ties(top_k, top_p):
    x = torch.tensor([[1.0, 3.0, 2.0, 3.0, -0.5, 2.0, 2.0, 0.25, float("-inf"), 1.0]])
    d = reference.sample_details(x, 1, _i32(9), 0.5, top_k, top_p)
    z = x[0].double() / 0.5
    vals = sorted(z.tolist(), reverse=True)
    keep = {i for i in range(10) if not top_k or float(z[i]) >= vals[top_k - 1]}
    mass = lambda s: sum(float(torch.exp(z[i] - z.max())) for i in s)      # noqa: E731
    # the largest value whose upper mass reaches top_p of the kept mass
    p32 = float(torch.tensor(top_p, dtype=torch.float32))
    t = max(v for v in vals if mass(i for i in keep if float(z[i]) >= v) >= p32 * mass(keep))
    keep = {i for i in keep if float(z[i]) >= t}
    assert set(torch.nonzero(d["keep"][0]).flatten().tolist()) == keep
    tok = int(d["tokens"][0])
    assert tok in keep and float(d["logprob"][0]) == pytest.approx(
        float(z[tok] - z.max()) - torch.tensor(mass(keep)).log().item(), abs=1e-5)


def test_padding_columns_are_never_chosen():
    x = torch.zeros(4, 16)
    x[:, :10] = -torch.rand(4, 10, generator=torch.Generator().manual_seed(0)) - 1.0
    for seed in range(20):
        for kw in (dict(), dict(top_k=3, top_p=0.5), dict(temperature=0.0)):
            tok, lp = ops.sample_tokens(x, seed, _i32(0, 1, 2, 3), vocab=10, **kw)
            assert int(tok.max()) < 10 and bool((lp <= 0).all())


def test_sample_argument_errors():
    x, c = torch.zeros(2, 8), _i32(0, 0)
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(temperature=-1.0),
               dict(vocab=0), dict(vocab=9)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ops.sample_tokens(x, 0, c, **kw)
    for bad in (c.long(), _i32(0), _i32(0, 0).unsqueeze(0), [0, 0]):
        with pytest.raises(ValueError, match="counter"):
            ops.sample_tokens(x, 0, bad)
    with pytest.raises(ValueError, match="seed"):
        ops.sample_tokens(x, 2 ** 31, c)
    with pytest.raises(RuntimeError, match="no-grad"):
        ops.sample_tokens(x.clone().requires_grad_(True), 0, c)


def test_seeded_generate_is_reproducible_and_returns_its_log_probabilities():
    torch.manual_seed(0)
    m = bert.BertForPreTraining(bert.BertConfig(**TINY, causal=True)).eval()
    prompt = torch.randint(1, TINY["vocab_size"], (2, 64),
                           generator=torch.Generator().manual_seed(1))
    run = lambda seed, **kw: m.generate(prompt, LENS, 6, temperature=0.8, top_k=20, seed=seed,  # noqa: E731
                                        return_logprobs=True, **kw)
    (a, la), (b, lb) = run(7), run(7)
    assert torch.equal(a, b) and torch.equal(la, lb) and tuple(la.shape) == (2, 6)
    assert any(not torch.equal(a, run(s)[0]) for s in (8, 9, 10))
    # the log-probabilities from the logits of prefill + decode_step fed the same tokens
    cache = KVCache(m.cfg, 2, 128, "cpu", torch.float32)
    logits = m.prefill(prompt, LENS, cache)
    for t in range(6):
        z = logits.bfloat16().float() / 0.8
        z = z.masked_fill(z < z.topk(20, dim=1).values[:, -1:], float("-inf"))
        torch.testing.assert_close(la[:, t], torch.log_softmax(z, 1)[[0, 1], a[:, t]],
                                   atol=1e-5, rtol=1e-5)
        logits = m.decode_step(a[:, t], cache)
    assert tuple(run(7, top_p=0.5)[0].shape) == (2, 6)
    for kw in (dict(top_p=0.9), dict(return_logprobs=True)):
        with pytest.raises(ValueError, match="seed"):
            m.generate(prompt, LENS, 2, temperature=0.8, **kw)
