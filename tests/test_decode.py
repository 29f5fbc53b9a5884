"""Incremental decoding on the reference path: ops.attention_decode / ops.kv_cache_fill, the
KV-cache methods of the causal BERT (prefill, decode_step, generate) and train.py --generate."""
import json

import pytest
import torch

from distributedtensorflow_amd import cli, ops
from distributedtensorflow_amd.models import KVCache, bert

TINY = dict(vocab_size=256, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
            intermediate_size=256, max_position_embeddings=128)
LENS = torch.tensor([5, 64])
STEPS = 8


def test_attention_decode_is_the_causal_forward_s_last_row():
    """Growing lengths 1 .. 70: each step's output is the last row of the causal forward over the
    tokens so far; the cache starts as NaN, so an unwritten row that is used shows."""
    B, H, S = 2, 3, 70
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * 64, generator=g)
    kc = torch.full((B, H, 128, 64), float("nan"))
    vc = kc.clone()
    for n in range(1, S + 1):
        pos = torch.full((B,), n - 1, dtype=torch.int32)
        out = ops.attention_decode(qkv[:, n - 1].contiguous(), kc, vc, pos, H)
        full = ops.attention_qkv(qkv[:, :n].reshape(B * n, -1), None, B, n, H, causal=True)
        torch.testing.assert_close(out, full.view(B, n, -1)[:, -1], atol=1e-5, rtol=1e-5)
    want = qkv.view(B, S, 3, H, 64)
    assert torch.equal(kc[:, :, :S], want[:, :, 1].permute(0, 2, 1, 3))
    assert torch.equal(vc[:, :, :S], want[:, :, 2].permute(0, 2, 1, 3))
    assert bool(kc[:, :, S:].isnan().all())
    with pytest.raises(RuntimeError, match="no-grad"):
        ops.attention_decode(qkv[:, 0].clone().requires_grad_(True), kc, vc, pos, H)
    with pytest.raises(ValueError, match="qkv_new"):
        ops.attention_decode(qkv[:, 0, :-64].contiguous(), kc, vc, pos, H)
    with pytest.raises(ValueError, match="capacity"):
        ops.attention_decode(qkv[:, 0].contiguous(), kc[:, :, :96].contiguous(),
                             vc[:, :, :96].contiguous(), pos, H)


@pytest.fixture(scope="module")
def tiny():
    """(model, sequences [B, 128], full causal forward logits [B, 128, V])."""
    torch.manual_seed(0)
    m = bert.BertForPreTraining(bert.BertConfig(**TINY, causal=True)).eval()
    ids = torch.randint(1, TINY["vocab_size"], (2, 128), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        full = m(ids).view(2, 128, -1)
    return m, ids, full


def test_prefill_and_decode_steps_match_the_full_forward(tiny):
    m, ids, full = tiny
    cache = KVCache(m.cfg, 2, 128, "cpu", torch.float32)
    logits = m.prefill(ids[:, :64].contiguous(), LENS, cache)
    rows = torch.arange(2)
    for t in range(STEPS + 1):
        torch.testing.assert_close(logits, full[rows, LENS - 1 + t], atol=1e-4, rtol=1e-4)
        assert torch.equal(cache.pos, (LENS + t).int())
        logits = m.decode_step(ids[rows, LENS + t], cache)


def test_greedy_generate_is_the_stepwise_argmax_of_the_full_forward(tiny):
    m, ids, _ = tiny
    m.train()
    got = m.generate(ids[:, :64].contiguous(), LENS, 5)
    assert m.training                                           # the flag is restored
    m.eval()
    seq = [ids[b, :LENS[b]].tolist() for b in range(2)]
    for t in range(5):
        for b in range(2):
            row = torch.zeros(1, 128, dtype=torch.int64)
            row[0, :len(seq[b])] = torch.tensor(seq[b])
            with torch.no_grad():
                nxt = int(m(row).view(128, -1)[len(seq[b]) - 1].argmax())
            assert int(got[b, t]) == nxt, (b, t)
            seq[b].append(nxt)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 5)
    eos = int(got[0, 0])
    stopped = m.generate(ids[:, :64].contiguous(), LENS, 5, eos_id=eos)
    assert stopped[0].tolist() == [eos] * 5


def test_sampling_is_reproducible_and_stays_in_the_top_k(tiny):
    m, ids, full = tiny
    prompt = ids[:, :64].contiguous()
    run = lambda seed: m.generate(prompt, LENS, 6, temperature=1.5, top_k=3,
                                  generator=torch.Generator().manual_seed(seed))
    a, b = run(7), run(7)
    assert torch.equal(a, b)
    assert any(not torch.equal(a, run(s)) for s in (8, 9, 10))
    top = full[torch.arange(2), LENS - 1].topk(3, dim=-1).indices       # the first token's set
    assert all(int(a[r, 0]) in top[r].tolist() for r in range(2))
    assert int(a.max()) < TINY["vocab_size"]


def test_generate_refusals(tiny):
    m, ids, _ = tiny
    prompt = ids[:, :64].contiguous()
    with pytest.raises(ValueError, match="capacity"):
        m.generate(prompt, LENS, 128 - 64 + 1)
    for bad in ([0, 5], [5, 65], [5]):
        with pytest.raises(ValueError, match="prompt_lens"):
            m.generate(prompt, torch.tensor(bad), 2)
    mlm = bert.BertForPreTraining(bert.BertConfig(**TINY))
    with pytest.raises(ValueError, match="causal"):
        mlm.generate(prompt, LENS, 2)
    with pytest.raises(ValueError, match="capacity"):
        KVCache(m.cfg, 2, 129, "cpu", torch.float32)
    assert KVCache(m.cfg, 2, 65, "cpu", torch.float32).k.shape == (2, 2, 2, 128, 64)


def test_cli_generate(monkeypatch, capsys):
    tiny_cfg = dict(vocab_size=30522, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                    intermediate_size=128, max_position_embeddings=32)
    monkeypatch.setattr(bert, "bert_base",
                        lambda **kw: bert.BertForPreTraining(bert.BertConfig(**tiny_cfg, **kw)))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        monkeypatch.delenv(k, raising=False)
    from distributedtensorflow_amd.train.global_step import reset_global_step
    reset_global_step()
    args = ["--model", "bert_base", "--device", "cpu", "--seq_len", "16", "--batch_size", "2",
            "--max_steps", "1", "--log_dir", ""]
    assert cli.main(args + ["--causal_lm", "--generate", "4", "--generate_prompt", "8"]) == 0
    reset_global_step()
    res = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert len(res["generated"]) == 2 and all(len(r) == 4 for r in res["generated"])
    assert all(0 <= t < 30522 for r in res["generated"] for t in r)
    assert res["generate_tokens_per_sec"] > 0
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--generate", "4"])
    assert "--generate needs --causal_lm" in str(e.value)
