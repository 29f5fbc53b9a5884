"""Causal language modelling on the CPU path: the reference attention under a lower-triangular
select, the causal BERT (no look-ahead), next-token targets, the causal token batches and the
CLI flag."""
import json
import math

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import cli
from distributedtensorflow_amd.data import DeviceTokenDataset, TokenMasking, causal_lm_targets
from distributedtensorflow_amd.models import bert
from distributedtensorflow_amd.ops import reference as R

D = 64


# ----------------------------------------------------------------------------- attention
def _naive(qkv, mask, B, S, H, p, seed):
    """fp64 softmax under a tril select, the keep set taken from keep_mask on the full
    [B, H, S, S] index space."""
    x = qkv.double().view(B, S, 3, H, D)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * D ** -0.5
    if mask is not None:
        s = s + mask.double().view(B, 1, 1, S)
    tril = torch.ones(S, S, dtype=torch.bool).tril()
    s = torch.where(tril, s, torch.full_like(s, float("-inf")))
    prob = torch.softmax(s, -1)
    if p > 0:
        idx = torch.arange(B * H * S * S).view(B, H, S, S)
        prob = torch.where(R.keep_mask(seed, idx, p), prob / (1.0 - p), torch.zeros_like(prob))
    return (prob @ v).permute(0, 2, 1, 3).reshape(B * S, H * D)


@pytest.mark.parametrize("S", [8, 64])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_reference_causal_attention_matches_naive_fp64(S, masked, p):
    B, H, seed = 2, 2, 1234
    g = torch.Generator().manual_seed(S + masked)
    qkv = torch.randn(B * S, 3 * H * D, generator=g)
    dy = torch.randn(B * S, H * D, generator=g)
    mask = None
    if masked:
        mask = torch.zeros(B, S)
        mask[1, S - 3:] = -10000.0
    a = qkv.clone().requires_grad_(True)
    out = R.attention_qkv(a, mask, B, S, H, p, True, seed=seed, causal=True)
    (ga,) = torch.autograd.grad(out, [a], dy)
    b = qkv.double().requires_grad_(True)
    want = _naive(b, mask, B, S, H, p, seed)
    (gb,) = torch.autograd.grad(want, [b], dy.double())
    torch.testing.assert_close(out.double(), want, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(ga.double(), gb, atol=1e-5, rtol=1e-5)
    # row 0 sees key 0 only: its output is V[0] (kept and rescaled, or dropped)
    assert not torch.equal(out, R.attention_qkv(qkv, mask, B, S, H, p, True, seed=seed))
    # the [B, H, S, D] form
    x = qkv.view(B, S, 3, H, D)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    if p == 0:
        m4 = None if mask is None else mask.view(B, 1, 1, S)
        o4 = R.attention(q, k, v, m4, causal=True)
        torch.testing.assert_close(o4.permute(0, 2, 1, 3).reshape(B * S, H * D).double(), want,
                                   atol=1e-5, rtol=1e-5)


# ----------------------------------------------------------------------------- model
TINY = dict(vocab_size=500, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
            intermediate_size=128, max_position_embeddings=16)


def test_causal_model_does_not_look_ahead():
    S, j = 16, 5
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 500, (3, S), generator=g)
    ids2 = ids.clone()
    ids2[:, j:] = (ids2[:, j:] + 1 + torch.randint(0, 400, (3, S - j), generator=g)) % 500
    same = {}
    for causal in (True, False):
        torch.manual_seed(1)
        m = bert.BertForPreTraining(bert.BertConfig(**TINY, causal=causal)).eval()
        with torch.no_grad():
            a, b = m(ids).view(3, S, -1), m(ids2).view(3, S, -1)
        assert a.shape == (3, S, 500)                 # the head scores every position
        same[causal] = torch.equal(a[:, :j], b[:, :j])
        assert not torch.equal(a[:, j:], b[:, j:])
    assert same[True]
    assert not same[False]                            # the check can fail


def test_config_default_and_flops():
    assert bert.BertConfig().causal is False
    cfg = bert.BertConfig()
    S, P = 128, 20
    mlm, lm = bert.mlm_flops_per_token(cfg, S, P), bert.causal_lm_flops_per_token(cfg, S)
    Hd, L, I, V = cfg.hidden_size, cfg.num_hidden_layers, cfg.intermediate_size, cfg.vocab_size
    gemm = 2 * (4 * Hd * Hd + 2 * Hd * I) * L
    assert lm == 3.0 * (gemm + 2 * S * Hd * L + 2 * (Hd * Hd + Hd * V))
    # the same body, the head over S positions instead of P, half the attention products
    assert math.isclose(lm - mlm, 3.0 * (2 * (Hd * Hd + Hd * V) * (1 - P / S) - 2 * S * Hd * L))


def test_saved_model_export_of_a_causal_model_raises(tmp_path):
    from distributedtensorflow_amd.train.saved_model import export_bert_saved_model
    m = bert.BertForPreTraining(bert.BertConfig(**TINY, causal=True))
    with pytest.raises(ValueError, match="causal"):
        export_bert_saved_model(str(tmp_path / "sm"), m, seq_len=16)
    assert not (tmp_path / "sm").exists()


# ----------------------------------------------------------------------------- targets
def _targets_loop(ids, mask):
    B, S = ids.shape
    lab = torch.zeros(B, S, dtype=torch.int64)
    w = torch.zeros(B, S, dtype=torch.float32)
    for b in range(B):
        for j in range(S - 1):
            lab[b, j] = int(ids[b, j + 1])
            w[b, j] = float(mask[b, j + 1])
    return lab, w


def test_causal_lm_targets_against_a_python_loop():
    ids = torch.tensor([[101, 7, 8, 9, 102, 0, 0, 0],          # tail padding
                        [101, 5, 6, 7, 8, 9, 10, 102],         # a full row
                        [101, 102, 0, 0, 0, 0, 0, 0],
                        [0, 0, 0, 0, 0, 0, 0, 0]])
    mask = (ids != 0).long()
    before = ids.clone(), mask.clone()
    lab, w = causal_lm_targets(ids, mask)
    wl, ww = _targets_loop(ids, mask)
    assert lab.dtype == torch.int64 and w.dtype == torch.float32
    assert torch.equal(lab, wl) and torch.equal(w, ww)
    assert torch.equal(ids, before[0]) and torch.equal(mask, before[1])      # pure
    assert w.sum(1).tolist() == [4.0, 7.0, 1.0, 0.0]
    lab, w = causal_lm_targets(ids[:, :1], mask[:, :1])                       # S = 1
    assert lab.tolist() == [[0]] * 4 and w.tolist() == [[0.0]] * 4


# ----------------------------------------------------------------------------- dataset
def _rows(N, S, seed, dtype=np.int32, vocab=30522):
    rng = np.random.RandomState(seed)
    t = rng.randint(1, vocab, (N, S)).astype(dtype)
    for i in range(N):
        t[i, S - rng.randint(0, S // 2):] = 0
    return t


def test_causal_dataset_batches_order_and_generators():
    toks = _rows(23, 16, seed=1)
    kw = dict(shuffle=True, seed=7, mask_seed=3, max_predictions=4)
    mlm = DeviceTokenDataset(toks, 4, "cpu", **kw)
    lm = DeviceTokenDataset(toks, 4, "cpu", objective="causal", **kw)
    state = lm._mask_gen.get_state().clone()
    full = torch.from_numpy(toks.astype(np.int64))
    for _ in range(8):                                           # over an epoch boundary
        a, b = next(mlm), next(lm)
        assert b["masked_lm_positions"] is None
        ids = b["input_ids"]
        assert ids.dtype == torch.int64 and ids.shape == (4, 16)
        assert torch.equal(b["input_mask"], (ids != 0).long())
        assert torch.count_nonzero(b["segment_ids"]) == 0
        lab, w = _targets_loop(ids, b["input_mask"])
        assert torch.equal(b["masked_lm_ids"], lab) and torch.equal(b["masked_lm_weights"], w)
        # the same examples in the same order as the masked-LM set: the real tokens agree
        # wherever the masked-LM batch left them alone, and every row is a row of the file
        assert torch.equal(a["input_mask"], b["input_mask"])
        for r in range(4):
            assert bool((full == ids[r]).all(1).any())
        kept = torch.ones_like(ids, dtype=torch.bool)
        kept.scatter_(1, a["masked_lm_positions"], False)
        assert torch.equal(a["input_ids"][kept], ids[kept])
    assert torch.equal(lm._mask_gen.get_state(), state)          # nothing drawn
    assert not torch.equal(mlm._mask_gen.get_state(), state)


def test_causal_single_pass_covers_every_example_once_over_two_shards():
    toks = _rows(23, 16, seed=2)
    seen = []
    for shard in (0, 1):
        d = DeviceTokenDataset(toks, 5, "cpu", objective="causal", num_shards=2,
                               shard_index=shard)
        state = d._mask_gen.get_state().clone()
        first = [b["input_ids"] for b in d.single_pass()]
        again = [b["input_ids"] for b in d.single_pass()]
        assert all(torch.equal(x, y) for x, y in zip(first, again))
        rows = torch.cat(first)
        assert torch.equal(rows, torch.from_numpy(toks[shard::2].astype(np.int64)))
        assert torch.equal(next(d)["input_ids"], rows[:5])       # the same batches in order
        assert torch.equal(d._mask_gen.get_state(), state)
        seen.append(rows)
    assert sum(len(r) for r in seen) == 23


def test_causal_dataset_reads_uint16_unsigned_and_refuses_a_table():
    toks = _rows(9, 16, seed=3, dtype=np.uint16, vocab=65000)
    toks[0, :4] = [65000 - 1, 40000, 32768, 32767]
    m = TokenMasking(vocab_size=65000)
    d = DeviceTokenDataset(toks, 3, "cpu", m, objective="causal")
    b = next(d)
    assert b["input_ids"][0, :4].tolist() == [64999, 40000, 32768, 32767]
    assert b["masked_lm_ids"][0, :3].tolist() == [40000, 32768, 32767]
    assert int(b["input_ids"].min()) >= 0
    with pytest.raises(ValueError, match="continuation"):
        DeviceTokenDataset(toks, 3, "cpu", m, objective="causal",
                           continuation=np.zeros(65000, dtype=np.uint8))
    with pytest.raises(ValueError, match="objective"):
        DeviceTokenDataset(toks, 3, "cpu", m, objective="prefix")
    # max_predictions plays no part: one above the sequence length is not an error here
    DeviceTokenDataset(toks, 3, "cpu", m, objective="causal", max_predictions=99)


# ----------------------------------------------------------------------------- CLI
def test_cli_refusals_and_help():
    with pytest.raises(SystemExit) as e:
        cli.main(["--model", "resnet50", "--causal_lm"])
    assert "--causal_lm needs a BERT model" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["--model", "mnist_cnn", "--causal_lm"])
    assert "--causal_lm needs a BERT model" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["--model", "bert_base", "--causal_lm", "--text_data", "D",
                  "--whole_word_mask"])
    assert "--causal_lm" in str(e.value) and "--whole_word_mask" in str(e.value)
    p = cli.build_parser()
    assert p.parse_args(["--model", "bert_base"]).causal_lm is False
    assert p.parse_args(["--model", "bert_base", "--causal_lm"]).causal_lm is True
    text = " ".join(p.format_help().split())
    assert "--mlm_prob and --max_predictions are ignored" in text


def test_cli_trains_and_evaluates_a_tiny_causal_lm(tmp_path, monkeypatch, capsys):
    tiny = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                intermediate_size=128, max_position_embeddings=16)       # head_dim 64
    made = []

    def make(**kw):
        made.append(bert.BertConfig(**tiny, **kw))
        return bert.BertForPreTraining(made[-1])

    monkeypatch.setattr(bert, "bert_base", make)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        monkeypatch.delenv(k, raising=False)
    vocab = 1200
    d = tmp_path / "set"
    d.mkdir()
    for split, n in (("train", 12), ("val", 7)):
        np.save(d / f"{split}_tokens.npy", _rows(n, 16, seed=n, vocab=vocab))
    val = np.load(d / "val_tokens.npy")
    with open(d / "meta.json", "w") as f:
        json.dump({"vocab_size": vocab}, f)
    base = ["--model", "bert_base", "--device", "cpu", "--text_data", str(d), "--batch_size", "4",
            "--max_steps", "2", "--log_dir", "", "--eval"]
    from distributedtensorflow_amd.train.global_step import reset_global_step
    out = {}
    for flag in (["--causal_lm", "--max_predictions", "99"], ["--max_predictions", "4"]):
        reset_global_step()                                       # each run counts from 0
        assert cli.main(base + flag) == 0
        res = json.loads([l for l in capsys.readouterr().out.splitlines()
                          if l.startswith("{")][-1])
        assert res["global_step"] == 2 and math.isfinite(res["final_loss"])
        assert math.isfinite(res["eval_loss"])
        out[flag[0] == "--causal_lm"] = res
    reset_global_step()
    lm, mlm = out[True], out[False]
    assert lm["causal_lm"] is True and made[0].causal is True
    assert lm["eval_perplexity"] == math.exp(lm["eval_loss"])
    assert lm["eval_count"] == int((val[:, 1:] != 0).sum())      # the non-pad next tokens
    assert 0.0 <= lm["eval_top_1"] <= 1.0
    assert "causal_lm" not in mlm and "eval_perplexity" not in mlm and made[1].causal is False


def test_cli_causal_lm_on_the_synthetic_set(monkeypatch, capsys):
    tiny = dict(vocab_size=30522, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                intermediate_size=128, max_position_embeddings=16)
    monkeypatch.setattr(bert, "bert_base",
                        lambda **kw: bert.BertForPreTraining(bert.BertConfig(**tiny, **kw)))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        monkeypatch.delenv(k, raising=False)
    from distributedtensorflow_amd.train.global_step import reset_global_step
    reset_global_step()
    assert cli.main(["--model", "bert_base", "--device", "cpu", "--causal_lm", "--seq_len", "16",
                     "--batch_size", "2", "--max_steps", "1", "--log_dir", "", "--eval",
                     "--eval_steps", "2"]) == 0
    reset_global_step()
    res = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert res["causal_lm"] is True and math.isfinite(res["final_loss"])
    assert res["eval_count"] == 2 * 2 * 15                       # every next token of 2 batches
    assert res["eval_perplexity"] == math.exp(res["eval_loss"])
