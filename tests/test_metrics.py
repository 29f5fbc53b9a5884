"""Evaluation on the CPU path: the rank rule of ops.eval_rows, streaming ClassificationMetrics,
the single-pass dataset iterators, train.evaluate / EvalHook and the CLI's --eval flags."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distributedtensorflow_amd as dtf
from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import DeviceArrayDataset, SyntheticImageNet, SyntheticMLM
from distributedtensorflow_amd.metrics import ClassificationMetrics, EmptyMetricsError
from distributedtensorflow_amd.ops import records, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")


def _tied_rows(n, v, seed=0):
    """randn * 3 rounded to bf16 (ties are common), as fp32 storage."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, v, generator=g) * 3).bfloat16().float()
    y = torch.randint(0, v, (n,), generator=g)
    return x, y


# ----------------------------------------------------------------------------- rank rule
@pytest.mark.parametrize("n,v", [(64, 10), (32, 1003), (6, 30522)])
def test_rank_is_position_in_stable_descending_sort(n, v):
    x, y = _tied_rows(n, v, seed=v)
    assert (x.sort(1).values.diff(dim=1) == 0).any(), "the inputs must contain ties"
    loss, rank = ops.eval_rows(x, y)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    pos = (order == y.unsqueeze(1)).int().argmax(1)
    assert rank.dtype == torch.int32 and loss.dtype == torch.float32
    assert torch.equal(rank.long(), pos.long())
    assert torch.equal(rank < 1, x.argmax(1) == y)
    assert torch.equal(ops.in_top_k(x, y, 5), pos < 5)
    ref = torch.nn.functional.cross_entropy(x.double(), y, reduction="none")
    torch.testing.assert_close(loss.double(), ref, rtol=1e-6, atol=1e-6)


def test_special_rows():
    V = 12
    x, y = _tied_rows(6, V, seed=3)
    x[0] = 1.5                                   # all-equal row: the rank is the label itself
    y[0] = 7
    y[1], y[2] = -1, V                           # ignored labels
    x[3, int(y[3])] = float("nan")               # NaN label logit: a miss
    loss, rank = ops.eval_rows(x, y)
    assert rank[0].item() == 7
    assert rank[1].item() == -1 and rank[2].item() == -1
    assert loss[1].item() == 0.0 and loss[2].item() == 0.0
    assert rank[3].item() == V
    assert not ops.in_top_k(x, y, V)[[1, 2, 3]].any()
    assert abs(loss[0].item() - float(np.log(V))) < 1e-6


def test_padding_columns_change_nothing():
    V, ld = 77, 80
    x, y = _tied_rows(9, V, seed=5)
    padded = torch.full((9, ld), 1e4)
    padded[:, :V] = x
    want = ops.eval_rows(x, y)
    got_vocab = ops.eval_rows(padded, y, vocab=V)
    got_view = ops.eval_rows(padded[:, :V], y)
    for got in (got_vocab, got_view):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_eval_rows_validates():
    x, y = _tied_rows(4, 10)
    with pytest.raises(ValueError):
        ops.eval_rows(x, y, vocab=11)
    with pytest.raises(ValueError):
        ops.eval_rows(x, y[:3])
    with pytest.raises(ValueError):
        ops.in_top_k(x, y, 0)


# ----------------------------------------------------------------------------- streaming metrics
def test_metrics_three_updates_equal_one():
    x, y = _tied_rows(99, 40, seed=11)
    whole = ClassificationMetrics(k=5).update(x, y)
    parts = ClassificationMetrics(k=5)
    for i in range(3):
        parts.update(x[33 * i:33 * (i + 1)], y[33 * i:33 * (i + 1)])
    a, b = whole.state, parts.state
    assert a.dtype == torch.float64
    assert a[0].item() == 99.0 and torch.equal(a[[0, 2, 3]], b[[0, 2, 3]])
    assert abs(a[1].item() - b[1].item()) <= 1e-12 * abs(a[1].item())
    _, rank = ops.eval_rows(x, y)
    assert a[2].item() == float((rank < 1).sum()) and a[3].item() == float((rank < 5).sum())
    res = whole.result()
    assert set(res) == {"loss", "top_1", "top_k", "count"}
    assert all(type(v) is float for v in res.values())
    assert res["top_1"] == a[2].item() / 99 and res["count"] == 99.0
    ref = torch.nn.functional.cross_entropy(x.double(), y).item()
    assert abs(res["loss"] - ref) < 1e-6


def test_metrics_zero_weights_drop_rows():
    x, y = _tied_rows(20, 10, seed=13)
    w = (torch.arange(20) % 2).float()
    x[0, int(y[0])] = float("nan")               # weight 0: even its NaN loss must not leak
    got = ClassificationMetrics(k=3).update(x, y, w).result()
    want = ClassificationMetrics(k=3).update(x[1::2], y[1::2]).result()
    assert got["count"] == 10.0 and got["top_1"] == want["top_1"] and got["top_k"] == want["top_k"]
    assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])


def test_metrics_empty_result_raises_and_reset():
    m = ClassificationMetrics()
    with pytest.raises(EmptyMetricsError):
        m.result()
    x, y = _tied_rows(5, 10)
    m.update(x, torch.full((5,), -1))            # every row ignored
    with pytest.raises(EmptyMetricsError):
        m.result()
    m.update(x, y)
    assert m.result()["count"] == 5.0
    m.reset()
    with pytest.raises(EmptyMetricsError):
        m.result()
    with pytest.raises(ValueError):
        ClassificationMetrics(k=0)


# ----------------------------------------------------------------------------- data
@pytest.mark.parametrize("shards", [1, 2, 3])
def test_device_array_single_pass_sees_every_example_once(shards):
    n, batch = 103, 8
    imgs = np.zeros((n, 8), np.uint8)
    imgs[:, 0] = np.arange(n)
    labels = np.arange(n)
    seen = []
    for s in range(shards):
        ds = DeviceArrayDataset(imgs, labels, batch, "cpu", torch.float32, shuffle=True,
                                num_shards=shards, shard_index=s, scale=1.0)
        next(ds)                                  # a training iteration in flight
        pos = (ds._pos, ds.epoch, ds._gen.get_state().clone())
        got = list(ds.single_pass())
        assert all(len(y) == batch for _, y in got[:-1]) and 0 < len(got[-1][1]) <= batch
        for x, y in got:
            assert torch.equal(x[:, 0].long(), y)
            seen += y.tolist()
        assert (ds._pos, ds.epoch) == pos[:2] and torch.equal(ds._gen.get_state(), pos[2])
        assert sum(len(y) for _, y in got) == len(range(s, n, shards))
    assert sorted(seen) == list(range(n))


def test_synthetic_single_pass_is_bounded_and_leaves_training_iteration():
    ds = SyntheticImageNet(2, 8, device="cpu", dtype=torch.float32, seed=7)
    next(ds)
    got = list(ds.single_pass(3))
    assert len(got) == 3 and ds.i == 1 and got[0][0] is ds.images[0] and got[2][0] is ds.images[0]
    mlm = SyntheticMLM(2, 16, vocab_size=50, max_predictions=4, device="cpu", seed=7)
    got = list(mlm.single_pass(5))
    assert len(got) == 5 and mlm.i == 0 and got[1] is mlm.batches[1]


# ----------------------------------------------------------------------------- evaluate
def _mlp_and_data(seed=0):
    torch.manual_seed(seed)
    model = dtf.models.MnistMLP(16)
    g = torch.Generator().manual_seed(100)
    xs = torch.rand(40, 784, generator=g)
    ys = torch.randint(0, 10, (40,), generator=g)
    return model, xs, ys


def test_evaluate_restores_mode_even_when_forward_raises():
    model, xs, ys = _mlp_and_data()
    model.train()

    def boom(model, batch):
        assert not model.training and not torch.is_grad_enabled()
        raise RuntimeError("forward failed")

    with pytest.raises(RuntimeError, match="forward failed"):
        dtf.train.evaluate(model, [(xs, ys)], ClassificationMetrics(), forward=boom)
    assert model.training
    model.eval()
    res = dtf.train.evaluate(model, [(xs[:20], ys[:20]), (xs[20:], ys[20:])],
                             ClassificationMetrics(k=3))
    assert not model.training and res["count"] == 40.0
    with torch.no_grad():
        want = (model(xs).argmax(1) == ys).double().mean().item()
    assert res["top_1"] == want


def test_evaluate_bert_dict_batches_use_weights():
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(1)
    cfg = BertConfig(vocab_size=70, hidden_size=64, num_hidden_layers=1, num_attention_heads=1,
                     intermediate_size=128, max_position_embeddings=16)
    model = BertForPreTraining(cfg)
    data = SyntheticMLM(3, 16, vocab_size=70, max_predictions=4, device="cpu", seed=3, pool=1)
    batch = dict(data.batches[0])
    w = torch.ones(3, 4)
    w[:, ::2] = 0
    batch["masked_lm_weights"] = w
    res = dtf.train.evaluate(model, [batch], ClassificationMetrics(k=5))
    assert model.training and res["count"] == 6.0
    model.eval()
    with torch.no_grad():
        logits = model(batch["input_ids"], batch["segment_ids"], batch["input_mask"],
                       batch["masked_lm_positions"])
    model.train()
    assert logits.shape == (12, 70)                  # the [:, :V] view of the padded decoder
    _, rank = reference.eval_rows(logits, batch["masked_lm_ids"])
    keep = w.reshape(-1) > 0
    assert res["top_1"] == (rank[keep] < 1).double().mean().item()
    assert res["top_k"] == (rank[keep] < 5).double().mean().item()


def _train_mlp(eval_after=None):
    from distributedtensorflow_amd.optimizers import AdamOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import global_step as gs_mod
    gs_mod.reset_global_step()
    model, xs, ys = _mlp_and_data(seed=5)
    imgs = (xs * 255).to(torch.uint8).numpy()
    losses, evals = [], []
    with OneDeviceStrategy("/cpu:0").scope():
        opt = AdamOptimizer(0.01)
        opt.build(list(model.parameters()))
        data = DeviceArrayDataset(imgs, ys.numpy(), 8, "cpu", torch.float32, shuffle=True, seed=3)
        for step in range(4):
            x, y = next(data)
            loss = ops.sparse_softmax_cross_entropy(model(x), y)
            opt.minimize(loss)
            losses.append(loss.detach().clone())
            if eval_after is not None and step + 1 == eval_after:
                live = records.live_count()
                evals.append(dtf.train.evaluate(model, data.single_pass(), ClassificationMetrics(),
                                                optimizer=opt))
                assert model.training and records.live_count() == live
    gs_mod.reset_global_step()
    return losses, [p.detach().clone() for p in model.parameters()], evals


def test_training_is_unperturbed_by_an_evaluation_between_steps():
    plain_losses, plain_params, _ = _train_mlp()
    losses, params, evals = _train_mlp(eval_after=2)
    assert len(evals) == 1 and evals[0]["count"] == 40.0
    assert all(torch.equal(a, b) for a, b in zip(losses, plain_losses))
    assert all(torch.equal(a, b) for a, b in zip(params, plain_params))
    assert not torch.equal(plain_losses[0], plain_losses[3])


def test_records_isolated_restores_the_outer_registry():
    records.end_step()
    outer = records.GradSlot()
    with records.isolated():
        assert records.live_count() == 0
        inner = records.GradSlot()
        assert records.live_count() == 1
    assert inner.released and not outer.released and records.live_count() == 1
    assert records.end_step() == 1 and outer.released


def test_eval_hook_fires_on_step_count_and_writes_scalars(tmp_path):
    from distributedtensorflow_amd.summary.events import EventFileWriter, read_scalars
    from distributedtensorflow_amd.train import EvalHook
    from distributedtensorflow_amd.train.hooks import SessionRunContext

    class _Sess:
        is_chief = True
        summary_writer = None
        global_step = 0

    calls = []

    def eval_fn():
        calls.append(sess.global_step)
        return {"loss": 1.5, "top_1": 0.25, "top_k": 0.5, "count": 8.0}

    sess = _Sess()
    with EventFileWriter(str(tmp_path)) as w:
        hook = EvalHook(eval_fn, 3, summary_writer=w)
        hook.after_create_session(sess)
        for step in range(1, 8):
            sess.global_step = step
            hook.after_run(SessionRunContext(None, sess), None)
    assert calls == [3, 6] and [s for s, _ in hook.results] == [3, 6]
    sc = read_scalars(str(tmp_path))
    assert sc["eval/top_1"] == [(3, 0.25), (6, 0.25)] and sc["eval/loss"][0] == (3, 1.5)
    assert "eval/count" not in sc and sc["eval/top_k"][1] == (6, 0.5)
    with pytest.raises(ValueError):
        EvalHook(eval_fn, 0)


# ----------------------------------------------------------------------------- CLI
def _env():
    e = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        e.pop(k, None)
    return e


def test_cli_eval_flags_mnist_mlp_cpu(tmp_path):
    from distributedtensorflow_amd.data import mnist
    from distributedtensorflow_amd.summary.events import read_scalars
    data_dir = str(tmp_path / "mnist")
    mnist.load_arrays(data_dir, "train")
    mnist.load_arrays(data_dir, "test")
    r = subprocess.run([sys.executable, TRAIN, "--model", "mnist_mlp", "--strategy", "onedevice",
                        "--device", "cpu", "--max_steps", "40", "--log_every", "20",
                        "--data_dir", data_dir, "--log_dir", str(tmp_path / "tb"), "--eval",
                        "--eval_every", "20", "--eval_top_k", "3"],
                       capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["global_step"] == 40
    assert res["eval_top_1"] == res["test_accuracy"] and res["test_accuracy"] > 0.5
    assert res["eval_top_k"] >= res["eval_top_1"] and res["eval_loss"] > 0
    runs = glob.glob(str(tmp_path / "tb" / "*"))
    assert len(runs) == 1
    sc = read_scalars(runs[0])
    assert [s for s, _ in sc["eval/top_1"]] == [20, 40]
    assert sc["eval/top_1"][-1][1] == pytest.approx(res["eval_top_1"], abs=1e-4)
    assert "eval/loss" in sc and "eval/top_k" in sc
