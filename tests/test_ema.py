"""tf.train.ExponentialMovingAverage of the variables on the CPU (the reference path): the decay
schedule, the per-step fp64 oracle under every optimizer, the ``n`` convention, checkpoints under
TF's names, ``swap()`` / ``evaluate(averages=)`` and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_util
from distributedtensorflow_amd import ops
from distributedtensorflow_amd import train as dtf_train
from distributedtensorflow_amd.optimizers import (AdamOptimizer, ExponentialMovingAverage,
                                                  MomentumOptimizer, SyncReplicasOptimizer)
from distributedtensorflow_amd.optimizers.moving_averages import EMA_BETWEEN_GRAPH
from distributedtensorflow_amd.parallel import OneDeviceStrategy
from distributedtensorflow_amd.train import Saver, list_variables, load_variable
from distributedtensorflow_amd.train import global_step as gs_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")
SUFFIX = "/ExponentialMovingAverage"


@pytest.fixture(autouse=True)
def _fresh_global_step():
    gs_mod.reset_global_step()
    yield
    gs_mod.reset_global_step()


# ---------------------------------------------------------------------------- schedule, errors

@pytest.mark.parametrize("decay", [0.9999, 0.5])
def test_decay_schedule(decay):
    ema = ExponentialMovingAverage(decay, num_updates=gs_mod.GlobalStep())
    for n in (1, 2, 10, 10 ** 6):
        want = np.float32(1.0 - min(decay, (1.0 + n) / (10.0 + n)))
        assert ema.a_at(n) == want and ema.a_at(n).dtype == np.float32
    assert ema.a_at(None) == np.float32(1.0 - decay)
    assert ema.decay_at(1) == min(decay, 2.0 / 11.0)


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_decay_must_be_inside_the_unit_interval(bad):
    with pytest.raises(ValueError, match="decay"):
        ExponentialMovingAverage(bad)


def test_zero_debias_is_refused():
    with pytest.raises(ValueError, match="zero_debias"):
        ExponentialMovingAverage(0.9, zero_debias=True)


def test_a_subset_of_the_variables_is_refused():
    ps = ema_util.make_params()
    opt = MomentumOptimizer(0.1, 0.9)
    opt.set_variable_averages(ExponentialMovingAverage(0.9), variables_to_average=ps[:1])
    with OneDeviceStrategy("cpu").scope():
        with pytest.raises(ValueError, match="variables_to_average"):
            opt.build(ps)
    with pytest.raises(ValueError, match="variables_to_average"):
        with OneDeviceStrategy("cpu").scope():
            SyncReplicasOptimizer(MomentumOptimizer(0.1, 0.9), 1,
                                  variable_averages=ExponentialMovingAverage(0.9),
                                  variables_to_average=ps[1:]).build(ps)


# ---------------------------------------------------------------------------- the update

@pytest.mark.parametrize("name", list(ema_util.OPTIMIZERS))
def test_every_optimizer_meets_the_per_step_oracle(name):
    ema = ExponentialMovingAverage(0.9)
    opt, _ = ema_util.run_optimizer_steps(name, "cpu", ema)
    assert opt.slots[-1].name == "ExponentialMovingAverage" and opt.slots[-1].buf is ema.buf
    assert float(ema.a_dev.item()) == float(np.float32(1.0 - 0.9))


def test_average_equal_to_variable_is_a_fixed_point():
    g = torch.Generator().manual_seed(3)
    var = torch.randn(1027, generator=g) * torch.logspace(-20, 20, 1027)
    for a in (1e-4, 0.1, 0.5, 0.999, 1.0):
        avg = var.clone()
        ops.ema_update(avg, var, torch.tensor([a], dtype=torch.float32))
        assert torch.equal(avg, var)


def test_reference_op_meets_the_oracle():
    g = torch.Generator().manual_seed(4)
    e, p = torch.randn(4099, generator=g), torch.randn(4099, generator=g)
    a = torch.tensor([1.0 - 0.9999], dtype=torch.float32)
    got = ops.ema_update(e.clone(), p, a)
    ema_util.assert_step(got, e, p, float(a))


def test_n_is_the_global_step_after_this_steps_increment():
    gstep = dtf_train.get_or_create_global_step()
    ema = ExponentialMovingAverage(0.9999, num_updates=gstep)
    with OneDeviceStrategy("cpu").scope():
        model = ema_util.BNNet()
        opt = MomentumOptimizer(0.1, 0.9, variable_averages=ema)
        opt.build(list(model.parameters()))
    for n in (1, 2, 3):
        x, y = ema_util.bn_batch(n)
        opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y), global_step=gstep)
        assert gstep.value() == n
        assert float(ema.a_dev.item()) == float(np.float32(1.0 - (1.0 + n) / (10.0 + n)))
    # without the object as ``global_step`` nothing increments it: n is its value as read
    x, y = ema_util.bn_batch(9)
    opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y))
    assert float(ema.a_dev.item()) == float(np.float32(1.0 - 4.0 / 13.0))


def test_sync_replicas_optimizer_forwards_the_average():
    ema = ExponentialMovingAverage(0.5)
    ps = ema_util.make_params()
    with OneDeviceStrategy("cpu").scope():
        opt = SyncReplicasOptimizer(MomentumOptimizer(0.1, 0.9), replicas_to_aggregate=1,
                                    variable_averages=ema, variables_to_average=list(ps))
        sp = opt.build(ps)
    assert opt.variable_averages is ema
    for p, g in zip(ps, ema_util.make_grads(0)):
        p.grad.copy_(g)
    before = ema.buf.clone()
    opt.apply_gradients()
    ema_util.assert_step(ema.buf, before, sp.master, 0.5)
    assert not torch.equal(ema.buf, before)


def test_between_graph_ps_refuses_the_average():
    from distributedtensorflow_amd.parallel import ps_device
    from distributedtensorflow_amd.parallel.ps_service import _Shard
    from distributedtensorflow_amd.parallel.strategy import Strategy

    class BetweenGraph(Strategy):
        mode = "between_graph"

    opt = AdamOptimizer(0.1, variable_averages=ExponentialMovingAverage(0.9))
    with BetweenGraph("cpu").scope():
        with pytest.raises(ValueError) as e:
            opt.build(ema_util.make_params())
    assert str(e.value) == EMA_BETWEEN_GRAPH and "between-graph" in EMA_BETWEEN_GRAPH
    assert opt.space is None
    cfg = opt.get_config()
    spec = {"names": ["dense/kernel", "dense/bias"], "shapes": [[4, 3], [3]], "optimizer": cfg}
    with pytest.raises(ValueError, match="between-graph"):
        _Shard(spec, torch.arange(15, dtype=torch.float32), torch.device("cpu"))
    host = AdamOptimizer(0.1)
    with OneDeviceStrategy("cpu").scope():
        sp = host.build(ema_util.make_params())
    with pytest.raises(ValueError, match="between-graph"):
        ps_device._make_optimizer(cfg, sp)


def test_get_config_carries_the_average_only_when_set():
    for name, factory in ema_util.OPTIMIZERS.items():
        plain = factory().get_config()
        assert "variable_averages" not in plain
        cfg = factory(variable_averages=ExponentialMovingAverage(0.75)).get_config()
        assert cfg == dict(plain, variable_averages={"decay": 0.75,
                                                     "name": "ExponentialMovingAverage"})
        json.dumps(cfg)
    # the dict is a description (it leaves num_updates out), not something to attach
    with pytest.raises(TypeError, match="ExponentialMovingAverage"):
        MomentumOptimizer(0.1, 0.9, variable_averages={"decay": 0.75})


def test_an_optimizer_that_overrides_refresh_hyper_still_refreshes_the_average():
    class Mine(MomentumOptimizer):
        def _refresh_hyper(self):
            self._lr_dev[0].fill_(self.learning_rate())

    gstep = dtf_train.get_or_create_global_step()
    ema = ExponentialMovingAverage(0.9999, num_updates=gstep)
    ps = ema_util.make_params()
    with OneDeviceStrategy("cpu").scope():
        opt = Mine(0.1, 0.9, variable_averages=ema)
        opt.build(ps)
    for n in (1, 2):
        for p, g in zip(ps, ema_util.make_grads(n)):
            p.grad.copy_(g)
        opt.apply_gradients(global_step=gstep)
        assert float(ema.a_dev.item()) == float(np.float32(1.0 - (1.0 + n) / (10.0 + n)))


# ---------------------------------------------------------------------------- checkpoints

def _setup(seed, decay=0.5, averages=True):
    gs_mod.reset_global_step()
    torch.manual_seed(seed)
    gstep = gs_mod.get_or_create_global_step()
    ema = ExponentialMovingAverage(decay, num_updates=gstep) if averages else None
    with OneDeviceStrategy("cpu").scope():
        model = ema_util.BNNet()
        opt = MomentumOptimizer(0.2, 0.9, variable_averages=ema)
        opt.build(list(model.parameters()))
    return model, opt, gstep, ema


def _train(model, opt, gstep, steps, first=0):
    for t in range(first, first + steps):
        x, y = ema_util.bn_batch(t)
        opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y), global_step=gstep)


def test_checkpoint_names_and_roundtrip(tmp_path):
    model, opt, gstep, ema = _setup(0)
    _train(model, opt, gstep, 3)
    prefix = Saver(model=model, optimizer=opt, global_step=gstep).save(
        None, str(tmp_path / "model.ckpt"), global_step=gstep)
    names = dict(list_variables(prefix))
    assert names["conv2d/kernel" + SUFFIX] == [3, 3, 1, 8]          # HWIO, as the variable
    assert names["dense/kernel" + SUFFIX] == [8, 10]
    assert names["batch_normalization/gamma" + SUFFIX] == [8]
    assert not any(n.startswith("batch_normalization/moving_") and n.endswith(SUFFIX)
                   for n in names)
    for p in opt.space.order:
        assert ema.average_name(p) == p._dtf_name + SUFFIX and ema.average_name(p) in names
    assert not torch.equal(ema.buf, opt.space.master)
    saved = ema.buf.clone()

    model2, opt2, gstep2, ema2 = _setup(123)
    assert not torch.equal(ema2.buf, saved)
    Saver(model=model2, optimizer=opt2, global_step=gstep2).restore(None, prefix)
    assert torch.equal(ema2.buf, saved) and torch.equal(opt2.space.master, opt.space.master)
    # the ramp continues from the restored global step, not from optimizer.iterations
    assert gstep2.value() == 3
    _train(model, opt, gstep, 1, first=3)
    _train(model2, opt2, gstep2, 1, first=3)
    assert float(ema2.a_dev.item()) == float(np.float32(1.0 - 5.0 / 14.0))
    assert torch.equal(ema2.buf, ema.buf)


def test_restoring_a_checkpoint_without_averages_starts_them_at_the_variables(tmp_path):
    model, opt, gstep, _ = _setup(0, averages=False)
    _train(model, opt, gstep, 2)
    prefix = Saver(model=model, optimizer=opt, global_step=gstep).save(
        None, str(tmp_path / "plain.ckpt"))
    assert not any(n.endswith(SUFFIX) for n, _ in list_variables(prefix))
    model2, opt2, gstep2, ema2 = _setup(5)
    missing = Saver(model=model2, optimizer=opt2, global_step=gstep2).restore(
        None, prefix, strict=True)
    assert missing == []
    assert torch.equal(opt2.space.master, opt.space.master)
    assert torch.equal(ema2.buf, opt2.space.master)
    # any other missing name behaves as before
    with pytest.raises(KeyError, match="nope"):
        Saver({"nope": torch.zeros(2)}).restore(None, prefix)


def test_variables_to_restore_loads_the_averages_into_a_fresh_model(tmp_path):
    model, opt, gstep, ema = _setup(0)
    _train(model, opt, gstep, 3)
    prefix = Saver(model=model, optimizer=opt, global_step=gstep).save(
        None, str(tmp_path / "model.ckpt"))
    torch.manual_seed(77)
    fresh = ema_util.BNNet()
    mapping = ema.variables_to_restore(fresh)
    assert "conv2d/kernel" + SUFFIX in mapping and "batch_normalization/moving_mean" in mapping
    assert Saver(mapping).restore(None, prefix) == []
    for p, q in zip(model.parameters(), fresh.parameters()):
        assert torch.equal(q.detach(), ema.average(p)) and not torch.equal(q.detach(), p.detach())
    assert torch.equal(fresh.bn.moving_mean, model.bn.moving_mean)


def test_bert_averages_export_under_the_tf_names_and_shapes(tmp_path):
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    cfg = BertConfig(vocab_size=200, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                     intermediate_size=256, max_position_embeddings=32, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0)
    ema = ExponentialMovingAverage(0.99)
    torch.manual_seed(3)
    with OneDeviceStrategy("cpu").scope():
        model = BertForPreTraining(cfg)
        opt = AdamOptimizer(1e-3, variable_averages=ema)
        opt.build(list(model.parameters()))
    prefix = Saver(model=model, optimizer=opt).save(None, str(tmp_path / "bert.ckpt"))
    names = dict(list_variables(prefix))
    pre = "bert/encoder/layer_0/attention/self/"
    for part in ("query", "key", "value"):
        assert names[f"{pre}{part}/kernel{SUFFIX}"] == [128, 128]
        assert names[f"{pre}{part}/bias{SUFFIX}"] == [128]
    assert names["bert/embeddings/word_embeddings" + SUFFIX] == [200, 128]
    assert names["cls/predictions/output_bias" + SUFFIX] == [200]
    assert not any("qkv" in n for n in names)
    np.testing.assert_array_equal(load_variable(prefix, f"{pre}key/kernel{SUFFIX}"),
                                  load_variable(prefix, f"{pre}key/kernel"))
    # average_name is per (fused) variable; average_names gives the checkpoint's names
    qkv = next(p for p in model.parameters() if p._dtf_name.endswith("qkv/kernel"))
    assert ema.average_name(qkv) == qkv._dtf_name + SUFFIX and ema.average_name(qkv) not in names
    assert ema.average_names(qkv) == [f"{pre}{part}/kernel{SUFFIX}"
                                      for part in ("query", "key", "value")]
    plain = next(p for p in model.parameters() if not getattr(p, "_dtf_splits", None))
    assert ema.average_names(plain) == [ema.average_name(plain)]
    assert all(n in names for p in model.parameters() for n in ema.average_names(p))
    mapping = ema.variables_to_restore(model)
    assert f"{pre}value/kernel{SUFFIX}" in mapping and not any("qkv" in n for n in mapping)
    assert tuple(mapping["bert/embeddings/word_embeddings" + SUFFIX][0].shape) == (200, 128)


# ---------------------------------------------------------------------------- swap, evaluate

def _eval(model, opt, ema=None):
    from distributedtensorflow_amd.metrics import ClassificationMetrics
    batches = [ema_util.bn_batch(900 + i) for i in range(2)]
    return dtf_train.evaluate(model, batches, ClassificationMetrics(k=5), optimizer=opt,
                              averages=ema)


def test_evaluate_on_the_averages():
    model, opt, gstep, ema = _setup(0)
    _train(model, opt, gstep, 4)
    raw, avg = _eval(model, opt), _eval(model, opt, ema)
    assert avg["loss"] != raw["loss"] and avg["count"] == raw["count"] == 32
    # a separate model loaded with the averaged weights (and the same moving statistics)
    torch.manual_seed(9)
    other = ema_util.BNNet()
    with torch.no_grad():
        for p, q in zip(model.parameters(), other.parameters()):
            q.copy_(ema.average(p))
        other.bn.moving_mean.copy_(model.bn.moving_mean)
        other.bn.moving_variance.copy_(model.bn.moving_variance)
    assert _eval(other, None) == avg
    assert model.training


def test_evaluate_refuses_averages_of_another_optimizer_or_model():
    model, opt, gstep, ema = _setup(0)
    other_model, other_opt, _, other_ema = _setup(1)
    with pytest.raises(ValueError, match="not attached to this optimizer"):
        _eval(model, opt, other_ema)
    with pytest.raises(ValueError, match="this model's variables"):
        _eval(other_model, opt, ema)
    with pytest.raises(ValueError, match="this model's variables"):
        _eval(other_model, None, ema)
    assert model.training and other_model.training
    assert _eval(model, opt, ema)["count"] == 32
    # through the TF1 wrapper as well
    with OneDeviceStrategy("cpu").scope():
        wrapped = SyncReplicasOptimizer(opt, 1)
    assert _eval(model, wrapped, ema)["count"] == 32


def test_training_after_an_evaluation_on_the_averages_is_bit_identical():
    ma, oa, ga, ea = _setup(0)
    _train(ma, oa, ga, 3)
    _eval(ma, oa, ea)
    _train(ma, oa, ga, 2, first=3)
    mb, ob, gb, eb = _setup(0)
    _train(mb, ob, gb, 5)
    assert torch.equal(oa.space.master, ob.space.master)
    assert len(oa.slots) == len(ob.slots) == 2
    for sa, sb in zip(oa.slots, ob.slots):
        assert torch.equal(sa.buf, sb.buf)
    assert torch.equal(ea.buf, eb.buf)
    assert torch.equal(ma.bn.moving_mean, mb.bn.moving_mean)
    assert torch.equal(ma.bn.moving_variance, mb.bn.moving_variance)
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p.detach(), q.detach())


def test_swap_puts_the_same_tensors_back_after_an_exception():
    model, opt, gstep, ema = _setup(0)
    _train(model, opt, gstep, 2)
    ps = list(model.parameters())
    ptrs = [p.data_ptr() for p in ps]
    grads = [p.grad for p in ps]
    values = [p.detach().clone() for p in ps]
    master = opt.space.master.clone()
    with pytest.raises(RuntimeError, match="boom"):
        with ema.swap():
            for p in ps:
                assert p.data_ptr() == ema.average(p).data_ptr()
                assert torch.equal(p.detach(), ema.average(p))
            with pytest.raises(RuntimeError, match="already active"):
                with ema.swap():
                    pass
            # the refused nested swap left the outer one in place
            assert ps[0].data_ptr() == ema.average(ps[0]).data_ptr()
            raise RuntimeError("boom")
    assert all(a is b for a, b in zip(model.parameters(), ps))
    for p, ptr, g, v in zip(ps, ptrs, grads, values):
        assert p.data_ptr() == ptr and p.grad is g and torch.equal(p.detach(), v)
        assert p.data_ptr() != ema.average(p).data_ptr()
    assert torch.equal(opt.space.master, master)
    with ema.swap():          # and it can be entered again
        pass


# ---------------------------------------------------------------------------- CLI

@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    from distributedtensorflow_amd.data import mnist
    d = tmp_path_factory.mktemp("mnist_ema")
    mnist.load_arrays(str(d), "train")
    mnist.load_arrays(str(d), "test")
    return str(d)


def _cli(data_dir, *extra, log_dir=""):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        env.pop(k, None)
    return subprocess.run([sys.executable, TRAIN, "--model", "mnist_mlp", "--device", "cpu",
                           *extra, "--train_steps", "3", "--data_dir", data_dir, "--log_dir",
                           log_dir],
                          capture_output=True, text=True, env=env, timeout=300)


def _result(r):
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


EMA_KEYS = ("eval_ema_loss", "eval_ema_top_1", "eval_ema_top_k")


def test_cli_ema_decay_evaluates_the_averaged_weights(data_dir, tmp_path):
    import glob
    from distributedtensorflow_amd.summary.events import read_scalars
    res = _result(_cli(data_dir, "--ema_decay", "0.9", "--eval", "--eval_every", "2",
                       log_dir=str(tmp_path / "tb")))
    assert res["global_step"] == 3
    for k in EMA_KEYS + ("eval_loss", "eval_top_1", "eval_top_k"):
        assert np.isfinite(res[k]), k
    assert res["eval_ema_loss"] != res["eval_loss"]
    # the EvalHook writes the averaged weights' figures next to the raw ones
    runs = glob.glob(str(tmp_path / "tb" / "*"))
    assert len(runs) == 1
    sc = read_scalars(runs[0])
    for tag in ("eval/loss", "eval/top_1", "eval/top_k", "eval/ema_loss", "eval/ema_top_1",
                "eval/ema_top_k"):
        assert [s for s, _ in sc[tag]] == [2], tag


def test_cli_ema_decay_checkpoints_the_averages(data_dir, tmp_path):
    res = _result(_cli(data_dir, "--ema_decay", "0.9", "--checkpoint_dir", str(tmp_path / "ck")))
    assert res["global_step"] == 3
    names = dict(list_variables(str(tmp_path / "ck")))
    for v in ("hid_w", "hid_b", "sm_w", "sm_b"):
        assert names[v + SUFFIX] == names[v]


def test_cli_without_ema_decay_reports_no_averaged_figures(data_dir):
    res = _result(_cli(data_dir, "--eval"))
    assert "eval_loss" in res and not any(k in res for k in EMA_KEYS)


def test_cli_between_graph_refuses_ema_decay(data_dir):
    r = _cli(data_dir, "--ema_decay", "0.9", "--job_name", "worker", "--ps_hosts",
             "127.0.0.1:1", "--worker_hosts", "127.0.0.1:2")
    assert r.returncode != 0 and EMA_BETWEEN_GRAPH in r.stderr
