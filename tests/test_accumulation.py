"""Gradient accumulation over micro-batches (``accumulation_steps=N``) on the CPU path: the
bit-exact oracle under every optimizer class, what held micro-steps leave alone, one large batch,
``N == 1``, validation, ``reset_accumulation`` and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd import train as dtf_train
from distributedtensorflow_amd.models import MnistCNN
from distributedtensorflow_amd.optimizers import (AdagradOptimizer, AdamOptimizer,
                                                  AdamWeightDecayOptimizer,
                                                  ExponentialMovingAverage,
                                                  GradientDescentOptimizer, LAMBOptimizer,
                                                  LARSOptimizer, MomentumOptimizer,
                                                  SyncReplicasOptimizer)
from distributedtensorflow_amd.parallel import OneDeviceStrategy
from distributedtensorflow_amd.train import global_step as gs_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")

# clip_norm low enough that the updates are clipped (asserted where it is used)
CLIP = 0.05

OPTIMIZERS = {
    "sgd": lambda **kw: GradientDescentOptimizer(0.05, **kw),
    "momentum": lambda **kw: MomentumOptimizer(0.05, 0.9, **kw),
    "nesterov": lambda **kw: MomentumOptimizer(0.05, 0.9, use_nesterov=True, **kw),
    "adam": lambda **kw: AdamOptimizer(1e-3, **kw),
    "adamw": lambda **kw: AdamWeightDecayOptimizer(1e-3, **kw),
    "adagrad": lambda **kw: AdagradOptimizer(0.01, **kw),
    "lamb": lambda **kw: LAMBOptimizer(1e-3, weight_decay=0.01, **kw),
    "lars": lambda **kw: LARSOptimizer(0.05, 0.9, weight_decay=1e-4, **kw),
    "momentum_clip": lambda **kw: MomentumOptimizer(0.05, 0.9, clip_norm=CLIP, **kw),
}


@pytest.fixture(autouse=True)
def _fresh_global_step():
    gs_mod.reset_global_step()
    yield
    gs_mod.reset_global_step()


def batch(i, n=8):
    g = torch.Generator().manual_seed(500 + i)
    return torch.rand(n, 784, generator=g), torch.randint(0, 10, (n,), generator=g)


def loss_of(model, xy):
    return ops.sparse_softmax_cross_entropy(model(xy[0]), xy[1])


def make(name, seed=11, **kw):
    torch.manual_seed(seed)
    with OneDeviceStrategy("cpu").scope():
        model = MnistCNN()
        opt = OPTIMIZERS[name](**kw)
        opt.build(list(model.parameters()))
    return model, opt


def oracle_update(model, opt, batches):
    """One update of a plain optimizer from the micro-batches' gradients summed in fp32 in
    micro-step order, multiplied once by 1 / N inside the update."""
    total = None
    for xy in batches:
        opt.compute_gradients(loss_of(model, xy))
        g = opt.space.grad.clone()
        total = g if total is None else total + g
    opt.space.grad.copy_(total)
    opt.iterations += 1
    opt._apply(1.0 / len(batches))


def assert_same_state(model, opt, ref_model, ref_opt):
    for (k, a), b in zip(model.state_dict().items(), ref_model.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(opt.space.master, ref_opt.space.master)
    assert len(opt.slots) == len(ref_opt.slots)
    for a, b in zip(opt.slots, ref_opt.slots):
        assert torch.equal(a.buf, b.buf), a.name
    if opt.clip_norm is not None:
        assert torch.equal(opt.last_grad_norm, ref_opt.last_grad_norm)


# ---------------------------------------------------------------------------- 1. the oracle

@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_every_optimizer_meets_the_bit_exact_oracle(name):
    N, updates = 3, 2
    model, opt = make(name, accumulation_steps=N)
    ref_model, ref_opt = make(name)
    assert torch.equal(opt.space.master, ref_opt.space.master)
    clipped = 0
    for u in range(updates):
        bs = [batch(u * N + k) for k in range(N)]
        for xy in bs:
            opt.minimize(loss_of(model, xy))
        oracle_update(ref_model, ref_opt, bs)
        assert_same_state(model, opt, ref_model, ref_opt)
        assert opt.iterations == ref_opt.iterations == u + 1
        if opt.clip_norm is not None:
            clipped += int(float(opt.last_grad_norm) > CLIP)
    if name == "momentum_clip":
        assert clipped >= 1
    assert not torch.equal(opt.space.master, make(name)[1].space.master)   # it trained


# ---------------------------------------------------------------------------- 2. held steps

def test_held_steps_move_nothing():
    N = 3
    gstep = dtf_train.get_or_create_global_step()
    calls = []

    def lr(step):
        calls.append(step)
        return 0.05

    ema = ExponentialMovingAverage(0.9999, num_updates=gstep)
    torch.manual_seed(11)
    with OneDeviceStrategy("cpu").scope():
        model = MnistCNN()
        opt = MomentumOptimizer(lr, 0.9, variable_averages=ema, accumulation_steps=N)
        opt.build(list(model.parameters()))
    assert opt.accumulation_steps == N and opt.accumulated == 0
    i = 0
    for update in (1, 2):
        state0 = {k: v.clone() for k, v in model.state_dict().items()}
        slots0 = [s.buf.clone() for s in opt.slots]
        ema0, it0, gs0, calls0 = ema.buf.clone(), opt.iterations, gstep.value(), len(calls)
        for held in range(1, N):
            assert opt.minimize(loss_of(model, batch(i)), global_step=gstep) is None
            i += 1
            assert opt.accumulated == held
            for k, v in model.state_dict().items():
                assert torch.equal(v, state0[k]), k
            for s, s0 in zip(opt.slots, slots0):
                assert torch.equal(s.buf, s0), s.name
            assert torch.equal(ema.buf, ema0)
            assert (opt.iterations, gstep.value(), len(calls)) == (it0, gs0, calls0)
        assert opt.minimize(loss_of(model, batch(i)), global_step=gstep) is None
        i += 1
        assert opt.accumulated == 0
        assert opt.iterations == it0 + 1 == update and gstep.value() == gs0 + 1 == update
        assert len(calls) == calls0 + 1
        assert all(not torch.equal(v, state0[k]) for k, v in model.state_dict().items())
        assert not torch.equal(ema.buf, ema0)
        # tests/test_ema.py's convention, n counted in updates
        n = update
        assert float(ema.a_dev.item()) == float(np.float32(1.0 - (1.0 + n) / (10.0 + n)))


# ---------------------------------------------------------------------------- 3. one large batch

def test_two_micro_batches_match_one_batch_of_both():
    model, opt = make("momentum", accumulation_steps=2)
    ref_model, ref_opt = make("momentum")
    a, b = batch(0, 16), batch(1, 16)
    opt.minimize(loss_of(model, a))
    opt.minimize(loss_of(model, b))
    ref_opt.minimize(loss_of(ref_model, (torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]))))
    # fp32 gradients summed in another order: tests/test_clip_distributed.py's tolerance
    torch.testing.assert_close(opt.space.master, ref_opt.space.master, atol=2e-5, rtol=1e-5)
    for s, r in zip(opt.slots, ref_opt.slots):
        torch.testing.assert_close(s.buf, r.buf, atol=2e-5, rtol=1e-5)


# ---------------------------------------------------------------------------- 4. N == 1

@pytest.mark.parametrize("name", ["momentum", "lamb", "momentum_clip"])
def test_one_step_is_todays_path(name):
    model, opt = make(name, accumulation_steps=1)
    ref_model, ref_opt = make(name)
    assert opt.space.accum is None and ref_opt.space.accum is None
    assert opt.get_config() == ref_opt.get_config()
    assert "accumulation_steps" not in opt.get_config()
    for i in range(3):
        opt.minimize(loss_of(model, batch(i)))
        ref_opt.minimize(loss_of(ref_model, batch(i)))
        assert opt.accumulated == 0
    assert_same_state(model, opt, ref_model, ref_opt)
    assert opt.iterations == 3


def test_config_names_the_steps_only_when_accumulating():
    assert MomentumOptimizer(0.1, 0.9, accumulation_steps=4).get_config()[
        "accumulation_steps"] == 4
    _, opt = make("adam", accumulation_steps=2)
    assert opt.space.accum is not None and opt.space.accum.shape == opt.space.grad.shape
    assert opt.space.accum.dtype == torch.float32


# ---------------------------------------------------------------------------- 5. validation

@pytest.mark.parametrize("bad", [0, -1, 2.5, True])
@pytest.mark.parametrize("name", ["momentum", "lamb", "adamw"])
def test_steps_must_be_a_positive_int(name, bad):
    with pytest.raises(ValueError, match="accumulation_steps"):
        OPTIMIZERS[name](accumulation_steps=bad)


def test_sync_replicas_optimizer_delegates():
    torch.manual_seed(11)
    with OneDeviceStrategy("cpu").scope():
        model = MnistCNN()
        opt = SyncReplicasOptimizer(MomentumOptimizer(0.05, 0.9, accumulation_steps=2), 1)
        opt.build(list(model.parameters()))
    ref_model, ref_opt = make("momentum")
    assert opt.accumulation_steps == 2
    opt.minimize(loss_of(model, batch(0)))
    assert opt.accumulated == 1 and opt.iterations == 0
    opt.minimize(loss_of(model, batch(1)))
    assert opt.accumulated == 0 and opt.iterations == 1
    oracle_update(ref_model, ref_opt, [batch(0), batch(1)])
    assert torch.equal(opt.space.master, ref_opt.space.master)


def test_between_graph_ps_refuses_accumulation():
    from distributedtensorflow_amd.optimizers.base import ACCUM_BETWEEN_GRAPH
    from distributedtensorflow_amd.parallel.strategy import Strategy

    class BetweenGraph(Strategy):
        mode = "between_graph"

        def make_gradient_reducer(self, space):
            raise AssertionError("the refusal comes before the reducer is made")

    assert "apply each pushed gradient on arrival" in ACCUM_BETWEEN_GRAPH
    with BetweenGraph("cpu").scope():
        model = MnistCNN()
        opt = MomentumOptimizer(0.05, 0.9, accumulation_steps=2)
        with pytest.raises(ValueError, match="apply each pushed gradient on arrival"):
            opt.build(list(model.parameters()))
        assert opt.space is None


# ---------------------------------------------------------------------------- 6. reset

def test_reset_drops_the_partial_accumulation():
    model, opt = make("momentum", accumulation_steps=2)
    ref_model, ref_opt = make("momentum")
    opt.minimize(loss_of(model, batch(7)))          # dropped below
    assert opt.accumulated == 1
    opt.reset_accumulation()
    assert opt.accumulated == 0 and opt.iterations == 0
    opt.minimize(loss_of(model, batch(0)))
    assert opt.accumulated == 1
    opt.minimize(loss_of(model, batch(1)))
    assert opt.accumulated == 0 and opt.iterations == 1
    oracle_update(ref_model, ref_opt, [batch(0), batch(1)])
    assert_same_state(model, opt, ref_model, ref_opt)


def test_sync_after_restore_resets():
    strat = OneDeviceStrategy("cpu")
    torch.manual_seed(11)
    with strat.scope():
        model = MnistCNN()
        opt = MomentumOptimizer(0.05, 0.9, accumulation_steps=2)
        opt.build(list(model.parameters()))
    opt.minimize(loss_of(model, batch(0)))
    assert opt.accumulated == 1
    strat.sync_after_restore(opt, None, restored=True)
    assert opt.accumulated == 0


# ---------------------------------------------------------------------------- 7. CLI

@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    from distributedtensorflow_amd.data import mnist
    d = tmp_path_factory.mktemp("mnist_accum")
    mnist.load_arrays(str(d), "train")
    return str(d)


def _train(data_dir, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        env.pop(k, None)
    cmd = [sys.executable, TRAIN, "--model", "mnist_mlp", "--strategy", "onedevice", "--device",
           "cpu", "--train_steps", "3", "--batch_size", "16", "--data_dir", data_dir,
           "--log_dir", "", *flags]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)


def _result(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_cli_counts_updates(data_dir):
    res = _result(_train(data_dir, "--accumulation_steps", "2"))
    assert res["global_step"] == 3 and res["accumulation_steps"] == 2
    assert res["final_loss"] is not None and np.isfinite(res["final_loss"])
    plain = _result(_train(data_dir))
    assert plain["global_step"] == 3 and "accumulation_steps" not in plain


def test_cli_refuses_bad_steps(data_dir):
    r = _train(data_dir, "--accumulation_steps", "0")
    assert r.returncode != 0 and "accumulation_steps" in r.stderr + r.stdout
    r = _train(data_dir, "--accumulation_steps", "2", "--job_name", "worker")
    assert r.returncode != 0
    assert "apply each pushed gradient on arrival" in r.stderr + r.stdout
