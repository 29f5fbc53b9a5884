"""LARSOptimizer and the label-smoothed cross-entropy on the CPU (the reference path): update
math against a numpy fp64 transcription of tf.contrib.opt.LARSOptimizer, the trust ratio's
degenerate cases, range-restricted applies, config / parameter-server factories, checkpoint
names and round trip, the loss against a hand-written fp64 evaluation, and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.optimizers import LARSOptimizer
from distributedtensorflow_amd.parallel import OneDeviceStrategy
from test_optimizers import _params, check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")


class Lars:
    """tf.contrib.opt.LARSOptimizer per tensor, in fp64."""

    def __init__(self, lr, mu=0.9, wd=1e-4, eeta=1e-3, eps=0.0, nesterov=False):
        self.lr, self.mu, self.wd, self.eeta, self.eps = lr, mu, wd, eeta, eps
        self.nesterov = nesterov

    def init(self, p):
        return {"a": np.zeros_like(p)}

    def step(self, p, g, s, t, dec):
        lr = self.lr(t) if callable(self.lr) else self.lr
        scaled = lr
        if dec:
            wn, gn = np.linalg.norm(p), np.linalg.norm(g)
            if wn > 0 and gn > 0:
                scaled = lr * self.eeta * wn / (gn + self.wd * wn + self.eps)
            g = g + self.wd * p
        u = scaled * g
        s["a"] = self.mu * s["a"] + u
        return p - (u + self.mu * s["a"] if self.nesterov else s["a"])


# eeta = 1 keeps the steps large enough for the comparison to mean something
CASES = [
    ("plain", lambda: LARSOptimizer(0.5, eeta=1.0, weight_decay=0.01),
     Lars(0.5, eeta=1.0, wd=0.01)),
    ("nesterov", lambda: LARSOptimizer(0.5, eeta=1.0, weight_decay=0.01, use_nesterov=True),
     Lars(0.5, eeta=1.0, wd=0.01, nesterov=True)),
    ("no_decay", lambda: LARSOptimizer(0.5, eeta=1.0, weight_decay=0.0, epsilon=1e-3),
     Lars(0.5, eeta=1.0, wd=0.0, eps=1e-3)),
    ("defaults", lambda: LARSOptimizer(0.5), Lars(0.5)),
]


@pytest.mark.parametrize("name,factory,oracle", CASES, ids=[c[0] for c in CASES])
def test_lars_matches_tf_math_cpu(name, factory, oracle):
    check(factory, oracle, "cpu", rtol=1e-5, atol=1e-6, steps=4)


def test_lars_follows_a_schedule():
    """apply_gradients advances ``iterations`` first: update t uses learning_rate(t)."""
    sched = lambda t: 0.5 / (1 + t)                                       # noqa: E731
    check(lambda: LARSOptimizer(sched, eeta=1.0), Lars(sched, eeta=1.0), "cpu")


def _one_var(value, grad, **kw):
    p = torch.nn.Parameter(value.clone())
    p._dtf_name = "dense/kernel"
    opt = LARSOptimizer(0.5, momentum=0.9, weight_decay=0.01, eeta=1e-3, **kw)
    with OneDeviceStrategy("cpu").scope():
        opt.build([p])
    p.grad.copy_(grad)
    opt.apply_gradients()
    return p.detach(), opt.slots[0].buf[:p.numel()].view(p.shape)


def test_trust_ratio_is_one_for_zero_weights_or_zero_gradients():
    g = torch.Generator().manual_seed(3)
    w, gr = torch.randn(6, 4, generator=g), torch.randn(6, 4, generator=g)
    zero = torch.zeros(6, 4)
    # all-zero weights: s = lr, g2 = g (+ wd * 0)
    p, a = _one_var(zero, gr)
    torch.testing.assert_close(a, 0.5 * gr, rtol=1e-6, atol=0)
    torch.testing.assert_close(p, -0.5 * gr, rtol=1e-6, atol=0)
    # all-zero gradients: s = lr, g2 = wd * w -- NOT lr * eeta * |w| / (wd * |w|)
    p, a = _one_var(w, zero)
    torch.testing.assert_close(a, 0.5 * 0.01 * w, rtol=1e-6, atol=0)
    torch.testing.assert_close(p, w - 0.5 * 0.01 * w, rtol=1e-6, atol=0)


def test_lars_range_restricted_apply():
    ps = _params("cpu")
    opt = LARSOptimizer(0.1, eeta=1.0)
    with OneDeviceStrategy("cpu").scope():
        sp = opt.build(ps)
    before, slot_before = sp.master.clone(), opt.slots[0].buf.clone()
    sp.grad.fill_(1.0)
    opt.iterations = 1
    lo, hi = sp.offsets[1], sp.offsets[3]
    opt._apply(1.0, (lo, hi))
    for was, now in ((before, sp.master), (slot_before, opt.slots[0].buf)):
        changed = (now != was).nonzero().flatten()
        assert changed.min() >= lo and changed.max() < hi
    # both variables inside the range moved
    assert (sp.master[lo:sp.offsets[2]] != before[lo:sp.offsets[2]]).any()
    assert (sp.master[sp.offsets[2]:hi] != before[sp.offsets[2]:hi]).any()


def test_lars_is_not_elementwise_and_leaves_gradients():
    ps = _params("cpu")
    opt = LARSOptimizer(0.1)
    assert opt.elementwise is False
    with OneDeviceStrategy("cpu").scope():
        sp = opt.build(ps)
    assert sp.elementwise is False
    sp.grad.normal_()
    g = sp.grad.clone()
    opt.apply_gradients()
    assert torch.equal(sp.grad, g)


def test_lars_config_roundtrip_and_ps_factories():
    opt = LARSOptimizer(0.25, momentum=0.8, weight_decay=3e-4, eeta=2e-3, epsilon=1e-9,
                        use_nesterov=True, name="LARS_x", chunk=1024)
    cfg = dict(opt.get_config())
    assert cfg["type"] == "lars"
    json.dumps(cfg)                                   # shipped to parameter-server tasks
    kind = cfg.pop("type")
    clone = type(opt)(**cfg)
    assert clone.get_config() == opt.get_config() and kind == "lars"

    # the in-process parameter-server shard
    from distributedtensorflow_amd.parallel.ps_service import _Shard
    shapes = [[4, 3], [3]]
    spec = {"names": ["dense/kernel", "dense/bias"], "shapes": shapes,
            "optimizer": opt.get_config()}
    shard = _Shard(spec, torch.arange(15, dtype=torch.float32), torch.device("cpu"))
    built = [v for v in vars(shard).values() if isinstance(v, LARSOptimizer)]
    assert len(built) == 1
    assert built[0].get_config() == opt.get_config()

    # the device-plane parameter-server shard
    from distributedtensorflow_amd.parallel import ps_device
    ps = _params("cpu")
    host = LARSOptimizer(0.1)
    with OneDeviceStrategy("cpu").scope():
        sp = host.build(ps)
    dev_opt = ps_device._make_optimizer(opt.get_config(), sp)
    assert isinstance(dev_opt, LARSOptimizer)
    assert dev_opt.get_config() == opt.get_config()
    assert dev_opt.slots[0].name == "LARS_x" and hasattr(dev_opt, "_norms")


def test_lars_slot_names():
    ps = _params("cpu")
    opt = LARSOptimizer(0.1)
    with OneDeviceStrategy("cpu").scope():
        opt.build(ps)
    names = sorted(opt.slot_variables())
    assert names == sorted(f"{p._dtf_name}/LARSOptimizer" for p in ps)
    assert opt.non_slot_variables() == {}


def test_lars_checkpoint_roundtrip(tmp_path):
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.optimizers.optimizers import polynomial_decay
    from distributedtensorflow_amd.train import Saver, list_variables, reset_global_step
    from distributedtensorflow_amd.train import global_step as gs_mod

    def setup(seed):
        reset_global_step()
        torch.manual_seed(seed)
        strat = OneDeviceStrategy("cpu")
        with strat.scope():
            model = MnistCNN()
            opt = LARSOptimizer(polynomial_decay(0.5, 8, power=2, warmup_steps=2), eeta=0.1)
            gstep = gs_mod.get_or_create_global_step()
            opt.build(list(model.parameters()))
        return model, opt, gstep

    g = torch.Generator().manual_seed(7)
    x, y = torch.rand(16, 784, generator=g), torch.randint(0, 10, (16,), generator=g)

    def train(model, opt, gstep, n):
        for _ in range(n):
            opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y, 0.1), global_step=gstep)

    try:
        model, opt, gstep = setup(0)
        train(model, opt, gstep, 3)
        prefix = Saver(model=model, optimizer=opt, global_step=gstep).save(
            None, str(tmp_path / "model.ckpt"), global_step=gstep)
        names = dict(list_variables(prefix))
        assert names["conv2d/kernel/LARSOptimizer"] == [5, 5, 1, 32]
        assert names["dense/bias/LARSOptimizer"] == [1024]
        slot, master = opt.slots[0].buf.clone(), opt.space.master.clone()
        train(model, opt, gstep, 2)
        want = opt.space.master.clone()

        model2, opt2, gstep2 = setup(123)
        assert not torch.equal(opt2.space.master, master)
        Saver(model=model2, optimizer=opt2, global_step=gstep2).restore(None, prefix)
        assert opt2.iterations == 3 and gstep2.value() == 3
        assert torch.equal(opt2.slots[0].buf, slot) and (slot != 0).any()
        assert torch.equal(opt2.space.master, master)
        # the schedule resumes at the restored step: two more steps land where the first run did
        train(model2, opt2, gstep2, 2)
        torch.testing.assert_close(opt2.space.master, want, rtol=1e-6, atol=1e-7)
    finally:
        reset_global_step()


# ---------------------------------------------------------------------------- label smoothing

def _xent_numpy(x, lab, e):
    """loss_b = lse - (1-e) x[label] - (e/V) sum_i x_i;  grad = (p - (1-e) onehot - e/V) / B."""
    x = x.astype(np.float64)
    B, V = x.shape
    mx = x.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))[:, 0]
    loss = lse - (1 - e) * x[np.arange(B), lab] - (e / V) * x.sum(1)
    onehot = np.zeros_like(x)
    onehot[np.arange(B), lab] = 1.0
    grad = (np.exp(x - lse[:, None]) - (1 - e) * onehot - e / V) / B
    return loss.mean(), grad


def test_label_smoothing_value_and_gradient_cpu():
    g = torch.Generator().manual_seed(11)
    x = (3 * torch.randn(5, 7, generator=g)).requires_grad_()
    lab = torch.randint(0, 7, (5,), generator=g)
    loss = ops.sparse_softmax_cross_entropy(x, lab, label_smoothing=0.1)
    loss.backward()
    want, want_grad = _xent_numpy(x.detach().numpy(), lab.numpy(), 0.1)
    np.testing.assert_allclose(loss.item(), want, rtol=1e-6)
    np.testing.assert_allclose(x.grad.numpy(), want_grad, rtol=1e-5, atol=1e-7)
    # smoothing changes the value
    assert abs(loss.item() - _xent_numpy(x.detach().numpy(), lab.numpy(), 0.0)[0]) > 1e-3


def test_label_smoothing_zero_is_the_old_call():
    g = torch.Generator().manual_seed(12)
    x = torch.randn(5, 7, generator=g)
    lab = torch.randint(0, 7, (5,), generator=g)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    la = ops.sparse_softmax_cross_entropy(xa, lab)
    lb = ops.sparse_softmax_cross_entropy(xb, lab, label_smoothing=0.0)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad)
    with pytest.raises(ValueError):
        ops.sparse_softmax_cross_entropy(x, lab, label_smoothing=1.5)


# ---------------------------------------------------------------------------- CLI

@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    from distributedtensorflow_amd.data import mnist
    d = tmp_path_factory.mktemp("mnist_lars")
    mnist.load_arrays(str(d), "train")
    return str(d)


def _cli(data_dir, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        env.pop(k, None)
    return subprocess.run([sys.executable, TRAIN, "--model", "mnist_mlp", "--strategy",
                           "onedevice", "--device", "cpu", "--optimizer", "lars", *extra,
                           "--label_smoothing", "0.1", "--train_steps", "5", "--data_dir",
                           data_dir, "--log_dir", ""],
                          capture_output=True, text=True, env=env, timeout=300)


def test_cli_lars_trains(data_dir):
    r = _cli(data_dir, "--learning_rate", "0.5")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    res = json.loads(lines[-1])
    assert res["global_step"] == 5
    assert res["final_loss"] is not None and np.isfinite(res["final_loss"])


def test_cli_lars_needs_a_learning_rate(data_dir):
    r = _cli(data_dir)
    assert r.returncode != 0
    assert "--learning_rate" in r.stderr


def test_cli_builds_the_large_batch_schedule():
    from distributedtensorflow_amd.cli import _make_optimizer
    from distributedtensorflow_amd.optimizers.optimizers import polynomial_decay
    opt = _make_optimizer("lars", 2.0, "resnet50", 15872, max_steps=100)
    assert isinstance(opt, LARSOptimizer) and opt.momentum == 0.9 and opt.weight_decay == 1e-4
    want = polynomial_decay(2.0, 100, power=2, warmup_steps=5)
    for t in (0, 4, 5, 50, 100):
        assert opt.learning_rate(t) == pytest.approx(want(t))
