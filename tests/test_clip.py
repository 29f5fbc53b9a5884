"""Global-norm clipping inside the optimizer update, and AdamWeightDecayOptimizer, on the CPU (the
reference path): a numpy fp64 oracle of tf.clip_by_global_norm followed by each optimizer's
documented update, bit-identity of a clip that never clips, the error paths and the CLI."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd.optimizers import (AdagradOptimizer, AdamOptimizer,
                                                  AdamWeightDecayOptimizer,
                                                  GradientDescentOptimizer, LAMBOptimizer,
                                                  LARSOptimizer, MomentumOptimizer)
from distributedtensorflow_amd.optimizers.base import default_decay_filter
from distributedtensorflow_amd.parallel import OneDeviceStrategy
from test_lars import Lars
from test_optimizers import Adagrad, Adam, Lamb, Momentum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")
STEPS = 3
GSCALE = 0.5
RTOL, ATOL = 1e-5, 1e-6         # test_optimizers.check's, and test_lars's
# odd sizes; the default filter decays the two kernels, BERT's filter everything but the bias and
# the LayerNorm variable
VARS = [("dense/kernel", (7, 5)), ("dense/bias", (5,)), ("conv2d/kernel", (3, 3, 2, 4)),
        ("LayerNorm/gamma", (131,)), ("bn/beta", (33,))]


class AdamW:
    """google-research/bert AdamWeightDecayOptimizer per tensor, in fp64."""

    def __init__(self, lr, wd=0.01, b1=0.9, b2=0.999, eps=1e-6):
        self.lr, self.wd, self.b1, self.b2, self.eps = lr, wd, b1, b2, eps

    def init(self, p):
        return {"m": np.zeros_like(p), "v": np.zeros_like(p)}

    def step(self, p, g, s, t, dec):
        s["m"] = self.b1 * s["m"] + (1 - self.b1) * g
        s["v"] = self.b2 * s["v"] + (1 - self.b2) * g * g
        u = s["m"] / (np.sqrt(s["v"]) + self.eps)
        return p - self.lr * (u + (self.wd * p if dec else 0.0))


def clip_by_global_norm(gs, clip):
    """tf.clip_by_global_norm in fp64 -> (clipped list, global norm)."""
    norm = math.sqrt(sum(float((g * g).sum()) for g in gs))
    return [g * clip / max(norm, clip) for g in gs], norm


def _bert_decay(v):
    return not any(k in v._dtf_name for k in ("LayerNorm", "layer_norm", "bias"))


# name -> (factory(**kw), oracle, decay filter, slot key(s) of the oracle state)
OPTIMIZERS = {
    "sgd": (lambda **kw: GradientDescentOptimizer(0.1, weight_decay=1e-2, **kw),
            Momentum(0.1, 0.0, wd=1e-2), default_decay_filter),
    "momentum": (lambda **kw: MomentumOptimizer(0.1, 0.9, weight_decay=1e-2, **kw),
                 Momentum(0.1, 0.9, wd=1e-2), default_decay_filter),
    "nesterov": (lambda **kw: MomentumOptimizer(0.05, 0.9, use_nesterov=True, **kw),
                 Momentum(0.05, 0.9, True), default_decay_filter),
    "adam": (lambda **kw: AdamOptimizer(0.01, 0.8, 0.99, 1e-6, **kw),
             Adam(0.01, 0.8, 0.99, 1e-6), default_decay_filter),
    "adagrad": (lambda **kw: AdagradOptimizer(0.01, **kw), Adagrad(0.01), default_decay_filter),
    "lamb": (lambda **kw: LAMBOptimizer(1e-3, weight_decay=0.01, **kw), Lamb(1e-3, 0.01),
             default_decay_filter),
    "lars": (lambda **kw: LARSOptimizer(0.5, eeta=1.0, weight_decay=0.01, **kw),
             Lars(0.5, eeta=1.0, wd=0.01), default_decay_filter),
    "adamw": (lambda **kw: AdamWeightDecayOptimizer(0.01, **kw), AdamW(0.01), _bert_decay),
}
# the global norm of GSCALE * g is ~ 0.5 * sqrt(261) = 8: clipped, not clipped, and S == 0
CLIPS = {"clipped": (1.0, False), "not_clipped": (100.0, False), "zero_gradient": (1.0, True)}


def make_params(device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for name, shape in VARS:
        p = torch.nn.Parameter(torch.randn(shape, generator=g, device="cpu").to(device))
        p._dtf_name = name
        ps.append(p)
    return ps


def make_grads(step, zero=False):
    # explicit CPU: inside a GPU strategy's scope the default device is the GPU
    g = torch.Generator().manual_seed(100 + step)
    return [torch.zeros(s, device="cpu") if zero else torch.randn(s, generator=g, device="cpu")
            for _, s in VARS]


def run_steps(opt, device, zero=False, gscale=GSCALE):
    """STEPS updates through ``_apply``; per step (masters, pre-clip norm) on the CPU."""
    ps = make_params(device)
    out = []
    with OneDeviceStrategy(device).scope():
        sp = opt.build(ps)
        for t in range(STEPS):
            sp.zero_grad()
            for p, g in zip(ps, make_grads(t, zero)):
                p.grad.copy_(g.to(device))
            opt.iterations += 1
            opt._apply(gscale)
            norm = None if opt.last_grad_norm is None else float(opt.last_grad_norm.item())
            out.append(([p.detach().cpu().clone() for p in ps], norm))
    return opt, ps, out


def oracle_steps(oracle, decays, clip, zero=False, gscale=GSCALE):
    """Per step (masters, pre-clip norm) of the fp64 oracle."""
    ps = make_params()
    cur = [p.detach().double().numpy().copy() for p in ps]
    state = [oracle.init(c) for c in cur]
    out = []
    for t in range(STEPS):
        gs, norm = clip_by_global_norm([g.double().numpy() * gscale for g in make_grads(t, zero)],
                                       clip)
        for i, p in enumerate(ps):
            cur[i] = oracle.step(cur[i], gs[i], state[i], t + 1, bool(decays(p)))
        out.append(([c.copy() for c in cur], norm))
    return out


@pytest.mark.parametrize("case", list(CLIPS))
@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_clipped_update_matches_the_oracle(name, case):
    factory, oracle, decays = OPTIMIZERS[name]
    clip, zero = CLIPS[case]
    _, _, got = run_steps(factory(clip_norm=clip), "cpu", zero)
    want = oracle_steps(oracle, decays, clip, zero)
    for t in range(STEPS):
        assert got[t][1] == pytest.approx(want[t][1], rel=1e-6, abs=0.0)
        if case == "clipped":
            assert want[t][1] > clip
        elif case == "not_clipped":
            assert 0 < want[t][1] < clip
        for (vname, _), a, b in zip(VARS, got[t][0], want[t][0]):
            np.testing.assert_allclose(a.double().numpy(), b, rtol=RTOL, atol=ATOL,
                                       err_msg=f"{vname}, step {t + 1}")


def test_the_clip_changes_the_update():
    """The oracle comparison above means something: clipped and unclipped runs differ."""
    factory = OPTIMIZERS["momentum"][0]
    _, _, a = run_steps(factory(clip_norm=1.0), "cpu")
    _, _, b = run_steps(factory(), "cpu")
    assert not torch.equal(a[-1][0][0], b[-1][0][0])


@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_a_clip_that_never_clips_is_bit_identical(name):
    factory = OPTIMIZERS[name][0]
    oa, _, a = run_steps(factory(clip_norm=1e30), "cpu")
    ob, _, b = run_steps(factory(), "cpu")
    for (pa, _), (pb, _) in zip(a, b):
        for x, y in zip(pa, pb):
            assert torch.equal(x, y)
    for sa, sb in zip(oa.slots, ob.slots):
        assert torch.equal(sa.buf, sb.buf)
    assert torch.equal(oa.space.master, ob.space.master)
    assert oa._gmul.item() == GSCALE and ob.last_grad_norm is None


def test_nonfinite_gradient_gives_a_nan_multiplier():
    opt = MomentumOptimizer(0.1, 0.9, clip_norm=1.0)
    ps = make_params()
    with OneDeviceStrategy("cpu").scope():
        sp = opt.build(ps)
    sp.grad.normal_()
    sp.grad[3] = float("inf")
    opt.iterations += 1
    opt._apply(1.0)
    assert math.isnan(opt._gmul.item())
    assert torch.isnan(sp.master).any()


# ---------------------------------------------------------------------------- AdamWeightDecay

def test_adamw_excluded_names_get_no_decay():
    """Zero gradients: only the decoupled decay moves a variable, by exactly lr * wd * p."""
    opt = AdamWeightDecayOptimizer(0.1, weight_decay_rate=0.5)
    ps = make_params()
    before = [p.detach().clone() for p in ps]
    with OneDeviceStrategy("cpu").scope():
        sp = opt.build(ps)
    sp.zero_grad()
    opt.apply_gradients()
    for (name, _), p, b in zip(VARS, ps, before):
        if name in ("dense/bias", "LayerNorm/gamma"):
            assert torch.equal(p.detach(), b), name
        else:
            torch.testing.assert_close(p.detach(), b * (1 - 0.1 * 0.5), rtol=1e-6, atol=1e-7)
    # a custom exclusion list is a list of re.search patterns
    custom = AdamWeightDecayOptimizer(0.1, exclude_from_weight_decay=["^conv"])
    assert [custom.decay_filter(p) for p in ps] == [True, True, False, True, True]


def test_adamw_has_no_bias_correction():
    """One step from zero slots: m = (1-b1) g, v = (1-b2) g^2, so the step is
    lr * (1-b1) / sqrt(1-b2) * sign(g) = 3.16 lr, where tf.train.AdamOptimizer's is lr."""
    lr = 0.01
    opt = AdamWeightDecayOptimizer(lr, weight_decay_rate=0.0, epsilon=1e-12)
    ps = make_params()
    before = [p.detach().clone() for p in ps]
    grads = make_grads(0)
    with OneDeviceStrategy("cpu").scope():
        opt.build(ps)
    for p, g in zip(ps, grads):
        p.grad.copy_(g)
    opt.apply_gradients()
    oracle = AdamW(lr, 0.0, eps=1e-12)
    for p, b, g in zip(ps, before, grads):
        want = oracle.step(b.double().numpy(), g.double().numpy(),
                           oracle.init(b.double().numpy()), 1, True)
        np.testing.assert_allclose(p.detach().double().numpy(), want, rtol=RTOL, atol=ATOL)
        step = (b - p.detach()).abs()
        torch.testing.assert_close(step, torch.full_like(step, lr * 0.1 / math.sqrt(0.001)),
                                   rtol=1e-3, atol=0)


def test_adamw_slot_names_and_no_beta_powers():
    opt = AdamWeightDecayOptimizer(0.1)
    ps = make_params()
    with OneDeviceStrategy("cpu").scope():
        opt.build(ps)
    assert opt.slot_names == ("adam_m", "adam_v")
    want = sorted(f"{n}/{s}" for n, _ in VARS for s in ("adam_m", "adam_v"))
    assert sorted(opt.slot_variables()) == want
    assert opt.non_slot_variables() == {}


def test_adamw_checkpoint_roundtrip(tmp_path):
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.optimizers.optimizers import polynomial_decay
    from distributedtensorflow_amd.train import Saver, list_variables, reset_global_step
    from distributedtensorflow_amd.train import global_step as gs_mod

    def setup(seed):
        reset_global_step()
        torch.manual_seed(seed)
        with OneDeviceStrategy("cpu").scope():
            model = MnistCNN()
            opt = AdamWeightDecayOptimizer(polynomial_decay(0.01, 8, warmup_steps=2),
                                           clip_norm=1.0)
            gstep = gs_mod.get_or_create_global_step()
            opt.build(list(model.parameters()))
        return model, opt, gstep

    g = torch.Generator().manual_seed(7)
    x, y = torch.rand(16, 784, generator=g), torch.randint(0, 10, (16,), generator=g)

    def train(model, opt, gstep, n):
        for _ in range(n):
            opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y), global_step=gstep)

    try:
        model, opt, gstep = setup(0)
        train(model, opt, gstep, 3)
        prefix = Saver(model=model, optimizer=opt, global_step=gstep).save(
            None, str(tmp_path / "model.ckpt"), global_step=gstep)
        names = dict(list_variables(prefix))
        assert names["conv2d/kernel/adam_m"] == [5, 5, 1, 32]
        assert names["dense/bias/adam_v"] == [1024]
        assert not any("beta1_power" in n or "beta2_power" in n for n in names)
        slots = [s.buf.clone() for s in opt.slots]
        master = opt.space.master.clone()
        train(model, opt, gstep, 2)
        want = opt.space.master.clone()

        model2, opt2, gstep2 = setup(123)
        Saver(model=model2, optimizer=opt2, global_step=gstep2).restore(None, prefix)
        assert opt2.iterations == 3 and gstep2.value() == 3
        for s, b in zip(opt2.slots, slots):
            assert torch.equal(s.buf, b) and (b != 0).any()
        assert torch.equal(opt2.space.master, master)
        train(model2, opt2, gstep2, 2)
        torch.testing.assert_close(opt2.space.master, want, rtol=1e-6, atol=1e-7)
    finally:
        reset_global_step()


# ---------------------------------------------------------------------------- error paths

@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_clip_norm_must_be_positive(bad):
    with pytest.raises(ValueError, match="clip_norm"):
        MomentumOptimizer(0.1, 0.9, clip_norm=bad)
    with pytest.raises(ValueError, match="clip_norm"):
        AdamWeightDecayOptimizer(0.1, clip_norm=bad)


def test_between_graph_ps_refuses_clip_norm():
    """The between-graph worker pushes gradient buckets from the backward hooks: no place for a
    global norm.  Refused at build on the worker, and in both PS-side optimizer factories."""
    from distributedtensorflow_amd.parallel import ps_device
    from distributedtensorflow_amd.parallel.ps_service import _Shard
    from distributedtensorflow_amd.parallel.strategy import Strategy

    class BetweenGraph(Strategy):
        mode = "between_graph"

    opt = AdamOptimizer(0.1, clip_norm=1.0)
    with BetweenGraph("cpu").scope():
        with pytest.raises(ValueError, match="between-graph"):
            opt.build(make_params())
    assert opt.space is None

    cfg = opt.get_config()
    spec = {"names": ["dense/kernel", "dense/bias"], "shapes": [[4, 3], [3]], "optimizer": cfg}
    with pytest.raises(ValueError, match="between-graph"):
        _Shard(spec, torch.arange(15, dtype=torch.float32), torch.device("cpu"))
    host = AdamOptimizer(0.1)
    with OneDeviceStrategy("cpu").scope():
        sp = host.build(make_params())
    with pytest.raises(ValueError, match="between-graph"):
        ps_device._make_optimizer(cfg, sp)
    # without the clip both factories build, adamw included
    made = ps_device._make_optimizer(AdamWeightDecayOptimizer(0.1).get_config(), sp)
    assert isinstance(made, AdamWeightDecayOptimizer) and made.slots[0].name == "adam_m"


def test_get_config_carries_clip_norm_only_when_set():
    want = {
        "sgd": {"type": "sgd", "learning_rate": 0.5, "weight_decay": 0.0},
        "momentum": {"type": "momentum", "learning_rate": 0.5, "momentum": 0.9,
                     "use_nesterov": False, "weight_decay": 0.0},
        "adam": {"type": "adam", "learning_rate": 0.5, "beta1": 0.9, "beta2": 0.999,
                 "epsilon": 1e-8},
        "adagrad": {"type": "adagrad", "learning_rate": 0.5, "initial_accumulator_value": 0.1},
        "lamb": {"type": "lamb", "learning_rate": 0.5, "beta1": 0.9, "beta2": 0.999,
                 "epsilon": 1e-6, "weight_decay": 0.01},
        "lars": {"type": "lars", "learning_rate": 0.5, "momentum": 0.9, "weight_decay": 1e-4,
                 "eeta": 1e-3, "epsilon": 0.0, "use_nesterov": False, "name": "LARSOptimizer",
                 "chunk": 4096},
        "adamw": {"type": "adamw", "learning_rate": 0.5, "weight_decay_rate": 0.01,
                  "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-6},
    }
    classes = {"sgd": GradientDescentOptimizer, "momentum": MomentumOptimizer,
               "adam": AdamOptimizer, "adagrad": AdagradOptimizer, "lamb": LAMBOptimizer,
               "lars": LARSOptimizer, "adamw": AdamWeightDecayOptimizer}
    for name, cls in classes.items():
        assert cls(0.5).get_config() == want[name]
        cfg = cls(0.5, clip_norm=2.0).get_config()
        assert cfg == dict(want[name], clip_norm=2.0)
        json.dumps(cfg)
        kind = cfg.pop("type")
        clone = cls(**cfg)
        assert clone.clip_norm == 2.0 and clone.get_config()["type"] == kind


# ---------------------------------------------------------------------------- CLI

@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    from distributedtensorflow_amd.data import mnist
    d = tmp_path_factory.mktemp("mnist_clip")
    mnist.load_arrays(str(d), "train")
    return str(d)


def _cli(data_dir, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        env.pop(k, None)
    return subprocess.run([sys.executable, TRAIN, "--model", "mnist_mlp", "--device", "cpu",
                           *extra, "--train_steps", "3", "--data_dir", data_dir, "--log_dir", ""],
                          capture_output=True, text=True, env=env, timeout=300)


def _result(r):
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_cli_clip_norm_reports_the_gradient_norm(data_dir):
    res = _result(_cli(data_dir, "--optimizer", "adam", "--clip_norm", "0.5"))
    assert res["global_step"] == 3
    assert np.isfinite(res["grad_norm"]) and res["grad_norm"] > 0
    assert np.isfinite(res["final_loss"])


def test_cli_without_clip_norm_reports_no_gradient_norm(data_dir):
    assert "grad_norm" not in _result(_cli(data_dir, "--optimizer", "adam"))


def test_cli_adamw_trains(data_dir):
    res = _result(_cli(data_dir, "--optimizer", "adamw", "--learning_rate", "0.01",
                       "--clip_norm", "1.0"))
    assert res["global_step"] == 3 and np.isfinite(res["final_loss"])
    assert res["grad_norm"] > 0


def test_cli_adamw_needs_a_learning_rate_with_an_image_model(data_dir):
    r = _cli(data_dir, "--optimizer", "adamw")
    assert r.returncode != 0 and "--learning_rate" in r.stderr


def test_cli_between_graph_refuses_clip_norm(data_dir):
    r = _cli(data_dir, "--clip_norm", "1.0", "--job_name", "worker", "--ps_hosts",
             "127.0.0.1:1", "--worker_hosts", "127.0.0.1:2")
    assert r.returncode != 0 and "between-graph" in r.stderr


def test_cli_adamw_is_the_bert_recipe_on_a_tiny_bert():
    """The CLI's adamw optimizer (BERT-paper learning rate, 1% warm-up, linear decay) with
    --clip_norm 1.0, on the small BERT the distributed CPU tests train (bert_base itself is
    too large for a CPU test)."""
    from distributedtensorflow_amd import cli
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    from distributedtensorflow_amd.optimizers.optimizers import polynomial_decay
    args = cli.build_parser().parse_args(["--model", "bert_base", "--optimizer", "adamw",
                                          "--clip_norm", "1.0", "--train_steps", "300"])
    opt = cli._make_optimizer(args.optimizer, 1e-4, args.model, 128, args.max_steps,
                              args.clip_norm)
    assert isinstance(opt, AdamWeightDecayOptimizer) and opt.clip_norm == 1.0
    want = polynomial_decay(1e-4, 300, warmup_steps=3)
    for t in (0, 2, 3, 150, 300):
        assert opt.learning_rate(t) == pytest.approx(want(t))
    cfg = BertConfig(vocab_size=200, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                     intermediate_size=256, max_position_embeddings=32, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0)
    torch.manual_seed(3)
    with OneDeviceStrategy("cpu").scope():
        model = BertForPreTraining(cfg)
        opt.build(list(model.parameters()))
        decayed = {p._dtf_name: opt.decay_filter(p) for p in opt.space.order}
        assert any(decayed.values()) and not all(decayed.values())
        assert not any(d for n, d in decayed.items() if "LayerNorm" in n or "bias" in n)
        g = torch.Generator().manual_seed(5)
        B, S, P = 2, 16, 4
        losses = []
        for _ in range(3):
            ids = torch.randint(0, 200, (B, S), generator=g)
            pos = torch.randint(0, S, (B, P), generator=g)
            lab = torch.randint(0, 200, (B, P), generator=g)
            loss = model(ids, torch.zeros(B, S, dtype=torch.long), torch.ones(B, S), pos, lab,
                         torch.ones(B, P))
            opt.minimize(loss)
            losses.append(float(loss))
            assert float(opt.last_grad_norm.item()) > 0
    assert all(np.isfinite(losses))
