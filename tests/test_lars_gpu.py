"""The LARS kernels (csrc/kernels/optim.hip: norm pass + slab-reduced update pass) and the
label-smoothed cross-entropy kernel (loss.hip) on the GPU.

LARS runs through LARSOptimizer as training does, against the numpy fp64 oracle of test_lars.py,
over tensors of one element, exactly one chunk, a second row that is scalar tail only, four rows,
a tail of 3, more rows than the 256-thread block that re-adds the partial sums covers in one trip,
all-zero weights, all-zero gradients and a non-decayed bias.  No float atomics: a second run is
bit-identical."""
import copy
import functools

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.optimizers import LARSOptimizer
from distributedtensorflow_amd.optimizers.optimizers import polynomial_decay
from distributedtensorflow_amd.parallel import OneDeviceStrategy
from test_lars import Lars
from test_optim_kernels_gpu import ATOL, RTOL, _range_restricted

pytestmark = pytest.mark.gpu

dev = "cuda"
STEPS = 3
CHUNK = 4096
# the update block adds its tensor's partial rows with a stride of 256 threads: 258 rows give
# threads 0 and 1 a second trip
LARS_VARS = [("a/kernel", (1, 1)), ("b/kernel", (64, 64)), ("c/kernel", (4097, 1)),
             ("d/kernel", (3 * CHUNK + 1, 1)), ("e/kernel", (4099, 1)),
             ("big/kernel", (257 * CHUNK + 3, 1)), ("zero/kernel", (32, 3)),
             ("still/kernel", (32, 3)), ("x/bias", (100,))]
# eeta = 0.1, wd = 0.01: steps of ~5% of |w|, far above the tolerance, so a wrong norm shows
LR, MU, WD, EETA, GSCALE = 0.5, 0.9, 0.01, 0.1, 0.5


@functools.lru_cache(maxsize=None)
def _lars_data():
    """(p0, per-step gradients) on the CPU; shared between tests and never written."""
    g = torch.Generator().manual_seed(7)
    ps = [torch.zeros(s) if n.startswith("zero") else torch.randn(s, generator=g)
          for n, s in LARS_VARS]
    gs = [[torch.zeros(s) if n.startswith("still") else torch.randn(s, generator=g)
           for n, s in LARS_VARS] for _ in range(STEPS)]
    return ps, gs


def _lars_run(nesterov):
    """Three LARS steps on the GPU; returns the optimizer, its variables and, per step, the
    masters and the momentum slot on the CPU."""
    p0, gs = _lars_data()
    ps = []
    for (name, _), v in zip(LARS_VARS, p0):
        p = torch.nn.Parameter(v.clone().to(dev))
        p._dtf_name = name
        ps.append(p)
    opt = LARSOptimizer(LR, MU, weight_decay=WD, eeta=EETA, use_nesterov=nesterov, chunk=CHUNK)
    per_step = []
    with OneDeviceStrategy(dev).scope():
        sp = opt.build(ps)
        for t in range(STEPS):
            sp.zero_grad()
            for p, g in zip(ps, gs[t]):
                p.grad.copy_(g)
            fed = sp.grad.clone()
            opt.iterations += 1
            opt._apply(GSCALE)
            assert torch.equal(sp.grad, fed), "the gradient buffer was written"
            per_step.append(([p.detach().cpu().clone() for p in ps],
                             [sp.view_of(opt.slots[0].buf, p).cpu().clone() for p in ps]))
    return opt, ps, per_step


@functools.lru_cache(maxsize=None)
def _oracle(nesterov):
    """Per step: (masters, momentum slots) of the fp64 oracle; computed once per variant."""
    p0, gs = _lars_data()
    oracle = Lars(LR, MU, WD, EETA, 0.0, nesterov)
    cur = [v.double().numpy().copy() for v in p0]
    state = [oracle.init(c) for c in cur]
    out = []
    for t in range(STEPS):
        for i, (name, _) in enumerate(LARS_VARS):
            cur[i] = oracle.step(cur[i], gs[t][i].double().numpy() * GSCALE, state[i], t + 1,
                                 "bias" not in name)
        out.append(([c.copy() for c in cur], [s["a"].copy() for s in state]))
    return out


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_lars_kernels_match_the_oracle(nesterov):
    opt, ps, per_step = _lars_run(nesterov)
    want = _oracle(nesterov)
    for t in range(STEPS):
        for i, (name, _) in enumerate(LARS_VARS):
            for got, ref, what in zip(per_step[t], want[t], ("master", "momentum slot")):
                np.testing.assert_allclose(got[i].double().numpy(), ref[i], rtol=RTOL, atol=ATOL,
                                           err_msg=f"{what} of {name}, step {t + 1}")
    for p in ps:
        assert torch.equal(p._dtf_shadow, p.detach().bfloat16())
    assert not opt.nonfinite_flag()
    # the zero tensors took the plain step (trust ratio 1), they did not stay put or blow up
    names = [n for n, _ in LARS_VARS]
    assert (per_step[-1][0][names.index("zero/kernel")] != 0).all()
    assert (per_step[0][1][names.index("still/kernel")] != 0).all()

    # a non-finite gradient in the last (one-element) row of the four-row tensor
    opt.space.zero_grad()
    ps[names.index("d/kernel")].grad[-1, 0] = float("inf")
    opt.iterations += 1
    opt._apply(1.0)
    assert opt.nonfinite_flag()


def test_lars_nonfinite_flag_in_a_non_decayed_tensor():
    """The norm pass skips non-decayed tensors: the update pass must flag their gradients."""
    opt, ps, _ = _lars_run(False)
    assert not opt.nonfinite_flag()
    opt.space.zero_grad()
    ps[-1].grad[-1] = float("nan")
    opt.iterations += 1
    opt._apply(1.0)
    assert opt.nonfinite_flag()


def test_lars_is_bitwise_reproducible():
    """Slab reduction: the per-tensor norms are added in one fixed order, so a second run from
    the same state gives the same bits -- masters and slots, every step."""
    _, _, first = _lars_run(False)
    _, _, again = _lars_run(False)
    for (pa, sa), (pb, sb) in zip(first, again):
        for a, b in zip(pa + sa, pb + sb):
            assert torch.equal(a, b)


def test_lars_range_restricted_apply_gpu():
    """Nothing outside [lo, hi) changes (master, slot, shadow); the inside matches the CPU twin.
    The filtered chunk table starts at variable 1, so first_row must index that table."""
    _range_restricted(lambda: LARSOptimizer(0.1, weight_decay=0.01, eeta=0.1), 1, 3)


def test_lars_graph_replay_matches_eager():
    """The learning rate changes every step: a value baked into the captured launch shows."""
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.train import GlobalStep, GraphedTrainStep
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = MnistCNN()
    g = torch.Generator(device=dev).manual_seed(1)
    batches = [(torch.rand(128, 784, device=dev, generator=g).to(torch.bfloat16),
                torch.randint(0, 10, (128,), device=dev, generator=g)) for _ in range(5)]
    res = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        with OneDeviceStrategy("/gpu:0").scope():
            opt = LARSOptimizer(polynomial_decay(0.5, 8, power=2, warmup_steps=2))
            opt.build(list(model.parameters()))
        gstep = GlobalStep()

        def step(x, y):
            loss = ops.sparse_softmax_cross_entropy(model(x), y, label_smoothing=0.1)
            opt.minimize(loss, global_step=gstep)
            return loss

        losses = []
        if graphed:
            # two eager warm-up steps, then the capture; the four replays see the learning
            # rates of steps 3..6
            fn = GraphedTrainStep(step, opt, [batches[0][0].clone(), batches[0][1].clone()],
                                  global_step=gstep, warmup=2)
            for x, y in batches[1:]:
                losses.append(fn(x, y).clone())
        else:
            for _ in range(2):
                step(*batches[0])
            for x, y in batches[1:]:
                losses.append(step(x, y))
        torch.cuda.synchronize()
        res.append((torch.stack(losses), opt.space.master.clone(), opt.slots[0].buf.clone(),
                    int(gstep), opt.iterations))
    (la, pa, sa, ga, ia), (lb, pb, sb, gb, ib) = res
    assert torch.equal(la, lb), (la, lb)
    assert torch.equal(pa, pb) and torch.equal(sa, sb)
    assert ga == gb == 6 and ia == ib == 6
    lrs = [polynomial_decay(0.5, 8, power=2, warmup_steps=2)(t) for t in range(1, 7)]
    assert len(set(lrs)) == 6


# ---------------------------------------------------------------------------- label smoothing

XENT_SHAPES = [(1, 10), (128, 10), (256, 1000), (7, 30522)]


def _native():
    from distributedtensorflow_amd.ops import native
    return native


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _xent_case(B, V, eps):
    """(logits, labels, reference loss, reference gradient); computed once, never written."""
    g = torch.Generator().manual_seed(B * 31 + V)
    x = (3 * torch.randn(B, V, generator=g)).to(dev)
    lab = torch.randint(0, V, (B,), generator=g).to(dev)
    from distributedtensorflow_amd.ops import reference
    xr = x.clone().requires_grad_()
    ref = reference.sparse_softmax_cross_entropy(xr, lab, eps)
    ref.backward()
    return x, lab, ref.detach(), xr.grad


@pytest.mark.parametrize("ldt", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("B,V", XENT_SHAPES, ids=[f"{b}x{v}" for b, v in XENT_SHAPES])
def test_label_smoothing_kernel(B, V, ldt):
    x, lab, ref, ref_grad = _xent_case(B, V, 0.1)
    xn = x.clone().requires_grad_()
    out = _native().sparse_softmax_cross_entropy(xn, lab.to(ldt), label_smoothing=0.1)
    out.backward()
    assert abs(out.item() - ref.item()) < 1e-4 * max(1.0, abs(ref.item()))
    assert _rel(xn.grad, ref_grad) < 1e-5
    # not the unsmoothed loss
    plain = _xent_case(B, V, 0.0)[2]
    assert abs(out.item() - plain.item()) > 1e-3


@pytest.mark.parametrize("B,V", [(128, 10), (7, 30522)])
def test_label_smoothing_zero_is_the_plain_kernel(B, V):
    x, lab, _, _ = _xent_case(B, V, 0.1)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    la = _native().sparse_softmax_cross_entropy(xa, lab)
    lb = _native().sparse_softmax_cross_entropy(xb, lab, label_smoothing=0.0)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad)


def test_label_smoothing_backward_scales_with_the_upstream_gradient():
    x, lab, _, ref_grad = _xent_case(128, 10, 0.1)
    xn = x.clone().requires_grad_()
    (0.5 * ops.sparse_softmax_cross_entropy(xn, lab, label_smoothing=0.1)).backward()
    assert _rel(xn.grad, 0.5 * ref_grad) < 1e-5
