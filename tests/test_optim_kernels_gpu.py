"""The fused optimizer kernels (csrc/kernels/optim.hip) past their grid cap.

Their grid is capped at 2048 blocks of 256 threads and each block then strides over the flat
buffer; the optimizer tests in test_optimizers.py stay inside one partial block.  Here the
kernels are called directly, as optimizers/optimizers.py calls them, at sizes where a block makes
a second and a third (partial) trip, where the float4 body of the momentum kernel meets its
scalar tail, and where a LAMB tensor spans several 4096-element chunks.  The reference is the
numpy fp64 transcription of the TF update math in test_optimizers.py.
"""
import functools
import math

import numpy as np
import pytest
import torch

from distributedtensorflow_amd.optimizers import AdamOptimizer, GradientDescentOptimizer, LAMBOptimizer
from distributedtensorflow_amd.optimizers.optimizers import clip_by_global_norm_
from distributedtensorflow_amd.parallel import OneDeviceStrategy
from test_optimizers import Adagrad, Adam, Lamb, Momentum, _grads, _params

pytestmark = pytest.mark.gpu

dev = "cuda"
RTOL, ATOL = 2e-5, 2e-6        # the tolerance of test_optimizer_kernels_gpu for these kernels
STEPS = 3
SLACK, SENT = 64, -7.25        # floats past n that no kernel may touch, and what they hold
TRIP = 2048 * 256              # elements one full grid covers per trip (4x that for float4)
MID = TRIP + 5                 # second trip of 5 elements (adam, adagrad, cast, sumsq)
BIG = TRIP * 4 * 2 + 4 * 256 + 3   # momentum: two full float4 trips, one block of a third, tail 3
# n % 4 covers 0..3 (1026 -> 2, 257 / 1025 -> 1); 1024: no scalar tail at all
SIZES = [1, 3, 255, 257, 1023, 1024, 1025, 1026, MID, BIG]


def _K():
    from distributedtensorflow_amd.ops import native
    return native.kernels()


def _st():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _data(n):
    """(p0, [g1, g2, g3]) fp32 on the CPU; shared between tests and never written."""
    g = torch.Generator().manual_seed(1000 + n % 9973)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(STEPS)]


def _buf(vals, dtype=torch.float32):
    """vals on the GPU followed by SLACK sentinel elements; torch allocations are 512-B aligned."""
    n = vals.numel()
    t = torch.full((n + SLACK,), SENT, device=dev, dtype=dtype)
    t[:n].copy_(vals)
    assert t.data_ptr() % 16 == 0
    return t


def _close(buf, n, ref, what):
    np.testing.assert_allclose(buf[:n].cpu().double().numpy(), ref, rtol=RTOL, atol=ATOL,
                               err_msg=what)


def _untouched(n, *bufs):
    for b in bufs:
        if b is not None:
            assert torch.equal(b[n:], torch.full_like(b[n:], SENT)), "wrote past n"


def _shadow_ok(shadow, p, n):
    if shadow is not None:
        assert torch.equal(shadow[:n], p[:n].bfloat16())


def _ptr(t):
    return 0 if t is None else t.data_ptr()


# (momentum, nesterov, wd, gscale, shadow)
SGD_VARIANTS = {
    "sgd": (0.0, False, 0.0, 1.0, False),
    "sgd_wd_gscale_shadow": (0.0, False, 1e-4, 0.5, True),
    "momentum": (0.9, False, 1e-4, 0.5, True),
    "nesterov": (0.9, True, 1e-4, 0.5, True),
    "nesterov_plain": (0.9, True, 0.0, 1.0, False),
}
# at BIG the fp64 reference is most of the time: momentum and Nesterov only
SGD_CASES = [(n, v) for n in SIZES for v in SGD_VARIANTS
             if n != BIG or v in ("momentum", "nesterov")]


@pytest.mark.parametrize("n,variant", SGD_CASES, ids=[f"{n}-{v}" for n, v in SGD_CASES])
def test_sgd_momentum_kernel(n, variant):
    mu, nesterov, wd, gscale, with_shadow = SGD_VARIANTS[variant]
    lr = 0.1
    p0, gs = _data(n)
    p, a, g = _buf(p0), _buf(torch.zeros(n)), _buf(gs[0])
    shadow = _buf(p0, torch.bfloat16) if with_shadow else None
    lr_dev = torch.tensor([lr, 0, 0, 0], device=dev, dtype=torch.float32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    oracle = Momentum(lr, mu, nesterov, wd)
    ref = p0.double().numpy().copy()
    state = oracle.init(ref)
    for t in range(STEPS):
        g[:n].copy_(gs[t])
        _K().sgd_momentum(p.data_ptr(), g.data_ptr(), a.data_ptr(), _ptr(shadow), n,
                          lr_dev.data_ptr(), mu, wd, gscale, int(nesterov), flag.data_ptr(), _st())
        ref = oracle.step(ref, gs[t].double().numpy() * gscale, state, t + 1, True)
        _close(p, n, ref, f"master, step {t + 1}")
        _close(a, n, state["a"], f"momentum slot, step {t + 1}")
        _shadow_ok(shadow, p, n)
    _untouched(n, p, a, g, shadow)
    assert flag.item() == 0


class AdamDecoupledDecay(Adam):
    """Adam plus the decoupled weight decay of the kernel and of AdamOptimizer._apply_reference:
    p -= lr_t * wd * p, with p the weight before this step's update."""

    def __init__(self, lr, wd, **kw):
        super().__init__(lr, **kw)
        self.wd = wd

    def step(self, p, g, s, t, dec):
        lr_t = self.lr * math.sqrt(1 - self.b2 ** t) / (1 - self.b1 ** t)
        return super().step(p, g, s, t, dec) - (lr_t * self.wd * p if dec else 0.0)


# (lr, b1, b2, eps, wd, gscale, shadow)
ADAM_VARIANTS = {
    "adam": (5e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, False),
    "adam_gscale_shadow": (0.01, 0.8, 0.99, 1e-6, 0.0, 0.5, True),
    "adam_wd": (0.01, 0.9, 0.999, 1e-8, 0.01, 0.5, True),
}
ADAM_SIZES = [n for n in SIZES if n != BIG]     # MID already gives these kernels a second trip


@pytest.mark.parametrize("variant", list(ADAM_VARIANTS))
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_kernel(n, variant):
    lr, b1, b2, eps, wd, gscale, with_shadow = ADAM_VARIANTS[variant]
    p0, gs = _data(n)
    p, m, v, g = _buf(p0), _buf(torch.zeros(n)), _buf(torch.zeros(n)), _buf(gs[0])
    shadow = _buf(p0, torch.bfloat16) if with_shadow else None
    lr_dev = torch.zeros(4, device=dev, dtype=torch.float32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    oracle = AdamDecoupledDecay(lr, wd, b1=b1, b2=b2, eps=eps)
    ref = p0.double().numpy().copy()
    state = oracle.init(ref)
    for t in range(STEPS):
        g[:n].copy_(gs[t])
        lr_dev[0] = lr * math.sqrt(1 - b2 ** (t + 1)) / (1 - b1 ** (t + 1))
        _K().adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(shadow), n,
                  lr_dev.data_ptr(), b1, b2, eps, wd, gscale, flag.data_ptr(), _st())
        ref = oracle.step(ref, gs[t].double().numpy() * gscale, state, t + 1, True)
        _close(p, n, ref, f"master, step {t + 1}")
        _close(m, n, state["m"], f"m, step {t + 1}")
        _close(v, n, state["v"], f"v, step {t + 1}")
        _shadow_ok(shadow, p, n)
    _untouched(n, p, m, v, g, shadow)
    assert flag.item() == 0


@pytest.mark.parametrize("gscale,with_shadow", [(1.0, False), (0.5, True)])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adagrad_kernel(n, gscale, with_shadow):
    lr = 0.01
    p0, gs = _data(n)
    oracle = Adagrad(lr)
    ref = p0.double().numpy().copy()
    state = oracle.init(ref)
    p, acc, g = _buf(p0), _buf(torch.full((n,), oracle.acc0)), _buf(gs[0])
    shadow = _buf(p0, torch.bfloat16) if with_shadow else None
    lr_dev = torch.tensor([lr, 0, 0, 0], device=dev, dtype=torch.float32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    for t in range(STEPS):
        g[:n].copy_(gs[t])
        _K().adagrad(p.data_ptr(), g.data_ptr(), acc.data_ptr(), _ptr(shadow), n,
                     lr_dev.data_ptr(), gscale, flag.data_ptr(), _st())
        ref = oracle.step(ref, gs[t].double().numpy() * gscale, state, t + 1, True)
        _close(p, n, ref, f"master, step {t + 1}")
        _close(acc, n, state["a"], f"accumulator, step {t + 1}")
        _shadow_ok(shadow, p, n)
    _untouched(n, p, acc, g, shadow)
    assert flag.item() == 0


def _launch(kernel, n, p, g, s1, s2, lr_dev, flag):
    if kernel == "sgd_momentum":
        _K().sgd_momentum(p.data_ptr(), g.data_ptr(), s1.data_ptr(), 0, n, lr_dev.data_ptr(), 0.9,
                          0.0, 1.0, 0, flag.data_ptr(), _st())
    elif kernel == "adam":
        _K().adam(p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), 0, n,
                  lr_dev.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, flag.data_ptr(), _st())
    else:
        _K().adagrad(p.data_ptr(), g.data_ptr(), s1.data_ptr(), 0, n, lr_dev.data_ptr(), 1.0,
                     flag.data_ptr(), _st())


# (kernel, n, index of the bad gradient, its value)
FLAG_CASES = [
    ("sgd_momentum", 3, 2, "inf"),                       # tail only
    ("sgd_momentum", BIG, BIG - 1, "inf"),               # last element of the scalar tail
    ("sgd_momentum", BIG, TRIP * 4, "nan"),              # first element of the last full trip
    ("sgd_momentum", BIG, TRIP * 4 * 2 + 5, "-inf"),     # in the partial third trip
    ("adam", MID, MID - 1, "inf"),                       # last element, second trip
    ("adam", 2 * TRIP + 5, TRIP, "nan"),                 # first element of the last full trip
    ("adagrad", MID, MID - 1, "inf"),
    ("adagrad", 2 * TRIP + 5, TRIP, "nan"),
]


@pytest.mark.parametrize("kernel,n,idx,bad", FLAG_CASES,
                         ids=[f"{k}-{n}-{i}-{b}" for k, n, i, b in FLAG_CASES])
def test_nonfinite_flag_in_late_trips(kernel, n, idx, bad):
    """All-finite gradients leave the flag at 0; a single non-finite gradient that only a late
    trip (or the scalar tail) reads sets it."""
    p, g = _buf(torch.ones(n)), _buf(_data(n)[1][0])
    s1, s2 = _buf(torch.full((n,), 0.1)), _buf(torch.zeros(n))
    lr_dev = torch.tensor([0.01, 0, 0, 0], device=dev, dtype=torch.float32)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    _launch(kernel, n, p, g, s1, s2, lr_dev, flag)
    assert flag.item() == 0
    g[idx] = float(bad)
    _launch(kernel, n, p, g, s1, s2, lr_dev, flag)
    assert flag.item() == 1
    _untouched(n, p, g, s1, s2)


@pytest.mark.parametrize("n", SIZES)
def test_sumsq_kernel(n):
    """All terms are positive: <= 8 adds per thread, a 6-level wave sum, 4 waves, <= 2048 atomics --
    a few tens of fp32 ulps."""
    x = _buf(_data(n)[0])
    out = torch.zeros(1, device=dev, dtype=torch.float32)
    _K().sumsq(x.data_ptr(), n, out.data_ptr(), _st())
    want = float((_data(n)[0].double() ** 2).sum())
    np.testing.assert_allclose(out.item(), want, rtol=1e-5, atol=0)
    _K().sumsq(x.data_ptr(), n, out.data_ptr(), _st())       # accumulates into `out`
    np.testing.assert_allclose(out.item(), 2 * want, rtol=1e-5, atol=0)


@pytest.mark.parametrize("n", SIZES)
def test_cast_f32_bf16_kernel(n):
    """Round to nearest even, as torch: random values over 12 decades plus exact ties (both
    neighbours), signed zeros and infinities at the front and at the very end."""
    v = _data(n)[0].clone()
    gen = torch.Generator().manual_seed(n)
    v *= 10 ** (torch.rand(n, generator=gen) * 12 - 6)
    special = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), -(1 + 3 * 2 ** -8),
                            1 + 2 ** -8 + 2 ** -20, 1 + 2 ** -8 - 2 ** -20, 0.0, -0.0,
                            float("inf"), float("-inf"), 3.3895314e38, 65504.0])
    k = min(n, special.numel())
    v[:k] = special[:k]
    v[n - 1] = special[(n - 1) % special.numel()]
    x = _buf(v)
    y = torch.full((n + SLACK,), SENT, device=dev, dtype=torch.bfloat16)
    _K().cast_f32_bf16(x.data_ptr(), y.data_ptr(), n, _st())
    assert torch.equal(y[:n].view(torch.int16), x[:n].bfloat16().view(torch.int16))
    _untouched(n, y)


# ---------------------------------------------------------------------------- LAMB (optimizer)

# one block per 4096-element chunk: 4097 -> two blocks, 3 * 4096 + 1 -> four blocks that all
# atomicAdd into the same norms[seg]; 2-D shapes are decayed, 1-D ones and biases are not
LAMB_VARS = [("a/kernel", (1, 1)), ("b/kernel", (64, 64)), ("c/kernel", (4097, 1)),
             ("d/kernel", (3 * 4096 + 1, 1)), ("zero/kernel", (32, 3)), ("x/bias", (100,))]
LAMB_LR, LAMB_WD, LAMB_GSCALE = 1e-3, 0.01, 0.5


@functools.lru_cache(maxsize=None)
def _lamb_data():
    g = torch.Generator().manual_seed(7)
    ps = [torch.zeros(s) if n.startswith("zero") else torch.randn(s, generator=g)
          for n, s in LAMB_VARS]
    gs = [[torch.randn(s, generator=g) for _, s in LAMB_VARS] for _ in range(STEPS)]
    return ps, gs


def _lamb_run():
    """Three LAMB steps on the GPU; returns the optimizer, its variables and, per step, the
    masters on the CPU."""
    p0, gs = _lamb_data()
    ps = []
    for (name, _), v in zip(LAMB_VARS, p0):
        p = torch.nn.Parameter(v.clone().to(dev))
        p._dtf_name = name
        ps.append(p)
    opt = LAMBOptimizer(LAMB_LR, weight_decay=LAMB_WD)
    per_step = []
    with OneDeviceStrategy(dev).scope():
        opt.build(ps)
        for t in range(STEPS):
            opt.space.zero_grad()
            for p, g in zip(ps, gs[t]):
                p.grad.copy_(g)
            opt.iterations += 1
            opt._apply(LAMB_GSCALE)
            per_step.append([p.detach().cpu().double().numpy().copy() for p in ps])
    return opt, ps, per_step


def test_lamb_multi_chunk_tensors():
    """LAMBOptimizer on the GPU against the fp64 oracle with tensors of one, two and four chunks,
    an all-zero tensor (trust ratio 1) and a non-decayed one; m, v and the bf16 shadow too.  A
    second run from the same state agrees to rtol 1e-6 of the values, or of the step they took
    (the float atomics into norms[seg] may arrive in another order: a few ulps of the trust
    ratio, which scales the whole step)."""
    p0, gs = _lamb_data()
    opt, ps, per_step = _lamb_run()
    oracle = Lamb(LAMB_LR, LAMB_WD)
    cur = [v.double().numpy().copy() for v in p0]
    state = [oracle.init(c) for c in cur]
    for t in range(STEPS):
        for i, (name, _) in enumerate(LAMB_VARS):
            cur[i] = oracle.step(cur[i], gs[t][i].double().numpy() * LAMB_GSCALE, state[i], t + 1,
                                 "bias" not in name)
            np.testing.assert_allclose(per_step[t][i], cur[i], rtol=RTOL, atol=ATOL,
                                       err_msg=f"{name}, step {t + 1}")
    sp = opt.space
    for i, p in enumerate(ps):
        for slot, key in zip(opt.slots, ("m", "v")):
            np.testing.assert_allclose(sp.view_of(slot.buf, p).cpu().double().numpy(),
                                       state[i][key], rtol=RTOL, atol=ATOL)
        assert torch.equal(p._dtf_shadow, p.detach().bfloat16())
    assert not opt.nonfinite_flag()

    _, _, again = _lamb_run()
    for i in range(len(ps)):
        step = np.abs(per_step[-1][i] - per_step[-2][i]).max()
        np.testing.assert_allclose(again[-1][i], per_step[-1][i], rtol=1e-6, atol=1e-6 * step)

    # a non-finite gradient in the last chunk of the four-chunk tensor
    sp.zero_grad()
    ps[3].grad[-1, 0] = float("inf")
    opt.iterations += 1
    opt._apply(1.0)
    assert opt.nonfinite_flag()


# ---------------------------------------------------------------------------- GPU twins

def _twin(factory, steps_before=1):
    """The same optimizer on the GPU and on the CPU (the reference path), same variables, one
    warm-up step so the slots are not all zero, then the same random gradients."""
    out = []
    for device in (dev, "cpu"):
        ps = _params(device)
        opt = factory()
        with OneDeviceStrategy(device).scope():
            sp = opt.build(ps)
        for t in range(steps_before + 1):
            sp.zero_grad()
            for p, g in zip(ps, _grads(ps, t)):
                p.grad.copy_(g.to(device))
            if t < steps_before:
                opt.iterations += 1
                opt._apply(1.0)
        out.append((opt, sp))
    return out


def _range_restricted(factory, lo_i, hi_i):
    (og, sg), (oc, sc) = _twin(factory)
    assert sg.offsets == sc.offsets and sg.numel == sc.numel
    lo, hi = sg.offsets[lo_i], sg.offsets[hi_i]
    before = [t.clone() for t in (sg.master, sg.shadow, *(s.buf for s in og.slots))]
    og.iterations += 1
    oc.iterations += 1
    og._apply(0.5, (lo, hi))
    oc._apply(0.5, (lo, hi))
    after = [sg.master, sg.shadow, *(s.buf for s in og.slots)]
    for b, a in zip(before, after):
        assert torch.equal(b[:lo], a[:lo]) and torch.equal(b[hi:], a[hi:])
    assert (before[0][lo:hi] != after[0][lo:hi]).any()
    for got, want in zip([sg.master, *(s.buf for s in og.slots)],
                         [sc.master, *(s.buf for s in oc.slots)]):
        np.testing.assert_allclose(got[lo:hi].cpu().double().numpy(),
                                   want[lo:hi].double().numpy(), rtol=RTOL, atol=ATOL)
    assert torch.equal(sg.shadow[lo:hi], sg.master[lo:hi].bfloat16())
    assert not og.nonfinite_flag()


def test_range_restricted_apply_gpu():
    """test_range_restricted_apply on the native branch: nothing outside [lo, hi) changes (master,
    slots, shadow) and the inside matches the CPU reference path from the same state."""
    _range_restricted(lambda: AdamOptimizer(0.1, weight_decay=0.01), 1, 2)


def test_lamb_range_restricted_apply_gpu():
    _range_restricted(lambda: LAMBOptimizer(0.1), 1, 3)


def test_clip_by_global_norm_gpu():
    (_, sg), (_, sc) = _twin(lambda: GradientDescentOptimizer(0.1), steps_before=0)
    for sp in (sg, sc):
        sp.grad.mul_(3.0)
    assert torch.equal(sg.grad.cpu(), sc.grad)
    n0 = sc.grad.double().norm().item()
    assert n0 > 1.0
    norm_g, norm_c = clip_by_global_norm_(sg, 1.0), clip_by_global_norm_(sc, 1.0)
    assert abs(norm_g.item() - n0) < 1e-4
    assert abs(norm_g.item() - norm_c.item()) < 1e-4
    assert abs(sg.grad.double().norm().item() - 1.0) < 1e-4
    np.testing.assert_allclose(sg.grad.cpu().numpy(), sc.grad.numpy(), rtol=RTOL, atol=ATOL)
    # below the threshold nothing is scaled
    kept = sg.grad.clone()
    clip_by_global_norm_(sg, 10.0)
    assert torch.equal(sg.grad, kept)
