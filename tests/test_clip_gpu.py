"""The deterministic global-norm pass (csrc/kernels/optim.hip: grad_norm partial + finish kernels)
and the clipped fused updates on the GPU.

The norm pass is called directly at sizes of one element, a scalar tail only, one element short
of a chunk, exactly one chunk, a second chunk of one element, and six chunks with a tail of 3
that two blocks walk in three trips; the optimizers then run as training runs them."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.optimizers import (AdagradOptimizer, AdamOptimizer,
                                                  AdamWeightDecayOptimizer,
                                                  GradientDescentOptimizer, LAMBOptimizer,
                                                  LARSOptimizer, MomentumOptimizer)
from distributedtensorflow_amd.parallel import OneDeviceStrategy
from test_clip import OPTIMIZERS, STEPS, run_steps
from test_optim_kernels_gpu import ATOL, RTOL, _twin

pytestmark = pytest.mark.gpu

dev = "cuda"
SENT = -7.25
# the longest chain of fp32 additions a square passes through inside a block of the partial
# kernel, as its comment states it: 8 + 2 + 1 + 6 + 3
D = 20


def _K():
    from distributedtensorflow_amd.ops import native
    return native.kernels()


def _st():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def CH():
    return _K().grad_norm_chunk()


@functools.lru_cache(maxsize=None)
def _values(n):
    """Mixed-sign normals on the CPU; shared between tests and never written."""
    return torch.randn(n, generator=torch.Generator().manual_seed(4000 + n % 9973))


def _norm_pass(x, n, max_blocks=0, extra=None, gscale=1.0, clip=1.0):
    """grad_norm over x[:n] (x: a device tensor or view) -> (S, norm, gmul) as the device wrote
    them; the slab past the last chunk must stay untouched."""
    nch = -(-n // CH())
    partial = torch.full((nch + 8,), SENT, device=dev, dtype=torch.float64)
    rec = torch.zeros(2, device=dev, dtype=torch.float64)
    _K().grad_norm(x.data_ptr(), n, partial.data_ptr(), max_blocks,
                   0 if extra is None else extra.data_ptr(),
                   0 if extra is None else extra.numel(), gscale, clip, rec.data_ptr(), _st())
    torch.cuda.synchronize()
    assert torch.equal(partial[nch:], torch.full_like(partial[nch:], SENT)), "wrote past nchunks"
    assert not (partial[:nch] == SENT).any()
    f = rec.view(torch.float32).cpu().numpy()
    return float(rec[0].item()), f[2], f[3]


def _sizes():
    c = CH()
    return [1, 3, c - 1, c, c + 1, 5 * c + 7]


@pytest.mark.parametrize("which", range(6))
def test_norm_pass_against_fp64(which):
    n = _sizes()[which]
    v = _values(n)
    x = v.to(dev)
    S64 = float((v.double() ** 2).sum())
    S, norm, _ = _norm_pass(x, n)
    # every term is non-negative: d + 1 roundings of sums on the way to the fp64 partial, and
    # the factor 2 for the rounding of the products
    assert abs(S - S64) <= 2 * (D + 1) * 2.0 ** -24 * S64, (S, S64)
    assert abs(float(norm) - math.sqrt(S)) <= float(np.spacing(norm))
    # the grid decides who adds a chunk, never how; and a second run gives the same bits
    for mb in (1, 2, 0):
        assert _norm_pass(x, n, max_blocks=mb)[0] == S
    assert _norm_pass(x, n)[0] == S


def test_norm_pass_three_trips():
    """Six chunks, two blocks: each makes three trips."""
    n = 5 * CH() + 7
    v = _values(n)
    S64 = float((v.double() ** 2).sum())
    S, _, _ = _norm_pass(v.to(dev), n, max_blocks=2)
    assert abs(S - S64) <= 2 * (D + 1) * 2.0 ** -24 * S64


def test_norm_pass_at_a_shard_offset():
    """A pointer 8 elements into a buffer (a shard's range start) gives the S of a copy of that
    slice, with 16-byte loads (offset 8) and without (offset 1)."""
    n = 5 * CH() + 7
    x = _values(n + 8).to(dev)
    for off in (8, 1):
        m = n + 8 - off - 5
        S_view, _, _ = _norm_pass(x[off:], m)
        S_copy, _, _ = _norm_pass(x[off:off + m].clone(), m)
        assert S_view == S_copy


def _host_gmul(S, gscale, clip):
    gs, c = float(np.float32(gscale)), float(np.float32(clip))
    return np.float32(gs * c / max(gs * math.sqrt(S), c))


def test_gmul():
    n = 5 * CH() + 7
    x = _values(n).to(dev)
    # clipped: gscale * sqrt(S) ~ 0.5 * sqrt(n) = 100
    for gscale, clip in ((0.5, 1.0), (1.0 / 3.0, 0.37), (1.0, 17.0)):
        S, norm, gmul = _norm_pass(x, n, gscale=gscale, clip=clip)
        assert norm > clip
        want = _host_gmul(S, gscale, clip)
        assert abs(float(gmul) - float(want)) <= float(np.spacing(want)), (gmul, want)
        assert abs(float(norm) - float(np.float32(gscale)) * math.sqrt(S)) <= \
            float(np.spacing(norm))
    # not clipped: exactly gscale, whatever the clip
    for gscale, clip in ((0.5, 1e6), (1.0 / 3.0, 12345.678), (1.0, 1e30)):
        _, norm, gmul = _norm_pass(x, n, gscale=gscale, clip=clip)
        assert norm < clip and gmul == np.float32(gscale)
    # S == 0
    S, norm, gmul = _norm_pass(torch.zeros(n, device=dev), n, gscale=1.0 / 3.0, clip=1.0)
    assert S == 0.0 and norm == 0.0 and gmul == np.float32(1.0 / 3.0)
    # a NaN (or an infinity) anywhere: a NaN multiplier
    for bad, at in ((float("nan"), n - 1), (float("inf"), CH() + 5)):
        y = x.clone()
        y[at] = bad
        _, _, gmul = _norm_pass(y, n, gscale=0.5, clip=1.0)
        assert math.isnan(gmul)


def test_extra_sums_are_added_in_order():
    """The other ranks' fp64 sums: S = (S_local + e0) + e1, and the multiplier follows."""
    n = CH() + 1
    x = _values(n).to(dev)
    S0, _, _ = _norm_pass(x, n)
    e = [1e-3 * S0 + 0.123456789, 3.0 * S0]
    extra = torch.tensor(e, device=dev, dtype=torch.float64)
    S, _, gmul = _norm_pass(x, n, extra=extra, gscale=0.5, clip=1.0)
    assert S == (S0 + e[0]) + e[1]
    want = _host_gmul(S, 0.5, 1.0)
    assert abs(float(gmul) - float(want)) <= float(np.spacing(want))


# ---------------------------------------------------------------------------- update wiring

# a/kernel: two full LAMB / LARS chunks and a third of 3 elements; 8195 % 4 == 3
WIRE_VARS = [("a/kernel", (8195, 1)), ("b/kernel", (64, 3)), ("c/bias", (100,)),
             ("LayerNorm/gamma", (37,))]
WIRE = {
    "sgd": lambda **kw: GradientDescentOptimizer(0.1, weight_decay=1e-2, **kw),
    "momentum": lambda **kw: MomentumOptimizer(0.1, 0.9, weight_decay=1e-2, **kw),
    "nesterov": lambda **kw: MomentumOptimizer(0.05, 0.9, use_nesterov=True, **kw),
    "adam": lambda **kw: AdamOptimizer(0.01, weight_decay=0.01, **kw),
    "adagrad": lambda **kw: AdagradOptimizer(0.01, **kw),
    "lamb": lambda **kw: LAMBOptimizer(1e-3, weight_decay=0.01, **kw),
    "lars": lambda **kw: LARSOptimizer(0.5, eeta=0.1, weight_decay=0.01, **kw),
    "adamw": lambda **kw: AdamWeightDecayOptimizer(0.01, **kw),
}
ELEMENTWISE = ("sgd", "momentum", "nesterov", "adam", "adagrad", "adamw")


@functools.lru_cache(maxsize=None)
def _wire_data():
    g = torch.Generator().manual_seed(11)
    return ([torch.randn(s, generator=g) for _, s in WIRE_VARS],
            [[torch.randn(s, generator=g) for _, s in WIRE_VARS] for _ in range(2)])


def _wire_build(opt):
    p0, _ = _wire_data()
    ps = []
    for (name, _), v in zip(WIRE_VARS, p0):
        p = torch.nn.Parameter(v.clone().to(dev))
        p._dtf_name = name
        ps.append(p)
    with OneDeviceStrategy(dev).scope():
        opt.build(ps)
    return ps


def _feed(opt, ps, t):
    opt.space.zero_grad()
    for p, g in zip(ps, _wire_data()[1][t]):
        p.grad.copy_(g)
    opt.iterations += 1


def _state(opt):
    sp = opt.space
    return [sp.master, sp.shadow, *(s.buf for s in opt.slots)]


def _tail_range(opt, ps):
    """The 8195 elements of a/kernel: a range whose length has a scalar tail of 3."""
    s = opt.space.offsets[opt.space.index[id(ps[0])]]
    return (s, s + 8195)


WIRE_CASES = [(n, False) for n in WIRE] + [(n, True) for n in ELEMENTWISE]


@pytest.mark.parametrize("name,tail", WIRE_CASES,
                         ids=[f"{n}-{'tail' if t else 'whole'}" for n, t in WIRE_CASES])
def test_clipped_step_is_the_unclipped_step_at_the_devices_multiplier(name, tail):
    """Master, slots and bf16 shadow, bit for bit, over two steps: clip_norm changes nothing but
    the factor, and the factor is the one the device holds."""
    a, b = WIRE[name](clip_norm=1.0), WIRE[name]()
    pa, pb = _wire_build(a), _wire_build(b)
    rng = _tail_range(a, pa) if tail else None
    assert a.space.shadow is not None
    for t in range(2):
        _feed(a, pa, t)
        _feed(b, pb, t)
        a._apply(0.5, rng)
        gmul = float(a._gmul.item())
        assert 0 < gmul < 0.5 and float(a.last_grad_norm.item()) > 1.0      # it clipped
        b._apply(gmul, rng)
        for x, y in zip(_state(a), _state(b)):
            assert torch.equal(x, y), (name, t)
    assert not a.nonfinite_flag() and not b.nonfinite_flag()


@pytest.mark.parametrize("name", list(WIRE))
def test_a_clip_that_never_clips_is_bit_identical_gpu(name):
    a, b = WIRE[name](clip_norm=1e30), WIRE[name]()
    pa, pb = _wire_build(a), _wire_build(b)
    for t in range(2):
        _feed(a, pa, t)
        _feed(b, pb, t)
        a._apply(0.5)
        b._apply(0.5)
        for x, y in zip(_state(a), _state(b)):
            assert torch.equal(x, y), (name, t)
    assert float(a._gmul.item()) == 0.5


def test_nonfinite_gradient_still_raises_the_flag():
    a = WIRE["momentum"](clip_norm=1.0)
    pa = _wire_build(a)
    _feed(a, pa, 0)
    pa[0].grad[-1, 0] = float("inf")
    a._apply(0.5)
    assert a.nonfinite_flag() and math.isnan(float(a._gmul.item()))


# ---------------------------------------------------------------------------- CPU against GPU

@pytest.mark.parametrize("name", list(OPTIMIZERS))
def test_clipped_steps_cpu_against_gpu(name):
    factory = OPTIMIZERS[name][0]
    _, _, got = run_steps(factory(clip_norm=1.0), dev)
    _, _, want = run_steps(factory(clip_norm=1.0), "cpu")
    for t in range(STEPS):
        assert want[t][1] > 1.0
        assert got[t][1] == pytest.approx(want[t][1], rel=1e-6, abs=0.0)
        for a, b in zip(got[t][0], want[t][0]):
            np.testing.assert_allclose(a.double().numpy(), b.double().numpy(), rtol=RTOL,
                                       atol=ATOL, err_msg=f"{name}, step {t + 1}")


# ---------------------------------------------------------------------------- range + extra

@pytest.mark.parametrize("name,lo_i,hi_i", [("adam", 1, 2), ("lamb", 1, 3)])
def test_range_restricted_clipped_apply(name, lo_i, hi_i):
    """A parameter-server owner's apply: the norm is that of its range plus the other owners'
    sums; nothing outside the range moves; the inside matches the CPU twin."""
    factory = {"adam": lambda: AdamOptimizer(0.1, weight_decay=0.01, clip_norm=1.0),
               "lamb": lambda: LAMBOptimizer(0.1, clip_norm=1.0)}[name]
    (og, sg), (oc, sc) = _twin(factory)
    lo, hi = sg.offsets[lo_i], sg.offsets[hi_i]
    others = [3.0, 5.0]
    before = [t.clone() for t in _state(og)]
    for o, sp in ((og, sg), (oc, sc)):
        o.iterations += 1
        o._apply(0.5, (lo, hi), torch.tensor(others, device=sp.device, dtype=torch.float64))
    for b, a in zip(before, _state(og)):
        assert torch.equal(b[:lo], a[:lo]) and torch.equal(b[hi:], a[hi:])
    assert (before[0][lo:hi] != sg.master[lo:hi]).any()
    want_norm = 0.5 * math.sqrt(float((sc.grad[lo:hi].double() ** 2).sum()) + sum(others))
    assert want_norm > 1.0
    assert float(og.last_grad_norm.item()) == pytest.approx(want_norm, rel=1e-6)
    assert float(oc.last_grad_norm.item()) == pytest.approx(want_norm, rel=1e-6)
    for got, want in zip([sg.master, *(s.buf for s in og.slots)],
                         [sc.master, *(s.buf for s in oc.slots)]):
        np.testing.assert_allclose(got[lo:hi].cpu().double().numpy(),
                                   want[lo:hi].double().numpy(), rtol=RTOL, atol=ATOL)
    assert torch.equal(sg.shadow[lo:hi], sg.master[lo:hi].bfloat16())


# ---------------------------------------------------------------------------- graph capture

def test_clipped_step_graph_replay_matches_eager():
    """Nothing in the clipped step touches the host: it captures as it is, and the norm is
    formed anew in every replay."""
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.train import GlobalStep, GraphedTrainStep
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = MnistCNN()
    g = torch.Generator(device=dev).manual_seed(1)
    batches = [(torch.rand(128, 784, device=dev, generator=g).to(torch.bfloat16),
                torch.randint(0, 10, (128,), device=dev, generator=g)) for _ in range(4)]
    res = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        with OneDeviceStrategy("/gpu:0").scope():
            opt = MomentumOptimizer(0.05, 0.9, clip_norm=0.25)
            opt.build(list(model.parameters()))
        gstep = GlobalStep()

        def step(x, y):
            loss = ops.sparse_softmax_cross_entropy(model(x), y)
            opt.minimize(loss, global_step=gstep)
            return loss

        losses, norms = [], []
        if graphed:
            fn = GraphedTrainStep(step, opt, [batches[0][0].clone(), batches[0][1].clone()],
                                  global_step=gstep, warmup=2)
            for x, y in batches[1:]:
                losses.append(fn(x, y).clone())
                norms.append(opt.last_grad_norm.clone())
        else:
            for _ in range(2):
                step(*batches[0])
            for x, y in batches[1:]:
                losses.append(step(x, y))
                norms.append(opt.last_grad_norm.clone())
        torch.cuda.synchronize()
        res.append((torch.stack(losses), torch.cat(norms), opt.space.master.clone(),
                    opt.slots[0].buf.clone(), int(gstep)))
    (la, na, pa, sa, ga), (lb, nb, pb, sb, gb) = res
    assert torch.equal(la, lb), (la, lb)
    assert torch.equal(na, nb), (na, nb)
    assert torch.equal(pa, pb) and torch.equal(sa, sb)
    assert ga == gb == 5
    assert len(set(nb.tolist())) == 3, nb          # a new norm in every replay
    assert (nb > 0.25).any(), nb                   # and the clip was at work
