"""The ExponentialMovingAverage pass on the device: the kernel against the per-step fp64 oracle at
its edges (unaligned range starts, scalar head and tail, several trips per block), every optimizer
class, graph replays with each step's own decay, and evaluation on the averaged weights."""
import copy

import numpy as np
import pytest
import torch

import ema_util

pytestmark = pytest.mark.gpu

GUARD = 64                      # canary elements (256 bytes) on both sides of the range
CANARY = -12345.678
BIG = 2 * 2048 * 256 * 4 + 5    # default cap: 2048 blocks x 256 threads x float4, two trips + tail


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _K():
    from distributedtensorflow_amd.ops import native
    return native.kernels()


def _launch(avg, var, n, a_dev, max_blocks=0):
    _K().ema_update(avg.data_ptr(), var.data_ptr(), n, a_dev.data_ptr(), max_blocks,
                    torch.cuda.current_stream().cuda_stream)


def _case(n, off, seed=0):
    """(avg buffer, var buffer, slice of the range): the range starts ``off`` elements past a
    256-byte-aligned address, with GUARD canaries on both sides."""
    g = torch.Generator().manual_seed(seed + 7 * n + off)
    total = GUARD + off + n + GUARD
    avg = torch.full((total,), CANARY, device="cuda")
    var = torch.full((total,), CANARY, device="cuda")
    assert avg.data_ptr() % 256 == 0 and var.data_ptr() % 256 == 0
    sl = slice(GUARD + off, GUARD + off + n)
    # normal-range values of mixed scale
    scale = torch.logspace(-3, 3, n) if n > 1 else torch.ones(1)
    avg[sl] = (torch.randn(n, generator=g) * scale).cuda()
    var[sl] = (torch.randn(n, generator=g) * scale.flip(0)).cuda()
    return avg, var, sl


def _check(n, off, blocks_list, a=1.0 - 0.9):
    a_dev = torch.tensor([a], device="cuda", dtype=torch.float32)
    avg0, var, sl = _case(n, off)
    outs = []
    for mb in blocks_list + blocks_list[:1]:            # the first once more: run to run
        avg = avg0.clone()
        _launch(avg[sl], var[sl], n, a_dev, mb)
        outs.append(avg)
    torch.cuda.synchronize()
    ema_util.assert_step(outs[0][sl], avg0[sl], var[sl], float(a_dev.item()),
                         f"n={n} off={off}")
    for o in outs:
        assert torch.equal(o, outs[0])
        assert (o[:sl.start] == CANARY).all() and (o[sl.stop:] == CANARY).all()
    assert (var[:sl.start] == CANARY).all() and (var[sl.stop:] == CANARY).all()
    if n > 8:
        assert not torch.equal(outs[0][sl], avg0[sl])
    # avg == var is a bit-exact fixed point
    fix = var.clone()
    _launch(fix[sl], var[sl], n, a_dev, blocks_list[-1])
    assert torch.equal(fix, var)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1027, 2049])
def test_kernel_meets_the_oracle_at_every_offset_and_grid_cap(n):
    for off in (0, 1, 2, 3):
        _check(n, off, [0, 1, 3])


def test_kernel_with_several_trips_per_block_under_the_default_cap():
    for off in (0, 3):
        _check(BIG, off, [0], a=1.0 - 0.9999)


@pytest.mark.parametrize("n", [5, 1027, 2049, 5000])
def test_buffers_misaligned_differently_take_the_scalar_path_for_every_element(n):
    """avg and var at different offsets inside their 16 bytes: no float4 form exists, and every
    element must still be updated, under a one-block grid and under the default one."""
    a_dev = torch.tensor([0.3], device="cuda")
    for off_a, off_v in ((1, 2), (0, 3), (2, 0)):
        avg0, _, sa = _case(n, off_a)
        _, var, sv = _case(n, off_v, seed=1)
        outs = []
        for mb in (1, 0, 3, 1):
            avg = avg0.clone()
            _launch(avg[sa], var[sv], n, a_dev, mb)
            outs.append(avg)
        torch.cuda.synchronize()
        ema_util.assert_step(outs[0][sa], avg0[sa], var[sv], 0.3, f"n={n} {off_a}/{off_v}")
        # every element moved: none silently keeps the old average
        assert (outs[0][sa] != avg0[sa]).all()
        for o in outs:
            assert torch.equal(o, outs[0])
            assert (o[:sa.start] == CANARY).all() and (o[sa.stop:] == CANARY).all()
        assert (var[:sv.start] == CANARY).all() and (var[sv.stop:] == CANARY).all()
        # the same bits as the aligned form of the same data
        var_al = avg0.clone()
        var_al[sa] = var[sv]
        al = avg0.clone()
        _launch(al[sa], var_al[sa], n, a_dev, 0)
        assert torch.equal(al, outs[0])


def test_an_optimizer_that_overrides_refresh_hyper_still_refreshes_the_average():
    from distributedtensorflow_amd.optimizers import (ExponentialMovingAverage,
                                                      MomentumOptimizer)
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import GlobalStep

    class Mine(MomentumOptimizer):
        def _refresh_hyper(self):
            self._lr_dev[0].fill_(self.learning_rate())

    gstep = GlobalStep()
    ema = ExponentialMovingAverage(0.9999, num_updates=gstep)
    ps = ema_util.make_params("cuda")
    with OneDeviceStrategy("cuda").scope():
        opt = Mine(0.1, 0.9, variable_averages=ema)
        opt.build(ps)
    for n in (1, 2):
        for p, g in zip(ps, ema_util.make_grads(n)):
            p.grad.copy_(g.cuda())
        opt.apply_gradients(global_step=gstep)
        assert float(ema.a_dev.item()) == float(np.float32(1.0 - (1.0 + n) / (10.0 + n)))


def test_zero_elements_is_a_no_op_and_bad_arguments_are_rejected():
    a_dev = torch.tensor([0.5], device="cuda")
    avg, var, sl = _case(4, 1)
    before = avg.clone()
    _launch(avg[sl], var[sl], 0, a_dev)
    torch.cuda.synchronize()
    assert torch.equal(avg, before)
    st = torch.cuda.current_stream().cuda_stream
    for args in ((avg.data_ptr(), var.data_ptr(), -1, a_dev.data_ptr()),
                 (0, var.data_ptr(), 4, a_dev.data_ptr()),
                 (avg.data_ptr(), 0, 4, a_dev.data_ptr()),
                 (avg.data_ptr(), var.data_ptr(), 4, 0)):
        with pytest.raises(ValueError):
            _K().ema_update(*args, 0, st)
    assert torch.equal(avg, before)


def test_nonfinite_variables_reach_their_own_element_only():
    n, a_dev = 1027, torch.tensor([0.25], device="cuda")
    avg0, var, sl = _case(n, 1)
    clean = avg0.clone()
    _launch(clean[sl], var[sl], n, a_dev)
    bad = {0: float("inf"), 2: float("-inf"), 5: float("nan"), 514: float("inf"),
           n - 1: float("nan")}
    for k, v in bad.items():
        var[sl.start + k] = v
    got = avg0.clone()
    _launch(got[sl], var[sl], n, a_dev)
    torch.cuda.synchronize()
    keep = torch.ones(got.numel(), dtype=torch.bool, device="cuda")
    for k, v in bad.items():
        keep[sl.start + k] = False
        x = float(got[sl.start + k])
        assert np.isnan(x) if np.isnan(v) else x == v, (k, x)
    assert torch.equal(got[keep], clean[keep])


def test_a_is_read_from_the_device_at_every_launch():
    n = 1027
    a_dev = torch.tensor([0.1], device="cuda")
    avg0, var, sl = _case(n, 2)
    first, second = avg0.clone(), avg0.clone()
    args = (second[sl].data_ptr(), var[sl].data_ptr(), n, a_dev.data_ptr(), 0,
            torch.cuda.current_stream().cuda_stream)
    _launch(first[sl], var[sl], n, a_dev)
    a_dev.fill_(0.75)
    _K().ema_update(*args)
    torch.cuda.synchronize()
    ema_util.assert_step(first[sl], avg0[sl], var[sl], 0.1)
    ema_util.assert_step(second[sl], avg0[sl], var[sl], 0.75)
    assert not torch.equal(first, second)


def test_op_layer_runs_the_kernel_on_slices():
    from distributedtensorflow_amd import ops
    a_dev = torch.tensor([0.3], device="cuda")
    avg0, var, sl = _case(2049, 3)
    got = avg0.clone()
    ops.ema_update(got[sl], var[sl], a_dev)
    want = avg0.clone()
    _launch(want[sl], var[sl], 2049, a_dev)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.ema_update(got[sl], var[sl].double(), a_dev)


@pytest.mark.parametrize("name", list(ema_util.OPTIMIZERS))
def test_every_optimizer_meets_the_per_step_oracle_on_the_device(name):
    from distributedtensorflow_amd.optimizers import ExponentialMovingAverage
    ema = ExponentialMovingAverage(0.9)
    opt, _ = ema_util.run_optimizer_steps(name, "cuda", ema)
    assert ema.buf.is_cuda and ema.a_dev.data_ptr() == opt._lr_dev.data_ptr() + 4


def _mnist_run(base, graphed, batches, warm):
    """Two eager warm-up steps and one step per batch; -> (averages, variables, a used last)."""
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import GlobalStep, GraphedTrainStep
    model = copy.deepcopy(base)
    gstep = GlobalStep()
    ema = dtf.train.ExponentialMovingAverage(0.9999, num_updates=gstep)
    with OneDeviceStrategy("/gpu:0").scope():
        opt = dtf.train.AdamOptimizer(1e-3, variable_averages=ema)
        opt.build(list(model.parameters()))

    def step(x, y):
        loss = ops.sparse_softmax_cross_entropy(model(x), y)
        opt.minimize(loss, global_step=gstep)
        return loss

    if graphed:
        fn = GraphedTrainStep(step, opt, [warm[0].clone(), warm[1].clone()], global_step=gstep,
                              warmup=2)
        for x, y in batches:
            fn(x, y)
    else:
        for _ in range(2):
            step(*warm)
        for x, y in batches:
            step(x, y)
    torch.cuda.synchronize()
    return ema.buf.clone(), opt.space.master.clone(), float(ema.a_dev.item()), int(gstep)


def test_graph_replays_use_each_steps_own_decay():
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = MnistCNN()
    g = torch.Generator(device="cuda").manual_seed(1)
    batches = [(torch.rand(32, 784, device="cuda", generator=g).to(torch.bfloat16),
                torch.randint(0, 10, (32,), device="cuda", generator=g)) for _ in range(5)]
    ea, pa, aa, sa = _mnist_run(base, False, batches[1:], batches[0])
    eb, pb, ab, sb = _mnist_run(base, True, batches[1:], batches[0])
    assert sa == sb == 6
    # the last step saw n = 6; a decay baked in at capture time would be n = 3's
    assert aa == ab == float(np.float32(1.0 - 7.0 / 16.0))
    assert torch.equal(pa, pb)
    assert torch.equal(ea, eb)
    assert not torch.equal(ea, pa)


def _eval(model, opt, ema=None):
    from distributedtensorflow_amd.metrics import ClassificationMetrics
    from distributedtensorflow_amd.train import evaluate
    g = torch.Generator(device="cuda").manual_seed(99)
    batches = [(torch.rand(32, 784, device="cuda", generator=g).to(torch.bfloat16),
                torch.randint(0, 10, (32,), device="cuda", generator=g)) for _ in range(2)]
    return evaluate(model, batches, ClassificationMetrics(k=5), optimizer=opt, averages=ema)


def test_evaluate_on_the_averages_on_the_device():
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.ops import native
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = MnistCNN()
    g = torch.Generator(device="cuda").manual_seed(5)
    batches = [(torch.rand(32, 784, device="cuda", generator=g).to(torch.bfloat16),
                torch.randint(0, 10, (32,), device="cuda", generator=g)) for _ in range(5)]

    def setup():
        model = copy.deepcopy(base)
        ema = dtf.train.ExponentialMovingAverage(0.5)
        with OneDeviceStrategy("/gpu:0").scope():
            opt = dtf.train.MomentumOptimizer(0.05, 0.9, variable_averages=ema)
            opt.build(list(model.parameters()))
        return model, opt, ema

    def train(model, opt, some):
        for x, y in some:
            opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y))

    ma, oa, ea = setup()
    train(ma, oa, batches[:3])
    ps = list(ma.parameters())
    shadows = [p._dtf_shadow for p in ps]
    ptrs = [p.data_ptr() for p in ps]
    with ea.swap():
        for p in ps:
            # the bf16 weights the ops see are the cast of the averages
            assert torch.equal(native._bf16_weight(p), ea.average(p).to(torch.bfloat16))
            assert p.data_ptr() == ea.average(p).data_ptr()
    for p, s, ptr in zip(ps, shadows, ptrs):
        assert p._dtf_shadow is s and p.data_ptr() == ptr
    raw, avg = _eval(ma, oa), _eval(ma, oa, ea)
    assert avg["loss"] != raw["loss"]
    # a model without an optimizer, loaded with the averaged weights (its bf16 weights are
    # cast on the fly)
    other = copy.deepcopy(base)
    with torch.no_grad():
        for p, q in zip(ps, other.parameters()):
            q.copy_(ea.average(p))
    assert _eval(other, None) == avg
    train(ma, oa, batches[3:])
    mb, ob, eb = setup()
    train(mb, ob, batches)
    torch.cuda.synchronize()
    assert torch.equal(oa.space.master, ob.space.master)
    assert torch.equal(oa.space.shadow, ob.space.shadow)
    for sa, sb in zip(oa.slots, ob.slots):
        assert torch.equal(sa.buf, sb.buf)
    assert torch.equal(ea.buf, eb.buf)
