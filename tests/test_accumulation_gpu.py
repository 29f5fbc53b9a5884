"""Gradient accumulation on the device: the ``grad_accumulate`` kernel against exact fp32 at its
edges (unaligned range starts, scalar head and tail, several trips per block, non-finite values),
the native models against the sum-then-update oracle bit for bit, a whole update of N micro-steps
replayed as one graph, and the per-bucket fold in the backward hooks on real RCCL at world 1."""
import copy
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

GUARD = 64                      # canary elements (256 bytes) on both sides of the range
CANARY = -12345.678
BIG = 2 * 2048 * 256 * 4 + 5    # default cap: 2048 blocks x 256 threads x float4, two trips + tail


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---------------------------------------------------------------------------- 1. the kernel

def _launch(dst, src, n, mode, max_blocks=0):
    from distributedtensorflow_amd.ops import native
    native.kernels().grad_accumulate(dst.data_ptr(), src.data_ptr(), n, mode, max_blocks,
                                     torch.cuda.current_stream().cuda_stream)


def _case(n, doff, soff, seed=0):
    """(dst buffer, src buffer, dst slice, src slice): the ranges start ``doff`` / ``soff``
    elements past a 256-byte-aligned address, with GUARD canaries on both sides."""
    g = torch.Generator().manual_seed(seed + 7 * n + 3 * doff + soff)
    dst = torch.full((GUARD + doff + n + GUARD,), CANARY, device="cuda")
    src = torch.full((GUARD + soff + n + GUARD,), CANARY, device="cuda")
    assert dst.data_ptr() % 256 == 0 and src.data_ptr() % 256 == 0
    dsl, ssl = slice(GUARD + doff, GUARD + doff + n), slice(GUARD + soff, GUARD + soff + n)
    # normal-range values of mixed scale: most adds round
    scale = torch.logspace(-3, 3, n) if n > 1 else torch.ones(1)
    dst[dsl] = (torch.randn(n, generator=g) * scale).cuda()
    src[ssl] = (torch.randn(n, generator=g) * scale.flip(0)).cuda()
    return dst, src, dsl, ssl


def _check(n, doff, soff, blocks_list):
    dst0, src, dsl, ssl = _case(n, doff, soff)
    d_cpu, s_cpu = dst0[dsl].cpu(), src[ssl].cpu()
    # one IEEE add: the oracle's own bits
    want = {0: s_cpu, 1: d_cpu + s_cpu}
    for mode in (0, 1):
        outs = []
        for mb in blocks_list + blocks_list[:1]:            # the first once more: run to run
            dst = dst0.clone()
            _launch(dst[dsl], src[ssl], n, mode, mb)
            outs.append(dst)
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o[dsl].cpu(), want[mode]), f"n={n} off=({doff},{soff}) mode={mode}"
            assert torch.equal(o, outs[0])
            assert (o[:dsl.start] == CANARY).all() and (o[dsl.stop:] == CANARY).all()
        assert (src[:ssl.start] == CANARY).all() and (src[ssl.stop:] == CANARY).all()
        assert torch.equal(src[ssl].cpu(), s_cpu)
        if n > 8:
            assert not torch.equal(outs[0][dsl], dst0[dsl])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1027, 2049])
def test_kernel_is_exact_at_every_offset_and_grid_cap(n):
    for off in (0, 1, 2, 3):
        _check(n, off, off, [0, 1, 3])


@pytest.mark.parametrize("doff,soff", [(1, 2), (0, 3), (2, 0)])
def test_kernel_with_differently_misaligned_buffers_writes_every_element(doff, soff):
    for n in (1, 5, 1027):
        _check(n, doff, soff, [0, 3])


def test_kernel_with_several_trips_per_block_under_the_default_cap():
    _check(BIG, 1, 1, [0])


def test_kernel_passes_non_finite_values_through():
    n = 1027
    dst0, src, dsl, ssl = _case(n, 3, 3)
    pos = {"nan": [0, 2, 5, 500, n - 1], "pinf": [1, 7, 600], "ninf": [3, 9, n - 2]}
    s = src[ssl]
    s[pos["nan"]] = float("nan")
    s[pos["pinf"]] = float("inf")
    s[pos["ninf"]] = float("-inf")
    for mode in (0, 1):
        dst = dst0.clone()
        _launch(dst[dsl], src[ssl], n, mode)
        got = dst[dsl].cpu()
        want = src[ssl].cpu() if mode == 0 else dst0[dsl].cpu() + src[ssl].cpu()
        assert torch.isnan(got[pos["nan"]]).all()
        assert (got[pos["pinf"]] == float("inf")).all()
        assert (got[pos["ninf"]] == float("-inf")).all()
        finite = torch.isfinite(want)
        assert int((~finite).sum()) == 11 and torch.equal(torch.isfinite(got), finite)
        assert torch.equal(got[finite], want[finite])


def test_op_refuses_what_the_kernel_cannot_take():
    from distributedtensorflow_amd import ops
    a = torch.zeros(8, device="cuda")
    with pytest.raises(ValueError):
        ops.grad_accumulate(a, torch.zeros(7, device="cuda"), True)
    with pytest.raises(ValueError):
        ops.grad_accumulate(a, torch.zeros(8, device="cuda", dtype=torch.float64), True)
    from distributedtensorflow_amd.ops import native
    with pytest.raises(ValueError):
        native.kernels().grad_accumulate(a.data_ptr(), a.data_ptr(), 8, 2, 0, 0)


# ---------------------------------------------------------------------------- 2. native models

def _oracle_update(opt, losses_fn, n):
    """One update of a plain optimizer from the micro-batches' flat gradients summed in fp32 in
    micro-step order on the device, multiplied once by 1 / n inside the update."""
    total = None
    for k in range(n):
        opt.compute_gradients(losses_fn(k))
        g = opt.space.grad.clone()
        total = g if total is None else total + g
    opt.space.grad.copy_(total)
    opt.iterations += 1
    opt._apply(1.0 / n)


def _compare(base, make_opt, loss_fn, n, updates=2):
    """``loss_fn(model, i)``: the loss of micro-batch ``i``."""
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    model, ref = copy.deepcopy(base), copy.deepcopy(base)
    with OneDeviceStrategy("/gpu:0").scope():
        opt = make_opt(accumulation_steps=n)
        opt.build(list(model.parameters()))
        ref_opt = make_opt()
        ref_opt.build(list(ref.parameters()))
    assert opt.space.accum is not None and ref_opt.space.accum is None
    start = opt.space.master.clone()
    for u in range(updates):
        for k in range(n):
            held = opt.space.master.clone()
            assert opt.minimize(loss_fn(model, u * n + k)) is None
            assert opt.accumulated == (k + 1) % n
            if k < n - 1:
                assert torch.equal(opt.space.master, held)
        _oracle_update(ref_opt, lambda k: loss_fn(ref, u * n + k), n)
        assert torch.equal(opt.space.master, ref_opt.space.master), f"update {u}"
        if opt.clip_norm is not None:
            assert torch.equal(opt.last_grad_norm, ref_opt.last_grad_norm)
            assert float(opt.last_grad_norm) > 0.0
    torch.cuda.synchronize()
    assert opt.iterations == ref_opt.iterations == updates
    assert not torch.equal(opt.space.master, start)
    for a, b in zip(opt.slots, ref_opt.slots):
        assert torch.equal(a.buf, b.buf), a.name
    if opt.space.shadow is not None:
        assert torch.equal(opt.space.shadow, ref_opt.space.shadow)
    bufs = list(zip(model.buffers(), ref.buffers()))
    for a, b in bufs:      # BatchNorm moving statistics: updated on every micro-batch
        assert torch.equal(a, b)
    assert not opt.nonfinite_flag()
    return len(bufs)


def test_mnist_cnn_meets_the_oracle_bit_for_bit():
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.optimizers import AdamOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = MnistCNN()
    g = torch.Generator().manual_seed(1)
    data = [(torch.rand(8, 784, generator=g).to(torch.bfloat16).cuda(),
             torch.randint(0, 10, (8,), generator=g).cuda()) for _ in range(6)]
    _compare(base, lambda **kw: AdamOptimizer(1e-3, **kw),
             lambda m, i: ops.sparse_softmax_cross_entropy(m(data[i][0]), data[i][1]), 3)


def test_resnet_meets_the_oracle_bit_for_bit():
    """Direct, overwriting weight-gradient writes into the flat buffer, and BatchNorm."""
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import resnet50
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = resnet50(num_classes=100)
    g = torch.Generator().manual_seed(3)
    data = [(torch.rand(8, 64, 64, 3, generator=g).to(torch.bfloat16).cuda(),
             torch.randint(0, 100, (8,), generator=g).cuda()) for _ in range(4)]
    nbuf = _compare(base, lambda **kw: MomentumOptimizer(0.05, 0.9, weight_decay=1e-4,
                                                         clip_norm=1.0, **kw),
                    lambda m, i: ops.sparse_softmax_cross_entropy(m(data[i][0]), data[i][1]), 2)
    assert nbuf > 0


def test_tiny_bert_meets_the_oracle_bit_for_bit():
    """The tied embedding: autograd-accumulated and direct gradients in one flat space."""
    from distributedtensorflow_amd.data.synthetic import SyntheticMLM
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    from distributedtensorflow_amd.optimizers import LAMBOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    cfg = BertConfig(vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                     intermediate_size=512, max_position_embeddings=128,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = BertForPreTraining(cfg)
    it = iter(SyntheticMLM(8, 64, max_predictions=10, device="cuda", seed=0, vocab_size=1000))
    data = []
    for _ in range(4):
        d = next(it)
        data.append([d[k].clone() for k in ("input_ids", "segment_ids", "input_mask",
                                            "masked_lm_positions", "masked_lm_ids")] +
                    [torch.ones_like(d["masked_lm_ids"], dtype=torch.float32)])
    _compare(base, lambda **kw: LAMBOptimizer(1e-3, weight_decay=0.01, **kw),
             lambda m, i: m(*data[i]), 2)


# ---------------------------------------------------------------------------- 3. graphs

def _cnn_batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(128, 784, generator=g).to(torch.bfloat16).cuda(),
             torch.randint(0, 10, (128,), generator=g).cuda()) for _ in range(n)]


def test_graphed_update_of_two_micro_steps_matches_eager():
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import GlobalStep, GraphedTrainStep
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = MnistCNN()
    data = _cnn_batches(8, 5)
    warm, pairs = data[:2], [data[2:4], data[4:6], data[6:8]]
    res = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        with OneDeviceStrategy("/gpu:0").scope():
            # a decaying learning rate: every replay must see its own update's value
            opt = dtf.train.AdamOptimizer(lambda t: 1e-3 / (1 + 0.1 * t), accumulation_steps=2)
            opt.build(list(model.parameters()))
        gstep = GlobalStep()

        def step(x1, y1, x2, y2):
            losses = []
            for x, y in ((x1, y1), (x2, y2)):
                loss = ops.sparse_softmax_cross_entropy(model(x), y)
                opt.minimize(loss, global_step=gstep)
                losses.append(loss.detach())
            return torch.stack(losses)

        flat = lambda pair: [t for xy in pair for t in xy]          # noqa: E731
        losses = []
        if graphed:
            fn = GraphedTrainStep(step, opt, [t.clone() for t in flat(warm)], global_step=gstep,
                                  warmup=2)
        else:
            for _ in range(2):                   # the graphed run's eager warm-up updates
                step(*flat(warm))
            fn = step
        it0, gs0 = opt.iterations, int(gstep)
        assert it0 == gs0 == 2 and opt.accumulated == 0
        for pair in pairs:
            losses.append(fn(*flat(pair)).clone())
        torch.cuda.synchronize()
        assert opt.iterations - it0 == 3 and int(gstep) - gs0 == 3 and opt.accumulated == 0
        res.append((torch.stack(losses), opt.space.master.clone(),
                    [s.buf.clone() for s in opt.slots]))
    (la, pa, sa), (lb, pb, sb) = res
    assert torch.equal(la, lb), (la, lb)
    assert torch.equal(pa, pb)
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)


def test_graphed_step_refuses_a_partial_update():
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import GraphedTrainStep
    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        model = MnistCNN()
        opt = dtf.train.AdamOptimizer(1e-3, accumulation_steps=2)
        opt.build(list(model.parameters()))
    (x, y), = _cnn_batches(1, 6)

    def step(x, y):
        loss = ops.sparse_softmax_cross_entropy(model(x), y)
        opt.minimize(loss)
        return loss

    with pytest.raises(RuntimeError, match="micro"):
        GraphedTrainStep(step, opt, [x, y], warmup=2)


# ---------------------------------------------------------------------------- 4. RCCL, world 1

UPDATES = 2


def _worker(tmp_path, kind, *args, forced=True):
    """One child at a time, under a subprocess timeout (tests/test_forced_reducer_gpu.py)."""
    from distributedtensorflow_amd.cluster.launcher import free_ports
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="4",
               DTF_FORCE_REDUCER="1" if forced else "0", DTF_COMM="c10d")
    script = [os.path.join(HERE, "accum_dist_worker.py"), kind, str(tmp_path), "model=resnet",
              "accum=2", f"updates={UPDATES}", f"out={kind}.pt", *args]
    if forced:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
               "1", "--master-addr", "127.0.0.1", "--master-port", str(free_ports(1)[0])] + script
    else:
        cmd = [sys.executable] + script
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return torch.load(tmp_path / f"{kind}.pt", weights_only=True)


@pytest.fixture(scope="module")
def plain_accumulation(tmp_path_factory):
    """The single-process accumulation run of the same seeds; computed once, never written."""
    res = _worker(tmp_path_factory.mktemp("accum_plain"), "plain", forced=False)
    assert res["reducer"] == "_NullReducer" and res["backend"] is None
    assert res["iterations"] == UPDATES and res["accumulated"] == 0
    return res


@pytest.mark.parametrize("kind,args,reducer", [
    ("mirrored", (), "BucketedAllReduce"),
    ("colocated_ps", ("num_ps=1",), "_ColocatedPSReducer"),
])
def test_fold_in_the_hooks_on_rccl_is_bit_identical(tmp_path, plain_accumulation, kind, args,
                                                    reducer):
    res = _worker(tmp_path, kind, *args)
    assert res["backend"] == "nccl" and res["reducer"] == reducer, res["reducer"]
    assert res["iterations"] == res["global_step"] == UPDATES and res["accumulated"] == 0
    st = res["stats"]
    assert st["n_buckets"] >= 2, st
    assert st["steps"] == UPDATES, st                 # held micro-steps communicated nothing
    assert st["early"] >= UPDATES and st["early"] + st["late"] == UPDATES * st["n_buckets"], st
    master, plain = res["master"], plain_accumulation["master"]
    assert master.shape == plain.shape
    diff = (master != plain).sum().item()
    assert diff == 0, f"{diff} of {master.numel()} master weights differ from the plain run"
