"""One rank of a data-parallel run whose optimizer accumulates gradients over micro-batches
(launched by tests/test_accumulation_distributed.py, one gloo process per rank on the CPU, and by
tests/test_accumulation_gpu.py at world 1 on RCCL).

    python accum_dist_worker.py <strategy> <out_dir> [key=value ...]

``strategy``: mirrored | colocated_ps | plain (one process, no process group).  Keys: ``opt``
(momentum | lamb | momentum_clip), ``num_ps``, ``accum`` (micro-batches per update), ``updates``,
``model`` (cnn: the MNIST CNN on the rank's shard of tests/dist_worker.py's global batches;
resnet: a small ResNet-50 on the GPU, every rank the same batches), ``out`` (file name).
As tests/dist_worker.py: every rank starts from its own seed and the strategy broadcasts rank 0's
variables.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dist_worker  # noqa: E402
import torch  # noqa: E402

CLIP = 1.0


def make_optimizer(name, accum, model="cnn"):
    from distributedtensorflow_amd.optimizers import LAMBOptimizer, MomentumOptimizer
    kw = {"accumulation_steps": accum}
    if name == "lamb":
        return LAMBOptimizer(1e-3, **kw)
    if name == "momentum_clip":
        return MomentumOptimizer(0.05, 0.9, clip_norm=CLIP, **kw)
    if model == "resnet":
        return MomentumOptimizer(0.05, 0.9, weight_decay=1e-4, **kw)
    return MomentumOptimizer(0.05, 0.9, **kw)


def micro_batch(i, rank=0, world=1):
    """Rank ``rank``'s shard of global micro-batch ``i`` (16 examples)."""
    per = 16 // world
    x, y = dist_worker.global_batch(i)
    return x[rank * per:(rank + 1) * per], y[rank * per:(rank + 1) * per]


def resnet_batch(i):
    g = torch.Generator().manual_seed(2000 + i)
    return (torch.rand(8, 64, 64, 3, generator=g, device="cpu").to(torch.bfloat16).cuda(),
            torch.randint(0, 100, (8,), generator=g, device="cpu").cuda())


def train(model, opt, updates, accum, rank=0, world=1, gstep=None, kind="cnn"):
    """``updates * accum`` micro-steps -> the pre-clip norm of every update (a host read per
    update: test only), or None without ``clip_norm``."""
    from distributedtensorflow_amd import ops
    norms = []
    for i in range(updates * accum):
        x, y = resnet_batch(i) if kind == "resnet" else micro_batch(i, rank, world)
        opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y), global_step=gstep)
        if opt.accumulated == 0 and opt.clip_norm is not None:
            norms.append(opt.last_grad_norm.clone())
    return torch.cat(norms) if norms else None


def main():
    kind, out = sys.argv[1], sys.argv[2]
    kw = dict(a.split("=", 1) for a in sys.argv[3:])
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd.parallel import (MirroredStrategy, OneDeviceStrategy,
                                                    ParameterServerStrategy)
    which = kw.get("model", "cnn")
    if kind == "mirrored":
        strat = MirroredStrategy()
    elif kind == "colocated_ps":
        strat = ParameterServerStrategy(num_ps=int(kw.get("num_ps", 1)))
    elif kind == "plain":
        strat = OneDeviceStrategy("/gpu:0" if which == "resnet" else "/cpu:0")
    else:
        raise SystemExit(f"unknown strategy {kind}")
    rank, world = strat.replica_id, strat.num_replicas_in_sync
    accum, updates = int(kw.get("accum", 2)), int(kw.get("updates", 3))
    torch.manual_seed(17 + 101 * rank)
    with strat.scope():
        if which == "resnet":
            from distributedtensorflow_amd.models import resnet50
            model = resnet50(num_classes=100)
        else:
            from distributedtensorflow_amd.models import MnistCNN
            model = MnistCNN()
        opt = make_optimizer(kw.get("opt", "momentum"), accum, which)
        gstep = dtf.train.get_or_create_global_step()
        opt.build(list(model.parameters()))
        norms = train(model, opt, updates, accum, rank, world, gstep, which)
        opt.synchronize_variables()
        fps = dtf.distribute.check_replicas_consistent(opt) if kind != "plain" else None
        if opt.space.device.type == "cuda":
            torch.cuda.synchronize()
    red = opt._reducer
    stats = getattr(red, "stats", None)
    torch.save({"state": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                "master": opt.space.master.detach().cpu().clone(),
                "global_step": gstep.value(), "iterations": opt.iterations,
                "accumulated": opt.accumulated, "fingerprints": fps, "norms": norms,
                "sharded": getattr(red, "sharded", None), "reducer": type(red).__name__,
                "stats": None if stats is None else
                {"steps": stats.steps, "early": stats.early, "late": stats.late,
                 "n_buckets": stats.n_buckets},
                "last_order": list(getattr(red, "last_order", ())),
                "backend": torch.distributed.get_backend()
                if torch.distributed.is_initialized() else None},
               os.path.join(out, kw.get("out", f"rank{rank}.pt")))
    strat.barrier()
    # results are on disk: leave without the interpreter teardown (see dist_worker.colocated_bert)
    sys.stdout.flush()
    os._exit(0)


if __name__ == "__main__":
    main()
