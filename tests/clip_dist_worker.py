"""One gloo rank of a data-parallel CPU run whose optimizer clips by global norm (launched by
tests/test_clip_distributed.py, one process per rank).

    python clip_dist_worker.py <strategy> <out_dir> [key=value ...]

As tests/dist_worker.py: every rank starts from its own seed (the strategy broadcasts rank 0's
variables), trains on its shard of the fixed global batch and saves its variables, and with them
the pre-clip norm of every step.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dist_worker  # noqa: E402
import torch  # noqa: E402

CLIP = 1.0


def make_optimizer(name):
    from distributedtensorflow_amd.optimizers import LAMBOptimizer, MomentumOptimizer
    if name == "lamb":
        return LAMBOptimizer(1e-3, clip_norm=CLIP)
    return MomentumOptimizer(0.05, 0.9, clip_norm=CLIP)


def train(model, opt, steps, rank=0, world=1, gstep=None):
    """-> the pre-clip norm of every step (a host read per step: test only)."""
    from distributedtensorflow_amd import ops
    per = 16 // world
    norms = []
    for step in range(steps):
        x, y = dist_worker.global_batch(step)
        x, y = x[rank * per:(rank + 1) * per], y[rank * per:(rank + 1) * per]
        opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y), global_step=gstep)
        norms.append(opt.last_grad_norm.clone())
    return torch.cat(norms)


def main():
    kind, out = sys.argv[1], sys.argv[2]
    kw = dict(a.split("=", 1) for a in sys.argv[3:])
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.parallel import MirroredStrategy, ParameterServerStrategy
    if kind == "mirrored":
        strat = MirroredStrategy()
    elif kind == "colocated_ps":
        strat = ParameterServerStrategy(num_ps=int(kw.get("num_ps", 1)))
    else:
        raise SystemExit(f"unknown strategy {kind}")
    rank, world = strat.replica_id, strat.num_replicas_in_sync
    torch.manual_seed(17 + 101 * rank)
    with strat.scope():
        model = MnistCNN()
        opt = make_optimizer(kw.get("opt", "momentum"))
        gstep = dtf.train.get_or_create_global_step()
        opt.build(list(model.parameters()))
        norms = train(model, opt, int(kw.get("steps", 3)), rank, world, gstep)
        opt.synchronize_variables()
        fps = dtf.distribute.check_replicas_consistent(opt)      # raises if replicas diverged
    torch.save({"state": {k: v.detach().clone() for k, v in model.state_dict().items()},
                "global_step": gstep.value(), "fingerprints": fps, "norms": norms,
                "sharded": getattr(opt._reducer, "sharded", None),
                "reducer": type(opt._reducer).__name__},
               os.path.join(out, f"rank{rank}.pt"))
    strat.barrier()
    # results are on disk: leave without the interpreter teardown (see dist_worker.colocated_bert)
    sys.stdout.flush()
    os._exit(0)


if __name__ == "__main__":
    main()
