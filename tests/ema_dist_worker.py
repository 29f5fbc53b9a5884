"""One gloo rank of a data-parallel CPU run whose optimizer keeps an ExponentialMovingAverage of
the variables (launched by tests/test_ema_distributed.py, one process per rank).

    python ema_dist_worker.py <strategy> <out_dir> [key=value ...]

As tests/clip_dist_worker.py.  After every step the rank waits for the variables, completes the
average buffer (by entering ``swap()``, by ``gather_state()``, and on the last step by the
session's checkpoint path) and records the variables, the averages and the ``a`` used.
"""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dist_worker  # noqa: E402
import torch  # noqa: E402

DECAY = 0.5


def main():
    kind, out = sys.argv[1], sys.argv[2]
    kw = dict(a.split("=", 1) for a in sys.argv[3:])
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.optimizers import LAMBOptimizer, MomentumOptimizer
    from distributedtensorflow_amd.parallel import MirroredStrategy, ParameterServerStrategy
    from distributedtensorflow_amd.train.checkpoint import Saver, collect_checkpoint_vars
    from distributedtensorflow_amd.train.session import _Session
    if kind == "mirrored":
        strat = MirroredStrategy()
    elif kind == "colocated_ps":
        strat = ParameterServerStrategy(num_ps=int(kw.get("num_ps", 1)))
    else:
        raise SystemExit(f"unknown strategy {kind}")
    rank, world = strat.replica_id, strat.num_replicas_in_sync
    steps = int(kw.get("steps", 3))
    torch.manual_seed(17 + 101 * rank)
    with strat.scope():
        model = MnistCNN()
        gstep = dtf.train.get_or_create_global_step()
        ema = dtf.train.ExponentialMovingAverage(DECAY, num_updates=gstep)
        if kw.get("opt", "momentum") == "lamb":
            opt = LAMBOptimizer(1e-3, variable_averages=ema)
        else:
            opt = MomentumOptimizer(0.05, 0.9, variable_averages=ema)
        opt.build(list(model.parameters()))
        sess = _Session(types.SimpleNamespace(
            optimizer=opt, global_step=gstep,
            saver=Saver(model=model, optimizer=opt, global_step=gstep)), strat, strat.is_chief,
            out, None)
        avgs, masters, a_used = [ema.buf.clone()], [opt.space.master.clone()], []
        prefix = None
        per = 16 // world
        for step in range(steps):
            x, y = dist_worker.global_batch(step)
            x, y = x[rank * per:(rank + 1) * per], y[rank * per:(rank + 1) * per]
            opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y), global_step=gstep)
            opt.synchronize_variables()
            if step == steps - 1:
                prefix = sess.save_checkpoint(os.path.join(out, "model.ckpt"), gstep.value())
            elif step % 2 == 0:
                with ema.swap():        # collective under the colocated parameter server
                    pass
            else:
                opt.gather_state()
            avgs.append(ema.buf.clone())
            masters.append(opt.space.master.clone())
            a_used.append(float(ema.a_dev.item()))
        fps = dtf.distribute.check_replicas_consistent(opt)      # raises if replicas diverged
    named = {k: (t.detach().clone(), layout)
             for k, (t, layout) in collect_checkpoint_vars(model, opt).items()
             if k.endswith("/ExponentialMovingAverage")}
    torch.save({"avgs": avgs, "masters": masters, "a": a_used, "named": named,
                "prefix": prefix, "global_step": gstep.value(), "fingerprints": fps,
                "sharded": getattr(opt._reducer, "sharded", None),
                "reducer": type(opt._reducer).__name__},
               os.path.join(out, f"rank{rank}.pt"))
    strat.barrier()
    # results are on disk: leave without the interpreter teardown (see dist_worker.colocated_bert)
    sys.stdout.flush()
    os._exit(0)


if __name__ == "__main__":
    main()
