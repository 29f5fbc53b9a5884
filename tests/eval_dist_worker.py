"""One rank of a two-process CPU (gloo) sharded evaluation, launched by
tests/test_eval_distributed.py like tests/dist_worker.py (RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT in the env).

    python eval_dist_worker.py <out_dir>

Every rank evaluates its shard of a fixed 103-example set under MirroredStrategy and saves
``metrics.result()`` (the collective read) and its local state to ``out_dir/rank<r>.pt``.

The model is a linear layer on integer-valued inputs and weights: its logits are exact in fp32
whatever the batch composition or the thread count, so the sharded and the single-process runs
see bit-identical rows and differ only by the order of the fp64 sums.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, BATCH, FEATURES, CLASSES, K = 103, 8, 16, 10, 3


def make_set():
    g = np.random.RandomState(7)
    return (g.randint(0, 8, size=(N, FEATURES)).astype(np.uint8),
            g.randint(0, CLASSES, size=(N,)).astype(np.int64))


class ExactLinear(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        w = torch.randint(-3, 4, (FEATURES, CLASSES), generator=g, device="cpu").float()
        self.w = torch.nn.Parameter(w)

    def forward(self, x):
        return (x.float() @ self.w) * 0.125        # integers / 8: exact, and ties are common


def run(num_shards, shard_index, strategy=None):
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd.data import DeviceArrayDataset
    imgs, labels = make_set()
    data = DeviceArrayDataset(imgs, labels, BATCH, "cpu", torch.float32, num_shards=num_shards,
                              shard_index=shard_index, scale=1.0)
    metrics = dtf.metrics.ClassificationMetrics(k=K, strategy=strategy)
    res = dtf.train.evaluate(ExactLinear(), data.single_pass(), metrics, strategy=strategy)
    return res, metrics.state.clone()


def main():
    out = sys.argv[1]
    from distributedtensorflow_amd.parallel import MirroredStrategy
    strat = MirroredStrategy(backend="gloo")
    assert strat.device.type == "cpu", strat.device       # the launcher hides the GPUs
    rank, world = strat.replica_id, strat.num_replicas_in_sync
    res, local = run(world, rank, strat)
    torch.save({"result": res, "local": local, "world": world, "collective": strat.collective},
               os.path.join(out, f"rank{rank}.pt"))
    strat.barrier()


if __name__ == "__main__":
    main()
