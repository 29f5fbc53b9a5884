"""tests/dist_worker.py with an optimizer factory that also knows "lars" (launched by
tests/test_lars_distributed.py, one process per gloo rank).

    python lars_dist_worker.py <strategy> <out_dir> [key=value ...]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dist_worker  # noqa: E402

_base_make_optimizer = dist_worker.make_optimizer


def make_optimizer(name):
    if name == "lars":
        from distributedtensorflow_amd.optimizers import LARSOptimizer
        # eeta = 0.1: steps large enough that a wrong trust ratio or a split tensor shows
        return LARSOptimizer(0.5, 0.9, weight_decay=1e-3, eeta=0.1)
    return _base_make_optimizer(name)


dist_worker.make_optimizer = make_optimizer

if __name__ == "__main__":
    dist_worker.main()
