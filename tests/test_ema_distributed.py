"""ExponentialMovingAverage over two gloo ranks on the CPU: mirrored replicas, a colocated
parameter server with sharded owners and one parameter server with owner ranges.  Once completed
(entering ``swap()``, ``gather_state()``, or the session's checkpoint path) every rank's average
buffer is bit-equal to rank 0's and meets the per-step oracle on the variables rank 0 recorded."""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ema_util  # noqa: E402

from distributedtensorflow_amd.cluster.launcher import free_ports  # noqa: E402
from distributedtensorflow_amd.train import list_variables, load_variable  # noqa: E402
from distributedtensorflow_amd.train.checkpoint import from_tf_layout  # noqa: E402

STEPS = 3


def _launch(kind, world, tmp_path, *args, timeout=240):
    """test_clip_distributed._launch for ema_dist_worker.py."""
    port = free_ports(1)[0]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   PYTHONPATH=ROOT)
        log = open(tmp_path / f"{kind}{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "ema_dist_worker.py"),
                                        kind, str(tmp_path), *args], env=env, stdout=log,
                                       stderr=subprocess.STDOUT), log))
    try:
        for p, _ in procs:
            p.wait(timeout=timeout)
    finally:
        for p, log in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
            log.close()
    for r, (p, _) in enumerate(procs):
        assert p.returncode == 0, open(tmp_path / f"{kind}{r}.log").read()[-3000:]
    return [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(world)]


def _assert_averages(results):
    r0 = results[0]
    assert all(r["global_step"] == STEPS for r in results)
    # n = the global step after the step's increment; decay 0.5 only from n = 8 on
    assert r0["a"] == [float(np.float32(1.0 - (1.0 + n) / (10.0 + n))) for n in (1, 2, 3)]
    assert torch.equal(r0["avgs"][0], r0["masters"][0])          # initialised to the variables
    for r in results[1:]:
        # (a rank that owns no range never forms ``a``: the averages below are what must agree)
        for t in range(STEPS + 1):
            assert torch.equal(r["avgs"][t], r0["avgs"][t]), f"averages diverged at step {t}"
            assert torch.equal(r["masters"][t], r0["masters"][t])
    for t in range(STEPS):
        ema_util.assert_step(r0["avgs"][t + 1], r0["avgs"][t], r0["masters"][t + 1], r0["a"][t],
                             f"step {t + 1}")
        assert not torch.equal(r0["avgs"][t + 1], r0["avgs"][t])
    assert not torch.equal(r0["avgs"][-1], r0["masters"][-1])


def _assert_checkpoint(results):
    """The chief's checkpoint holds the complete averages, in the variables' layouts."""
    r0 = results[0]
    assert r0["prefix"] and all(r["prefix"] is None for r in results[1:])
    names = {n for n, _ in list_variables(r0["prefix"])}
    assert r0["named"] and set(r0["named"]) <= names
    for name, (t, layout) in r0["named"].items():
        got = from_tf_layout(load_variable(r0["prefix"], name), layout)
        assert torch.equal(got.reshape(t.shape), t), name


def test_ema_mirrored_two_ranks(tmp_path):
    res = _launch("mirrored", 2, tmp_path)
    _assert_averages(res)
    _assert_checkpoint(res)


def test_ema_colocated_ps_sharded_owners(tmp_path):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=2", "opt=momentum")
    assert all(r["sharded"] is True and r["reducer"] == "_ColocatedPSReducer" for r in res)
    _assert_averages(res)
    _assert_checkpoint(res)


def test_ema_one_ps_owner_ranges(tmp_path):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=1", "opt=momentum")
    assert all(r["sharded"] is False and r["reducer"] == "_ColocatedPSReducer" for r in res)
    _assert_averages(res)
    _assert_checkpoint(res)
