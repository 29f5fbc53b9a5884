"""LARS over two gloo ranks on the CPU: mirrored replicas and a colocated parameter server stay
bit-identical to each other and match one process on the concatenated batch; the per-tensor
trust ratio keeps the parameter server's owners on variable boundaries."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import lars_dist_worker  # noqa: E402  (installs the "lars" factory into dist_worker)

from distributedtensorflow_amd.cluster.launcher import free_ports  # noqa: E402

dist_worker = lars_dist_worker.dist_worker
STEPS = 3


def _launch(kind, world, tmp_path, *args, timeout=240):
    """test_distributed._launch for lars_dist_worker.py."""
    port = free_ports(1)[0]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   PYTHONPATH=ROOT)
        log = open(tmp_path / f"{kind}{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable,
                                        os.path.join(HERE, "lars_dist_worker.py"), kind,
                                        str(tmp_path), *args], env=env, stdout=log,
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
    return [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(world)]


@pytest.fixture(scope="module")
def single_process():
    """Three LARS steps in one process on the whole batch; computed once, never written."""
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import global_step as gs_mod
    gs_mod.reset_global_step()
    torch.manual_seed(17)
    init = None
    with OneDeviceStrategy("cpu").scope():
        model = MnistCNN()
        opt = dist_worker.make_optimizer("lars")
        opt.build(list(model.parameters()))
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for step in range(STEPS):
            x, y = dist_worker.global_batch(step)
            opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y))
    gs_mod.reset_global_step()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    # the run must have moved every variable for the comparison below to mean anything
    assert all(not torch.equal(state[k], init[k]) for k in state)
    return state


def _assert_replicas(results, ref):
    assert all(r["fingerprints"] == results[0]["fingerprints"] for r in results)
    for r in results[1:]:
        for k in ref:
            assert torch.equal(r["state"][k], results[0]["state"][k]), f"replicas diverged at {k}"
    for k in ref:       # the LAMB test's tolerance: a trust ratio normalises fp noise
        torch.testing.assert_close(results[0]["state"][k], ref[k], atol=2e-5, rtol=1e-5)
    assert all(r["global_step"] == STEPS for r in results)


def test_lars_mirrored_two_ranks_matches_single_process(tmp_path, single_process):
    res = _launch("mirrored", 2, tmp_path, "opt=lars")
    _assert_replicas(res, single_process)


def test_lars_colocated_ps_keeps_variable_aligned_owners(tmp_path, single_process):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=2", "opt=lars")
    assert all(r["sharded"] is False for r in res)
    _assert_replicas(res, single_process)
