"""Global-norm clipping over two gloo ranks on the CPU: mirrored replicas, a colocated parameter
server with sharded owners and one with owner ranges.  Every rank must form the same global norm
(no owner holds the whole reduced gradient in the colocated forms), stay bit-identical to the
other and match one process on the concatenated batch."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clip_dist_worker  # noqa: E402

from distributedtensorflow_amd.cluster.launcher import free_ports  # noqa: E402

STEPS = 3


def _launch(kind, world, tmp_path, *args, timeout=240):
    """test_distributed._launch for clip_dist_worker.py."""
    port = free_ports(1)[0]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   PYTHONPATH=ROOT)
        log = open(tmp_path / f"{kind}{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable,
                                        os.path.join(HERE, "clip_dist_worker.py"), kind,
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
    """{optimizer: (variables, per-step norms)} of three clipped steps in one process on the
    whole batch; computed once, never written."""
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import global_step as gs_mod
    out = {}
    for name in ("momentum", "lamb"):
        gs_mod.reset_global_step()
        torch.manual_seed(17)
        with OneDeviceStrategy("cpu").scope():
            model = MnistCNN()
            opt = clip_dist_worker.make_optimizer(name)
            opt.build(list(model.parameters()))
            norms = clip_dist_worker.train(model, opt, STEPS)
        gs_mod.reset_global_step()
        # the comparison below is about clipped steps: at least two of the three were
        assert int((norms > clip_dist_worker.CLIP).sum()) >= 2, norms
        out[name] = ({k: v.detach().clone() for k, v in model.state_dict().items()}, norms)
    return out


def _assert_replicas(results, ref):
    state, norms = ref
    assert all(r["fingerprints"] == results[0]["fingerprints"] for r in results)
    for r in results[1:]:
        for k in state:
            assert torch.equal(r["state"][k], results[0]["state"][k]), f"replicas diverged at {k}"
        # the same global norm on every rank, to the bit
        assert torch.equal(r["norms"], results[0]["norms"])
    for k in state:     # test_lars_distributed's tolerance
        torch.testing.assert_close(results[0]["state"][k], state[k], atol=2e-5, rtol=1e-5)
    # the norm is a sum over the whole gradient: fp32 gradients summed in another order
    torch.testing.assert_close(results[0]["norms"], norms, atol=0, rtol=1e-5)
    assert all(r["global_step"] == STEPS for r in results)


def test_clip_mirrored_two_ranks(tmp_path, single_process):
    res = _launch("mirrored", 2, tmp_path, "opt=momentum")
    _assert_replicas(res, single_process["momentum"])


def test_clip_colocated_ps_sharded_owners(tmp_path, single_process):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=2", "opt=momentum")
    assert all(r["sharded"] is True and r["reducer"] == "_ColocatedPSReducer" for r in res)
    _assert_replicas(res, single_process["momentum"])


def test_clip_colocated_ps_owner_ranges(tmp_path, single_process):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=2", "opt=lamb")
    assert all(r["sharded"] is False and r["reducer"] == "_ColocatedPSReducer" for r in res)
    _assert_replicas(res, single_process["lamb"])
