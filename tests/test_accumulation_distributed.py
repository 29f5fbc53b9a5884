"""Gradient accumulation over two gloo ranks on the CPU: mirrored replicas, a colocated parameter
server with sharded owners and one with owner ranges.  The ranks must stay bit-identical to each
other, match one process that accumulates the concatenated micro-batches, count updates (not
micro-steps) and communicate nothing on held micro-steps."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import accum_dist_worker  # noqa: E402

from distributedtensorflow_amd.cluster.launcher import free_ports  # noqa: E402

UPDATES, ACCUM = 3, 2


def _launch(kind, world, tmp_path, *args, timeout=240):
    """test_distributed._launch for accum_dist_worker.py."""
    port = free_ports(1)[0]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   PYTHONPATH=ROOT)
        log = open(tmp_path / f"{kind}{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable,
                                        os.path.join(HERE, "accum_dist_worker.py"), kind,
                                        str(tmp_path), f"accum={ACCUM}", f"updates={UPDATES}",
                                        *args], env=env, stdout=log,
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
    """{optimizer: (variables, per-update norms)} of three updates of two whole micro-batches
    each in one process; computed once, never written."""
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    from distributedtensorflow_amd.train import global_step as gs_mod
    out = {}
    for name in ("momentum", "lamb", "momentum_clip"):
        gs_mod.reset_global_step()
        torch.manual_seed(17)
        with OneDeviceStrategy("cpu").scope():
            model = MnistCNN()
            opt = accum_dist_worker.make_optimizer(name, ACCUM)
            opt.build(list(model.parameters()))
            norms = accum_dist_worker.train(model, opt, UPDATES, ACCUM)
        gs_mod.reset_global_step()
        assert opt.iterations == UPDATES and opt.accumulated == 0
        if name == "momentum_clip":
            # the comparison is about clipped updates: at least two of the three were
            assert int((norms > accum_dist_worker.CLIP).sum()) >= 2, norms
        out[name] = ({k: v.detach().clone() for k, v in model.state_dict().items()}, norms)
    return out


def _assert_replicas(results, ref):
    state, norms = ref
    assert all(r["fingerprints"] == results[0]["fingerprints"] for r in results)
    for r in results[1:]:
        for k in state:
            assert torch.equal(r["state"][k], results[0]["state"][k]), f"replicas diverged at {k}"
    for k in state:     # test_clip_distributed's tolerance: fp32 gradients summed in another order
        torch.testing.assert_close(results[0]["state"][k], state[k], atol=2e-5, rtol=1e-5)
    for r in results:
        assert r["global_step"] == UPDATES and r["iterations"] == UPDATES
        assert r["accumulated"] == 0
        # held micro-steps communicated nothing and left the records of the last update
        st = r["stats"]
        assert st["steps"] == UPDATES, st
        assert st["early"] + st["late"] == UPDATES * st["n_buckets"], st
        assert len(r["last_order"]) == st["n_buckets"] > 0
    if norms is not None:
        for r in results[1:]:      # the same global norm on every rank, to the bit
            assert torch.equal(r["norms"], results[0]["norms"])
        assert results[0]["norms"].numel() == UPDATES
        torch.testing.assert_close(results[0]["norms"], norms, atol=0, rtol=1e-5)


def test_accumulation_mirrored_two_ranks(tmp_path, single_process):
    res = _launch("mirrored", 2, tmp_path, "opt=momentum")
    assert all(r["reducer"] == "BucketedAllReduce" for r in res)
    _assert_replicas(res, single_process["momentum"])


def test_accumulation_mirrored_two_ranks_clipped(tmp_path, single_process):
    res = _launch("mirrored", 2, tmp_path, "opt=momentum_clip")
    _assert_replicas(res, single_process["momentum_clip"])


def test_accumulation_colocated_ps_sharded_owners(tmp_path, single_process):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=2", "opt=momentum")
    assert all(r["sharded"] is True and r["reducer"] == "_ColocatedPSReducer" for r in res)
    _assert_replicas(res, single_process["momentum"])


def test_accumulation_colocated_ps_sharded_owners_clipped(tmp_path, single_process):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=2", "opt=momentum_clip")
    assert all(r["sharded"] is True for r in res)
    _assert_replicas(res, single_process["momentum_clip"])


def test_accumulation_colocated_ps_owner_ranges(tmp_path, single_process):
    res = _launch("colocated_ps", 2, tmp_path, "num_ps=2", "opt=lamb")
    assert all(r["sharded"] is False and r["reducer"] == "_ColocatedPSReducer" for r in res)
    _assert_replicas(res, single_process["lamb"])
