"""Sharded evaluation over two gloo ranks on the CPU: every rank's ``result()`` equals the
single-process result over the whole set (counts and hits exactly, the loss to fp64
reassociation), and the shards partition the set."""
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import eval_dist_worker  # noqa: E402

from distributedtensorflow_amd.cluster.launcher import free_ports  # noqa: E402


def _launch(world, tmp_path, timeout=60):
    """test_distributed._launch for eval_dist_worker.py."""
    port = free_ports(1)[0]
    procs = []
    for r in range(world):
        # a CPU / gloo world wherever the test runs: on a GPU node the strategy would otherwise
        # pick cuda:LOCAL_RANK and the nccl backend for these CPU tensors
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        log = open(tmp_path / f"eval{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable,
                                        os.path.join(HERE, "eval_dist_worker.py"),
                                        str(tmp_path)], env=env, stdout=log,
                                       stderr=subprocess.STDOUT), log))
    try:
        for p, _ in procs:
            p.wait(timeout=timeout)
    except subprocess.TimeoutExpired:
        for p, _ in procs:
            p.kill()
        raise AssertionError("\n".join(open(tmp_path / f"eval{r}.log").read()[-2000:]
                                       for r in range(world)))
    finally:
        for p, log in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
            log.close()
    for r, (p, _) in enumerate(procs):
        assert p.returncode == 0, open(tmp_path / f"eval{r}.log").read()[-3000:]
    return [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(world)]


def test_two_rank_sharded_evaluation_matches_single_process(tmp_path):
    want, state = eval_dist_worker.run(1, 0)
    assert want["count"] == eval_dist_worker.N == 103
    assert 0 < want["top_1"] < want["top_k"] < 1          # the comparison means something
    res = _launch(2, tmp_path)
    assert all(r["world"] == 2 and r["collective"] for r in res)
    # the shards partition the set: 52 + 51 examples, hit counts add up exactly
    assert [r["local"][0].item() for r in res] == [52.0, 51.0]
    both = res[0]["local"] + res[1]["local"]
    assert torch.equal(both[[0, 2, 3]], state[[0, 2, 3]])
    for r in res:
        got = r["result"]
        assert got["count"] == want["count"]
        assert got["top_1"] == want["top_1"] and got["top_k"] == want["top_k"]
        assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    assert res[0]["result"] == res[1]["result"]
