"""Time gradient accumulation on the device (profiles/ACCUM.md).

    python tools/accum_bench.py [--sizes 25600000,110000000] [--iters 100] [--rounds 5]
                                [--models resnet50,bert_base] [--accum 4] [--steps 8] [--out F]

**The pass.**  Per size of a flat space the HIP kernel (``ops.grad_accumulate``) is timed in both
modes -- the store ``dst = src`` and the add ``dst += src`` -- next to torch's ``copy_`` and
``add_`` on the same buffers: windows of ``iters`` back-to-back calls between two HIP events, the
arms alternating, after a warm-up round.  One JSON line per size reports the median and the spread
of the per-call times and the bytes each arm's algorithm has to move (8 per element for the store,
12 for the add): algorithm bytes per second between back-to-back calls, not measured HBM traffic.

**In a training run.**  Per model (the benchmark's ResNet-50 at batch 1984 and BERT-base at batch
512 x 128 tokens, one device) the time of a micro-step with ``accumulation_steps = accum`` is
compared with the time of a step of the same run with ``accumulation_steps = 1``: windows of
``steps`` updates (``steps * accum`` micro-steps) against windows of ``steps * accum`` plain
steps between two HIP events, alternating, one warm-up round and ``rounds`` measured ones.  Both
arms run on ONE optimizer, built with the accumulator: the plain arm sets its
``accumulation_steps`` to 1 for the window, which is exactly the path an optimizer built without
the keyword takes (every accumulation branch tests that number).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bytes per element: the store reads src and writes dst; the add also reads dst
BYTES = {"kernel_store": 8, "torch_copy_": 8, "kernel_add": 12, "torch_add_": 12}


def _stats(ts, unit):
    med = statistics.median(ts)
    return {f"{unit}_median": round(med, 3), f"{unit}_min": round(min(ts), 3),
            f"{unit}_max": round(max(ts), 3)}


def bench_pass(torch, n, iters, rounds):
    from distributedtensorflow_amd import ops
    g = torch.Generator(device="cuda").manual_seed(n)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    accum = torch.randn(n, device="cuda", generator=g) * 1e-3
    loose = accum.clone()
    # the kernel and torch agree to the bit before anything is timed
    a, b = accum.clone(), accum.clone()
    ops.grad_accumulate(a, grad, True)
    b.add_(grad)
    assert torch.equal(a, b)
    ops.grad_accumulate(a, grad, False)
    assert torch.equal(a, grad)
    del a, b
    calls = {
        "kernel_store": lambda: ops.grad_accumulate(accum, grad, False),
        "torch_copy_": lambda: loose.copy_(grad),
        "kernel_add": lambda: ops.grad_accumulate(accum, grad, True),
        "torch_add_": lambda: loose.add_(grad),
    }

    def window(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / iters * 1e3        # us per call

    times = {k: [] for k in calls}
    for r in range(rounds + 1):
        for k, fn in calls.items():
            t = window(fn)
            if r:                                             # round 0 warms up
                times[k].append(t)
    res = {"what": "pass", "elements": n, "device": torch.cuda.get_device_name(0),
           "iters": iters, "rounds": rounds}
    for k, ts in times.items():
        res[k] = dict(_stats(ts, "us"), bytes=BYTES[k] * n)
        res[k]["gb_per_s"] = round(BYTES[k] * n / res[k]["us_median"] / 1e3, 1)
    return res


def build_run(torch, name, accum):
    """-> (micro_step(), optimizer) of the benchmark's workload on one device."""
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    torch.manual_seed(1234)
    g = torch.Generator(device="cuda").manual_seed(1234)
    with OneDeviceStrategy("/gpu:0").scope():
        if name == "resnet50":
            from distributedtensorflow_amd.models import resnet50
            from distributedtensorflow_amd.optimizers import MomentumOptimizer
            model = resnet50()
            opt = MomentumOptimizer(0.1, momentum=0.9, weight_decay=1e-4,
                                    accumulation_steps=accum)
            x = torch.randn(1984, 224, 224, 3, device="cuda", generator=g).to(torch.bfloat16)
            y = torch.randint(0, 1000, (1984,), device="cuda", generator=g)

            def loss_fn():
                return ops.sparse_softmax_cross_entropy(model(x), y)
        else:
            from distributedtensorflow_amd.data.synthetic import SyntheticMLM
            from distributedtensorflow_amd.models.bert import bert_base
            from distributedtensorflow_amd.optimizers import LAMBOptimizer
            model = bert_base()
            opt = LAMBOptimizer(1e-3, weight_decay=0.01, accumulation_steps=accum)
            d = next(iter(SyntheticMLM(512, 128, max_predictions=20, device="cuda", seed=1234)))
            batch = (d["input_ids"], d["segment_ids"], d["input_mask"],
                     d["masked_lm_positions"], d["masked_lm_ids"],
                     torch.ones_like(d["masked_lm_ids"], dtype=torch.float32))

            def loss_fn():
                return model(*batch)
        model.train()
        opt.build(list(model.parameters()))

    def micro_step():
        return opt.minimize(loss_fn())
    return micro_step, opt


def bench_run(torch, name, accum, steps, rounds):
    micro_step, opt = build_run(torch, name, accum)
    red = opt._reducer

    def window(n_accum):
        # the plain arm: accumulation_steps = 1 takes no accumulation branch anywhere
        opt.reset_accumulation()
        red.hold = red.fold = False
        opt.accumulation_steps = n_accum
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps * accum):
            micro_step()
        end.record()
        end.synchronize()
        assert opt.accumulated == 0
        return start.elapsed_time(end) / (steps * accum)          # ms per (micro-)step

    times = {"plain_step": [], "micro_step": []}
    for r in range(rounds + 1):
        for k, n_accum in (("plain_step", 1), ("micro_step", accum)):
            t = window(n_accum)
            if r:                                                 # round 0 warms up
                times[k].append(t)
    res = {"what": "run", "model": name, "elements": opt.space.numel, "accum": accum,
           "device": torch.cuda.get_device_name(0), "micro_steps_per_window": steps * accum,
           "rounds": rounds,
           "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    for k, ts in times.items():
        res[k] = dict(_stats(ts, "ms"), windows=[round(t, 3) for t in ts])
    res["micro_over_plain"] = round(res["micro_step"]["ms_median"] /
                                    res["plain_step"]["ms_median"], 4)
    res["micro_minus_plain_us"] = round((res["micro_step"]["ms_median"] -
                                         res["plain_step"]["ms_median"]) * 1e3, 1)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="25600000,110000000")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--models", default="resnet50,bert_base")
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8, help="updates per window of the run arms")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench: needs a GPU (a CPU timing says nothing about the kernel)")

    lines = []

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for n in (int(s) for s in args.sizes.split(",") if s):
        emit(bench_pass(torch, n, args.iters, args.rounds))
        torch.cuda.empty_cache()
    for name in (m for m in args.models.split(",") if m):
        emit(bench_run(torch, name, args.accum, args.steps, args.rounds))
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
