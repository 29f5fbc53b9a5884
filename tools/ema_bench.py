"""Time the ExponentialMovingAverage pass over one flat space: the HIP kernel (``ops.ema_update``)
against the torch-op composition that computes the same thing, ``avg.sub_((avg - var) * a)`` --
what the project would run without the kernel -- and the Adam update for scale (profiles/EMA.md).

    python tools/ema_bench.py [--sizes 25600000,110000000] [--iters 100] [--rounds 5] [--out F]

Per size the three arms are timed in windows of ``iters`` back-to-back calls between two HIP
events, alternating, after a warm-up round.  One JSON line per size reports the median and the
spread of the per-call times and the bytes each arm's algorithm has to move: algorithm bytes per
second between back-to-back calls, not measured HBM traffic.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bytes per parameter: the kernel reads avg and var and writes avg; the composition also writes and
# re-reads the difference and the product (two temporaries), 28 at the least
BYTES = {"ema_kernel": 12, "torch_ops": 28, "adam_update": 30}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="25600000,110000000")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: needs a GPU (a CPU timing says nothing about the kernel)")
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.optimizers import AdamOptimizer, ExponentialMovingAverage
    from distributedtensorflow_amd.parallel import OneDeviceStrategy

    lines = []
    for n in (int(s) for s in args.sizes.split(",")):
        p = torch.nn.Parameter(torch.randn(n, 1, device="cuda"))
        p._dtf_name = "w/kernel"
        ema = ExponentialMovingAverage(args.decay)
        opt = AdamOptimizer(1e-3, variable_averages=ema)
        plain = AdamOptimizer(1e-3)
        with OneDeviceStrategy("/gpu:0").scope():
            sp = opt.build([p])
        sp.grad.normal_(std=1e-3)
        opt._refresh_ema()               # a = 1 - decay on the device
        avg, var, a_dev = ema.buf, sp.master, ema.a_dev
        avg.normal_()
        loose = avg.clone()
        # the update for scale runs without the average attached
        q = torch.nn.Parameter(torch.randn(n, 1, device="cuda"))
        q._dtf_name = "w/kernel"
        with OneDeviceStrategy("/gpu:0").scope():
            plain.build([q])
        plain.space.grad.normal_(std=1e-3)

        def adam_update():
            plain.iterations += 1
            plain._apply(1.0)

        calls = {
            "ema_kernel": lambda: ops.ema_update(avg, var, a_dev),
            "torch_ops": lambda: loose.sub_((loose - var) * a_dev),
            "adam_update": adam_update,
        }
        # the two forms agree before anything is timed
        check = avg.clone()
        ops.ema_update(check, var, a_dev)
        want = avg - (avg - var) * a_dev
        assert float((check - want).abs().max()) <= 2.0 ** -20 * float(
            torch.maximum(avg.abs(), var.abs()).max())
        del check, want

        def window(fn):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fn()
            end.record()
            end.synchronize()
            return start.elapsed_time(end) / args.iters * 1e3        # us per call

        times = {k: [] for k in calls}
        for r in range(args.rounds + 1):
            for k, fn in calls.items():
                t = window(fn)
                if r:                                                 # round 0 warms up
                    times[k].append(t)
        res = {"elements": n, "device": torch.cuda.get_device_name(0), "iters": args.iters,
               "rounds": args.rounds, "decay": args.decay}
        for k, ts in times.items():
            med = statistics.median(ts)
            res[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2),
                      "us_max": round(max(ts), 2), "bytes": BYTES[k] * n,
                      "gb_per_s": round(BYTES[k] * n / med / 1e3, 1)}
        res["kernel_over_torch_ops"] = round(res["ema_kernel"]["us_median"] /
                                             res["torch_ops"]["us_median"], 3)
        res["kernel_over_adam_update"] = round(res["ema_kernel"]["us_median"] /
                                               res["adam_update"]["us_median"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del opt, plain, calls, avg, var, loose, p, q, sp, ema
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
