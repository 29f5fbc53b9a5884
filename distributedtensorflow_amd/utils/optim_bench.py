"""Time the fused optimizer updates on a model's flat parameter space (profiles/LARS.md).

    python -m distributedtensorflow_amd.utils.optim_bench [--model resnet50] [--iters 200]
                                                          [--rounds 5] [--out FILE]

Each optimizer gets its own copy of the model; the gradients are random and fixed.  A round
times ``iters`` back-to-back applies of each optimizer between two HIP events, alternating the
optimizers, after a warm-up round; one JSON line reports the median and the spread of the
per-apply times, the bytes each update has to move and the rate that corresponds to.
"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys

# bytes per parameter: master r/w 8, gradient 4, momentum r/w 8, bf16 shadow 2; LARS reads
# master and gradient once more for the norms
BYTES_PER_PARAM = {"momentum": 22, "lars": 30}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs a GPU (a CPU timing says nothing about the kernels)")
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd.parallel import OneDeviceStrategy

    torch.manual_seed(0)
    with OneDeviceStrategy("/gpu:0").scope():
        base = getattr(dtf.models, args.model)()
    opts = {}
    for name in ("momentum", "lars"):
        model = copy.deepcopy(base)
        with OneDeviceStrategy("/gpu:0").scope():
            opt = (dtf.train.MomentumOptimizer(0.1, 0.9, weight_decay=1e-4) if name == "momentum"
                   else dtf.train.LARSOptimizer(0.1, 0.9, weight_decay=1e-4))
            sp = opt.build(list(model.parameters()))
        sp.grad.normal_(std=1e-3)
        opts[name] = (opt, model)

    def window(opt):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            opt.iterations += 1
            opt._apply(1.0)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / args.iters * 1e3        # us per apply

    times = {name: [] for name in opts}
    for r in range(args.rounds + 1):
        for name, (opt, _) in opts.items():
            t = window(opt)
            if r:                                                 # round 0 warms up
                times[name].append(t)
    for opt, _ in opts.values():
        assert not opt.nonfinite_flag()
    numel = sum(p.numel() for p in base.parameters())
    res = {"model": args.model, "parameters": numel, "device": torch.cuda.get_device_name(0),
           "iters": args.iters, "rounds": args.rounds}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"us_per_apply_median": round(med, 2), "us_min": round(min(ts), 2),
                     "us_max": round(max(ts), 2),
                     "bytes_per_apply": BYTES_PER_PARAM[name] * numel,
                     "gb_per_s": round(BYTES_PER_PARAM[name] * numel / med / 1e3, 1)}
    res["lars_over_momentum"] = round(res["lars"]["us_per_apply_median"] /
                                      res["momentum"]["us_per_apply_median"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
