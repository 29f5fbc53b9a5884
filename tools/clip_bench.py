"""Time the clipped Adam step: the deterministic norm pass + the update that reads its multiplier
from the device (``AdamOptimizer(clip_norm=...)``) against the loose ``clip_by_global_norm_``
(sum of squares with a float atomic, small torch ops, ``grad.mul_``) followed by the plain Adam
update (profiles/CLIP.md).

    python tools/clip_bench.py [--sizes 25600000,110000000] [--iters 100] [--rounds 5] [--out F]

Per size, five things are timed in windows of ``iters`` back-to-back calls between two HIP events,
alternating, after a warm-up round: the two whole steps, the two clips alone and the Adam update
alone.  One JSON line per size reports the median and the spread of the per-call times and the
bytes each clip has to move.  The gradient is random with a norm above ``clip``.  The fused
step never rewrites it, so every call clips; the legacy clip scales its own copy in the first
call and multiplies by about 1 in every later one -- the same work either way.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bytes per parameter each clip moves: the norm pass reads g; the legacy clip reads g for the sum
# of squares, then reads and writes it in grad.mul_
CLIP_BYTES = {"norm_pass": 4, "legacy_clip": 12}
ADAM_BYTES = 30      # master r/w 8, g 4, m r/w 8, v r/w 8, bf16 shadow 2


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="25600000,110000000")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench: needs a GPU (a CPU timing says nothing about the kernels)")
    from distributedtensorflow_amd.optimizers import AdamOptimizer, clip_by_global_norm_
    from distributedtensorflow_amd.parallel import OneDeviceStrategy

    lines = []
    for n in (int(s) for s in args.sizes.split(",")):
        opts = {}
        for name in ("fused", "legacy"):
            p = torch.nn.Parameter(torch.zeros(n, 1, device="cuda"))
            p._dtf_name = "w/kernel"
            opt = AdamOptimizer(1e-3, clip_norm=args.clip if name == "fused" else None)
            with OneDeviceStrategy("/gpu:0").scope():
                sp = opt.build([p])
            sp.grad.normal_(std=1e-3)
            opts[name] = opt
        fused, legacy = opts["fused"], opts["legacy"]
        legacy.space.grad.copy_(fused.space.grad)
        whole = [(0, n)]

        def fused_step():
            fused.iterations += 1
            fused._apply(1.0)

        def legacy_step():
            clip_by_global_norm_(legacy.space, args.clip)
            legacy.iterations += 1
            legacy._apply(1.0)

        calls = {
            "fused_step": fused_step,
            "legacy_step": legacy_step,
            "norm_pass": lambda: fused._grad_norm_pass(1.0, whole),
            "legacy_clip": lambda: clip_by_global_norm_(legacy.space, args.clip),
            "adam_update": lambda: legacy._apply(1.0),
        }

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
        assert not fused.nonfinite_flag() and not legacy.nonfinite_flag()
        res = {"elements": n, "device": torch.cuda.get_device_name(0), "iters": args.iters,
               "rounds": args.rounds, "grad_norm": round(float(fused.last_grad_norm.item()), 6)}
        for k, ts in times.items():
            med = statistics.median(ts)
            res[k] = {"us_median": round(med, 2), "us_min": round(min(ts), 2),
                      "us_max": round(max(ts), 2)}
            if k in CLIP_BYTES:
                res[k]["bytes"] = CLIP_BYTES[k] * n
                res[k]["gb_per_s"] = round(CLIP_BYTES[k] * n / med / 1e3, 1)
            elif k == "adam_update":
                res[k]["bytes"] = ADAM_BYTES * n
                res[k]["gb_per_s"] = round(ADAM_BYTES * n / med / 1e3, 1)
        res["fused_over_legacy_step"] = round(res["fused_step"]["us_median"] /
                                              res["legacy_step"]["us_median"], 3)
        res["norm_pass_over_legacy_clip"] = round(res["norm_pass"]["us_median"] /
                                                  res["legacy_clip"]["us_median"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del opts, fused, legacy, calls
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
