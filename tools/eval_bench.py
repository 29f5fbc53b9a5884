#!/usr/bin/env python
"""Time the evaluation kernels against what the training ops offer for the same three numbers.

    python tools/eval_bench.py                    # kernel arms at the BERT and ResNet shapes
    python tools/eval_bench.py --resnet50         # train.evaluate vs training step, images/s

Arms, run in ONE process, alternating call by call, timed with device events after a warm-up of
every shape:
  (a) ops.eval_rows + metrics_accumulate: loss, top-1 and top-k from one read of the logits;
  (b) the training loss op under no_grad (mlm_loss for the bf16 BERT logits,
      sparse_softmax_cross_entropy for the fp32 ResNet logits) plus torch.topk on the logits and
      the comparison with the labels.
Shapes: BERT evaluation logits bf16 N = 10240, V = 30522, ld = 30528 (the [:, :V] view);
ResNet logits fp32 (what the model emits) N = 1984, V = 1000.
Prints one JSON line per shape: median / min / p10 / p90 of each arm in microseconds and arm
(a)'s achieved bytes/s counted from one read of the logits.  Needs a GPU: fails without one.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _stats(us):
    s = sorted(us)
    n = len(s)
    return {"median_us": round(s[n // 2], 1), "min_us": round(s[0], 1),
            "p10_us": round(s[n // 10], 1), "p90_us": round(s[(9 * n) // 10], 1)}


def _time_alternating(arms, calls, warmup):
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in arms}
    for _ in range(calls):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: _stats([a.elapsed_time(b) * 1e3 for a, b in v]) for k, v in ev.items()}


def bench_kernels(calls, warmup, k):
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.ops import native
    shapes = [("bert_logits", torch.bfloat16, 10240, 30522, 30528),
              ("resnet_logits", torch.float32, 1984, 1000, 1000)]
    for name, dtype, N, V, ld in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        full = (torch.randn(N, ld, device="cuda", generator=g) * 3).to(dtype)
        logits = full[:, :V]
        labels = torch.randint(0, V, (N,), device="cuda", generator=g)
        weights = torch.ones(N, device="cuda")
        state = torch.zeros(4, dtype=torch.float64, device="cuda")
        sink = {}

        def new():
            rows, rank = ops.eval_rows(logits, labels)
            native.metrics_accumulate(state, rows, rank, None, k)

        def old():
            with torch.no_grad():
                if dtype == torch.bfloat16:
                    sink["loss"] = ops.mlm_loss(full, labels, weights, vocab=V)
                else:
                    sink["loss"] = ops.sparse_softmax_cross_entropy(logits, labels)
                top = torch.topk(logits, k, dim=1).indices
                hit = top == labels.unsqueeze(1)
                sink["top_1"] = hit[:, 0].sum()
                sink["top_k"] = hit.any(1).sum()

        res = _time_alternating({"eval_rows+accumulate": new, "loss_op+topk": old}, calls, warmup)
        nbytes = N * V * full.element_size()
        a = res["eval_rows+accumulate"]
        print(json.dumps({"shape": name, "dtype": str(dtype).replace("torch.", ""), "N": N,
                          "V": V, "ld": ld, "k": k, "calls_per_arm": calls,
                          "logit_bytes": nbytes,
                          "new_GBps_at_median": round(nbytes / a["median_us"] / 1e3, 1),
                          **{f"{arm}.{m}": v for arm, st in res.items() for m, v in st.items()}}),
              flush=True)
        del full, logits


def bench_resnet50(batch, steps, warmup):
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    data = dtf.data.SyntheticImageNet(batch, 224, device="cuda", pool=1)
    with OneDeviceStrategy("cuda").scope():
        model = dtf.models.resnet50()
        opt = MomentumOptimizer(0.1, 0.9, weight_decay=1e-4)
        opt.build(list(model.parameters()))

    def train_steps(n):
        for _ in range(n):
            x, y = next(data)
            opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y))

    def eval_steps(n):
        return dtf.train.evaluate(model, data.single_pass(n),
                                  dtf.metrics.ClassificationMetrics(k=5), optimizer=opt)

    out = {"model": "resnet50", "batch": batch, "steps": steps}
    for name, fn in (("train", train_steps), ("evaluate", eval_steps)):
        fn(warmup)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(steps)
        b.record()
        torch.cuda.synchronize()
        out[f"{name}_images_per_s"] = round(steps * batch / (a.elapsed_time(b) / 1e3), 1)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calls", type=int, default=100, help="timed calls per arm (at least 50)")
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--k", type=int, default=5)
    p.add_argument("--resnet50", action="store_true",
                   help="train.evaluate vs the training step at --batch instead of the kernel arms")
    p.add_argument("--batch", type=int, default=1984)
    p.add_argument("--steps", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU present")
    if args.calls < 50:
        raise SystemExit("eval_bench: at least 50 timed calls per arm")
    if args.resnet50:
        bench_resnet50(args.batch, args.steps, max(1, min(args.warmup, 2)))
    else:
        bench_kernels(args.calls, args.warmup, args.k)
    return 0


if __name__ == "__main__":
    sys.exit(main())
