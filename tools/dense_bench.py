"""The GEMMs of one decode step, each on its own: the skinny-M weight-streaming kernel
(csrc/kernels/dense_skinny.hip) against the route the step takes today.

    python tools/dense_bench.py [--rounds 5] [--iters 50] [--ms 1,8,16,64] [--splits 1,2,3,4,6]

BERT-base's four layer GEMMs and the 30528 x 768 vocabulary GEMM of the head, M = 1, 8, 16, 64.
Arms, alternating in one process, device events around ``iters`` calls, medians of ``rounds``:
  parent  ops.dense(impl=BERT_GEMM) under no-grad with the GEMM's own bias (the FFN pair:
          ops.dense_gelu_dense without ``impl``), what decode_step runs by default;
  skinny  ops.dense(impl="skinny") (the FFN pair: dense_gelu_dense(impl="skinny")).
Every call takes the next of a ring of weight copies that together exceed the 256 MB last-level
cache, so the weights come from HBM; the weights carry bf16 shadows as after an optimizer build,
so no arm casts them.  One JSON line per (GEMM, M): microseconds of each arm and the skinny
kernel's GB/s over the weight bytes as a share of the 8 TB/s peak.  ``--splits`` adds the skinny
kernel at each forced K split (through the binding) to the line.

``--w8`` adds the arm ``skinny_w8``: the same calls on the FP8 pairs of the ring's weights
(``ops.weight_quantize_fp8``, csrc/kernels/dense_skinny_f8.hip).  The ring is then sized by the
FP8 bytes, half the bf16 bytes, so that both arms' weights exceed the last-level cache; the line
gains the arm's GB/s over ITS weight bytes (bytes and scales) and ``w8_speedup``, skinny / skinny_w8.

    python tools/dense_bench.py --tail [--ms 1,8,16,64]

``--tail`` times a whole layer from the attention output on instead, through the ops, the same
ring and windows: ``gemm="skinny"`` (5 launches) against ``gemm="skinny_ln"`` (3 launches, the
LayerNorms deferred into the skinny kernel); one JSON line per M.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedtensorflow_amd import ops  # noqa: E402
from distributedtensorflow_amd.models.bert import BERT_GEMM  # noqa: E402
from distributedtensorflow_amd.ops import native  # noqa: E402

PEAK_GBS = 8000.0
RING_BYTES = 320 << 20
# name, N, K, bias, or for the FFN pair the second GEMM's N
GEMMS = (("qkv", 2304, 768, True), ("attn_out", 768, 768, False), ("ffn_pair", 3072, 768, 768),
         ("ffn2", 768, 3072, False), ("vocab", 30528, 768, True))


def _weight(n, k, gen):
    w = torch.nn.Parameter(0.02 * torch.randn(n, k, device="cuda", generator=gen))
    w._dtf_shadow = w.detach().to(torch.bfloat16)
    return w


def _med(v):
    return sorted(v)[len(v) // 2]


def bench(name, N, K, extra, M, a, gen):
    pair = name == "ffn_pair"
    wbytes = 2 * N * K + (2 * extra * N if pair else 0)
    w8bytes = wbytes // 2 + wbytes // 32                   # a byte per weight, 4 per 64 of them
    ring = min(1024 if a.w8 else 512, -(-RING_BYTES // (w8bytes if a.w8 else wbytes)))
    ws = [_weight(N, K, gen) for _ in range(ring)]
    w2 = [_weight(extra, N, gen) for _ in range(ring)] if pair else None
    if a.w8:
        qs = [ops.weight_quantize_fp8(w) for w in ws]
        q2 = [ops.weight_quantize_fp8(w) for w in w2] if pair else None
    b = torch.randn(N, device="cuda", generator=gen) if (pair or extra) else None
    x = torch.randn(M, K, device="cuda", generator=gen).bfloat16()
    if pair:
        arms = {"parent": lambda i: ops.dense_gelu_dense(x, ws[i], b, w2[i]),
                "skinny": lambda i: ops.dense_gelu_dense(x, ws[i], b, w2[i], impl="skinny")}
    else:
        arms = {"parent": lambda i: ops.dense(x, ws[i], b, impl=BERT_GEMM),
                "skinny": lambda i: ops.dense(x, ws[i], b, impl="skinny")}
        for s in a.splits:
            if s <= K // 64:
                arms[f"skinny_splits{s}"] = (
                    lambda i, s=s: native._dense_skinny(x, ws[i], b, splits=s))
    if a.w8 and pair:
        arms["skinny_w8"] = lambda i: ops.dense_gelu_dense(x, qs[i], b, q2[i], impl="skinny")
    elif a.w8:
        arms["skinny_w8"] = lambda i: ops.dense(x, qs[i], b, impl="skinny")
    us = {k: [] for k in arms}
    with torch.no_grad():
        for r in range(a.rounds + 1):                          # round 0 warms every arm up
            for k, fn in arms.items():
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                for i in range(a.iters):
                    fn((r * a.iters + i) % ring)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    us[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        same = float((arms["parent"](0).float() - arms["skinny"](0).float()).abs().max())
        if a.w8:
            same8 = float((arms["skinny"](0).float() - arms["skinny_w8"](0).float()).abs().max())
    rec = {"probe": "dense_skinny", "gemm": name, "M": M, "N": N, "K": K, "ring": ring,
           "ring_MB": round(ring * wbytes / 2 ** 20), "max_abs_diff": round(same, 4),
           "auto_splits": native._K.dense_skinny_splits(M, N, K)}
    for k in arms:
        rec[f"{k}_us"] = round(_med(us[k]), 2)
        rec[f"{k}_spread_us"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
    gbs = wbytes / (_med(us["skinny"]) * 1e-6) / 1e9
    rec["skinny_weight_GBs"] = round(gbs)
    rec["skinny_share_of_peak"] = round(gbs / PEAK_GBS, 3)
    rec["speedup"] = round(_med(us["parent"]) / _med(us["skinny"]), 2)
    if a.w8:
        gbs = w8bytes / (_med(us["skinny_w8"]) * 1e-6) / 1e9
        rec["skinny_w8_weight_GBs"] = round(gbs)
        rec["skinny_w8_share_of_peak"] = round(gbs / PEAK_GBS, 3)
        rec["w8_speedup"] = round(_med(us["skinny"]) / _med(us["skinny_w8"]), 2)
        rec["w8_max_abs_diff"] = round(same8, 4)
    print(json.dumps(rec), flush=True)


def bench_tail(M, a, gen, H=768, I=3072, eps=1e-12):
    """A BERT-base layer from the attention output on, arms alternating: "skinny" (output
    projection, bias + residual + LayerNorm kernel, FFN pair, LayerNorm kernel: 5 launches)
    against "skinny_ln" (the LayerNorms deferred into the GEMMs: 3 launches)."""
    ring = min(512, -(-RING_BYTES // (2 * (H * H + 2 * H * I))))
    wo, w1, w2 = ([_weight(n, k, gen) for _ in range(ring)] for n, k in ((H, H), (I, H), (H, I)))
    vec = lambda n, at=0.0: at + 0.1 * torch.randn(n, device="cuda", generator=gen)  # noqa: E731
    bo, b1, b2 = vec(H), vec(I), vec(H)
    lns = [(vec(H, 1.0), vec(H), eps) for _ in range(3)]       # of the input, attention, output
    ctx, t = (torch.randn(M, H, device="cuda", generator=gen).bfloat16() for _ in range(2))

    def skinny(i):
        s = ops.dense(ctx, wo[i], None, impl="skinny")
        x1 = ops.bias_dropout_add_layer_norm(s, bo, xn, lns[1][0], lns[1][1], 0.0, False, eps)
        o = ops.dense_gelu_dense(x1, w1[i], b1, w2[i], impl="skinny")
        return ops.bias_dropout_add_layer_norm(o, b2, x1, lns[2][0], lns[2][1], 0.0, False, eps)

    def skinny_ln(i):
        t1 = ops.dense(ctx, wo[i], bo, impl="skinny", residual=t, residual_ln=lns[0])
        t2 = ops.dense_gelu_dense(t1, w1[i], b1, w2[i], impl="skinny", pre_ln=lns[1], b2=b2,
                                  residual=t1, residual_ln=lns[1])
        return t2

    arms = {"skinny": skinny, "skinny_ln": skinny_ln}
    us = {k: [] for k in arms}
    with torch.no_grad():
        xn = ops.layer_norm(t, *lns[0])                        # the parent arm's normalised input
        for r in range(a.rounds + 1):                          # round 0 warms every arm up
            for k, fn in arms.items():
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                for i in range(a.iters):
                    fn((r * a.iters + i) % ring)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    us[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        same =float((skinny(0).float() - ops.layer_norm(skinny_ln(0), *lns[2]).float())
                     .abs().max())
    rec = {"probe": "layer_tail", "M": M, "H": H, "I": I, "ring": ring,
           "max_abs_diff": round(same, 4)}
    for k in arms:
        rec[f"{k}_us"] = round(_med(us[k]), 2)
        rec[f"{k}_spread_us"] = [round(min(us[k]), 2), round(max(us[k]), 2)]
    rec["speedup"] = round(_med(us["skinny"]) / _med(us["skinny_ln"]), 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ms", default="1,8,16,64")
    ap.add_argument("--splits", default="", help="forced K splits to time as well, e.g. 1,2,4")
    ap.add_argument("--gemms", default=",".join(g[0] for g in GEMMS))
    ap.add_argument("--w8", action="store_true",
                    help="add the arm 'skinny_w8': the skinny kernel on FP8 weight pairs")
    ap.add_argument("--tail", action="store_true",
                    help="time a whole layer tail instead: 'skinny' against 'skinny_ln'")
    a = ap.parse_args()
    a.splits = [int(s) for s in a.splits.split(",") if s]
    if not torch.cuda.is_available():
        raise SystemExit("dense_bench needs a GPU")
    gen = torch.Generator(device="cuda").manual_seed(0)
    if a.tail:
        for M in (int(m) for m in a.ms.split(",")):
            bench_tail(M, a, gen)
        return
    for name, N, K, extra in GEMMS:
        if name in a.gemms.split(","):
            for M in (int(m) for m in a.ms.split(",")):
                bench(name, N, K, extra, M, a, gen)


if __name__ == "__main__":
    main()
