"""Generation with the KV cache against the only alternative without it: re-running the padded
causal forward over the whole prefix for every token and taking its last row.

    python tools/generate_bench.py [--batch 8] [--prompt 64] [--new 128] [--rounds 3]

BERT-base, causal, greedy, random weights.  Both arms run in this process in alternation; one JSON
line with the median seconds and tokens per second of each, and the route the M = batch GEMMs of a
decode step take (``_dense_gemm_native``: the persistent MFMA GEMM, else ``F.linear``).

    python tools/generate_bench.py --sample [--rounds 3] [--new 128]

``--sample`` times the pick of the next token instead.  Per call: the fused ``ops.sample_tokens``
(csrc/kernels/sample.hip) on the padded [B, 30528] bf16 logits against ``_pick`` on their
``[:, :30522]`` slice copy (what ``generate`` without a seed runs per token), B = 8 and 64, the arms
alternating in one process, device events around 20 calls each, medians of 15 such windows.  End to
end: tokens per second of ``generate(seed=...)`` against ``generate(generator=...)`` at
temperature 0.8, top_k 50.  One JSON line per measurement.

    python tools/generate_bench.py --prefill_chunk 64 [--batch 8] [--rounds 3]

``--prefill_chunk T`` times the prefill of a 512-token prompt in one causal forward against
``prefill(chunk=T)`` (append attention, T tokens at a time), alternating in one process, with the
peak of ``torch.cuda.max_memory_allocated`` of each.

    python tools/generate_bench.py --decode_gemm skinny [--batch 64] [--shadows]

``--decode_gemm skinny`` times ``generate(decode_gemm="skinny")`` (csrc/kernels/dense_skinny.hip)
against plain ``generate`` instead of the recompute arm; ``--shadows`` first gives the weights the
bf16 shadows an optimizer build leaves, so neither arm casts its fp32 masters on every call.
``--decode_gemm skinny_ln`` times ``generate(decode_gemm="skinny_ln")`` (the layers' LayerNorms
deferred into the skinny kernel) against ``generate(decode_gemm="skinny")``, which then takes the
``kv_cache_*`` fields of the line.  ``--decode_gemm skinny_w8`` / ``skinny_ln_w8`` time the FP8-weight
form (csrc/kernels/dense_skinny_f8.hip; every call quantises the weights first, as ``generate``
does) against ``skinny`` / ``skinny_ln`` in the same way.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedtensorflow_amd import ops  # noqa: E402
from distributedtensorflow_amd.models import bert  # noqa: E402
from distributedtensorflow_amd.ops import native  # noqa: E402


def recompute(model, prompt, plen, n_new):
    """Greedy decoding at the parent's means: the causal forward over the prefix, padded to a
    multiple of 64, once per token."""
    B = prompt.shape[0]
    seq = torch.zeros(B, plen + n_new, dtype=torch.int64, device=prompt.device)
    seq[:, :plen] = prompt[:, :plen]
    with torch.no_grad():
        for t in range(n_new):
            n = plen + t
            S = -(-n // 64) * 64
            ids = torch.zeros(B, S, dtype=torch.int64, device=prompt.device)
            ids[:, :n] = seq[:, :n]
            seq[:, n] = model(ids).view(B, S, -1)[:, n - 1].argmax(-1)
    return seq[:, plen:]


def _med(v):
    return sorted(v)[len(v) // 2]


def sample_bench(a):
    V, ld, calls, windows = 30522, 30528, 20, 15
    gen = torch.Generator(device="cuda").manual_seed(0)
    for B in (8, 64):
        logits = torch.zeros(B, ld, device="cuda")
        logits[:, :V] = 3.0 * torch.randn(B, V, device="cuda", generator=gen)
        logits = logits.bfloat16()
        pos = torch.arange(B, device="cuda", dtype=torch.int32)
        for T, k, p in ((0.0, 0, 1.0), (0.8, 0, 1.0), (0.8, 50, 1.0), (0.8, 50, 0.9),
                        (0.8, 0, 0.9)):
            arms = {"fused": lambda: ops.sample_tokens(logits, 7, pos, T, k, p, V)}
            if p == 1.0:                                   # _pick has no top_p
                arms["pick"] = lambda: bert._pick(logits[:, :V], T, k, gen)
            us = {n: [] for n in arms}
            for w in range(windows + 1):                   # window 0 warms both arms up
                for n, fn in arms.items():
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    for _ in range(calls):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if w:
                        us[n].append(e0.elapsed_time(e1) * 1e3 / calls)
            rec = {"probe": "sample_pick", "B": B, "V": V, "temperature": T, "top_k": k, "top_p": p}
            for n in arms:
                rec[f"{n}_us"] = round(_med(us[n]), 2)
                rec[f"{n}_spread_us"] = [round(min(us[n]), 2), round(max(us[n]), 2)]
            print(json.dumps(rec), flush=True)
    torch.manual_seed(0)
    model = bert.bert_base(causal=True).cuda().eval()
    B, P = 8, 64
    prompt = torch.randint(1, V, (B, P), device="cuda")
    lens = torch.full((B,), P)
    arms = {"seeded": lambda: model.generate(prompt, lens, a.new, 0.8, 50, seed=7),
            "generator": lambda: model.generate(prompt, lens, a.new, 0.8, 50, generator=gen)}
    times = {n: [] for n in arms}
    for r in range(a.rounds + 1):
        for n, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[n].append(time.perf_counter() - t0)
    rec = {"probe": "generate_sampled", "model": "bert_base", "B": B, "prompt": P, "new": a.new,
           "temperature": 0.8, "top_k": 50, "rounds": a.rounds}
    for n in arms:
        rec[f"{n}_s"] = round(_med(times[n]), 4)
        rec[f"{n}_spread_s"] = [round(min(times[n]), 4), round(max(times[n]), 4)]
        rec[f"{n}_tokens_per_sec"] = round(B * a.new / _med(times[n]), 1)
    print(json.dumps(rec), flush=True)


def prefill_bench(a):
    """One-shot against chunked prefill of a 512-token prompt: median time and the peak of
    ``torch.cuda.max_memory_allocated`` above what is allocated before the call."""
    torch.manual_seed(0)
    model = bert.bert_base(causal=True).cuda().eval()
    B, P, T = a.batch, 512, a.prefill_chunk
    prompt = torch.randint(1, 30522, (B, P), device="cuda")
    lens = torch.full((B,), P)
    cache = bert.KVCache(model.cfg, B, P, "cuda")
    arms = {"one_shot": lambda: model.prefill(prompt, lens, cache),
            "chunked": lambda: model.prefill(prompt, lens, cache, chunk=T)}
    times, peak, outs = {k: [] for k in arms}, {}, {}
    for r in range(a.rounds + 1):                     # round 0 warms both arms up
        for k, fn in arms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            outs[k] = fn()
            torch.cuda.synchronize()
            if r:
                times[k].append(time.perf_counter() - t0)
                peak[k] = torch.cuda.max_memory_allocated() - base
    rec = {"probe": "prefill_chunk", "model": "bert_base", "B": B, "prompt": P, "chunk": T,
           "rounds": a.rounds,
           "same_argmax": float((outs["one_shot"].argmax(-1) == outs["chunked"].argmax(-1))
                                .float().mean())}
    for k in arms:
        rec[f"{k}_ms"] = round(_med(times[k]) * 1e3, 3)
        rec[f"{k}_spread_ms"] = [round(min(times[k]) * 1e3, 3), round(max(times[k]) * 1e3, 3)]
        rec[f"{k}_peak_MB"] = round(peak[k] / 2 ** 20, 1)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill_chunk", type=int, default=0, metavar="T",
                    help="time prefill(chunk=T) against the one-shot prefill of 512 tokens")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--kv_dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: generate(kv_dtype='fp8') against the bf16 cache instead of the "
                         "recompute arm; same_tokens is then the share of greedy tokens that agree")
    ap.add_argument("--decode_gemm",
                    choices=["default", "skinny", "skinny_ln", "skinny_w8", "skinny_ln_w8"],
                    default="default",
                    help="skinny: generate(decode_gemm='skinny') against the default GEMMs instead "
                         "of the recompute arm; skinny_ln: generate(decode_gemm='skinny_ln') "
                         "against the 'skinny' arm (kv_cache_* in the output is then that arm); "
                         "skinny_w8 / skinny_ln_w8: the FP8-weight form against 'skinny' / "
                         "'skinny_ln' (same_tokens is then the share of greedy tokens that agree)")
    ap.add_argument("--shadows", action="store_true",
                    help="give the weights bf16 shadows as an optimizer build does, so no GEMM of "
                         "either arm casts its fp32 master per call")
    a = ap.parse_args()
    if a.sample:
        return sample_bench(a)
    if a.prefill_chunk:
        return prefill_bench(a)
    if a.decode_gemm != "default" and a.kv_dtype == "fp8":
        raise SystemExit("--decode_gemm and --kv_dtype fp8 each replace the second arm")
    torch.manual_seed(0)
    model = bert.bert_base(causal=True).cuda().eval()
    if a.shadows:
        for p in model.parameters():
            if p.dim() == 2:
                p._dtf_shadow = p.detach().to(torch.bfloat16)
    B, P = a.batch, a.prompt
    Sp = -(-P // 64) * 64
    prompt = torch.zeros(B, Sp, dtype=torch.int64, device="cuda")
    prompt[:, :P] = torch.randint(1, 30522, (B, P), device="cuda")
    lens = torch.full((B,), P)
    arms = {"kv_cache": lambda: model.generate(prompt, lens, a.new),
            "recompute": lambda: recompute(model, prompt, P, a.new)}
    if a.kv_dtype == "fp8":
        arms["recompute"] = lambda: model.generate(prompt, lens, a.new, kv_dtype="fp8")
    second = {"fp8": "kv_cache_fp8"}.get(a.kv_dtype)
    if a.decode_gemm == "skinny":
        arms["recompute"] = lambda: model.generate(prompt, lens, a.new, decode_gemm="skinny")
        second = "kv_cache_skinny"
    if a.decode_gemm == "skinny_ln":                  # against the "skinny" arm, not the default
        arms["kv_cache"] = lambda: model.generate(prompt, lens, a.new, decode_gemm="skinny")
        arms["recompute"] = lambda: model.generate(prompt, lens, a.new, decode_gemm="skinny_ln")
        second = "kv_cache_skinny_ln"
    if a.decode_gemm.endswith("_w8"):                 # against the same GEMMs on bf16 weights
        base = a.decode_gemm[:-3]
        arms["kv_cache"] = lambda: model.generate(prompt, lens, a.new, decode_gemm=base)
        arms["recompute"] = lambda: model.generate(prompt, lens, a.new, decode_gemm=a.decode_gemm)
        second = "kv_cache_" + a.decode_gemm
    times = {k: [] for k in arms}
    outs = {}
    for r in range(a.rounds + 1):                     # round 0 warms both arms up
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[k] = fn()
            torch.cuda.synchronize()
            if r:
                times[k].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    cfg = model.cfg
    Hd, I = cfg.hidden_size, cfg.intermediate_size
    if second:                                        # the second arm is the FP8 cache / skinny GEMMs
        arms = {"kv_cache": None, second: None}
        times[second], outs[second] = times.pop("recompute"), outs["recompute"]
    rec = {"probe": "generate", "model": "bert_base", "B": B, "prompt": P, "new": a.new,
           "rounds": a.rounds, "kv_dtype": a.kv_dtype, "decode_gemm": a.decode_gemm,
           "shadows": a.shadows,
           "same_tokens": float((outs["kv_cache"] == outs["recompute"]).float().mean()),
           "decode_gemm_native": {f"{n}x{k}": bool(native._dense_gemm_native(B, n, k))
                                  for n, k in ((3 * Hd, Hd), (Hd, Hd), (I, Hd), (Hd, I))}}
    for k in arms:
        rec[f"{k}_s"] = round(med(times[k]), 4)
        rec[f"{k}_spread_s"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        rec[f"{k}_tokens_per_sec"] = round(B * a.new / med(times[k]), 1)
    if second:                                        # of the second arm over plain generate
        rec["speedup"] = round(med(times["kv_cache"]) / med(times[second]), 2)
    else:
        rec["speedup"] = round(med(times["recompute"]) / med(times["kv_cache"]), 2)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
