#!/usr/bin/env python
"""Time the fused masked-LM example kernel, the same rule composed of torch ops, and a BERT
training step fed by it.

    python tools/mlm_data_bench.py                 # kernel vs torch ops, two shapes
    python tools/mlm_data_bench.py --bert_base     # step time: DeviceTokenDataset vs synthetic

Kernel arms (uint16 tokens, a 1 GiB set so that rows come from HBM, random example indices), run
in ONE process, alternating call by call, timed with device events after a warm-up of every shape:
  (a) ops.mlm_mask_tokens: gather + masks + selection + replacement, six outputs, one launch;
  (b) reference.mlm_mask_tokens on the same device tensors: the same rule, bit for bit, as a
      composition of torch ops (hashes in int64, a sort for the selection, scatters for the slots);
  (c) ops.mlm_mask_tokens with a continuation table: the whole-word instantiation of the kernel
      on the same rows and indices.  The table flags the top 19 % of the ids (BERT's vocabulary
      holds 19 % of ## pieces), so a word is a random id below them and the flagged ids after it:
      1.23 tokens on average.  Checked against reference.mlm_mask_tokens before it is timed.
Shapes: B = 512, S = 128, P = 20 and B = 128, S = 512, P = 76.  The two arms' outputs are compared
before anything is timed.  Prints one JSON line per shape: median / min / p10 / p90 of each arm
in microseconds, arm (a)'s effective GB/s over the token bytes read plus the bytes written, and
arm (c)'s median over arm (a)'s.

--bert_base: BERT-base training steps at --batch, S = 128, P = 20, fed alternately by
SyntheticMLM, by a DeviceTokenDataset and by a DeviceTokenDataset with a continuation table
(whole-word masking), --rounds runs of --steps steps each in the order S T W S T W ..., one model,
one process.  Prints every run's ms / step, each feed's median, and the spread (max - min) among
the synthetic runs themselves.

Rows are [CLS] a [SEP] b [SEP] pad...; --short_prob of them have a random length 20..S and the
rest are full (create_pretraining_data.py's short_seq_prob, 0.1 there and here; 1.0 makes 42% of
all positions padding).  Needs a GPU: fails without one.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

KEYS = ("input_ids", "segment_ids", "input_mask", "masked_lm_positions", "masked_lm_ids",
        "masked_lm_weights")


def _stats(us):
    s = sorted(us)
    n = len(s)
    return {"median_us": round(s[n // 2], 1), "min_us": round(s[0], 1),
            "p10_us": round(s[n // 10], 1), "p90_us": round(s[(9 * n) // 10], 1)}


def _time_alternating(arms, calls, warmup):
    """``arms``: (name, fn) pairs, called in this order ``calls`` times over; a name that comes
    twice is one arm whose samples are pooled."""
    for _ in range(warmup):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k, _ in arms}
    for _ in range(calls):
        for k, fn in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: _stats([a.elapsed_time(b) * 1e3 for a, b in v]) for k, v in ev.items()}


def token_rows(N, S, masking, device, seed=1, shortest=20, short_prob=0.1):
    """[CLS] a [SEP] b [SEP] pad... rows -> int16 storage [N, S] on ``device`` (the ids stay below
    32768, so the reinterpretation is the identity).  A row is full with probability
    1 - short_prob, else of a random length shortest..S: create_pretraining_data.py's
    short_seq_prob, 0.1 by default there too."""
    g = torch.Generator(device=device).manual_seed(seed)
    assert masking.vocab_size <= 32768
    t = torch.randint(1000, masking.vocab_size, (N, S), device=device, generator=g,
                      dtype=torch.int32).to(torch.int16)
    L = torch.randint(shortest, S + 1, (N, 1), device=device, generator=g)
    L = torch.where(torch.rand(N, 1, device=device, generator=g) < short_prob, L,
                    torch.full_like(L, S))
    mid = 2 + (torch.rand(N, 1, device=device, generator=g) * (L - 4).float()).long()
    j = torch.arange(S, device=device).unsqueeze(0)
    t[:, 0] = masking.cls_id
    t = torch.where((j == mid) | (j == L - 1), torch.full_like(t, masking.sep_id), t)
    return torch.where(j >= L, torch.full_like(t, masking.pad_id), t).contiguous()


def continuation_table(masking, device, share=0.19):
    """uint8 [vocab_size] with the top ``share`` of the ids flagged as continuation pieces."""
    table = torch.zeros(masking.vocab_size, dtype=torch.uint8, device=device)
    table[int(masking.vocab_size * (1 - share)):] = 1
    return table


def bench_kernels(calls, warmup, set_bytes, short_prob):
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.data import TokenMasking
    from distributedtensorflow_amd.ops import reference
    m = TokenMasking()
    table = continuation_table(m, "cuda")
    for name, B, S, P in (("b512_s128_p20", 512, 128, 20), ("b128_s512_p76", 128, 512, 76)):
        N = set_bytes // (2 * S)
        tokens = token_rows(N, S, m, "cuda", short_prob=short_prob)
        g = torch.Generator(device="cuda").manual_seed(2)
        idx = torch.randint(0, N, (B,), device="cuda", generator=g)
        new_out = ops.mlm_mask_tokens(tokens, idx, 12345, P, m)
        old_out = reference.mlm_mask_tokens(tokens, idx, 12345, P, m)
        same = all(torch.equal(new_out[k], old_out[k]) for k in KEYS)
        if not same:
            raise SystemExit(f"mlm_data_bench: {name}: the kernel and the torch ops disagree")
        word_out = ops.mlm_mask_tokens(tokens, idx, 12345, P, m, continuation=table)
        word_ref = reference.mlm_mask_tokens(tokens, idx, 12345, P, m, continuation=table)
        if not all(torch.equal(word_out[k], word_ref[k]) for k in KEYS):
            raise SystemExit(f"mlm_data_bench: {name}: the whole-word kernel and the torch ops "
                             "disagree")
        filled = float(word_out["masked_lm_weights"].sum() / new_out["masked_lm_weights"].sum())
        sink = {}
        seeds = iter(range(1, 1 << 30))

        def new():
            sink["x"] = ops.mlm_mask_tokens(tokens, idx, next(seeds), P, m)

        def old():
            sink["y"] = reference.mlm_mask_tokens(tokens, idx, next(seeds), P, m)

        def words():
            sink["z"] = ops.mlm_mask_tokens(tokens, idx, next(seeds), P, m, continuation=table)

        # each kernel is timed right after a torch arm, as the token kernel always was: right
        # after the other kernel it measured 17 us lower at both shapes (profiles/MLM_DATA.md)
        res = _time_alternating([("mlm_mask_tokens", new), ("torch_composition", old),
                                 ("mlm_mask_words", words), ("torch_composition", old)],
                                calls, warmup)
        read, written = B * S * 2 + B * 8, 3 * B * S * 8 + B * P * 20
        a, t = res["mlm_mask_tokens"], res["torch_composition"]
        print(json.dumps({"shape": name, "B": B, "S": S, "P": P, "rows_in_set": N,
                          "storage": "uint16", "short_prob": short_prob,
                          "calls_per_arm": calls, "outputs_equal": same,
                          "bytes_read": read, "bytes_written": written,
                          "new_GBps_at_median": round((read + written) / a["median_us"] / 1e3, 1),
                          "torch_over_new_at_median": round(t["median_us"] / a["median_us"], 1),
                          "words_over_tokens_at_median": round(
                              res["mlm_mask_words"]["median_us"] / a["median_us"], 2),
                          "words_budget_filled": round(filled, 4),
                          **{f"{arm}.{k}": v for arm, st in res.items() for k, v in st.items()}}),
              flush=True)
        del tokens, sink, new_out, old_out, word_out, word_ref


def bench_bert_base(batch, steps, rounds, warmup, short_prob):
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd.data import DeviceTokenDataset, TokenMasking
    from distributedtensorflow_amd.models import bert
    from distributedtensorflow_amd.optimizers import LAMBOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    S, P, m = 128, 20, TokenMasking()
    rows = token_rows(max(65536, 2 * batch), S, m, "cpu",
                      short_prob=short_prob).numpy().view("uint16")
    feeds = {
        "synthetic": dtf.data.SyntheticMLM(batch, S, max_predictions=P, device="cuda"),
        "device_tokens": DeviceTokenDataset(rows, batch, "cuda", m, P, shuffle=True),
        "device_tokens_words": DeviceTokenDataset(
            rows, batch, "cuda", m, P, shuffle=True,
            continuation=continuation_table(m, "cpu").numpy()),
    }
    with OneDeviceStrategy("cuda").scope():
        model = bert.bert_base()
        opt = LAMBOptimizer(1e-4, weight_decay=0.01)
        opt.build(list(model.parameters()))

    def train_steps(data, n):
        for _ in range(n):
            b = next(data)
            w = b.get("masked_lm_weights")
            if w is None:
                w = torch.ones_like(b["masked_lm_ids"], dtype=torch.float32)
            opt.minimize(model(b["input_ids"], b["segment_ids"], b["input_mask"],
                               b["masked_lm_positions"], b["masked_lm_ids"], w))

    for data in feeds.values():
        train_steps(data, warmup)
    torch.cuda.synchronize()
    runs = {k: [] for k in feeds}
    for _ in range(rounds):
        for k, data in feeds.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            train_steps(data, steps)
            b.record()
            torch.cuda.synchronize()
            runs[k].append(round(a.elapsed_time(b) / steps, 3))
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    syn = runs["synthetic"]
    print(json.dumps({"model": "bert_base", "batch": batch, "seq_len": S, "max_predictions": P,
                      "short_prob": short_prob, "pad_share": round(float((rows == 0).mean()), 4),
                      "steps_per_run": steps, "rounds": rounds, "order": "S T W S T W ...",
                      "ms_per_step_runs": runs, "ms_per_step_median": med,
                      "device_tokens_minus_synthetic_ms": round(
                          med["device_tokens"] - med["synthetic"], 3),
                      "words_minus_device_tokens_ms": round(
                          med["device_tokens_words"] - med["device_tokens"], 3),
                      "synthetic_spread_ms": round(max(syn) - min(syn), 3)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calls", type=int, default=200, help="timed calls per arm (at least 50)")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--set_mb", type=int, default=1024, help="size of the resident token set")
    p.add_argument("--short_prob", type=float, default=0.1,
                   help="share of rows shorter than S (random length 20..S), the rest are full")
    p.add_argument("--bert_base", action="store_true",
                   help="BERT-base step time by feed instead of the kernel arms")
    p.add_argument("--batch", type=int, default=512, help="--bert_base: examples per step")
    p.add_argument("--steps", type=int, default=10, help="--bert_base: steps per timed run")
    p.add_argument("--rounds", type=int, default=4, help="--bert_base: runs per feed (at least 3)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlm_data_bench: no GPU present")
    if args.bert_base:
        if args.rounds < 3:
            raise SystemExit("mlm_data_bench: at least 3 runs per feed")
        bench_bert_base(args.batch, args.steps, args.rounds, max(1, min(args.warmup, 3)),
                        args.short_prob)
    else:
        if args.calls < 50:
            raise SystemExit("mlm_data_bench: at least 50 timed calls per arm")
        bench_kernels(args.calls, args.warmup, args.set_mb << 20, args.short_prob)
    return 0


if __name__ == "__main__":
    sys.exit(main())
