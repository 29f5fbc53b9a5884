"""BERT attention kernels (csrc/kernels/nlp.hip) at the BERT-base b512 shape: time per call of
the forward and the backward (delta + dK/dV + dQ), with and without attention dropout, and the
max error of the dropout-free path against an fp32 PyTorch reference on a slice of the batch.

    python tools/attn_bench.py [--batch 512] [--seq 128] [--heads 12] [--iters 20]

``--causal`` times the causal kernels against the non-causal ones instead: S = 128, 256, 512 and
1024 at the batch that keeps B * S at ``--batch * --seq`` tokens, dropout off and at 0.1, both
variants in this process in alternation (``--rounds`` rounds of ``--iters`` calls each); one JSON
line per (S, dropout) with the median and the min-max spread of each and their ratio next to the
share of 64 x 64 tiles a causal kernel visits, (n + 1) / (2 n) at n = S / 64.  The non-causal
side is what the op runs: at S = 128 the fused backward, with the keep bits under dropout.

``--decode`` times the incremental-decoding kernel (csrc/kernels/attn_decode.hip) instead: one
query per sequence against a cache of ``len`` keys for B in {1, 8, 64} and len in {128, 512, 2048},
with the launcher's own ``splits`` and with ``splits = 1``, both arms in this process in
alternation; every call takes the next of a ring of caches (512 MB in all, at most 64), so that
the larger shapes stream from HBM rather than from a cache that one call has just filled.  One
JSON line per shape: median time, spread, the bytes the algorithm must move (K and V once,
``2 * len * 128 * B * H``, plus the fp32 partials written and read back) and bytes / time.

``--append`` times the append-attention kernels (csrc/kernels/attn_append.hip): T in {8, 16, 64,
128} new tokens that bring a cache to ``len`` keys, same B, len and cache ring.  Arms, alternating
in this process: ``attention_append`` with the launcher's ``splits``; T successive
``attention_decode`` calls; the causal forward over all ``len`` tokens (what a caller without the
kernel recomputes); and at B = 1 explicit ``splits`` 1 / 2 / 4 / 8, the evidence for the split
threshold.  One JSON line per shape with the median and spread of each arm in microseconds.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedtensorflow_amd.ops import native  # noqa: E402

_K = native.kernels()


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def causal_main(a):
    H, D, dev = a.heads, 64, "cuda"
    tokens = a.batch * a.seq
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    scale = D ** -0.5
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for S in (128, 256, 512, 1024):
        B = max(1, tokens // S)
        g = torch.Generator(device=dev).manual_seed(S)
        qkv = (torch.randn(B * S, 3 * H * D, device=dev, generator=g) * 0.5).to(torch.bfloat16)
        mask = torch.zeros(B, S, device=dev)
        mask[:, S - 8:] = -10000.0
        do = torch.randn(B * S, H * D, device=dev, generator=g).to(torch.bfloat16)
        out = torch.empty(B * S, H * D, device=dev, dtype=torch.bfloat16)
        lse = torch.empty(B, H, S, device=dev)
        delta = torch.empty_like(lse)
        dqkv = torch.empty_like(qkv)
        for p in (0.0, 0.1):
            nk = _K.attn_keep_words(B, S, H, p)
            keep = torch.empty(max(nk, 1), device=dev, dtype=torch.int32)
            kp = keep.data_ptr() if nk else 0

            def fwd(c):
                _K.attn_fwd(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S,
                            H, scale, p, 1234, st(), 0 if c else kp, c)

            def bwd(c):
                _K.attn_bwd(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), do.data_ptr(),
                            lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, S, H, scale, p,
                            1234, st(), 0, 0 if c else kp, c)

            t = {(k, c): [] for k in ("fwd", "bwd") for c in (0, 1)}
            for _ in range(a.rounds):
                for c in (0, 1):
                    t["fwd", c].append(timeit(lambda: fwd(c), a.iters))
                for c in (0, 1):                     # (out / lse are this variant's: fwd first)
                    fwd(c)
                    t["bwd", c].append(timeit(lambda: bwd(c), a.iters))
            n = S // 64
            rec = {"probe": "attn_causal", "B": B, "S": S, "H": H, "dropout": p,
                   "rounds": a.rounds, "iters": a.iters, "tile_share": round((n + 1) / (2 * n), 4)}
            for k in ("fwd", "bwd"):
                for c, name in ((0, "full"), (1, "causal")):
                    v = t[k, c]
                    rec[f"{k}_{name}_ms"] = round(med(v), 4)
                    rec[f"{k}_{name}_spread"] = [round(min(v), 4), round(max(v), 4)]
                rec[f"{k}_ratio"] = round(med(t[k, 1]) / med(t[k, 0]), 4)
            print(json.dumps(rec), flush=True)


def _f8_ring(kc, vc):
    """The bf16 cache ring as FP8 caches -> (k bytes, k scales, v bytes, v scales)."""
    from distributedtensorflow_amd.ops import reference
    k8, ks = reference.kv_quantize_rows(kc)
    v8, vs = reference.kv_quantize_rows(vc)
    return k8.contiguous(), ks.contiguous(), v8.contiguous(), vs.contiguous()


def decode_main(a):
    H, dev = a.heads, "cuda"
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for B in (1, 8, 64):
        for n in (128, 512, 2048):
            kv_bytes = 2 * n * 128 * B * H
            ring = max(2, min(64, (512 << 20) // kv_bytes))
            g = torch.Generator(device=dev).manual_seed(n + B)
            kc = (torch.randn(ring, B, H, n, 64, device=dev, generator=g) * 0.5).to(torch.bfloat16)
            vc = torch.randn(ring, B, H, n, 64, device=dev, generator=g).to(torch.bfloat16)
            new = (torch.randn(B, 3 * H * 64, device=dev, generator=g) * 0.5).to(torch.bfloat16)
            pos = torch.full((B,), n - 1, device=dev, dtype=torch.int32)
            out = torch.empty(B, H * 64, device=dev, dtype=torch.bfloat16)
            auto = _K.attn_decode_splits(B, H, n)
            ws = torch.empty(max(1, _K.attn_decode_ws_floats(B, H, auto)), device=dev)
            turn = [0]

            def call(splits):
                i = turn[0] = (turn[0] + 1) % ring
                _K.attn_decode(new.data_ptr(), pos.data_ptr(), kc[i].data_ptr(), vc[i].data_ptr(),
                               out.data_ptr(), ws.data_ptr(), B, H, n, n, splits, 0.125, st())

            if a.kv_dtype == "fp8":
                # the same ring as an FP8 cache (68 bytes a row), alternating with the bf16 one
                k8, ks, v8, vs = _f8_ring(kc, vc)

                def call8(splits):
                    i = turn[0] = (turn[0] + 1) % ring
                    _K.attn_decode_f8(new.data_ptr(), pos.data_ptr(), k8[i].data_ptr(),
                                      v8[i].data_ptr(), ks[i].data_ptr(), vs[i].data_ptr(),
                                      out.data_ptr(), ws.data_ptr(), B, H, n, n, splits, 0.125,
                                      st())

                t = {"bf16": [], "fp8": []}
                for _ in range(a.rounds):
                    t["bf16"].append(timeit(lambda: call(auto), a.iters))
                    t["fp8"].append(timeit(lambda: call8(auto), a.iters))
                rec = {"probe": "attn_decode_f8", "B": B, "H": H, "len": n, "ring": ring,
                       "rounds": a.rounds, "iters": a.iters, "splits_auto": auto}
                for k, row in (("bf16", 128), ("fp8", 68)):
                    moved = 2 * n * row * B * H + (2 * 4 * B * H * auto * 66 if auto > 1 else 0)
                    rec[f"{k}_us"] = round(med(t[k]) * 1e3, 2)
                    rec[f"{k}_spread_us"] = [round(min(t[k]) * 1e3, 2), round(max(t[k]) * 1e3, 2)]
                    rec[f"{k}_GBps"] = round(moved / (med(t[k]) * 1e-3) / 1e9, 1)
                rec["speedup"] = round(med(t["bf16"]) / med(t["fp8"]), 3)
                print(json.dumps(rec), flush=True)
                continue
            arms = {"auto": auto, "one": 1}
            t = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, sp in arms.items():
                    t[k].append(timeit(lambda: call(sp), a.iters))
            rec = {"probe": "attn_decode", "B": B, "H": H, "len": n, "ring": ring,
                   "rounds": a.rounds, "iters": a.iters, "splits_auto": auto}
            for k, sp in arms.items():
                moved = kv_bytes + (2 * 4 * B * H * sp * 66 if sp > 1 else 0)
                rec[f"{k}_us"] = round(med(t[k]) * 1e3, 2)
                rec[f"{k}_spread_us"] = [round(min(t[k]) * 1e3, 2), round(max(t[k]) * 1e3, 2)]
                rec[f"{k}_bytes"] = moved
                rec[f"{k}_GBps"] = round(moved / (med(t[k]) * 1e-3) / 1e9, 1)
            print(json.dumps(rec), flush=True)


def append_main(a):
    H, dev = a.heads, "cuda"
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for B in (1, 8, 64):
        for n in (128, 512, 2048):
            kv_bytes = 2 * n * 128 * B * H
            ring = max(2, min(64, (512 << 20) // kv_bytes))
            g = torch.Generator(device=dev).manual_seed(n + B)
            kc = (torch.randn(ring, B, H, n, 64, device=dev, generator=g) * 0.5).to(torch.bfloat16)
            vc = torch.randn(ring, B, H, n, 64, device=dev, generator=g).to(torch.bfloat16)
            qkv = (torch.randn(B * n, 3 * H * 64, device=dev, generator=g) * 0.5).to(torch.bfloat16)
            lse = torch.empty(B * H * n, device=dev)
            f8 = _f8_ring(kc, vc) if a.kv_dtype == "fp8" else None
            for T in (8, 16, 64, 128):
                new = qkv.view(B, n, -1)[:, n - T:]
                steps = new.transpose(0, 1).contiguous()            # [T, B, 3*H*64]
                new = new.reshape(B * T, -1).contiguous()
                pos = torch.full((B,), n - T, device=dev, dtype=torch.int32)
                pos_t = [pos + i for i in range(T)]
                out = torch.empty(B * n, H * 64, device=dev, dtype=torch.bfloat16)
                auto = _K.attn_append_splits(B, H, T, n)
                dsp = _K.attn_decode_splits(B, H, n)
                ws = torch.empty(max(1, _K.attn_append_ws_floats(B, H, T, max(auto, 8)),
                                     _K.attn_decode_ws_floats(B, H, dsp)), device=dev)
                turn = [0]

                def append(splits):
                    i = turn[0] = (turn[0] + 1) % ring
                    _K.attn_append(new.data_ptr(), pos.data_ptr(), 0, kc[i].data_ptr(),
                                   vc[i].data_ptr(), out.data_ptr(), ws.data_ptr(), B, T, H, n, n,
                                   splits, 0.125, st())

                def decode():
                    i = turn[0] = (turn[0] + 1) % ring
                    for t in range(T):
                        _K.attn_decode(steps[t].data_ptr(), pos_t[t].data_ptr(), kc[i].data_ptr(),
                                       vc[i].data_ptr(), out.data_ptr(), ws.data_ptr(), B, H, n, n,
                                       dsp, 0.125, st())

                def forward():                                       # n % 64 == 0: it fits
                    _K.attn_fwd(qkv.data_ptr(), 0, out.data_ptr(), lse.data_ptr(), B, n, H, 0.125,
                                0.0, 1234, st(), 0, 1)

                arms = {"append": lambda: append(auto), "decode_x_T": decode,
                        "causal_forward": forward}
                if a.kv_dtype == "fp8":                              # fp8 against bf16 only
                    def append8():
                        i = turn[0] = (turn[0] + 1) % ring
                        _K.attn_append_f8(new.data_ptr(), pos.data_ptr(), 0, f8[0][i].data_ptr(),
                                          f8[2][i].data_ptr(), f8[1][i].data_ptr(),
                                          f8[3][i].data_ptr(), out.data_ptr(), ws.data_ptr(), B, T,
                                          H, n, n, auto, 0.125, st())
                    arms = {"append": arms["append"], "append_fp8": append8}
                # the split threshold's evidence: explicit splits at the launch-bound batch
                explicit = () if f8 is not None else (1, 2, 4, 8) if B == 1 else (1,)
                for sp in explicit:
                    if sp != auto and sp <= n // 64:
                        arms[f"append_splits{sp}"] = lambda sp=sp: append(sp)
                t = {k: [] for k in arms}
                for _ in range(a.rounds):
                    for k, fn in arms.items():
                        t[k].append(timeit(fn, a.iters))
                rec = {"probe": "attn_append", "B": B, "H": H, "T": T, "len": n, "ring": ring,
                       "rounds": a.rounds, "iters": a.iters, "splits_auto": auto}
                for k in arms:
                    rec[f"{k}_us"] = round(med(t[k]) * 1e3, 2)
                    rec[f"{k}_spread_us"] = [round(min(t[k]) * 1e3, 2), round(max(t[k]) * 1e3, 2)]
                print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", action="store_true",
                    help="time the incremental-decoding kernel (see above)")
    ap.add_argument("--append", action="store_true",
                    help="time the append-attention kernel against its alternatives (see above)")
    ap.add_argument("--kv_dtype", choices=["bf16", "fp8"], default="bf16",
                    help="--decode / --append: fp8 times the FP8-cache kernels against the bf16 "
                         "ones on the same ring, arms alternating")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--causal", action="store_true",
                    help="time the causal kernels against the non-causal ones (see above)")
    ap.add_argument("--rounds", type=int, default=5, help="--causal / --decode: alternation rounds")
    a = ap.parse_args()
    if a.causal:
        return causal_main(a)
    if a.decode:
        return decode_main(a)
    if a.append:
        return append_main(a)
    B, S, H, D = a.batch, a.seq, a.heads, 64
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(B * S, 3 * H * D, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    mask = torch.zeros(B, S, device=dev)
    mask[:, S - 8:] = -10000.0
    do = torch.randn(B * S, H * D, device=dev, generator=g).to(torch.bfloat16)
    out = torch.empty(B * S, H * D, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, device=dev)
    delta = torch.empty_like(lse)
    dqkv = torch.empty_like(qkv)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    scale = D ** -0.5
    flops_f = 4.0 * B * H * S * S * D
    # dropout runs with and without the forward's stored keep decisions (attn_keep_words)
    for p, use_keep in ((0.0, False), (0.1, False), (0.1, True)):
        nk = _K.attn_keep_words(B, S, H, p) if use_keep else 0
        if use_keep and not nk:
            continue
        keep = torch.empty(max(nk, 1), device=dev, dtype=torch.int32)
        kp = keep.data_ptr() if nk else 0
        fwd = lambda: _K.attn_fwd(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), lse.data_ptr(),  # noqa: E731
                                  B, S, H, scale, p, 1234, st(), kp)
        bwd = lambda: _K.attn_bwd(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), do.data_ptr(),  # noqa: E731
                                  lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, S, H,
                                  scale, p, 1234, st(), 0, kp)
        tf = timeit(fwd, a.iters)
        tb = timeit(bwd, a.iters)
        if p > 0.0:
            # same keep decisions either way: the backward's outputs are bit-identical
            fwd()
            bwd()
            torch.cuda.synchronize()
            if not use_keep:
                ref_dqkv = dqkv.clone()
        rec = {"probe": "attn", "B": B, "S": S, "H": H, "dropout": p, "keep_bits": use_keep,
               "fwd_ms": round(tf, 4),
               "bwd_ms": round(tb, 4), "fwd_tflops": round(flops_f / tf / 1e9, 1),
               "bwd_tflops": round(2.5 * flops_f / tb / 1e9, 1)}
        if p == 0.0:
            # fp32 reference on the first 8 sequences
            n = 8
            q3 = qkv[: n * S].float().view(n, S, 3, H, D)
            q, k, v = (q3[:, :, i].permute(0, 2, 1, 3).requires_grad_(True) for i in range(3))
            s = (q @ k.transpose(-1, -2)) * scale + mask[:n, None, None, :]
            o = torch.softmax(s, -1) @ v
            o2 = o.permute(0, 2, 1, 3).reshape(n * S, H * D)
            o2.backward(do[: n * S].float())
            rec["fwd_max_err"] = float((out[: n * S].float() - o2.detach()).abs().max())
            dq3 = dqkv[: n * S].float().view(n, S, 3, H, D)
            for i, t in enumerate((q, k, v)):
                ref = t.grad.permute(0, 2, 1, 3)
                rec["d%s_max_rel" % "qkv"[i]] = float((dq3[:, :, i] - ref).abs().max()
                                                       / ref.abs().max())
        if use_keep:
            rec["dqkv_bit_identical_to_rehash"] = bool(torch.equal(dqkv, ref_dqkv))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
