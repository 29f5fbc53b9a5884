#!/usr/bin/env python
"""Time Mixup / CutMix inside the augmentation kernel, the two-label loss, and a ResNet-50
training step fed with and without mixing.

    python tools/mix_bench.py                 # the image arms, three shapes
    python tools/mix_bench.py --loss          # two-label loss vs two single-label losses
    python tools/mix_bench.py --resnet50      # step time: DeviceImageDataset with / without a mix

Image arms (B = 1984, bf16 output, ImageNet channel statistics, the shapes of
tools/augment_bench.py), run in ONE process, alternating call by call, timed with device events
after a warm-up of every arm; row b's partner is row B - 1 - b:
  (a) ops.augment_images, the unmixed kernel;
  (b) ops.augment_mix_images, every row Mixup (lam_q uniform in [1, 65535], no box);
  (c) ops.augment_mix_images, every row CutMix at l = 0.5 (box sides floor(O sqrt(0.5)), centres
      uniform, clipped as the dataset clips them);
  (d) ops.augment_mix_images, no row mixed (lam_q = 65536, no box);
  (e) arm (a) followed by lam * x + (1 - lam) * x.flip(0) in torch: the two-pass alternative.
Prints one JSON line per shape: median / min / p10 / p90 of each arm in microseconds.  --arms a,d
times a subset, so that two arms alternate with nothing between them (an arm's time depends on
what the call before it left in the caches).

--loss: ops.mixed_softmax_cross_entropy against lam * loss(a) + (1 - lam) * loss(b) formed from
two ops.sparse_softmax_cross_entropy calls (one lam for the batch: the only form two mean losses
can express), forward and backward, fp32 logits [1984, 1000], label smoothing 0.1.

--resnet50: ResNet-50 training steps at --batch, 224 x 224, fed alternately by a
DeviceImageDataset without (P) and with (M) ImageMix(0.2, 1.0), --rounds runs of --steps steps
each in the order P M P M ..., one model, one process.  Prints every run's ms / step, each feed's
median, and the spread (max - min) among the unmixed runs themselves.
Needs a GPU: fails without one.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
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


def bench_images(calls, warmup, B, arms):
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.data import ImageAugment
    from distributedtensorflow_amd.data import images as dimg
    shapes = [("rrc_160_to_224", 160, 224, 4096, "rrc"), ("rrc_256_to_224", 256, 224, 4096, "rrc"),
              ("pad_crop_32_to_32", 32, 32, 50000, "pad_crop")]
    lut = ImageAugment(224, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD).lut(
        3, torch.bfloat16, "cuda")
    for name, S, O, N, mode in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        images = torch.randint(0, 256, (N, S, S, 3), device="cuda", generator=g, dtype=torch.uint8)
        idx = torch.randperm(N, device="cuda", generator=g)[:B]
        flip = (torch.rand(B, device="cuda", generator=g) < 0.5).to(torch.uint8)
        if mode == "rrc":
            u = torch.rand(B, 10, 4, device="cuda", generator=g, dtype=torch.float64)
            boxes = dimg.rrc_boxes(u, S, S)
        else:
            u = torch.rand(B, 2, device="cuda", generator=g, dtype=torch.float64)
            boxes = dimg.pad_crop_boxes(u, S, S, (O, O), 4)
        partner = torch.arange(B - 1, -1, -1, device="cuda", dtype=torch.int32)
        q_mix = torch.randint(1, 65536, (B,), device="cuda", generator=g, dtype=torch.int32)
        q_one = torch.full((B,), 65536, device="cuda", dtype=torch.int32)
        no_cut = torch.zeros(B, 4, device="cuda", dtype=torch.int32)
        side = int(math.floor(O * math.sqrt(0.5)))
        c = torch.randint(0, O, (B, 2), device="cuda", generator=g)
        lo, hi = (c - side // 2).clamp(0, O), (c + side // 2).clamp(0, O)
        cut = torch.cat([lo, hi - lo], dim=1).to(torch.int32)
        lam = (q_mix.float() / 65536.0).view(B, 1, 1, 1).to(torch.bfloat16)
        sink = {}

        def plain():
            sink["a"] = ops.augment_images(images, idx, boxes, flip, lut, (O, O))

        def mixed(lam_q, box, key):
            def run():
                sink[key] = ops.augment_mix_images(images, idx, boxes, flip, lut, (O, O), partner,
                                                   lam_q, box)
            return run

        def two_pass():
            x = ops.augment_images(images, idx, boxes, flip, lut, (O, O))
            sink["e"] = lam * x + (1 - lam) * x.flip(0)

        every = {"a_augment_images": plain, "b_mixup": mixed(q_mix, no_cut, "b"),
                 "c_cutmix": mixed(q_one, cut, "c"), "d_unmixed": mixed(q_one, no_cut, "d"),
                 "e_two_pass_torch": two_pass}
        res = _time_alternating({k: fn for k, fn in every.items() if k[0] in arms}, calls, warmup)
        same = bool(torch.equal(sink["a"], sink["d"])) if "a" in sink and "d" in sink else None
        print(json.dumps({"shape": name, "B": B, "source": S, "out": O, "dtype": "bfloat16",
                          "calls_per_arm": calls, "cut_side": side, "d_equals_a": same,
                          **{f"{arm}.{m}": v for arm, st in res.items() for m, v in st.items()}}),
              flush=True)
        del images, sink


def bench_loss(calls, warmup, B, V=1000):
    from distributedtensorflow_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    x = (3 * torch.randn(B, V, device="cuda", generator=g)).requires_grad_()
    a = torch.randint(0, V, (B,), device="cuda", generator=g)
    b = a.flip(0)
    lam_s = 0.3
    lam = torch.full((B,), lam_s, device="cuda")

    def pair():
        x.grad = None
        ops.mixed_softmax_cross_entropy(x, a, b, lam, 0.1).backward()

    def two_calls():
        x.grad = None
        (lam_s * ops.sparse_softmax_cross_entropy(x, a, 0.1) +
         (1 - lam_s) * ops.sparse_softmax_cross_entropy(x, b, 0.1)).backward()

    res = _time_alternating({"two_label_loss": pair, "two_single_label_losses": two_calls}, calls,
                            warmup)
    print(json.dumps({"B": B, "V": V, "dtype": "float32", "label_smoothing": 0.1,
                      "calls_per_arm": calls, "what": "forward + backward",
                      **{f"{arm}.{m}": v for arm, st in res.items() for m, v in st.items()}}),
          flush=True)


def bench_resnet50(batch, steps, rounds, warmup):
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.data import DeviceImageDataset, ImageAugment, ImageMix
    from distributedtensorflow_amd.data import images as dimg
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    rng = np.random.RandomState(0)
    N, S = max(4096, 2 * batch), 160
    imgs = rng.randint(0, 256, (N, S, S, 3), dtype=np.uint8)
    labels = rng.randint(0, 1000, N)
    aug = ImageAugment(224, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD)
    feeds = {"plain": DeviceImageDataset(imgs, labels, batch, "cuda", aug, shuffle=True),
             "mixed": DeviceImageDataset(imgs, labels, batch, "cuda", aug, shuffle=True,
                                         mix=ImageMix(0.2, 1.0))}
    del imgs
    with OneDeviceStrategy("cuda").scope():
        model = dtf.models.resnet50()
        opt = MomentumOptimizer(0.1, 0.9, weight_decay=1e-4)
        opt.build(list(model.parameters()))

    def train_steps(data, n):
        for _ in range(n):
            x, y = next(data)
            if isinstance(y, tuple):
                loss = ops.mixed_softmax_cross_entropy(model(x), *y)
            else:
                loss = ops.sparse_softmax_cross_entropy(model(x), y)
            opt.minimize(loss)

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
    pl = runs["plain"]
    print(json.dumps({"model": "resnet50", "batch": batch, "image_size": 224, "source": S,
                      "mix": "ImageMix(0.2, 1.0)", "steps_per_run": steps, "rounds": rounds,
                      "order": "P M P M ...", "ms_per_step_runs": runs, "ms_per_step_median": med,
                      "mixed_minus_plain_ms": round(med["mixed"] - med["plain"], 3),
                      "plain_spread_ms": round(max(pl) - min(pl), 3)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calls", type=int, default=100, help="timed calls per arm (at least 50)")
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch", type=int, default=1984)
    p.add_argument("--arms", default="a,b,c,d,e", help="the image arms to time (letters of a,b,c,d,e)")
    p.add_argument("--loss", action="store_true", help="the two-label loss instead of the images")
    p.add_argument("--resnet50", action="store_true",
                   help="ResNet-50 step time with / without mixing instead of the image arms")
    p.add_argument("--steps", type=int, default=10, help="--resnet50: steps per timed run")
    p.add_argument("--rounds", type=int, default=4, help="--resnet50: runs per feed (at least 3)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: no GPU present")
    if args.resnet50:
        if args.rounds < 3:
            raise SystemExit("mix_bench: at least 3 runs per feed")
        bench_resnet50(args.batch, args.steps, args.rounds, max(1, min(args.warmup, 3)))
    else:
        if args.calls < 50:
            raise SystemExit("mix_bench: at least 50 timed calls per arm")
        arms = args.arms.split(",")
        if not arms or set(arms) - set("abcde"):
            raise SystemExit("mix_bench: --arms takes letters of a,b,c,d,e")
        if args.loss:
            bench_loss(args.calls, args.warmup, args.batch)
        else:
            bench_images(args.calls, args.warmup, args.batch, arms)
    return 0


if __name__ == "__main__":
    sys.exit(main())
