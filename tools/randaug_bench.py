#!/usr/bin/env python
"""Time RandAugment inside the augmentation kernel, next to the two kernels it extends, and a
ResNet-50 training step fed with and without it.

    python tools/randaug_bench.py                 # the image arms at B = 256 and 1984
    python tools/randaug_bench.py --resnet50      # step time: DeviceImageDataset with / without

Image arms (160 x 160 x 3 -> 224 x 224 bf16, random-resized-crop boxes, ImageNet channel
statistics), run in ONE process, alternating call by call, timed with device events after a
warm-up of every arm; row b's partner is row B - 1 - b:
  (a) ops.augment_images, the plain kernel;
  (b) ops.augment_mix_images, every row Mixup (lam_q uniform in [1, 65535], no box);
  (c) ops.augment_rand_images under ImageRandAugment()'s default plan (two layers, m9, mstd 0.5,
      prob 0.5: about 2 rows in 5 carry a map, about 2 in 5 a pointwise op), no partner;
  (d) arm (c) with arm (b)'s mix;
  (e) ops.augment_rand_images with the all-identity plan (every row on the separable path);
  (f) arm (e) with arm (b)'s mix;
  (g) ops.augment_rand_images with every row rotated and two pointwise ops: the slowest plan.
Prints one JSON line per batch size: median / min / p10 / p90 of each arm in microseconds, the
output-write bound (B * 224 * 224 * 3 * 2 bytes at --hbm_gbs, the achievable HBM rate) and
whether (e) equals (a) and (f) equals (b) bit for bit.  --arms a,e times a subset, so that two
arms alternate with nothing between them.

--resnet50: ResNet-50 training steps at --batch, 224 x 224, fed alternately by a
DeviceImageDataset without (P) and with (R) ImageRandAugment(), --rounds runs of --steps steps
each in the order P R P R ..., one model, one process.  Prints every run's ms / step, each feed's
median, and the spread (max - min) among the plain runs themselves.
Needs a GPU: fails without one.
"""
import argparse
import json
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


def bench_images(calls, warmup, batches, arms, hbm_gbs, S=160, O=224, N=4096):
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.data import ImageAugment, ImageRandAugment, randaugment_plan
    from distributedtensorflow_amd.data import images as dimg
    lut = ImageAugment(O, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD).lut(
        3, torch.bfloat16, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    images = torch.randint(0, 256, (N, S, S, 3), device="cuda", generator=g, dtype=torch.uint8)
    for B in batches:
        idx = torch.randint(0, N, (B,), device="cuda", generator=g)
        flip = (torch.rand(B, device="cuda", generator=g) < 0.5).to(torch.uint8)
        boxes = dimg.rrc_boxes(torch.rand(B, 10, 4, device="cuda", generator=g,
                                          dtype=torch.float64), S, S)
        partner = torch.arange(B - 1, -1, -1, device="cuda", dtype=torch.int32)
        q_mix = torch.randint(1, 65536, (B,), device="cuda", generator=g, dtype=torch.int32)
        no_cut = torch.zeros(B, 4, device="cuda", dtype=torch.int32)
        mix = (partner, q_mix, no_cut)
        cpu = torch.Generator().manual_seed(2)
        ra = ImageRandAugment()
        default = tuple(t.cuda() for t in randaugment_plan(*ra.draw(B, cpu), (O, O), ra))
        every = ImageRandAugment(num_layers=3, prob=1.0, ops=("rotate", "color", "brightness"))
        u, z = every.draw(B, cpu)
        u[:, :, 0] = torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64)     # one of each
        slowest = tuple(t.cuda() for t in randaugment_plan(u, z, (O, O), every))
        ident = (torch.tensor([[65536, 0, 0, 0, 65536, 0]], dtype=torch.int32,
                              device="cuda").repeat(B, 1),
                 torch.zeros(B, 2, dtype=torch.int32, device="cuda"),
                 torch.zeros(B, 2, dtype=torch.int32, device="cuda"))
        sink = {}

        def plain():
            sink["a"] = ops.augment_images(images, idx, boxes, flip, lut, (O, O))

        def mixed():
            sink["b"] = ops.augment_mix_images(images, idx, boxes, flip, lut, (O, O), *mix)

        def rand(plan, m, key):
            def run():
                sink[key] = ops.augment_rand_images(images, idx, boxes, flip, lut, (O, O), *plan,
                                                    *m)
            return run

        every_arm = {"a_augment_images": plain, "b_mixup": mixed,
                     "c_rand_default": rand(default, (), "c"),
                     "d_rand_default_mixup": rand(default, mix, "d"),
                     "e_rand_identity": rand(ident, (), "e"),
                     "f_rand_identity_mixup": rand(ident, mix, "f"),
                     "g_rand_rotate_all": rand(slowest, (), "g")}
        res = _time_alternating({k: fn for k, fn in every_arm.items() if k[0] in arms}, calls,
                                warmup)

        def same(x, y):
            return bool(torch.equal(sink[x], sink[y])) if x in sink and y in sink else None

        mapped = int((default[0] != ident[0][:1]).any(1).sum())
        pointwise = int((default[1] != 0).any(1).sum())
        out_bytes = B * O * O * 3 * 2
        print(json.dumps({"B": B, "source": S, "out": O, "dtype": "bfloat16",
                          "calls_per_arm": calls, "rows_with_a_map": mapped,
                          "rows_with_a_pointwise_op": pointwise,
                          "output_write_bound_us": round(out_bytes / (hbm_gbs * 1e3), 1),
                          "e_equals_a": same("a", "e"), "f_equals_b": same("b", "f"),
                          **{f"{arm}.{m}": v for arm, st in res.items() for m, v in st.items()}}),
              flush=True)
        del sink


def bench_resnet50(batch, steps, rounds, warmup):
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.data import DeviceImageDataset, ImageAugment, ImageRandAugment
    from distributedtensorflow_amd.data import images as dimg
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    rng = np.random.RandomState(0)
    N, S = max(4096, 2 * batch), 160
    imgs = rng.randint(0, 256, (N, S, S, 3), dtype=np.uint8)
    labels = rng.randint(0, 1000, N)
    aug = ImageAugment(224, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD)
    feeds = {"plain": DeviceImageDataset(imgs, labels, batch, "cuda", aug, shuffle=True),
             "rand": DeviceImageDataset(imgs, labels, batch, "cuda", aug, shuffle=True,
                                        rand=ImageRandAugment())}
    del imgs
    with OneDeviceStrategy("cuda").scope():
        model = dtf.models.resnet50()
        opt = MomentumOptimizer(0.1, 0.9, weight_decay=1e-4)
        opt.build(list(model.parameters()))

    def train_steps(data, n):
        for _ in range(n):
            x, y = next(data)
            opt.minimize(ops.sparse_softmax_cross_entropy(model(x), y))

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
                      "rand": "ImageRandAugment()", "steps_per_run": steps, "rounds": rounds,
                      "order": "P R P R ...", "ms_per_step_runs": runs, "ms_per_step_median": med,
                      "rand_minus_plain_ms": round(med["rand"] - med["plain"], 3),
                      "plain_spread_ms": round(max(pl) - min(pl), 3)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calls", type=int, default=100, help="timed calls per arm (at least 50)")
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batches", default="256,1984", help="the image arms' batch sizes")
    p.add_argument("--arms", default="a,b,c,d,e,f,g", help="the image arms to time")
    p.add_argument("--hbm_gbs", type=float, default=6300.0,
                   help="HBM rate of the output-write bound, GB/s")
    p.add_argument("--resnet50", action="store_true",
                   help="ResNet-50 step time with / without RandAugment instead of the image arms")
    p.add_argument("--batch", type=int, default=1984, help="--resnet50: the batch size")
    p.add_argument("--steps", type=int, default=10, help="--resnet50: steps per timed run")
    p.add_argument("--rounds", type=int, default=4, help="--resnet50: runs per feed (at least 3)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench: no GPU present")
    if args.resnet50:
        if args.rounds < 3:
            raise SystemExit("randaug_bench: at least 3 runs per feed")
        bench_resnet50(args.batch, args.steps, args.rounds, max(1, min(args.warmup, 3)))
    else:
        if args.calls < 50:
            raise SystemExit("randaug_bench: at least 50 timed calls per arm")
        arms = args.arms.split(",")
        if not arms or set(arms) - set("abcdefg"):
            raise SystemExit("randaug_bench: --arms takes letters of a,b,c,d,e,f,g")
        bench_images(args.calls, args.warmup, [int(b) for b in args.batches.split(",")], arms,
                     args.hbm_gbs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
