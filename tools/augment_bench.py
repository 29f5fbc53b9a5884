#!/usr/bin/env python
"""Time the fused augmentation kernel, a torch composition of the same transform, and a
ResNet-50 training step fed by it.

    python tools/augment_bench.py                 # kernel vs torch, three shapes
    python tools/augment_bench.py --resnet50      # step time: DeviceImageDataset vs synthetic

Kernel arms (B = 1984, bf16 output, ImageNet channel statistics), run in ONE process,
alternating call by call, timed with device events after a warm-up of every shape:
  (a) ops.augment_images: gather + crop + bilinear resize + flip + normalise, one launch;
  (b) torch: index_select, affine grid + grid_sample (bilinear, half-pixel centres), flip through
      the grid, normalise, cast, to NHWC.  The comparator is for TIME only: it blends in floating
      point and samples past the box edge, so it is not bit-equal to (a).
Shapes: random-resized-crop of a 160 x 160 and of a 256 x 256 source to 224 x 224, and pad-crop
(pad 4) of a 32 x 32 source to 32 x 32.  Prints one JSON line per shape: median / min / p10 / p90
of each arm in microseconds and arm (a)'s effective GB/s over the bytes of the boxes read (the
part inside the image) plus the bytes written.

--resnet50: ResNet-50 training steps at --batch, 224 x 224, fed alternately by SyntheticImageNet
and by a DeviceImageDataset (random-resized-crop from 160 x 160), --rounds runs of --steps steps
each in the order S I S I ..., one model, one process.  Prints every run's ms / step, each
feed's median, and the spread (max - min) among the synthetic runs themselves.
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


def _torch_arm(images, idx, boxes, flip, mean, std, out_hw):
    """index_select + grid_sample + normalise: the same transform composed of torch ops."""
    Hs, Ws = images.shape[1:3]
    b = boxes.float()
    y0, x0, h, w = b.unbind(1)
    sx = torch.where(flip.bool(), -w, w) / Ws            # a negative x scale flips
    theta = torch.zeros(len(idx), 2, 3, device=images.device)
    theta[:, 0, 0] = sx
    theta[:, 0, 2] = (2 * x0 + w) / Ws - 1
    theta[:, 1, 1] = h / Hs
    theta[:, 1, 2] = (2 * y0 + h) / Hs - 1
    m = mean.view(1, 3, 1, 1)
    s = std.view(1, 3, 1, 1)

    def run():
        x = images.index_select(0, idx).permute(0, 3, 1, 2).float()
        grid = torch.nn.functional.affine_grid(theta, (len(idx), 3) + tuple(out_hw),
                                               align_corners=False)
        y = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="border",
                                            align_corners=False)
        return ((y / 255.0 - m) / s).to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
    return run


def bench_kernels(calls, warmup, B):
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.data import ImageAugment
    from distributedtensorflow_amd.data import images as dimg
    shapes = [("rrc_160_to_224", 160, 224, 4096, "rrc"), ("rrc_256_to_224", 256, 224, 4096, "rrc"),
              ("pad_crop_32_to_32", 32, 32, 50000, "pad_crop")]
    lut = ImageAugment(224, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD).lut(
        3, torch.bfloat16, "cuda")
    mean = torch.tensor(dimg.IMAGENET_MEAN, device="cuda")
    std = torch.tensor(dimg.IMAGENET_STD, device="cuda")
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
        sink = {}

        def new():
            sink["x"] = ops.augment_images(images, idx, boxes, flip, lut, (O, O))

        tarm = _torch_arm(images, idx, boxes, flip, mean, std, (O, O))

        def old():
            sink["y"] = tarm()

        res = _time_alternating({"augment_images": new, "torch_composition": old}, calls, warmup)
        y0, x0, h, w = boxes.long().unbind(1)
        ih = (torch.minimum(y0 + h, torch.tensor(S, device="cuda")) - y0.clamp(min=0)).clamp(min=0)
        iw = (torch.minimum(x0 + w, torch.tensor(S, device="cuda")) - x0.clamp(min=0)).clamp(min=0)
        read = int((ih * iw).sum()) * 3
        written = B * O * O * 3 * 2
        a = res["augment_images"]
        print(json.dumps({"shape": name, "B": B, "source": S, "out": O, "dtype": "bfloat16",
                          "calls_per_arm": calls, "box_bytes_read": read,
                          "bytes_written": written,
                          "new_GBps_at_median": round((read + written) / a["median_us"] / 1e3, 1),
                          **{f"{arm}.{m}": v for arm, st in res.items() for m, v in st.items()}}),
              flush=True)
        del images, sink


def bench_resnet50(batch, steps, rounds, warmup):
    import distributedtensorflow_amd as dtf
    from distributedtensorflow_amd import ops
    from distributedtensorflow_amd.data import DeviceImageDataset, ImageAugment
    from distributedtensorflow_amd.data import images as dimg
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    rng = np.random.RandomState(0)
    N, S = max(4096, 2 * batch), 160
    imgs = rng.randint(0, 256, (N, S, S, 3), dtype=np.uint8)
    labels = rng.randint(0, 1000, N)
    feeds = {
        "synthetic": dtf.data.SyntheticImageNet(batch, 224, device="cuda", pool=2),
        "device_images": DeviceImageDataset(
            imgs, labels, batch, "cuda",
            ImageAugment(224, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD), shuffle=True),
    }
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
    syn = runs["synthetic"]
    print(json.dumps({"model": "resnet50", "batch": batch, "image_size": 224, "source": S,
                      "steps_per_run": steps, "rounds": rounds, "order": "S I S I ...",
                      "ms_per_step_runs": runs, "ms_per_step_median": med,
                      "device_images_minus_synthetic_ms": round(
                          med["device_images"] - med["synthetic"], 3),
                      "synthetic_spread_ms": round(max(syn) - min(syn), 3)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calls", type=int, default=100, help="timed calls per arm (at least 50)")
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch", type=int, default=1984)
    p.add_argument("--resnet50", action="store_true",
                   help="ResNet-50 step time by feed instead of the kernel arms")
    p.add_argument("--steps", type=int, default=10, help="--resnet50: steps per timed run")
    p.add_argument("--rounds", type=int, default=4, help="--resnet50: runs per feed (at least 3)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: no GPU present")
    if args.resnet50:
        if args.rounds < 3:
            raise SystemExit("augment_bench: at least 3 runs per feed")
        bench_resnet50(args.batch, args.steps, args.rounds, max(1, min(args.warmup, 3)))
    else:
        if args.calls < 50:
            raise SystemExit("augment_bench: at least 50 timed calls per arm")
        bench_kernels(args.calls, args.warmup, args.batch)
    return 0


if __name__ == "__main__":
    sys.exit(main())
