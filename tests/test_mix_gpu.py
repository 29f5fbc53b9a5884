"""Mixup / CutMix on the device: the mixing kernel (csrc/kernels/augment.hip,
dtf_augment_mix_images) bit for bit against ops/reference.py on the case table of
tests/test_mix.py (both store paths, both output dtypes, blocks that take several trips, partner
and example indices out of range), the two-label loss (csrc/kernels/loss.hip) against fp64, a GPU
DeviceImageDataset with a mix against the same dataset on the host, and training on mixed
batches, in process and through train.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import DeviceImageDataset, ImageAugment, ImageMix, MixedLabels
from distributedtensorflow_amd.data import images as dimg
from distributedtensorflow_amd.ops import native, reference
from test_mix import (B, OUT_HWS, TRAIN, XENT_SHAPES, _env, lut_of, mix_inputs, plans, rel,
                      write_set, xent_case)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
I32 = torch.int32


def _run_gpu(images, idx, boxes, flip, lut, out_hw, partner, lam_q, cut, fill=0, **kw):
    fn = native.augment_mix_images if kw else ops.augment_mix_images
    out = fn(images.cuda(), idx.cuda(), boxes.cuda(), flip.cuda(), lut.cuda(), out_hw,
             partner.cuda(), lam_q.cuda(), cut.cuda(), fill, **kw)
    assert out.is_cuda and out.dtype == lut.dtype and out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["vector", "tail"])
def test_kernel_equals_reference(dtype, C, out_hw):
    assert ((out_hw[1] * C) % 8 == 0) == (out_hw == (8, 8))      # the path the id names
    images, idx, boxes, flip = mix_inputs(C)
    lut = lut_of(C, dtype)
    for partner, lam_q, cut in plans(out_hw):
        want = reference.augment_mix_images(images, idx, boxes, flip, lut, out_hw, partner, lam_q,
                                            cut, fill=17)
        got = _run_gpu(images, idx, boxes, flip, lut, out_hw, partner, lam_q, cut, fill=17)
        assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("out_hw", [(16, 16), (15, 13)], ids=["vector", "tail"])
def test_unmixed_plan_equals_augment_images(dtype, out_hw):
    images, idx, boxes, flip = mix_inputs(3)
    lut = lut_of(3, dtype)
    plain = ops.augment_images(images.cuda(), idx.cuda(), boxes.cuda(), flip.cuda(), lut.cuda(),
                               out_hw, 17).cpu()
    partner = torch.tensor([4, 3, 2, 1, 0], dtype=I32)
    got = _run_gpu(images, idx, boxes, flip, lut, out_hw, partner,
                   torch.full((B,), 65536, dtype=I32), torch.zeros(B, 4, dtype=I32), fill=17)
    assert torch.equal(got, plain)
    got = _run_gpu(images, idx, boxes, flip, lut, out_hw, partner, torch.zeros(B, dtype=I32),
                   torch.zeros(B, 4, dtype=I32), fill=17)
    assert torch.equal(got, plain[partner.long()])


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("out_hw", [(16, 16), (15, 13)], ids=["vector", "tail"])
def test_several_trips_equal_the_default_launch(dtype, out_hw):
    nb, Hs, Ws, C = 64, 20, 24, 3
    Ho, Wo = out_hw
    g = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (10, Hs, Ws, C), generator=g, dtype=torch.uint8)
    idx = torch.randint(0, 10, (nb,), generator=g)
    boxes = dimg.rrc_boxes(torch.rand(nb, 10, 4, generator=g, dtype=torch.float64), Hs, Ws)
    boxes[::7, :2] -= 3                                    # some reach outside
    flip = (torch.rand(nb, generator=g) < 0.5).to(torch.uint8)
    lut = lut_of(C, dtype)
    # rows in turn: Mixup, CutMix (some boxes reaching outside), unmixed
    partner = torch.arange(nb - 1, -1, -1, dtype=I32)
    lam_q = torch.randint(0, 65537, (nb,), generator=g, dtype=I32)
    cut = torch.stack([torch.randint(-2, Ho, (nb,), generator=g),
                       torch.randint(-2, Wo, (nb,), generator=g),
                       torch.randint(1, Ho, (nb,), generator=g),
                       torch.randint(1, Wo, (nb,), generator=g)], dim=1).to(I32)
    kind = torch.arange(nb) % 3
    lam_q[kind != 0] = 65536
    cut[kind != 1] = 0
    want = reference.augment_mix_images(images, idx, boxes, flip, lut, out_hw, partner, lam_q,
                                        cut, fill=9)
    args = (images, idx, boxes, flip, lut, out_hw, partner, lam_q, cut)
    default = _run_gpu(*args, fill=9)
    three = _run_gpu(*args, fill=9, max_blocks=3)
    one = _run_gpu(*args, fill=9, max_blocks=1)
    assert torch.equal(default, want) and torch.equal(three, want) and torch.equal(one, want)


@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["vector", "tail"])
def test_indices_out_of_range_read_as_specified(out_hw):
    images, idx, boxes, flip = mix_inputs(3)
    lut = lut_of(3, BF16)
    N = images.shape[0]
    whole = [0, 0, out_hw[0], out_hw[1]]
    partner = torch.tensor([4, B, 2, -1, 0], dtype=I32)         # rows 1 and 3: no partner
    lam_q = torch.tensor([32768, 100, 0, 65536, 32768], dtype=I32)
    cut = torch.tensor([[0] * 4, whole, [0] * 4, whole, [1, 1, 3, 3]], dtype=I32)
    bad = torch.tensor([3, 0, 2, 1, N])                          # row 4 reads fill ...
    got = _run_gpu(images, bad, boxes, flip, lut, out_hw, partner, lam_q, cut, fill=17)
    # ... which is what an image of fill bytes gives, on either side of a mix
    filled = torch.cat([images, torch.full_like(images[:1], 17)])
    ok_partner = torch.tensor([4, 1, 2, 3, 0], dtype=I32)        # own partner: unmixed
    want = reference.augment_mix_images(filled, bad, boxes, flip, lut, out_hw, ok_partner, lam_q,
                                        cut, fill=17)
    assert torch.equal(got, want)
    plain = reference.augment_images(filled, bad, boxes, flip, lut, out_hw, fill=17)
    assert torch.equal(got[1], plain[1]) and torch.equal(got[3], plain[3])
    neg = torch.tensor([-1, 0, 2, 1, 3])
    got = _run_gpu(images, neg, boxes, flip, lut, out_hw, partner, lam_q, cut, fill=17)
    want = reference.augment_mix_images(filled, torch.tensor([N, 0, 2, 1, 3]), boxes, flip, lut,
                                        out_hw, ok_partner, lam_q, cut, fill=17)
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------- the loss

GPU_XENT_SHAPES = XENT_SHAPES + [(7, 30522)]


@pytest.mark.parametrize("ldt", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("nb,V", GPU_XENT_SHAPES, ids=[f"{b}x{v}" for b, v in GPU_XENT_SHAPES])
def test_two_label_loss_matches_fp64(nb, V, eps, ldt):
    x, a, b, lam, ref, ref_grad = xent_case(nb, V, eps)
    a, b, lam = a.to(ldt).cuda(), b.to(ldt).cuda(), lam.cuda()
    xn = x.cuda().requires_grad_()
    out = native.mixed_softmax_cross_entropy(xn, a, b, lam, eps)
    out.backward()
    assert abs(out.item() - ref.item()) < 1e-4 * max(1.0, abs(ref.item()))
    assert rel(xn.grad.cpu(), ref_grad) < 1e-5
    # a second run is bit-identical
    x2 = x.cuda().requires_grad_()
    out2 = ops.mixed_softmax_cross_entropy(x2, a, b, lam, eps)
    out2.backward()
    assert torch.equal(out2, out) and torch.equal(x2.grad, xn.grad)


def test_two_label_loss_upstream_gradient_and_single_label_limit():
    x, a, b, lam, _, ref_grad = xent_case(128, 1000, 0.1)
    xg, a, b, lam = x.cuda(), a.cuda(), b.cuda(), lam.cuda()
    xn = xg.clone().requires_grad_()
    (0.5 * ops.mixed_softmax_cross_entropy(xn, a, b, lam, 0.1)).backward()
    assert rel(xn.grad.cpu(), 0.5 * ref_grad) < 1e-5
    assert xn.grad.dtype == torch.float32
    # bf16 logits are upcast, and the gradient comes back in bf16
    xb = xg.to(BF16).requires_grad_()
    ops.mixed_softmax_cross_entropy(xb, a, b, lam, 0.1).backward()
    assert xb.grad.dtype == BF16 and bool(torch.isfinite(xb.grad).all())
    for eps in (0.0, 0.1):
        one = ops.sparse_softmax_cross_entropy(xg, a, eps).item()
        got = ops.mixed_softmax_cross_entropy(xg, a, b, torch.ones_like(lam), eps).item()
        assert abs(got - one) < 1e-4 * one
        mixed = ops.mixed_softmax_cross_entropy(xg, a, b, torch.full_like(lam, 0.3), eps).item()
        assert abs(mixed - one) > 1e-3


# ----------------------------------------------------------------------------- the dataset

@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_device_dataset_equals_the_cpu_dataset(mode):
    rng = np.random.RandomState(3)
    imgs = rng.randint(0, 256, (24, 12, 10, 3)).astype(np.uint8)
    labels = rng.randint(0, 10, 24)
    aug = ImageAugment((8, 8), mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3), fill=7)
    mix = ImageMix(mixup_alpha=0.4, cutmix_alpha=1.0, mode=mode)
    kw = dict(dtype=BF16, shuffle=False, seed=1, aug_seed=2, mix=mix, mix_seed=3)
    cpu = DeviceImageDataset(imgs, labels, 6, "cpu", aug, **kw)
    gpu = DeviceImageDataset(imgs, labels, 6, "cuda", aug, **kw)
    mixed = False
    for _ in range(6):                                     # over an epoch boundary
        xc, yc = next(cpu)
        xg, yg = next(gpu)
        assert isinstance(yg, MixedLabels) and xg.is_cuda and xg.dtype == BF16
        assert yg.lam.dtype == torch.float32 and yg.labels_b.dtype == yc.labels_b.dtype
        assert torch.equal(xg.cpu(), xc)
        assert all(torch.equal(g.cpu(), c) for g, c in zip(yg, yc))
        mixed |= bool((yc.lam < 1).any())
    assert mixed
    for (xc, yc), (xg, yg) in zip(cpu.single_pass(), gpu.single_pass()):
        assert torch.equal(xg.cpu(), xc) and torch.equal(yg.cpu(), yc)


# ----------------------------------------------------------------------------- end to end

def test_resnet50_trains_on_mixed_batches(tmp_path):
    from distributedtensorflow_amd.models import resnet50
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    rng = np.random.RandomState(0)
    imgs = rng.randint(0, 256, (32, 72, 72, 3)).astype(np.uint8)
    aug = ImageAugment(64, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD)
    train = DeviceImageDataset(imgs, rng.randint(0, 10, 32), 8, "cuda", aug, shuffle=True, seed=0,
                               aug_seed=1, mix=ImageMix(0.2, 1.0), mix_seed=2)
    torch.manual_seed(0)
    with OneDeviceStrategy("cuda").scope():
        model = resnet50(num_classes=10).cuda()
        opt = MomentumOptimizer(0.05, 0.9, weight_decay=1e-4)
        opt.build(list(model.parameters()))
        params = [p for p in model.parameters() if p.requires_grad]
        before = [p.detach().float().clone() for p in params]
        for _ in range(3):
            x, y = next(train)
            assert x.shape == (8, 64, 64, 3) and x.dtype == BF16 and isinstance(y, MixedLabels)
            loss = ops.mixed_softmax_cross_entropy(model(x), *y, 0.1)
            opt.minimize(loss)
            assert math.isfinite(float(loss))
        moved = [not torch.equal(p.detach().float(), q) for p, q in zip(params, before)]
    assert moved[0] and moved[-1] and sum(moved) > len(moved) // 2


def test_cli_trains_with_the_mixing_flags(tmp_path):
    d = str(tmp_path / "set")
    write_set(d)
    r = subprocess.run([sys.executable, TRAIN, "--model", "mnist_cnn", "--image_data", d,
                        "--augment", "pad_crop", "--batch_size", "32", "--train_steps", "3",
                        "--mixup_alpha", "0.2", "--cutmix_alpha", "1.0", "--log_dir",
                        str(tmp_path / "tb")],
                       capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["global_step"] == 3 and math.isfinite(res["final_loss"])
    assert res["mixup_alpha"] == 0.2 and res["cutmix_alpha"] == 1.0
