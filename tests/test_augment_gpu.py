"""The augmentation kernel (csrc/kernels/augment.hip) against ops/reference.py on the CPU, bit
for bit: both store paths (16-B vector stores where Wo * C % 8 == 0, the scalar tail otherwise),
both output dtypes, blocks that take several trips, image offsets past 2 GiB, the
DeviceImageDataset on the device against the same dataset on the host, and two ResNet-50
training steps plus an evaluation fed by it."""
import math

import numpy as np
import pytest
import torch

import distributedtensorflow_amd as dtf
from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import DeviceImageDataset, ImageAugment
from distributedtensorflow_amd.data import images as dimg
from distributedtensorflow_amd.metrics import ClassificationMetrics
from distributedtensorflow_amd.ops import native, reference

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _lut(C, dtype):
    return ImageAugment(4, mean=(0.485, 0.456, 0.406)[:C], std=(0.229, 0.224, 0.225)[:C]).lut(
        C, dtype, "cpu")


def _run_gpu(images, idx, boxes, flip, lut, out_hw, fill=0, **kw):
    fn = native.augment_images if kw else ops.augment_images
    out = fn(images.cuda(), idx.cuda(), boxes.cuda(), flip.cuda(), lut.cuda(), out_hw, fill, **kw)
    assert out.is_cuda and out.dtype == lut.dtype and out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", [(8, 8), (5, 7)], ids=["vector", "tail"])
def test_kernel_equals_reference(dtype, C, out_hw):
    Hs, Ws = 12, 10
    Ho, Wo = out_hw
    assert ((Wo * C) % 8 == 0) == (out_hw == (8, 8))      # the path the id names
    g = torch.Generator().manual_seed(100 * C + Ho)
    images = torch.randint(0, 256, (4, Hs, Ws, C), generator=g, dtype=torch.uint8)
    lut = _lut(C, dtype)
    idx = torch.tensor([3, 0, 3, 1, 2])                   # repeated and unordered
    boxes = torch.tensor([[1, 2, Ho, Wo],                 # identity: the output's size
                          [0, 0, Hs, Ws],                 # downscale
                          [2, 3, 3, 4],                   # upscale
                          [-2, -2, Hs + 4, Ws + 4],       # 2 pixels outside on every side
                          [5, 6, 1, 1]], dtype=torch.int32)
    for flips in ([1, 0, 1, 0, 1], [0, 1, 0, 1, 0]):
        flip = torch.tensor(flips, dtype=torch.uint8)
        want = reference.augment_images(images, idx, boxes, flip, lut, out_hw, fill=17)
        got = _run_gpu(images, idx, boxes, flip, lut, out_hw, fill=17)
        assert torch.equal(got, want)
    # the identity box is a copy through the table
    copy = lut[torch.arange(C).view(1, 1, C), images[3, 1:1 + Ho, 2:2 + Wo].long()]
    assert torch.equal(got[0], copy)


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("out_hw", [(16, 16), (15, 13)], ids=["vector", "tail"])
def test_several_trips_equal_the_default_launch(dtype, out_hw):
    B, Hs, Ws, C = 64, 20, 24, 3
    g = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (10, Hs, Ws, C), generator=g, dtype=torch.uint8)
    idx = torch.randint(0, 10, (B,), generator=g)
    u = torch.rand(B, 10, 4, generator=g, dtype=torch.float64)
    boxes = dimg.rrc_boxes(u, Hs, Ws)
    boxes[::7, :2] -= 3                                    # some reach outside
    flip = (torch.rand(B, generator=g) < 0.5).to(torch.uint8)
    lut = _lut(C, dtype)
    want = reference.augment_images(images, idx, boxes, flip, lut, out_hw, fill=9)
    default = _run_gpu(images, idx, boxes, flip, lut, out_hw, fill=9)
    capped = _run_gpu(images, idx, boxes, flip, lut, out_hw, fill=9, max_blocks=2)
    one = _run_gpu(images, idx, boxes, flip, lut, out_hw, fill=9, max_blocks=1)
    assert torch.equal(default, want) and torch.equal(capped, want) and torch.equal(one, want)


def test_addressing_past_2_gib():
    Hs, Ws = 256, 1 << 20
    images = torch.empty(9, Hs, Ws, 1, dtype=torch.uint8, device="cuda")    # 2.25 GiB
    assert images.numel() > (1 << 31)
    g = torch.Generator(device="cuda").manual_seed(1)
    for row in (0, 8):
        images[row].copy_(torch.randint(0, 256, (Hs, Ws, 1), generator=g, dtype=torch.uint8,
                                        device="cuda"))
    small = torch.stack([images[0], images[8]]).cpu()
    idx = torch.tensor([8, 0])
    boxes = torch.tensor([[Hs - 20, Ws - 30, 20, 30],      # the last bytes of row 8: past 2 GiB
                          [Hs - 5, Ws - 9, 12, 20]],       # row 0's far corner, reaching outside
                         dtype=torch.int32)
    assert 8 * Hs * Ws + (Hs - 20) * Ws > (1 << 31)
    flip = torch.tensor([0, 1], dtype=torch.uint8)
    for dtype, out_hw in ((BF16, (8, 8)), (torch.float32, (5, 7))):
        lut = _lut(1, dtype)
        want = reference.augment_images(small, torch.tensor([1, 0]), boxes, flip, lut, out_hw,
                                        fill=3)
        got = ops.augment_images(images, idx.cuda(), boxes.cuda(), flip.cuda(), lut.cuda(),
                                 out_hw, fill=3).cpu()
        assert torch.equal(got, want)
    del images
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode,dtype", [("random_resized_crop", torch.float32),
                                        ("random_resized_crop", BF16), ("pad_crop", BF16)])
def test_device_dataset_equals_the_cpu_dataset(mode, dtype):
    """The crop boxes (float64 on the device against float64 on the host), the flips and the
    kernel: a GPU dataset's batches are the CPU dataset's."""
    rng = np.random.RandomState(3)
    imgs = rng.randint(0, 256, (23, 12, 10, 3)).astype(np.uint8)
    labels = rng.randint(0, 10, 23)
    aug = ImageAugment((8, 8), mode=mode, mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3), fill=7)
    kw = dict(dtype=dtype, seed=1, aug_seed=2)
    cpu = DeviceImageDataset(imgs, labels, 6, "cpu", aug, **kw)
    gpu = DeviceImageDataset(imgs, labels, 6, "cuda", aug, chunk_bytes=5 * 360, **kw)
    assert gpu.images.is_cuda and torch.equal(gpu.images.cpu(), cpu.images)
    for _ in range(5):                                     # over an epoch boundary
        xc, yc = next(cpu)
        xg, yg = next(gpu)
        assert xg.is_cuda and xg.dtype == dtype and xg.shape == (6, 8, 8, 3)
        assert torch.equal(xg.cpu(), xc) and torch.equal(yg.cpu(), yc)
    for (xc, yc), (xg, yg) in zip(cpu.single_pass(), gpu.single_pass()):
        assert torch.equal(xg.cpu(), xc) and torch.equal(yg.cpu(), yc)
    # the boxes alone, at a size where rounding has many chances to differ
    u = torch.rand(4096, 10, 4, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    assert torch.equal(dimg.rrc_boxes(u.cuda(), 160, 144).cpu(), dimg.rrc_boxes(u, 160, 144))


def test_resnet50_trains_and_evaluates_on_an_image_set(tmp_path):
    from distributedtensorflow_amd.models import resnet50
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    rng = np.random.RandomState(0)
    for split, n in (("train", 32), ("val", 20)):
        np.save(tmp_path / f"{split}_images.npy", rng.randint(0, 256, (n, 72, 72, 3)).astype(np.uint8))
        np.save(tmp_path / f"{split}_labels.npy", rng.randint(0, 10, n))
    aug = ImageAugment(64, mean=dimg.IMAGENET_MEAN, std=dimg.IMAGENET_STD)
    train = DeviceImageDataset(*dimg.load_arrays(str(tmp_path), "train", 10), 8, "cuda", aug,
                               shuffle=True, seed=0, aug_seed=1)
    val = DeviceImageDataset(*dimg.load_arrays(str(tmp_path), "val", 10), 8, "cuda", aug)
    torch.manual_seed(0)
    with OneDeviceStrategy("cuda").scope():
        model = resnet50(num_classes=10).cuda()
        opt = MomentumOptimizer(0.05, 0.9, weight_decay=1e-4)
        opt.build(list(model.parameters()))
        for _ in range(2):
            x, y = next(train)
            assert x.shape == (8, 64, 64, 3) and x.dtype == BF16
            loss = ops.sparse_softmax_cross_entropy(model(x), y)
            opt.minimize(loss)
            assert math.isfinite(float(loss))
        res = dtf.train.evaluate(model, val.single_pass(), ClassificationMetrics(k=5),
                                 optimizer=opt)
    assert res["count"] == 20.0 and math.isfinite(res["loss"])
    assert 0.0 <= res["top_1"] <= res["top_k"] <= 1.0
