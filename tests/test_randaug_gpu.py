"""RandAugment on the device: the kernel (csrc/kernels/augment.hip, dtf_augment_rand_images) bit
for bit against ops/reference.py on the case table of tests/test_randaug.py (both store paths,
both output dtypes, with and without a partner), blocks that take several trips, several row
tiles and column chunks, the 1024 limit, indices out of range, the identity plan against the two
other kernels, an unknown op code, a GPU DeviceImageDataset with ``rand`` against the same
dataset on the host, and training on such batches, in process and through train.py."""
import functools
import json
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import (DeviceImageDataset, ImageAugment, ImageMix,
                                            ImageRandAugment, MixedLabels, randaugment_plan)
from distributedtensorflow_amd.data import images as dimg
from distributedtensorflow_amd.ops import native, reference
from test_randaug import (B, FILL, IDENTITY, OUT_HWS, RA_FILL, TRAIN, _env, cases, lut_of,
                          mix_plans, q16, rand_inputs, rand_plans, rotation, write_set)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
I32 = torch.int32


def _cuda(t):
    return None if t is None else t.cuda()


def _run_gpu(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, partner=None, lam_q=None,
             cut=None, fill=0, ra_fill=128, **kw):
    fn = native.augment_rand_images if kw else ops.augment_rand_images
    out = fn(images.cuda(), idx.cuda(), boxes.cuda(), flip.cuda(), lut.cuda(), out_hw, aff.cuda(),
             pops.cuda(), ppar.cuda(), _cuda(partner), _cuda(lam_q), _cuda(cut), fill, ra_fill,
             **kw)
    assert out.is_cuda and out.dtype == lut.dtype and out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["vector", "tail"])
def test_kernel_equals_reference(out_hw, C, dtype, mixed):
    assert ((out_hw[1] * C) % 8 == 0) == (out_hw == (16, 16))     # the path the id names
    images, idx, boxes, flip = rand_inputs(C)
    lut = lut_of(C, dtype)
    for plan in cases(C, out_hw, mixed):
        want = reference.augment_rand_images(images, idx, boxes, flip, lut, out_hw, *plan,
                                             fill=FILL, ra_fill=RA_FILL)
        got = _run_gpu(images, idx, boxes, flip, lut, out_hw, *plan, fill=FILL, ra_fill=RA_FILL)
        assert torch.equal(got, want)


def _random_case(nb, Hs, Ws, C, out_hw, seed, n_img=10, L=2):
    """A batch of nb rows under the default plan at prob 0.8 and, by turns, Mixup, CutMix (some
    boxes reaching outside) and no mix."""
    Ho, Wo = out_hw
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (n_img, Hs, Ws, C), generator=g, dtype=torch.uint8)
    idx = torch.randint(0, n_img, (nb,), generator=g)
    boxes = dimg.rrc_boxes(torch.rand(nb, 10, 4, generator=g, dtype=torch.float64), Hs, Ws)
    boxes[::7, :2] -= 3                                    # some reach outside
    flip = (torch.rand(nb, generator=g) < 0.5).to(torch.uint8)
    ra = ImageRandAugment(num_layers=L, prob=0.8)
    aff, pops, ppar = randaugment_plan(*ra.draw(nb, g), out_hw, ra)
    partner = torch.arange(nb - 1, -1, -1, dtype=I32)
    lam_q = torch.randint(0, 65537, (nb,), generator=g, dtype=I32)
    cut = torch.stack([torch.randint(-2, Ho, (nb,), generator=g),
                       torch.randint(-2, Wo, (nb,), generator=g),
                       torch.randint(1, Ho + 1, (nb,), generator=g),
                       torch.randint(1, Wo + 1, (nb,), generator=g)], dim=1).to(I32)
    kind = torch.arange(nb) % 3
    lam_q[kind != 0] = 65536
    cut[kind != 1] = 0
    return (images, idx, boxes, flip), (aff, pops, ppar), (partner, lam_q, cut)


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["vector", "tail"])
def test_several_trips_equal_the_default_launch(dtype, out_hw):
    data, plan, mix = _random_case(64, 20, 24, 3, out_hw, 5)
    lut = lut_of(3, dtype)
    for m in ((), mix):
        want = reference.augment_rand_images(*data, lut, out_hw, *plan, *m, fill=9, ra_fill=200)
        for kw in (dict(), dict(max_blocks=3), dict(max_blocks=1)):
            got = _run_gpu(*data, lut, out_hw, *plan, *m, fill=9, ra_fill=200, **kw)
            assert torch.equal(got, want), kw


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", [(40, 16), (5, 264), (3, 259)],
                         ids=["three_row_tiles", "two_chunks_vector", "two_chunks_tail"])
def test_several_tiles_and_chunks(out_hw, C):
    Ho, Wo = out_hw
    nb = 7
    data, (aff, pops, ppar), mix = _random_case(nb, 20, 24, C, out_hw, 6)
    # rows 0 .. 3: maps that carry pixels across the tile and chunk boundaries (a mirror, a
    # shift by most of a chunk, a rotation, a shear that sweeps the columns); row 4: the identity
    fixed = [q16(-1, 0, Wo, 0, -1, Ho), q16(1, 0, -200.5 if Wo > 256 else -3.5, 0, 1, 1.0),
             rotation(17.0, Ho, Wo), q16(1, 4.0, -8.0, 0.05, 1, 0), IDENTITY]
    aff[:5] = torch.tensor(fixed, dtype=I32)
    assert int((aff[5:] != torch.tensor(IDENTITY, dtype=I32)).any(1).sum()) > 0
    lut = lut_of(C, BF16)
    for m in ((), mix):
        want = reference.augment_rand_images(*data, lut, out_hw, aff, pops, ppar, *m, fill=9)
        for kw in (dict(), dict(max_blocks=2)):
            got = _run_gpu(*data, lut, out_hw, aff, pops, ppar, *m, fill=9, **kw)
            assert torch.equal(got, want), kw


@functools.lru_cache(maxsize=None)
def _limit_case():
    """B = 2 at Ho = Wo = 1024, the tables' length: a rotated row and its identity partner."""
    out_hw = (1024, 1024)
    images, idx, boxes, flip = rand_inputs(3)
    idx, boxes, flip = idx[:2], boxes[:2].clone(), flip[:2]
    aff = torch.tensor([rotation(-29.5, 1024, 1024), IDENTITY], dtype=I32)
    pops = torch.tensor([[6, 3], [2, 0]], dtype=I32)
    ppar = torch.tensor([[124518, 110], [77, 0]], dtype=I32)
    lut = lut_of(3, BF16)
    mix = (torch.tensor([1, 0], dtype=I32), torch.tensor([40000, 65536], dtype=I32),
           torch.tensor([[0, 0, 0, 0], [1000, 1000, 100, 100]], dtype=I32))
    args = (images, idx, boxes, flip, lut, out_hw, aff, pops, ppar)
    return args, mix, reference.augment_rand_images(*args, *mix, fill=FILL, ra_fill=RA_FILL)


def test_the_largest_output():
    args, mix, want = _limit_case()
    got = _run_gpu(*args, *mix, fill=FILL, ra_fill=RA_FILL)
    assert torch.equal(got, want)
    # B = 1, unmixed: row 0 alone, whose last rows and columns hold the rotation's fill
    one = tuple(t[:1] if i in (1, 2, 3, 6, 7, 8) else t for i, t in enumerate(args))
    got1 = _run_gpu(*one, fill=FILL, ra_fill=RA_FILL)
    want1 = reference.augment_rand_images(*one, fill=FILL, ra_fill=RA_FILL)
    assert torch.equal(got1, want1)
    with pytest.raises(ValueError):
        _run_gpu(*args[:5], (1025, 8), *args[6:])


@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["vector", "tail"])
def test_indices_out_of_range_read_as_specified(out_hw):
    images, idx, boxes, flip = rand_inputs(3)
    lut = lut_of(3, BF16)
    N = images.shape[0]
    aff, pops, ppar = rand_plans(out_hw)[-1]
    whole = [0, 0, out_hw[0], out_hw[1]]
    partner = torch.tensor([5, B, 3, -1, 1, 0], dtype=I32)        # rows 1 and 3: no partner
    lam_q = torch.tensor([32768, 100, 0, 65536, 20000, 32768], dtype=I32)
    cut = torch.tensor([[0] * 4, whole, [0] * 4, whole, [1, 1, 3, 3], [0] * 4], dtype=I32)
    # a bad index reads as fill through the virtual image, on either side of a mix: what an
    # image of fill bytes gives
    filled = torch.cat([images, torch.full_like(images[:1], FILL)])
    ok_partner = torch.tensor([5, 1, 3, 3, 1, 0], dtype=I32)      # own partner: unmixed
    for bad, seen in ((torch.tensor([3, 0, 9, 1, 3, N]), N), (torch.tensor([-1, 0, 9, 1, 3, 7]), 0),
                      (torch.tensor([3, N + 5, 9, 1, 3, 7]), 1)):
        got = _run_gpu(images, bad, boxes, flip, lut, out_hw, aff, pops, ppar, partner, lam_q,
                       cut, fill=FILL, ra_fill=RA_FILL)
        as_fill = bad.clone()
        as_fill[(bad < 0) | (bad >= N)] = N
        want = reference.augment_rand_images(filled, as_fill, boxes, flip, lut, out_hw, aff, pops,
                                             ppar, ok_partner, lam_q, cut, fill=FILL,
                                             ra_fill=RA_FILL)
        assert torch.equal(got, want)
        plain = _run_gpu(images, bad, boxes, flip, lut, out_hw, aff, pops, ppar, fill=FILL,
                         ra_fill=RA_FILL)
        assert torch.equal(plain, reference.augment_rand_images(
            filled, as_fill, boxes, flip, lut, out_hw, aff, pops, ppar, fill=FILL,
            ra_fill=RA_FILL))
        assert torch.equal(got[1], plain[1]) and torch.equal(got[3], plain[3])


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["vector", "tail"])
def test_identity_plan_equals_the_other_kernels(out_hw, C, dtype):
    images, idx, boxes, flip = rand_inputs(C)
    lut = lut_of(C, dtype)
    dev = [t.cuda() for t in (images, idx, boxes, flip, lut)]
    aff = torch.tensor([IDENTITY] * B, dtype=I32)
    plain = ops.augment_images(*dev, out_hw, FILL).cpu()
    for L in (1, 4):
        zeros = torch.zeros(B, L, dtype=I32)
        got = _run_gpu(images, idx, boxes, flip, lut, out_hw, aff, zeros, zeros, fill=FILL,
                       ra_fill=RA_FILL)
        assert torch.equal(got, plain)
        for partner, lam_q, cut in mix_plans(out_hw):
            want = ops.augment_mix_images(*dev, out_hw, partner.cuda(), lam_q.cuda(), cut.cuda(),
                                          FILL).cpu()
            got = _run_gpu(images, idx, boxes, flip, lut, out_hw, aff, zeros, zeros, partner,
                           lam_q, cut, fill=FILL, ra_fill=RA_FILL)
            assert torch.equal(got, want)


def test_unknown_op_code_acts_as_none_and_parameters_are_clamped():
    out_hw = (16, 16)
    images, idx, boxes, flip = rand_inputs(3)
    lut = lut_of(3, BF16)
    aff, pops, ppar = rand_plans(out_hw)[-1]
    pops = pops.clone()
    pops[:, 1] = torch.tensor([7, -1, 100, 1 << 30, -(1 << 31), 9], dtype=I32)
    ppar = ppar.clone()
    ppar[:, 1] = torch.tensor([5, -5, 1 << 30, -(1 << 31), 255, 0], dtype=I32)
    none = pops.clone()
    none[:, 1] = 0
    zero = ppar.clone()
    zero[:, 1] = 0
    want = reference.augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff, none, zero,
                                         fill=FILL, ra_fill=RA_FILL)
    got = _run_gpu(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, fill=FILL,
                   ra_fill=RA_FILL)
    assert torch.equal(got, want)
    # a parameter outside its range acts as the nearest end of the range
    codes = torch.tensor([[2, 2, 3, 3, 5, 6]], dtype=I32).T.contiguous()
    wild = torch.tensor([[-9, 1 << 30, -(1 << 31), 1 << 20, (1 << 31) - 1, -1]], dtype=I32).T
    ends = torch.tensor([[0, 256, 0, 128, 1 << 18, 0]], dtype=I32).T.contiguous()
    want = reference.augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff, codes, ends,
                                         fill=FILL, ra_fill=RA_FILL)
    got = _run_gpu(images, idx, boxes, flip, lut, out_hw, aff, codes, wild.contiguous(),
                   fill=FILL, ra_fill=RA_FILL)
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------- the dataset

@pytest.mark.parametrize("mix", [False, True], ids=["rand", "rand_mix"])
def test_device_dataset_equals_the_cpu_dataset(mix):
    rng = np.random.RandomState(3)
    imgs = rng.randint(0, 256, (24, 12, 10, 3)).astype(np.uint8)
    labels = rng.randint(0, 10, 24)
    aug = ImageAugment((8, 8), mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3), fill=7)
    # no shuffle: the order's generator lives on the dataset's device
    kw = dict(dtype=BF16, shuffle=False, seed=1, aug_seed=2,
              rand=ImageRandAugment(num_layers=3, prob=0.8), rand_seed=4)
    if mix:
        kw.update(mix=ImageMix(mixup_alpha=0.4, cutmix_alpha=1.0, mode="elem"), mix_seed=3)
    cpu = DeviceImageDataset(imgs, labels, 6, "cpu", aug, **kw)
    gpu = DeviceImageDataset(imgs, labels, 6, "cuda", aug, **kw)
    plain = DeviceImageDataset(imgs, labels, 6, "cpu", aug, dtype=BF16, shuffle=False, seed=1,
                               aug_seed=2)
    changed = False
    for _ in range(6):                                     # over an epoch boundary
        xc, yc = next(cpu)
        xg, yg = next(gpu)
        assert xg.is_cuda and xg.dtype == BF16 and isinstance(yg, MixedLabels) == mix
        assert torch.equal(xg.cpu(), xc)
        if mix:
            assert all(torch.equal(g.cpu(), c) for g, c in zip(yg, yc))
        else:
            assert torch.equal(yg.cpu(), yc)
        changed |= not torch.equal(next(plain)[0], xc)
    assert changed
    for (xc, yc), (xg, yg) in zip(cpu.single_pass(), gpu.single_pass()):
        assert torch.equal(xg.cpu(), xc) and torch.equal(yg.cpu(), yc)


# ----------------------------------------------------------------------------- end to end

def test_mnist_cnn_trains_on_randaugmented_batches():
    from distributedtensorflow_amd.models import MnistCNN
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    rng = np.random.RandomState(0)
    imgs = rng.randint(0, 256, (64, 32, 32, 1)).astype(np.uint8)
    aug = ImageAugment(28, mode="pad_crop")
    train = DeviceImageDataset(imgs, rng.randint(0, 10, 64), 16, "cuda", aug, shuffle=True, seed=0,
                               aug_seed=1, mix=ImageMix(0.2, 1.0), mix_seed=2,
                               rand=ImageRandAugment(), rand_seed=3)
    torch.manual_seed(0)
    with OneDeviceStrategy("cuda").scope():
        model = MnistCNN(num_classes=10).cuda()
        opt = MomentumOptimizer(0.05, 0.9)
        opt.build(list(model.parameters()))
        params = [p for p in model.parameters() if p.requires_grad]
        before = [p.detach().float().clone() for p in params]
        for _ in range(3):
            x, y = next(train)
            assert x.shape == (16, 28, 28, 1) and x.dtype == BF16 and isinstance(y, MixedLabels)
            loss = ops.mixed_softmax_cross_entropy(model(x), *y, 0.1)
            opt.minimize(loss)
            assert math.isfinite(float(loss))
        moved = [not torch.equal(p.detach().float(), q) for p, q in zip(params, before)]
    assert moved[0] and moved[-1] and sum(moved) > len(moved) // 2


def test_cli_trains_with_randaugment_and_mixup(tmp_path):
    d = str(tmp_path / "set")
    write_set(d)
    r = subprocess.run([sys.executable, TRAIN, "--model", "mnist_cnn", "--image_data", d,
                        "--augment", "pad_crop", "--batch_size", "32", "--train_steps", "3",
                        "--randaugment", "2", "--mixup_alpha", "0.2", "--log_dir",
                        str(tmp_path / "tb")],
                       capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["global_step"] == 3 and math.isfinite(res["final_loss"])
    assert res["randaugment"] == 2 and res["mixup_alpha"] == 0.2 and res["ra_prob"] == 0.5
