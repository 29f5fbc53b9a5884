"""Image augmentation on the CPU path: the integer sampling rule of ops.augment_images against a
per-pixel Python oracle, the crop-box functions against a numpy float64 oracle, the
DeviceImageDataset (order, determinism, single_pass, sharded / chunked upload), the .npy loader's
errors and the CLI's --image_data flags.  Every comparison is exact."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import DeviceArrayDataset, DeviceImageDataset, ImageAugment
from distributedtensorflow_amd.data import images as dimg
from distributedtensorflow_amd.ops import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")


# ----------------------------------------------------------------------------- the sampling rule

def _axis(o, O, side):
    pos = ((2 * o + 1) * side * 256) // (2 * O) - 128
    pos = min(max(pos, 0), (side - 1) * 256)
    i0, f = pos >> 8, pos & 255
    return i0, min(i0 + 1, side - 1), f


def scalar_oracle(images, idx, boxes, flip, lut, out_hw, fill):
    """The issue's rule, one output element at a time, on Python ints."""
    img = images.numpy()
    N, Hs, Ws, C = img.shape
    Ho, Wo = out_hw
    B = len(idx)
    out = torch.empty(B, Ho, Wo, C, dtype=lut.dtype)

    def px(n, y, x, c):
        return int(img[n, y, x, c]) if 0 <= y < Hs and 0 <= x < Ws else fill

    for b in range(B):
        n = int(idx[b])
        y0, x0, h, w = (int(v) for v in boxes[b])
        for oy in range(Ho):
            iy0, iy1, fy = _axis(oy, Ho, h)
            for ox in range(Wo):
                oxs = Wo - 1 - ox if int(flip[b]) else ox
                ix0, ix1, fx = _axis(oxs, Wo, w)
                for c in range(C):
                    top = (256 - fx) * px(n, y0 + iy0, x0 + ix0, c) + \
                        fx * px(n, y0 + iy0, x0 + ix1, c)
                    bot = (256 - fx) * px(n, y0 + iy1, x0 + ix0, c) + \
                        fx * px(n, y0 + iy1, x0 + ix1, c)
                    v = ((256 - fy) * top + fy * bot + 32768) >> 16
                    assert 0 <= v <= 255
                    out[b, oy, ox, c] = lut[c, v]
    return out


def _set(N, Hs, Ws, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, Hs, Ws, C), generator=g, dtype=torch.uint8)


def _lut(C, dtype=torch.float32):
    return ImageAugment(4, mean=(0.485, 0.456, 0.406)[:C], std=(0.229, 0.224, 0.225)[:C]).lut(
        C, dtype, "cpu")


# boxes over a 7 x 9 source: whole image, inner crop, 2 pixels outside on every side, 1 x 1
BOXES_7x9 = [(0, 0, 7, 9), (1, 2, 4, 5), (-2, -2, 11, 13), (3, 4, 1, 1)]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", [(5, 7), (11, 13), (7, 9)])
def test_reference_matches_scalar_oracle(C, out_hw):
    images = _set(3, 7, 9, C, seed=C)
    lut = _lut(C)
    idx, boxes, flip = [], [], []
    for k, box in enumerate(BOXES_7x9):
        for f in (0, 1):
            idx.append((2 * k + f) % 3)
            boxes.append(box)
            flip.append(f)
    idx = torch.tensor(idx)
    boxes = torch.tensor(boxes, dtype=torch.int32)
    flip = torch.tensor(flip, dtype=torch.uint8)
    got = reference.augment_images(images, idx, boxes, flip, lut, out_hw, fill=17)
    want = scalar_oracle(images, idx, boxes, flip, lut, out_hw, 17)
    assert got.dtype == lut.dtype and got.shape == want.shape
    assert torch.equal(got, want)
    assert torch.equal(ops.augment_images(images, idx, boxes, flip, lut, out_hw, fill=17), want)


@pytest.mark.parametrize("C", [3, 1])
def test_box_of_the_output_size_is_a_pure_copy_through_the_table(C):
    images = _set(2, 7, 9, C, seed=5)
    lut = _lut(C)
    idx = torch.tensor([1, 0])
    boxes = torch.tensor([[0, 0, 7, 9]] * 2, dtype=torch.int32)
    flip = torch.tensor([0, 1], dtype=torch.uint8)
    got = reference.augment_images(images, idx, boxes, flip, lut, (7, 9))
    want = lut[torch.arange(C).view(1, 1, 1, C), images[idx].long()]
    want[1] = want[1].flip(1)
    assert torch.equal(got, want)
    # the pad-crop case: an output-sized box shifted outside copies pixels and reads fill
    boxes = torch.tensor([[-2, 3, 7, 9]] * 2, dtype=torch.int32)
    got = reference.augment_images(images, idx, boxes, torch.zeros(2, dtype=torch.uint8), lut,
                                   (7, 9), fill=17)
    padded = torch.full((2, 7 + 4, 9 + 6, C), 17, dtype=torch.uint8)
    padded[:, 2:9, 0:9] = images[idx]
    want = lut[torch.arange(C).view(1, 1, 1, C), padded[:, 0:7, 3:12].long()]
    assert torch.equal(got, want)


def test_bf16_table_and_argument_checks():
    images = _set(2, 7, 9, 3)
    lut = _lut(3, torch.bfloat16)
    idx = torch.tensor([0, 1])
    boxes = torch.tensor([[1, 1, 5, 6]] * 2, dtype=torch.int32)
    flip = torch.tensor([1, 0], dtype=torch.uint8)
    got = reference.augment_images(images, idx, boxes, flip, lut, (5, 7))
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, scalar_oracle(images, idx, boxes, flip, lut, (5, 7), 0))
    with pytest.raises(ValueError):
        reference.augment_images(images, idx, boxes.long(), flip, lut, (5, 7))
    with pytest.raises(ValueError):
        reference.augment_images(images, idx, boxes, flip, lut[:2], (5, 7))
    with pytest.raises(ValueError):
        reference.augment_images(images, torch.tensor([0, 2]), boxes, flip, lut, (5, 7))
    with pytest.raises(ValueError):
        reference.augment_images(images.float(), idx, boxes, flip, lut, (5, 7))


# ----------------------------------------------------------------------------- crop boxes

def rrc_oracle(u, Hs, Ws, scale, ratio):
    """numpy float64, one example and one attempt at a time."""
    u = np.asarray(u, dtype=np.float64)
    out = np.zeros((u.shape[0], 4), dtype=np.int32)
    for b in range(u.shape[0]):
        for k in range(u.shape[1]):
            u0, u1, u2, u3 = u[b, k]
            area = (Hs * Ws) * (scale[0] + (scale[1] - scale[0]) * u0)
            l0, l1 = math.log(ratio[0]), math.log(ratio[1])
            ar = np.exp(l0 + (l1 - l0) * u1)
            w = np.floor(np.sqrt(area * ar) + 0.5)
            h = np.floor(np.sqrt(area / ar) + 0.5)
            if 1 <= w <= Ws and 1 <= h <= Hs:
                out[b] = (np.floor(u3 * (Hs - h + 1)), np.floor(u2 * (Ws - w + 1)), h, w)
                break
        else:
            r = Ws / Hs
            if r < ratio[0]:
                w, h = Ws, int(math.floor(Ws / ratio[0] + 0.5))
            elif r > ratio[1]:
                h, w = Hs, int(math.floor(Hs * ratio[1] + 0.5))
            else:
                h, w = Hs, Ws
            out[b] = ((Hs - h) // 2, (Ws - w) // 2, h, w)
    return out


def test_rrc_boxes_match_the_numpy_oracle_and_stay_inside():
    Hs, Ws, scale, ratio = 64, 48, (0.08, 1.0), (3 / 4, 4 / 3)
    u = torch.rand(512, 10, 4, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    got = dimg.rrc_boxes(u, Hs, Ws, scale, ratio)
    assert got.dtype == torch.int32 and got.shape == (512, 4)
    assert np.array_equal(got.numpy(), rrc_oracle(u.numpy(), Hs, Ws, scale, ratio))
    y0, x0, h, w = got.long().unbind(1)
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= Hs).all() and (x0 + w <= Ws).all()
    # the sample has examples whose first attempt is rejected, and boxes of many sizes
    first = rrc_oracle(u[:, :1].numpy(), Hs, Ws, scale, ratio)
    assert (first != got.numpy()).any() and len(set(map(tuple, got.tolist()))) > 400


@pytest.mark.parametrize("Hs,Ws,want", [(64, 48, (0, 0, 64, 48)),      # 0.75: inside the range
                                        (100, 30, (30, 0, 40, 30)),     # narrower than 3 / 4
                                        (30, 100, (0, 30, 30, 40))])    # wider than 4 / 3
def test_rrc_boxes_fall_back_to_the_central_crop(Hs, Ws, want):
    # area = the whole image at the extreme aspect ratio: w or h overshoots in all ten attempts
    u = torch.zeros(3, 10, 4, dtype=torch.float64)
    u[..., 0] = 1.0
    u[..., 1] = 1.0 if Hs >= Ws else 0.0
    got = dimg.rrc_boxes(u, Hs, Ws, (0.08, 1.0), (3 / 4, 4 / 3))
    assert got.tolist() == [list(want)] * 3
    assert np.array_equal(got.numpy(), rrc_oracle(u.numpy(), Hs, Ws, (0.08, 1.0), (3 / 4, 4 / 3)))


def test_pad_crop_and_center_boxes():
    u = torch.rand(4096, 2, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = dimg.pad_crop_boxes(u, 32, 40, (28, 32), 4)
    assert got.dtype == torch.int32
    y0, x0, h, w = got.unbind(1)
    assert (h == 28).all() and (w == 32).all()
    assert y0.min() == -4 and y0.max() == 32 + 4 - 28             # every offset of the range
    assert x0.min() == -4 and x0.max() == 40 + 4 - 32
    assert sorted(set(y0.tolist())) == list(range(-4, 9))
    edge = dimg.pad_crop_boxes(torch.tensor([[0.0, 0.0], [1.0 - 2 ** -53, 1.0 - 2 ** -53]],
                                            dtype=torch.float64), 32, 32, (32, 32), 4)
    assert edge.tolist() == [[-4, -4, 32, 32], [4, 4, 32, 32]]
    with pytest.raises(ValueError):
        dimg.pad_crop_boxes(u, 32, 32, (41, 32), 4)
    assert dimg.center_boxes(256, 256).tolist() == [[16, 16, 224, 224]]
    assert dimg.center_boxes(72, 100, 0.875).tolist() == [[4, 6, 63, 88]]      # 87.5 rounds up
    assert dimg.center_boxes(32, 32, 1.0).tolist() == [[0, 0, 32, 32]]


# ----------------------------------------------------------------------------- the dataset

def _arrays(N=23, Hs=12, Ws=10, C=3, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, (N, Hs, Ws, C)).astype(np.uint8),
            rng.randint(0, 10, N).astype(np.int64))


def _aug(mode="random_resized_crop", **kw):
    return ImageAugment((8, 8), mode=mode, mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3), **kw)


def test_dataset_keeps_the_example_order_of_the_array_dataset():
    imgs, labels = _arrays()
    labels = np.arange(len(labels))                       # the label names the example
    plain = DeviceArrayDataset(imgs, labels, 5, "cpu", shuffle=True, seed=11)
    aug = DeviceImageDataset(imgs, labels, 5, "cpu", _aug(), shuffle=True, seed=11, aug_seed=3)
    none = DeviceImageDataset(imgs, labels, 5, "cpu", _aug("none", flip=False), shuffle=True,
                              seed=11)
    for _ in range(11):                                   # across two epoch boundaries
        y = next(plain)[1]
        assert torch.equal(next(aug)[1], y) and torch.equal(next(none)[1], y)
    assert aug.epoch == plain.epoch == 2


def test_dataset_is_deterministic_and_augments():
    imgs, labels = _arrays()
    a = DeviceImageDataset(imgs, labels, 6, "cpu", _aug(), shuffle=True, seed=1, aug_seed=2)
    b = DeviceImageDataset(imgs, labels, 6, "cpu", _aug(), shuffle=True, seed=1, aug_seed=2)
    c = DeviceImageDataset(imgs, labels, 6, "cpu", _aug(), shuffle=True, seed=1, aug_seed=3)
    differs = False
    for _ in range(5):
        xa, ya = next(a)
        xb, yb = next(b)
        xc, yc = next(c)
        assert xa.shape == (6, 8, 8, 3) and xa.dtype == torch.float32
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(ya, yc)
        differs |= not torch.equal(xa, xc)
    assert differs                                        # the augmentation seed matters
    # mode "none" without flips is the plain resize of the whole image
    d = DeviceImageDataset(imgs, labels, 4, "cpu", _aug("none", flip=False))
    x, _ = next(d)
    t = d.images
    want = reference.augment_images(t, torch.arange(4), torch.tensor([[0, 0, 12, 10]] * 4,
                                                                      dtype=torch.int32),
                                    torch.zeros(4, dtype=torch.uint8), d._lut, (8, 8))
    assert torch.equal(x, want)


def test_single_pass_covers_every_example_once_and_leaves_training_alone():
    imgs, labels = _arrays(N=23)
    labels = np.arange(23)
    seen = []
    for shard in range(2):
        d = DeviceImageDataset(imgs, labels, 5, "cpu", _aug(), shuffle=True, seed=4, aug_seed=9,
                               num_shards=2, shard_index=shard)
        ref = DeviceImageDataset(imgs, labels, 5, "cpu", _aug(), shuffle=True, seed=4, aug_seed=9,
                                 num_shards=2, shard_index=shard)
        next(d), next(ref)
        first = [(x.clone(), y.clone()) for x, y in d.single_pass()]
        again = list(d.single_pass())
        sizes = [len(y) for _, y in first]
        assert sizes == ([5, 5, 2] if shard == 0 else [5, 5, 1])        # remainder included
        for (x1, y1), (x2, y2) in zip(first, again):
            assert torch.equal(x1, x2) and torch.equal(y1, y2)
        # the evaluation transform: centre crop, no flip
        box = dimg.center_boxes(12, 10, 0.875)
        y = torch.cat([y for _, y in first])
        want = reference.augment_images(d.images, torch.arange(d.n), box.expand(d.n, 4).contiguous(),
                                        torch.zeros(d.n, dtype=torch.uint8), d._lut, (8, 8))
        assert torch.equal(torch.cat([x for x, _ in first]), want)
        seen += y.tolist()
        xa, ya = next(d)                                   # training went on undisturbed
        xb, yb = next(ref)
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert sorted(seen) == list(range(23))


def test_chunked_sharded_upload_equals_one_piece():
    imgs, labels = _arrays(N=23)
    row = imgs[0].size
    for shards in (1, 2, 3):
        for shard in range(shards):
            whole = DeviceImageDataset(imgs, labels, 2, "cpu", _aug(), num_shards=shards,
                                       shard_index=shard)
            for rows in (1, 3, 4):
                part = DeviceImageDataset(imgs, labels, 2, "cpu", _aug(), num_shards=shards,
                                          shard_index=shard, chunk_bytes=rows * row)
                assert torch.equal(part.images, whole.images)
                assert torch.equal(part.labels, whole.labels)
            assert np.array_equal(whole.images.numpy(), imgs[shard::shards])
            assert np.array_equal(whole.labels.numpy(), labels[shard::shards])


# ----------------------------------------------------------------------------- loader

def _save(d, split, images, labels):
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, f"{split}_images.npy"), images)
    np.save(os.path.join(d, f"{split}_labels.npy"), labels)


def test_load_arrays_and_its_errors(tmp_path):
    imgs, labels = _arrays(N=6)
    d = str(tmp_path / "ok")
    _save(d, "train", imgs, labels)
    got_i, got_l = dimg.load_arrays(d, "train", num_classes=10)
    assert isinstance(got_i, np.memmap) and np.array_equal(got_i, imgs)
    assert np.array_equal(got_l, labels)
    bad = {
        "dtype": (imgs.astype(np.float32), labels),
        "rank": (imgs[..., 0], labels),
        "channels": (np.concatenate([imgs, imgs[..., :1]], axis=3), labels),
        "length": (imgs, labels[:5]),
        "label_dtype": (imgs, labels.astype(np.float32)),
        "label_range": (imgs, np.full(6, 10)),
        "label_negative": (imgs, np.full(6, -1)),
    }
    for name, (i, l) in bad.items():
        d = str(tmp_path / name)
        _save(d, "val", i, l)
        with pytest.raises(ValueError):
            dimg.load_arrays(d, "val", num_classes=10)
    with pytest.raises(FileNotFoundError):
        dimg.load_arrays(str(tmp_path / "ok"), "val")


# ----------------------------------------------------------------------------- CLI

def _env():
    e = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        e.pop(k, None)
    return e


def test_cli_image_data_mnist_cnn_cpu(tmp_path):
    d = str(tmp_path / "set")
    rng = np.random.RandomState(0)
    _save(d, "train", rng.randint(0, 256, (40, 32, 32, 1)).astype(np.uint8), rng.randint(0, 10, 40))
    _save(d, "val", rng.randint(0, 256, (13, 32, 32, 1)).astype(np.uint8), rng.randint(0, 10, 13))
    r = subprocess.run([sys.executable, TRAIN, "--model", "mnist_cnn", "--device", "cpu",
                        "--image_data", d, "--augment", "pad_crop", "--train_steps", "2",
                        "--log_dir", str(tmp_path / "tb"), "--eval"],
                       capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["global_step"] == 2 and math.isfinite(res["final_loss"])
    assert 0.0 <= res["eval_top_1"] <= 1.0 and res["eval_count"] == 13
