"""HBM-resident image sets with fused on-device augmentation.

A pre-resized uint8 image set fits the device whole (ImageNet at 64 x 64 is 15.7 GB, at
160 x 160 98 GB, of 288 GB of HBM3E), so it is uploaded once and every training batch is ONE
kernel (``ops.augment_images``): gather, random-resized-crop or pad-crop, bilinear resize, flip,
per-channel normalisation, cast to the compute dtype, NHWC.  No host pipeline and no per-step
copy of pixels; the only per-step host work is drawing the crop / flip uniforms from the
dataset's own CPU generator and forming the B crop boxes from them (20 bytes per example reach
the device), which is what makes a CPU and a GPU dataset with the same seeds yield the same
batches.

On disk a set is two arrays per split in one directory (:func:`load_arrays`):

    {split}_images.npy   uint8 [N, H, W, C], C in {1, 3}   (memory-mapped, never copied whole)
    {split}_labels.npy   integers [N] in [0, num_classes)

Crop boxes are (y0, x0, h, w) in source pixels, int32, one pure function per mode:
:func:`rrc_boxes`, :func:`pad_crop_boxes`, :func:`center_boxes`.

Sample mixing (:class:`ImageMix`: Mixup, CutMix) happens in the same kernel
(``ops.augment_mix_images``): :func:`mix_plan` turns the draws of a third CPU generator into each
row's partner, blend weight and cut box, and the batch's labels become
:class:`MixedLabels` for ``ops.mixed_softmax_cross_entropy``.

RandAugment (:class:`ImageRandAugment`) happens in the same kernel too
(``ops.augment_rand_images``): :func:`randaugment_plan` turns the draws of a fourth CPU generator
into each row's composed affine map and its pointwise ops.
"""
from __future__ import annotations

import collections
import math
import os

import numpy as np
import torch

from .device import DeviceArrayDataset, upload_sharded

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
RRC_ATTEMPTS = 10


def load_arrays(data_dir, split, num_classes=None):
    """-> (images, labels) of ``{split}_images.npy`` (uint8 NHWC, memory-mapped) and
    ``{split}_labels.npy``.  Raises ValueError on a wrong dtype or rank, a length mismatch, or
    a label outside ``[0, num_classes)``."""
    ipath = os.path.join(data_dir, f"{split}_images.npy")
    lpath = os.path.join(data_dir, f"{split}_labels.npy")
    images = np.load(ipath, mmap_mode="r")
    labels = np.load(lpath)
    if images.dtype != np.uint8:
        raise ValueError(f"{ipath}: dtype {images.dtype}, expected uint8")
    if images.ndim != 4 or images.shape[3] not in (1, 3):
        raise ValueError(f"{ipath}: shape {images.shape}, expected [N, H, W, C] with C in (1, 3)")
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"{lpath}: {labels.dtype} {labels.shape}, expected integers [N]")
    if len(labels) != len(images):
        raise ValueError(f"{lpath}: {len(labels)} labels for {len(images)} images")
    if len(labels) and int(labels.min()) < 0:
        raise ValueError(f"{lpath}: negative label {int(labels.min())}")
    if num_classes is not None and len(labels) and int(labels.max()) >= num_classes:
        raise ValueError(f"{lpath}: label {int(labels.max())} >= num_classes {num_classes}")
    return images, labels


# ----------------------------------------------------------------------------- crop boxes

def _round(x):
    return torch.floor(x + 0.5)                         # half-up


def _fallback_box(Hs, Ws, ratio):
    """The central crop at the aspect ratio nearest the image's inside ``ratio``."""
    in_ratio = Ws / Hs
    if in_ratio < ratio[0]:
        w, h = Ws, int(math.floor(Ws / ratio[0] + 0.5))
    elif in_ratio > ratio[1]:
        h, w = Hs, int(math.floor(Hs * ratio[1] + 0.5))
    else:
        h, w = Hs, Ws
    h, w = min(max(h, 1), Hs), min(max(w, 1), Ws)
    return (Hs - h) // 2, (Ws - w) // 2, h, w


def rrc_boxes(u, Hs, Ws, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop boxes (torchvision's / TF official ResNet's semantics) from supplied
    uniforms ``u`` [B, 10, 4] -> int32 [B, 4] on ``u``'s device, computed in float64.

    Attempt k: ``area = Hs Ws lerp(scale, u0)``, ``ar = exp(lerp(log ratio, u1))``,
    ``w = round(sqrt(area ar))``, ``h = round(sqrt(area / ar))`` (half-up), valid iff
    ``1 <= w <= Ws`` and ``1 <= h <= Hs``; ``x0 = floor(u2 (Ws - w + 1))``,
    ``y0 = floor(u3 (Hs - h + 1))``.  The first valid attempt wins; with none, the central
    crop at the nearest aspect ratio inside ``ratio``."""
    if u.dim() != 3 or u.shape[2] != 4:
        raise ValueError("rrc_boxes: u must be [B, attempts, 4]")
    u = u.to(torch.float64)
    area = (Hs * Ws) * (scale[0] + (scale[1] - scale[0]) * u[..., 0])
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    ar = torch.exp(l0 + (l1 - l0) * u[..., 1])
    w = _round(torch.sqrt(area * ar))
    h = _round(torch.sqrt(area / ar))
    valid = (w >= 1) & (w <= Ws) & (h >= 1) & (h <= Hs)
    x0 = torch.minimum(torch.floor(u[..., 2] * (Ws - w + 1)), Ws - w)
    y0 = torch.minimum(torch.floor(u[..., 3] * (Hs - h + 1)), Hs - h)
    cand = torch.stack([y0, x0, h, w], dim=2).to(torch.int32)            # [B, A, 4]
    first = torch.argmax(valid.to(torch.uint8), dim=1)                    # first maximal index
    pick = cand.gather(1, first.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
    fb = torch.tensor(_fallback_box(Hs, Ws, ratio), dtype=torch.int32, device=u.device)
    return torch.where(valid.any(dim=1, keepdim=True), pick, fb.unsqueeze(0))


def pad_crop_boxes(u, Hs, Ws, out_hw, pad):
    """Pad-and-crop boxes (the CIFAR transform) from uniforms ``u`` [B, 2]: the box has the
    output's size and its offsets are uniform in ``[-pad, Hs + pad - Ho]`` x
    ``[-pad, Ws + pad - Wo]``, so the resize is an exact copy and the padding reads ``fill``."""
    Ho, Wo = out_hw
    ny, nx = Hs + 2 * pad - Ho + 1, Ws + 2 * pad - Wo + 1
    if ny < 1 or nx < 1:
        raise ValueError(f"pad_crop_boxes: output {out_hw} exceeds the padded {Hs}x{Ws} image")
    u = u.to(torch.float64)
    y0 = torch.clamp(torch.floor(u[:, 0] * ny), max=ny - 1) - pad
    x0 = torch.clamp(torch.floor(u[:, 1] * nx), max=nx - 1) - pad
    return torch.stack([y0, x0, torch.full_like(y0, Ho), torch.full_like(x0, Wo)],
                       dim=1).to(torch.int32)


def center_boxes(Hs, Ws, fraction=0.875):
    """The evaluation transform: the central ``fraction`` of each side -> int32 [1, 4]."""
    h = min(max(int(math.floor(Hs * fraction + 0.5)), 1), Hs)
    w = min(max(int(math.floor(Ws * fraction + 0.5)), 1), Ws)
    return torch.tensor([[(Hs - h) // 2, (Ws - w) // 2, h, w]], dtype=torch.int32)


# ----------------------------------------------------------------------------- sample mixing

MixedLabels = collections.namedtuple("MixedLabels", ["labels_a", "labels_b", "lam"])
MixedLabels.__doc__ = """The labels of a mixed batch: the target of row b is ``lam[b]`` of class
``labels_a[b]`` and ``1 - lam[b]`` of class ``labels_b[b]`` (``lam`` fp32 [B]); the arguments of
``ops.mixed_softmax_cross_entropy`` in order."""


class ImageMix:
    """Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) of a :class:`DeviceImageDataset`,
    with timm's ``Mixup`` semantics.  ``mixup_alpha`` / ``cutmix_alpha``: the Beta(alpha, alpha)
    parameters, 0 = that method off.  ``prob``: the chance that a batch (an example) is mixed at
    all.  ``switch_prob``: with both methods on, the chance of CutMix.  ``mode``: "batch" (one
    draw per batch) or "elem" (one per example).  Row b's partner is row B - 1 - b."""

    MODES = ("batch", "elem")

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5,
                 mode="batch"):
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        if not (self.mixup_alpha >= 0 and self.cutmix_alpha >= 0) or \
                math.isinf(self.mixup_alpha) or math.isinf(self.cutmix_alpha):
            raise ValueError("ImageMix: the alphas must be finite and >= 0")
        if self.mixup_alpha == 0 and self.cutmix_alpha == 0:
            raise ValueError("ImageMix: one of mixup_alpha and cutmix_alpha must be > 0")
        if not (0 <= self.prob <= 1 and 0 <= self.switch_prob <= 1):
            raise ValueError("ImageMix: prob and switch_prob must be in [0, 1]")
        if mode not in self.MODES:
            raise ValueError(f"ImageMix: mode {mode!r} not in {self.MODES}")
        self.mode = mode

    def draw(self, B, generator):
        """The draws of one batch from ``generator`` (CPU) -> (u, g) for :func:`mix_plan`:
        ``u`` float64 [R, 4] uniforms, then ``g`` = (Mixup's, CutMix's) float64 [R, 2] standard
        gammas of shape alpha, None for an alpha of 0; R = 1 per batch, B per example."""
        R = B if self.mode == "elem" else 1
        u = torch.rand(R, 4, generator=generator, dtype=torch.float64, device="cpu")
        g = tuple(torch._standard_gamma(torch.full((R, 2), a, dtype=torch.float64, device="cpu"),
                                        generator) if a > 0 else None
                  for a in (self.mixup_alpha, self.cutmix_alpha))
        return u, g


def mix_plan(u, g, B, out_hw, mix):
    """The mixing plan of one batch from supplied draws (:meth:`ImageMix.draw`), computed on the
    host in float64 -> (partner int32 [B], lam_q int32 [B], cut int32 [B, 4], lam fp32 [B]).

    Per draw row (one for the batch, or one per example): applied iff ``u0 < prob``; CutMix iff
    only ``cutmix_alpha > 0``, or both are and ``u1 < switch_prob``; ``l = g0 / (g0 + g1)`` of
    the chosen method's gammas (0.5 if the sum is 0), a Beta(alpha, alpha) draw.
    Mixup: ``lam_q = floor(l 65536 + 0.5)``, ``lam = lam_q / 65536``, no box.
    CutMix (timm's ``rand_bbox``): ``r = sqrt(1 - l)``, box size ``(floor(Ho r), floor(Wo r))``,
    centre ``(min(floor(u2 Ho), Ho - 1), min(floor(u3 Wo), Wo - 1))``, edges
    ``clamp(centre -/+ size // 2, 0, O)``; ``lam_q = 65536`` and ``lam = 1 - area / (Ho Wo)`` of
    the clipped box.  Not applied: ``lam_q = 65536``, no box, ``lam = 1``.
    ``partner[b] = B - 1 - b``."""
    Ho, Wo = (int(v) for v in out_hw)
    R = B if mix.mode == "elem" else 1
    if tuple(u.shape) != (R, 4):
        raise ValueError(f"mix_plan: u must be [{R}, 4]")
    g_mix, g_cut = g
    for a, t in ((mix.mixup_alpha, g_mix), (mix.cutmix_alpha, g_cut)):
        if (a > 0) != (t is not None) or (t is not None and tuple(t.shape) != (R, 2)):
            raise ValueError(f"mix_plan: g holds one [{R}, 2] draw per alpha > 0, else None")
    u = u.to(torch.float64)           # the plan is formed on the host, whatever the default

    def beta(t):
        t = t.to(torch.float64)
        s = t[:, 0] + t[:, 1]
        return torch.where(s > 0, t[:, 0] / torch.where(s > 0, s, torch.ones_like(s)),
                           torch.full_like(s, 0.5))

    applied = u[:, 0] < mix.prob
    if g_mix is None:
        is_cut = torch.ones(R, dtype=torch.bool, device="cpu")
    elif g_cut is None:
        is_cut = torch.zeros(R, dtype=torch.bool, device="cpu")
    else:
        is_cut = u[:, 1] < mix.switch_prob
    zero = torch.zeros(R, dtype=torch.float64, device="cpu")
    l_mix = beta(g_mix) if g_mix is not None else zero + 1.0
    l_cut = beta(g_cut) if g_cut is not None else zero + 1.0

    q_mix = torch.floor(l_mix * 65536.0 + 0.5)
    r = torch.sqrt(1.0 - l_cut)
    ch, cw = torch.floor(Ho * r), torch.floor(Wo * r)
    cy = torch.clamp(torch.floor(u[:, 2] * Ho), max=Ho - 1)
    cx = torch.clamp(torch.floor(u[:, 3] * Wo), max=Wo - 1)
    hy, hx = torch.floor(ch / 2), torch.floor(cw / 2)
    y_lo, y_hi = torch.clamp(cy - hy, 0, Ho), torch.clamp(cy + hy, 0, Ho)
    x_lo, x_hi = torch.clamp(cx - hx, 0, Wo), torch.clamp(cx + hx, 0, Wo)
    box = torch.stack([y_lo, x_lo, y_hi - y_lo, x_hi - x_lo], dim=1)
    lam_cut = 1.0 - (y_hi - y_lo) * (x_hi - x_lo) / float(Ho * Wo)

    cutting = applied & is_cut
    lam_q = torch.where(applied & ~is_cut, q_mix, zero + 65536.0)
    lam = torch.where(cutting, lam_cut, lam_q / 65536.0)
    cut = torch.where(cutting.unsqueeze(1), box, torch.zeros_like(box))
    if float(lam.min()) < 0.0 or float(lam.max()) > 1.0:
        raise ValueError("mix_plan: lam outside [0, 1]")
    partner = torch.arange(B - 1, -1, -1, dtype=torch.int32, device="cpu")
    return (partner, lam_q.to(torch.int32).expand(B).contiguous(),
            cut.to(torch.int32).expand(B, 4).contiguous(),
            lam.to(torch.float32).expand(B).contiguous())


# ----------------------------------------------------------------------------- RandAugment

RAND_OPS = ("rotate", "shear_x", "shear_y", "translate_x", "translate_y", "invert", "solarize",
            "solarize_add", "posterize", "brightness", "color")
_RAND_GEOMETRIC = 5                 # the first five of RAND_OPS resample; the others are pointwise
# the pointwise op codes of ops.augment_rand_images, by position in RAND_OPS
_RAND_CODE = {5: 1, 6: 2, 7: 3, 8: 4, 9: 5, 10: 6}


class ImageRandAugment:
    """RandAugment (Cubuk et al. 2020) of a :class:`DeviceImageDataset`, with the semantics of
    timm's ``rand-m{magnitude}-mstd{mstd}-inc1``: each of ``num_layers`` layers picks one of
    ``ops`` uniformly, applies it with chance ``prob`` at level
    ``clamp(magnitude + mstd * N(0, 1), 0, 10) / 10`` under the "increasing" magnitude maps and
    a random sign.  ``ops``: names out of :data:`RAND_OPS` (default: all eleven, timm's
    increasing set without AutoContrast, Equalize, Contrast and Sharpness).  ``translate``: the
    largest shift as a share of the output's side."""

    def __init__(self, num_layers=2, magnitude=9.0, mstd=0.5, prob=0.5, ops=None, translate=0.45):
        self.num_layers = int(num_layers)
        self.magnitude, self.mstd = float(magnitude), float(mstd)
        self.prob, self.translate = float(prob), float(translate)
        if not 1 <= self.num_layers <= 4 or self.num_layers != num_layers:
            raise ValueError("ImageRandAugment: num_layers must be 1, 2, 3 or 4")
        if not 0 <= self.magnitude <= 10:
            raise ValueError("ImageRandAugment: magnitude must be in [0, 10]")
        if not (self.mstd >= 0 and math.isfinite(self.mstd)):
            raise ValueError("ImageRandAugment: mstd must be finite and >= 0")
        if not 0 <= self.prob <= 1:
            raise ValueError("ImageRandAugment: prob must be in [0, 1]")
        if not math.isfinite(self.translate):
            raise ValueError("ImageRandAugment: translate must be finite")
        self.ops = tuple(RAND_OPS if ops is None else ops)
        unknown = [o for o in self.ops if o not in RAND_OPS]
        if unknown or not self.ops:
            raise ValueError(f"ImageRandAugment: ops {unknown or self.ops} not in {RAND_OPS}")

    def draw(self, B, generator):
        """The draws of one batch from ``generator`` (CPU) -> (u, z) for
        :func:`randaugment_plan`: ``u`` float64 [B, L, 3] uniforms, ``z`` float64 [B, L] standard
        normals (drawn whatever ``mstd`` is, so the stream does not depend on it)."""
        u = torch.rand(B, self.num_layers, 3, generator=generator, dtype=torch.float64,
                       device="cpu")
        z = torch.randn(B, self.num_layers, generator=generator, dtype=torch.float64,
                        device="cpu")
        return u, z


def randaugment_plan(u, z, out_hw, ra):
    """The RandAugment plan of one batch from supplied draws (:meth:`ImageRandAugment.draw`),
    computed on the host in float64 -> (aff int32 [B, 6], pops int32 [B, L], ppar int32 [B, L]),
    the arguments of ``ops.augment_rand_images``.

    Per example and layer k: the op is ``ops[min(floor(u0 K), K - 1)]`` of the K ops, applied iff
    ``u1 < prob``; ``sign = -1`` iff ``u2 >= 0.5``;
    ``l = clamp(magnitude + mstd z, 0, 10) / 10``.  Magnitudes (timm's increasing maps): Rotate
    ``sign 30 l`` degrees; ShearX / ShearY ``sign 0.3 l``; TranslateX / TranslateY
    ``sign translate l Wo`` (``Ho``) pixels; Solarize ``m = 256 - floor(256 l)``; SolarizeAdd
    ``m = min(128, floor(110 l))``; Posterize ``bits = max(0, 4 - floor(4 l))``,
    ``m = 256 - (1 << (8 - bits))``; Brightness / Color factor ``max(0.1, 1 + sign 0.9 l)``,
    ``m = floor(65536 factor + 0.5)``.

    A geometric op is its inverse (output -> input) matrix in pixel-centre coordinates, PIL's
    convention: ShearX s ``(1, s, 0, 0, 1, 0)``, ShearY s ``(1, 0, 0, s, 1, 0)``, TranslateX t
    ``(1, 0, t, 0, 1, 0)``, TranslateY t ``(1, 0, 0, 0, 1, t)``, Rotate by theta degrees about
    ``(cx, cy) = (Wo / 2, Ho / 2)`` with ``r = -theta pi / 180``:
    ``(cos r, sin r, cx - cx cos r - cy sin r, -sin r, cos r, cy + cx sin r - cy cos r)``.  The
    geometric ops of an example compose in layer order, ``M = M_g1 M_g2 ...`` (the last op's map
    meets the output pixel first), and each of M's six entries becomes
    ``floor(65536 value + 0.5)``.  Layers that were geometric or not applied hold code 0."""
    Ho, Wo = (int(v) for v in out_hw)
    L = ra.num_layers
    if u.dim() != 3 or tuple(u.shape[1:]) != (L, 3) or tuple(z.shape) != (u.shape[0], L):
        raise ValueError(f"randaugment_plan: u must be [B, {L}, 3] and z [B, {L}]")
    u, z = u.to(torch.float64), z.to(torch.float64)   # formed on the host, whatever the default
    B, K = u.shape[0], len(ra.ops)
    kinds = torch.tensor([RAND_OPS.index(o) for o in ra.ops], dtype=torch.int64, device="cpu")
    kind = kinds[torch.clamp(torch.floor(u[..., 0] * K), max=K - 1).long()]        # [B, L]
    applied = u[..., 1] < ra.prob
    one = torch.ones(B, L, dtype=torch.float64, device="cpu")
    zero = torch.zeros_like(one)
    sign = torch.where(u[..., 2] >= 0.5, -one, one)
    l = torch.clamp(ra.magnitude + ra.mstd * z, 0.0, 10.0) / 10.0

    def on(k):
        return applied & (kind == RAND_OPS.index(k))

    # ---- the geometric ops: each layer's matrix (the identity where it has none)
    r = -(sign * 30.0 * l) * (math.pi / 180.0)
    cs, sn = torch.cos(r), torch.sin(r)
    cx, cy = Wo / 2.0, Ho / 2.0
    shear, shift = sign * 0.3 * l, sign * ra.translate * l
    rot = on("rotate")
    a = torch.where(rot, cs, one)
    b = torch.where(rot, sn, torch.where(on("shear_x"), shear, zero))
    c = torch.where(rot, cx - cx * cs - cy * sn, torch.where(on("translate_x"), shift * Wo, zero))
    d = torch.where(rot, -sn, torch.where(on("shear_y"), shear, zero))
    e = torch.where(rot, cs, one)
    f = torch.where(rot, cy + cx * sn - cy * cs, torch.where(on("translate_y"), shift * Ho, zero))
    A, Bm, Cm, D, E, F = a[:, 0], b[:, 0], c[:, 0], d[:, 0], e[:, 0], f[:, 0]
    for k in range(1, L):                                  # M = M M_k, entry by entry
        a2, b2, c2, d2, e2, f2 = a[:, k], b[:, k], c[:, k], d[:, k], e[:, k], f[:, k]
        A, Bm, Cm, D, E, F = (A * a2 + Bm * d2, A * b2 + Bm * e2, A * c2 + Bm * f2 + Cm,
                              D * a2 + E * d2, D * b2 + E * e2, D * c2 + E * f2 + F)
    aff = torch.floor(torch.stack([A, Bm, Cm, D, E, F], dim=1) * 65536.0 + 0.5)

    # ---- the pointwise ops
    bits = torch.clamp(4.0 - torch.floor(4.0 * l), min=0.0)
    factor = torch.floor(torch.clamp(1.0 + sign * 0.9 * l, min=0.1) * 65536.0 + 0.5)
    par = {"invert": zero, "solarize": 256.0 - torch.floor(256.0 * l),
           "solarize_add": torch.clamp(torch.floor(110.0 * l), max=128.0),
           "posterize": 256.0 - torch.pow(2.0, 8.0 - bits), "brightness": factor,
           "color": factor}
    pops, ppar = zero, zero
    for i, code in _RAND_CODE.items():
        hit = on(RAND_OPS[i])
        pops = torch.where(hit, zero + code, pops)
        ppar = torch.where(hit, par[RAND_OPS[i]], ppar)
    return (aff.to(torch.int32).contiguous(), pops.to(torch.int32).contiguous(),
            ppar.to(torch.int32).contiguous())


# ----------------------------------------------------------------------------- the dataset

class ImageAugment:
    """The transform of a :class:`DeviceImageDataset`.

    ``out_size``: int or (Ho, Wo).  ``mode``: "random_resized_crop" (``scale``, ``ratio``),
    "pad_crop" (``pad``; the output must not exceed the padded image) or "none" (the whole
    image, resized).  ``flip``: random horizontal flips in training.  ``mean`` / ``std``: per
    channel, on the [0, 1] scale (default 0 / 1: plain x / 255).  ``eval_fraction``: the centre
    crop of ``single_pass()`` (default 0.875 under random_resized_crop, else the whole image).
    ``fill``: the byte read outside the image."""

    MODES = ("random_resized_crop", "pad_crop", "none")

    def __init__(self, out_size, mode="random_resized_crop", scale=(0.08, 1.0),
                 ratio=(3.0 / 4.0, 4.0 / 3.0), pad=4, flip=True, mean=None, std=None,
                 eval_fraction=None, fill=0):
        if mode not in self.MODES:
            raise ValueError(f"ImageAugment: mode {mode!r} not in {self.MODES}")
        self.out_hw = (int(out_size),) * 2 if np.isscalar(out_size) else \
            tuple(int(v) for v in out_size)
        if len(self.out_hw) != 2 or min(self.out_hw) < 1:
            raise ValueError(f"ImageAugment: out_size {out_size}")
        self.out_size = self.out_hw
        if not (0 < scale[0] <= scale[1] and 0 < ratio[0] <= ratio[1]):
            raise ValueError("ImageAugment: scale and ratio must be positive increasing pairs")
        self.mode, self.scale, self.ratio = mode, tuple(scale), tuple(ratio)
        self.pad, self.flip, self.fill = int(pad), bool(flip), int(fill)
        self.mean, self.std = mean, std
        if eval_fraction is None:
            eval_fraction = 0.875 if mode == "random_resized_crop" else 1.0
        if not 0 < eval_fraction <= 1:
            raise ValueError("ImageAugment: eval_fraction must be in (0, 1]")
        self.eval_fraction = float(eval_fraction)

    def lut(self, channels, dtype, device):
        """[C, 256] table of (v / 255 - mean_c) / std_c, built in float64 and cast once."""
        mean = (0.0,) * channels if self.mean is None else tuple(self.mean)
        std = (1.0,) * channels if self.std is None else tuple(self.std)
        if len(mean) != channels or len(std) != channels:
            raise ValueError(f"ImageAugment: mean / std need {channels} entries")
        v = torch.arange(256, dtype=torch.float64, device="cpu").unsqueeze(0) / 255.0
        t = (v - torch.tensor(mean, dtype=torch.float64, device="cpu").unsqueeze(1)) / \
            torch.tensor(std, dtype=torch.float64, device="cpu").unsqueeze(1)
        return t.to(dtype).to(device).contiguous()


class DeviceImageDataset(DeviceArrayDataset):
    """A :class:`DeviceArrayDataset` of uint8 NHWC images whose batches are augmented on the
    device by one kernel.  ``__next__`` applies the training transform of ``augment``;
    ``single_pass()`` applies the centre crop without a flip and touches neither generator, so
    an evaluation between two steps leaves training bit-identical.  Example order, epochs,
    sharding and the shuffle generator are the parent's; crop and flip uniforms come from a
    second, CPU generator (``aug_seed``), so the order is the same with and without augmentation
    and the same seeds give the same batches on the CPU and on the GPU.

    ``mix``: an :class:`ImageMix`.  Training batches are then mixed inside the same kernel
    (``ops.augment_mix_images``) and ``__next__`` yields ``(x, MixedLabels)``; the plan's draws
    come from a third CPU generator (``mix_seed``), so example order and crops are those of the
    unmixed dataset.  ``single_pass()`` never mixes.

    ``rand``: an :class:`ImageRandAugment`.  Training batches then go through
    ``ops.augment_rand_images`` (with the mixing plan when ``mix`` is set too); the plan's draws
    come from a fourth CPU generator (``rand_seed``), so example order, crops, flips and the mix
    are those of the same dataset without it.  ``single_pass()`` never applies it.

    Upload: the (possibly memory-mapped) array is copied ``chunk_bytes`` at a time into a
    preallocated device tensor, the shard selection applied per chunk, so the host never holds
    a second copy of the set.  ``flatten``: batches are [B, Ho * Wo * C] (the MLP's input)."""

    def __init__(self, images, labels, batch_size, device, augment, dtype=None, shuffle=False,
                 seed=0, aug_seed=0, num_shards=1, shard_index=0, drop_remainder=True,
                 chunk_bytes=256 << 20, flatten=False, mix=None, mix_seed=0, rand=None,
                 rand_seed=0):
        device = torch.device(device)
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] not in (1, 3):
            raise ValueError("DeviceImageDataset: images must be uint8 [N, H, W, C], C in (1, 3)")
        if len(labels) != len(images):
            raise ValueError(f"DeviceImageDataset: {len(labels)} labels for {len(images)} images")
        if not 0 <= shard_index < num_shards:
            raise ValueError(f"DeviceImageDataset: shard {shard_index} of {num_shards}")
        self.images = self._upload(images, device, num_shards, shard_index, int(chunk_bytes))
        labs = torch.as_tensor(np.ascontiguousarray(labels)).long()
        self.labels = labs[shard_index::num_shards].to(device)
        self.n = len(self.labels)
        self.batch_size = batch_size
        self.device = device
        self.dtype = dtype or (torch.bfloat16 if device.type == "cuda" else torch.float32)
        self.scale = 1.0 / 255.0
        self.shuffle = shuffle
        self.drop_remainder = drop_remainder
        self._gen = torch.Generator(device=device)
        self._gen.manual_seed(seed)
        self._order = None
        self._pos = 0
        self.epoch = 0
        if self.n < batch_size:
            raise ValueError(f"dataset of {self.n} examples < batch size {batch_size}")
        self.augment = augment
        self.flatten = bool(flatten)
        Hs, Ws, C = self.images.shape[1:]
        if augment.mode == "pad_crop":
            pad_crop_boxes(torch.zeros(1, 2, device="cpu"), Hs, Ws, augment.out_hw, augment.pad)   # validates
        self._lut = augment.lut(C, self.dtype, device)
        self._aug_gen = torch.Generator(device="cpu")
        self._aug_gen.manual_seed(aug_seed)
        self._eval_box = center_boxes(Hs, Ws, augment.eval_fraction).to(device)
        self._whole_box = torch.tensor([[0, 0, Hs, Ws]], dtype=torch.int32, device=device)
        if mix is not None and not isinstance(mix, ImageMix):
            raise ValueError("DeviceImageDataset: mix must be an ImageMix")
        self.mix = mix
        if mix is not None:
            self._mix_gen = torch.Generator(device="cpu")
            self._mix_gen.manual_seed(mix_seed)
        if rand is not None and not isinstance(rand, ImageRandAugment):
            raise ValueError("DeviceImageDataset: rand must be an ImageRandAugment")
        if rand is not None and max(augment.out_hw) > 1024:
            raise ValueError("DeviceImageDataset: rand needs output sides of at most 1024")
        self.rand = rand
        if rand is not None:
            self._rand_gen = torch.Generator(device="cpu")
            self._rand_gen.manual_seed(rand_seed)

    @staticmethod
    def _upload(images, device, num_shards, shard_index, chunk_bytes):
        return upload_sharded(images, device, num_shards, shard_index, chunk_bytes)

    def _uniforms(self, B, k):
        """[B, k] float64 uniforms of the augmentation generator (host)."""
        return torch.rand(B, k, generator=self._aug_gen, dtype=torch.float64, device="cpu")

    def _to_device(self, t):
        if self.device.type == "cuda":
            return t.pin_memory().to(self.device, non_blocking=True)
        return t

    def _train_boxes(self, B, plan=None):
        """-> (boxes int32 [B, 4], flip u8 [B]) of one training batch, on the dataset's device.
        The boxes are B-sized, so they are formed on the host, where the uniforms are drawn (a few
        dozen small device launches per step would cost more than the augmentation kernel
        itself), and reach the device as one int32 [B, 5] copy: (y0, x0, h, w, flip).
        ``plan``: host int32 [B, k] columns that ride the same copy (the mixing plan); the
        result then has a third element, those columns on the device."""
        a = self.augment
        Hs, Ws = self.images.shape[1:3]
        if a.mode == "random_resized_crop":
            r = self._uniforms(B, RRC_ATTEMPTS * 4 + 1)
            boxes = rrc_boxes(r[:, :-1].reshape(B, RRC_ATTEMPTS, 4), Hs, Ws, a.scale, a.ratio)
        elif a.mode == "pad_crop":
            r = self._uniforms(B, 3)
            boxes = pad_crop_boxes(r[:, :2], Hs, Ws, a.out_hw, a.pad)
        elif a.flip:
            r = self._uniforms(B, 1)
            boxes = torch.tensor([[0, 0, Hs, Ws]], dtype=torch.int32, device="cpu").expand(B, 4)
        else:                                   # nothing random: no draw, no copy
            fixed = (self._whole_box.expand(B, 4).contiguous(),
                     torch.zeros(B, dtype=torch.uint8, device=self.device))
            return fixed if plan is None else fixed + (self._to_device(plan),)
        flip = (r[:, -1] < 0.5) if a.flip else torch.zeros(B, dtype=torch.bool, device="cpu")
        cols = [boxes, flip.to(torch.int32).unsqueeze(1)] + ([] if plan is None else [plan])
        both = self._to_device(torch.cat(cols, dim=1))
        out = both[:, :4].contiguous(), both[:, 4].to(torch.uint8)
        return out if plan is None else out + (both[:, 5:],)

    def _train_mixed(self, idx):
        """One mixed training batch: the plan rides the boxes' copy as 7 more int32 columns
        (partner, lam_q, the cut box, the bits of lam)."""
        from .. import ops
        B = idx.numel()
        partner, lam_q, cut, lam = mix_plan(*self.mix.draw(B, self._mix_gen), B,
                                            self.augment.out_hw, self.mix)
        plan = torch.cat([partner.unsqueeze(1), lam_q.unsqueeze(1), cut,
                          lam.view(torch.int32).unsqueeze(1)], dim=1)
        boxes, flip, plan = self._train_boxes(B, plan)
        partner = plan[:, 0].contiguous()
        x = ops.augment_mix_images(self.images, idx.contiguous(), boxes, flip, self._lut,
                                   self.augment.out_hw, partner, plan[:, 1].contiguous(),
                                   plan[:, 2:6].contiguous(), self.augment.fill)
        if self.flatten:
            x = x.reshape(B, -1)
        labels = self.labels.index_select(0, idx)
        return x, MixedLabels(labels, labels.index_select(0, partner.long()),
                              plan[:, 6].contiguous().view(torch.float32))

    def _train_rand(self, idx):
        """One training batch under RandAugment: its plan rides the boxes' copy as 6 + 2 L more
        int32 columns (the map, the op codes, their parameters), ahead of the mixing plan's 7
        when there is a mix."""
        from .. import ops
        B, L = idx.numel(), self.rand.num_layers
        cols = list(randaugment_plan(*self.rand.draw(B, self._rand_gen), self.augment.out_hw,
                                     self.rand))
        if self.mix is not None:
            partner, lam_q, cut, lam = mix_plan(*self.mix.draw(B, self._mix_gen), B,
                                                self.augment.out_hw, self.mix)
            cols += [partner.unsqueeze(1), lam_q.unsqueeze(1), cut,
                     lam.view(torch.int32).unsqueeze(1)]
        boxes, flip, plan = self._train_boxes(B, torch.cat(cols, dim=1))
        rand = (plan[:, :6].contiguous(), plan[:, 6:6 + L].contiguous(),
                plan[:, 6 + L:6 + 2 * L].contiguous())
        labels = self.labels.index_select(0, idx)
        if self.mix is None:
            x = ops.augment_rand_images(self.images, idx.contiguous(), boxes, flip, self._lut,
                                        self.augment.out_hw, *rand, fill=self.augment.fill)
        else:
            plan = plan[:, 6 + 2 * L:]
            partner = plan[:, 0].contiguous()
            x = ops.augment_rand_images(self.images, idx.contiguous(), boxes, flip, self._lut,
                                        self.augment.out_hw, *rand, partner,
                                        plan[:, 1].contiguous(), plan[:, 2:6].contiguous(),
                                        fill=self.augment.fill)
            labels = MixedLabels(labels, labels.index_select(0, partner.long()),
                                 plan[:, 6].contiguous().view(torch.float32))
        if self.flatten:
            x = x.reshape(B, -1)
        return x, labels

    def single_pass(self, batch_size=None):
        """This shard's examples in order, once, the remainder batch included, under the
        evaluation transform (centre crop, no flip).  Touches neither generator nor the
        training position."""
        bs = int(batch_size or self.batch_size)
        for pos in range(0, self.n, bs):
            idx = torch.arange(pos, min(pos + bs, self.n), device=self.device)
            yield self._gather(idx, train=False)

    def _gather(self, idx, train=True):
        from .. import ops
        B = idx.numel()
        if train and self.rand is not None:
            return self._train_rand(idx)
        if train and self.mix is not None:
            return self._train_mixed(idx)
        if train:
            boxes, flip = self._train_boxes(B)
        else:
            boxes = self._eval_box.expand(B, 4).contiguous()
            flip = torch.zeros(B, dtype=torch.uint8, device=self.device)
        x = ops.augment_images(self.images, idx.contiguous(), boxes, flip, self._lut,
                               self.augment.out_hw, self.augment.fill)
        if self.flatten:
            x = x.reshape(B, -1)
        return x, self.labels.index_select(0, idx)
