"""RandAugment on the CPU path: the integer rule of ops.augment_rand_images against a per-pixel
Python oracle, its identities and argument checks, randaugment_plan against hand-computed values,
the rule and the plan against PIL, the DeviceImageDataset with and without ``rand``, and the CLI
flags.  Every comparison but PIL's is exact."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import (DeviceImageDataset, ImageAugment, ImageMix,
                                            ImageRandAugment, MixedLabels, randaugment_plan)
from distributedtensorflow_amd.ops import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")
I32 = torch.int32
F64 = torch.float64
ONE = 65536
IDENTITY = [ONE, 0, 0, 0, ONE, 0]


# ----------------------------------------------------------------------------- the case table
# (shared with tests/test_randaug_gpu.py, which runs the kernel on it)

HS, WS, B = 20, 24, 6
OUT_HWS = [(16, 16), (15, 13)]             # Wo * C % 8 == 0 (16-B stores) and the tail path
FILL, RA_FILL = 17, 99
# every op code with the extremes of its parameter, and a value between them
POINT_OPS = [(0, 0), (1, 0), (2, 0), (2, 256), (2, 128), (3, 0), (3, 128), (3, 60), (4, 0),
             (4, 255), (4, 240), (5, 0), (5, 1 << 18), (5, 6554), (5, 95027), (6, 0),
             (6, 1 << 18), (6, 36045)]
REVERSAL = [5, 4, 3, 2, 1, 0]


def q16(*m):
    return [int(math.floor(v * ONE + 0.5)) for v in m]


def rotation(deg, Ho, Wo):
    r = -deg * math.pi / 180.0
    cs, sn, cx, cy = math.cos(r), math.sin(r), Wo / 2.0, Ho / 2.0
    return q16(cs, sn, cx - cx * cs - cy * sn, -sn, cs, cy + cx * sn - cy * cs)


def maps(Ho, Wo):
    return [IDENTITY,
            rotation(17.0, Ho, Wo),                        # corners leave the virtual image
            q16(1, 0.3, -2.25, -0.2, 1, 1.5),              # both shears and a shift
            q16(1, 0, Wo - 3.5, 0, 1, 0),                  # all but three columns outside
            q16(1, 0, 0, 0, 1, 2.0 * Ho),                  # everything outside
            q16(-1, 0, Wo, 0, 0.5, -0.75),                 # a mirror, rows doubled, one row outside
            rotation(-29.5, Ho, Wo)]


def rand_inputs(C):
    """(images, idx, boxes, flip): rows and their partners differ in image, box and flip."""
    g = torch.Generator().manual_seed(70 + C)
    images = torch.randint(0, 256, (10, HS, WS, C), generator=g, dtype=torch.uint8)
    idx = torch.tensor([3, 0, 9, 1, 3, 7])
    boxes = torch.tensor([[0, 0, HS, WS], [1, 2, 8, 5], [-2, -2, HS + 4, WS + 4], [3, 4, 1, 1],
                          [2, 1, 15, 17], [10, 12, 16, 16]], dtype=I32)
    flip = torch.tensor([1, 0, 1, 0, 0, 1], dtype=torch.uint8)
    return images, idx, boxes, flip


def rand_plans(out_hw):
    """[(aff, pops, ppar)], int32: L = 1 plans that walk every (code, parameter) over the rows,
    the maps rotating against them, and L = 4 plans with chains of four."""
    ms = maps(*out_hw)
    out = []
    for s in range(0, len(POINT_OPS), B):                  # L = 1
        pairs = [POINT_OPS[(s + i) % len(POINT_OPS)] for i in range(B)]
        aff = [ms[(s // B + i) % len(ms)] for i in range(B)]
        out.append((aff, [[c] for c, _ in pairs], [[m] for _, m in pairs]))
    for s in (0, 7):                                       # L = 4
        pairs = [[POINT_OPS[(s + 4 * i + k * (i + 1)) % len(POINT_OPS)] for k in range(4)]
                 for i in range(B)]
        aff = [ms[(s + 3 + i) % len(ms)] for i in range(B)]
        out.append((aff, [[c for c, _ in row] for row in pairs],
                    [[m for _, m in row] for row in pairs]))
    return [tuple(torch.tensor(t, dtype=I32) for t in plan) for plan in out]


def mix_plans(out_hw):
    """[(partner, lam_q, cut)]: every row kind next to every other; cut boxes cross the edges."""
    Ho, Wo = out_hw
    cuts = [(0, 0, 0, 0), (-2, -1, 4, 4), (Ho - 2, Wo - 2, 5, 5), (0, 0, Ho, Wo), (2, 3, 3, 2),
            (1, 1, 0, 4)]
    out = [(REVERSAL, [0, 32768, 65536, 1, 65535, 20000], [cuts[0]] * B),
           (REVERSAL, [65536] * B, cuts),
           ([1, 2, 0, 3, 5, 4], [32768, -5, 70000, 100, 65000, 0],
            [cuts[4], cuts[0], cuts[1], cuts[3], cuts[2], cuts[0]])]
    return [tuple(torch.tensor(t, dtype=I32) for t in plan) for plan in out]


def lut_of(C, dtype=torch.float32):
    return ImageAugment(4, mean=(0.485, 0.456, 0.406)[:C], std=(0.229, 0.224, 0.225)[:C]).lut(
        C, dtype, "cpu")


def cases(C, out_hw, mixed):
    """Every (aff, pops, ppar, partner, lam_q, cut) of the table; without a mix the last three
    are None."""
    for i, plan in enumerate(rand_plans(out_hw)):
        if not mixed:
            yield plan + (None, None, None)
        else:
            mp = mix_plans(out_hw)
            yield plan + mp[i % len(mp)]


# ----------------------------------------------------------------------------- the rule

def _axis(o, O, side):
    pos = ((2 * o + 1) * side * 256) // (2 * O) - 128
    pos = min(max(pos, 0), (side - 1) * 256)
    i0, f = pos >> 8, pos & 255
    return i0, min(i0 + 1, side - 1), f


def _clamp(t):
    return min(max(t, 0), 255)


def scalar_oracle(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, partner, lam_q, cut,
                  fill, ra_fill):
    """The issue's rule, one output pixel at a time, on Python ints."""
    img = images.numpy()
    N, Hs, Ws, C = img.shape
    Ho, Wo = out_hw
    nb = len(idx)
    out = torch.empty(nb, Ho, Wo, C, dtype=lut.dtype)

    def px(n, y, x, c):
        return int(img[n, y, x, c]) if 0 <= y < Hs and 0 <= x < Ws else fill

    def virtual(row, oy, ox, c):
        n = int(idx[row])
        y0, x0, h, w = (int(t) for t in boxes[row])
        iy0, iy1, fy = _axis(oy, Ho, h)
        ix0, ix1, fx = _axis(Wo - 1 - ox if int(flip[row]) else ox, Wo, w)
        top = (256 - fx) * px(n, y0 + iy0, x0 + ix0, c) + fx * px(n, y0 + iy0, x0 + ix1, c)
        bot = (256 - fx) * px(n, y0 + iy1, x0 + ix0, c) + fx * px(n, y0 + iy1, x0 + ix1, c)
        return ((256 - fy) * top + fy * bot + 32768) >> 16

    def value(row, oy, ox):
        a, b, c, d, e, f = (int(t) for t in aff[row])
        u = (a * (2 * ox + 1) + b * (2 * oy + 1) + 2 * c) >> 17
        v = (d * (2 * ox + 1) + e * (2 * oy + 1) + 2 * f) >> 17
        if 0 <= u < Wo and 0 <= v < Ho:
            x = [virtual(row, v, u, ch) for ch in range(C)]
        else:
            x = [ra_fill] * C
        for k in range(pops.shape[1]):
            code, m = int(pops[row, k]), int(ppar[row, k])
            if code == 1:
                x = [255 - t for t in x]
            elif code == 2:
                x = [t if t < m else 255 - t for t in x]
            elif code == 3:
                x = [min(255, t + m) if t < 128 else t for t in x]
            elif code == 4:
                x = [t & m for t in x]
            elif code == 5:
                x = [_clamp((t * m) >> 16) for t in x]
            elif code == 6 and C == 3:
                g = (19595 * x[0] + 38470 * x[1] + 7471 * x[2] + 32768) >> 16
                x = [_clamp((65536 * g + m * (t - g)) >> 16) for t in x]
            else:
                assert code in (0, 6)
        assert all(0 <= t <= 255 for t in x)
        return x

    for b in range(nb):
        if partner is not None:
            p = int(partner[b])
            q = min(max(int(lam_q[b]), 0), 65536)
            cy, cx, ch, cw = (int(t) for t in cut[b])
        for oy in range(Ho):
            for ox in range(Wo):
                v = value(b, oy, ox)
                if partner is not None and p != b:
                    vb = value(p, oy, ox)
                    inside = cy <= oy < cy + ch and cx <= ox < cx + cw
                    v = [tb if inside else (q * ta + (65536 - q) * tb + 32768) >> 16
                         for ta, tb in zip(v, vb)]
                for c in range(C):
                    out[b, oy, ox, c] = lut[c, v[c]]
    return out


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["16x16", "15x13"])
def test_reference_matches_scalar_oracle(C, out_hw, dtype, mixed):
    images, idx, boxes, flip = rand_inputs(C)
    lut = lut_of(C, dtype)
    table = list(cases(C, out_hw, mixed))
    if dtype == torch.bfloat16:
        table = table[:1] + table[-1:]                     # the table lookup is the only new part
    Ls, codes, outside = set(), set(), []
    for aff, pops, ppar, partner, lam_q, cut in table:
        got = reference.augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar,
                                            partner, lam_q, cut, fill=FILL, ra_fill=RA_FILL)
        want = scalar_oracle(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, partner,
                             lam_q, cut, FILL, RA_FILL)
        assert got.dtype == lut.dtype and got.shape == want.shape
        assert torch.equal(got, want)
        assert torch.equal(ops.augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff,
                                                   pops, ppar, partner, lam_q, cut, fill=FILL,
                                                   ra_fill=RA_FILL), want)
        Ls.add(pops.shape[1])
        codes |= set(zip(pops.flatten().tolist(), ppar.flatten().tolist()))
    if dtype == torch.float32:                             # the table covers what it says
        assert Ls == {1, 4} and codes >= set(POINT_OPS)


def test_the_maps_send_part_and_all_of_the_output_outside():
    for Ho, Wo in OUT_HWS:
        share = []
        for a, b, c, d, e, f in maps(Ho, Wo):
            n = 0
            for oy in range(Ho):
                for ox in range(Wo):
                    u = (a * (2 * ox + 1) + b * (2 * oy + 1) + 2 * c) >> 17
                    v = (d * (2 * ox + 1) + e * (2 * oy + 1) + 2 * f) >> 17
                    n += not (0 <= u < Wo and 0 <= v < Ho)
            share.append(n / (Ho * Wo))
        assert share[0] == 0 and share[4] == 1
        assert all(0 < s < 1 for s in share[1:4] + share[5:])


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_hw", OUT_HWS, ids=["16x16", "15x13"])
def test_identity_plan_is_the_unaugmented_op(C, out_hw):
    images, idx, boxes, flip = rand_inputs(C)
    lut = lut_of(C)
    aff = torch.tensor([IDENTITY] * B, dtype=I32)
    plain = reference.augment_images(images, idx, boxes, flip, lut, out_hw, fill=FILL)
    for L in (1, 4):
        zeros = torch.zeros(B, L, dtype=I32)
        got = ops.augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff, zeros, zeros,
                                      fill=FILL, ra_fill=RA_FILL)
        assert torch.equal(got, plain)
        for partner, lam_q, cut in mix_plans(out_hw):
            want = reference.augment_mix_images(images, idx, boxes, flip, lut, out_hw, partner,
                                                lam_q, cut, fill=FILL)
            got = ops.augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff, zeros, zeros,
                                          partner, lam_q, cut, fill=FILL, ra_fill=RA_FILL)
            assert torch.equal(got, want)
    # and a plan that is not the identity is not
    aff2, pops, ppar = rand_plans(out_hw)[0]
    assert not torch.equal(ops.augment_rand_images(images, idx, boxes, flip, lut, out_hw, aff2,
                                                   pops, ppar, fill=FILL), plain)


def test_argument_checks():
    images, idx, boxes, flip = rand_inputs(3)
    lut = lut_of(3)
    aff, pops, ppar = rand_plans((16, 16))[0]
    partner, lam_q, cut = mix_plans((16, 16))[0]

    def call(out_hw=(16, 16), **kw):
        a = dict(aff=aff, pops=pops, ppar=ppar)
        a.update(kw)
        return ops.augment_rand_images(images, idx, boxes, flip, lut, out_hw, **a)

    call()
    call(partner=partner, lam_q=lam_q, cut=cut)
    five = torch.zeros(B, 5, dtype=I32)
    none = torch.zeros(B, 0, dtype=I32)
    wide = torch.zeros(B, 8, dtype=I32)
    for bad in (dict(aff=aff.long()), dict(aff=aff[:, :5]), dict(aff=aff[:5]),
                dict(aff=aff.to("meta")), dict(aff=wide[:, :6]),        # not contiguous
                dict(pops=pops.long()), dict(pops=pops[:5]), dict(pops=pops.reshape(-1)),
                dict(pops=pops.to("meta")), dict(pops=wide[:, :1], ppar=ppar),
                dict(ppar=ppar.float()), dict(ppar=torch.cat([ppar, ppar], 1)),
                dict(ppar=ppar.to("meta")), dict(ppar=wide[:, :1]),
                dict(pops=five, ppar=five), dict(pops=none, ppar=none),  # L outside [1, 4]
                dict(out_hw=(1025, 16)), dict(out_hw=(16, 1025)),
                dict(ra_fill=256), dict(ra_fill=-1),
                dict(partner=partner), dict(partner=partner, lam_q=lam_q),
                dict(lam_q=lam_q, cut=cut),                              # all given or all None
                dict(partner=partner.long(), lam_q=lam_q, cut=cut)):
        with pytest.raises(ValueError):
            call(**bad)
    # the CPU path refuses what the rule does not define
    for code in (-1, 7):
        with pytest.raises(ValueError, match="code"):
            call(pops=torch.full_like(pops, code))
    for code, m in ((2, -1), (2, 257), (3, -1), (3, 129), (4, -1), (4, 256), (5, -1),
                    (5, (1 << 18) + 1), (6, -1), (6, (1 << 18) + 1)):
        with pytest.raises(ValueError, match="parameter"):
            call(pops=torch.full_like(pops, code), ppar=torch.full_like(ppar, m))
    call(pops=torch.zeros_like(pops), ppar=torch.full_like(ppar, -7))   # none takes no parameter
    with pytest.raises(ValueError, match="partner"):
        call(partner=torch.tensor([5, 4, B, 2, 1, 0], dtype=I32), lam_q=lam_q, cut=cut)
    with pytest.raises(ValueError, match="index"):
        ops.augment_rand_images(images, torch.tensor([3, 0, 10, 1, 3, 7]), boxes, flip, lut,
                                (16, 16), aff, pops, ppar)


# ----------------------------------------------------------------------------- the plan

NAMES = ("rotate", "shear_x", "shear_y", "translate_x", "translate_y", "invert", "solarize",
         "solarize_add", "posterize", "brightness", "color")


def _plan(rows, out_hw=(20, 30), **kw):
    """rows: per example a list of (op name, u1, u2, z) per layer, under all eleven ops."""
    ra = ImageRandAugment(num_layers=len(rows[0]), **kw)
    u = torch.tensor([[[(NAMES.index(n) + 0.5) / 11, u1, u2] for n, u1, u2, _ in row]
                      for row in rows], dtype=F64)
    z = torch.tensor([[t for _, _, _, t in row] for row in rows], dtype=F64)
    aff, pops, ppar = randaugment_plan(u, z, out_hw, ra)
    assert aff.dtype == pops.dtype == ppar.dtype == I32
    assert aff.shape == (len(rows), 6) and pops.shape == ppar.shape == z.shape
    assert aff.is_contiguous() and pops.is_contiguous() and ppar.is_contiguous()
    return aff.tolist(), pops.tolist(), ppar.tolist()


# magnitude 5 with mstd 5: z = -1, 0, 1 is l = 0, 0.5, 1
LEVELS = dict(magnitude=5.0, mstd=5.0, prob=1.0)


def test_plan_default_ops_and_settings():
    ra = ImageRandAugment()
    assert ra.ops == NAMES and ra.num_layers == 2 and ra.magnitude == 9.0 and ra.mstd == 0.5
    assert ra.prob == 0.5 and ra.translate == 0.45
    for kw in (dict(num_layers=0), dict(num_layers=5), dict(magnitude=-0.1), dict(magnitude=10.5),
               dict(mstd=-1.0), dict(prob=-0.1), dict(prob=1.1), dict(ops=("rotate", "cutout"))):
        with pytest.raises(ValueError):
            ImageRandAugment(**kw)


def test_plan_pointwise_magnitudes_at_three_levels():
    def pars(name, u2=0.0):
        aff, pops, ppar = _plan([[(name, 0.0, u2, z)] for z in (-1.0, 0.0, 1.0)], **LEVELS)
        assert aff == [IDENTITY] * 3
        return [p[0] for p in pops], [m[0] for m in ppar]

    assert pars("invert") == ([1] * 3, [0] * 3)
    assert pars("solarize") == ([2] * 3, [256, 128, 0])
    assert pars("solarize_add") == ([3] * 3, [0, 55, 110])
    assert pars("posterize") == ([4] * 3, [240, 192, 0])          # 4, 2, 0 bits
    # factors 1, 1.45, 1.9 and, with the sign flipped, 1, 0.55, max(0.1, 0.1)
    assert pars("brightness") == ([5] * 3, [65536, 95027, 124518])
    assert pars("brightness", 0.5) == ([5] * 3, [65536, 36045, 6554])
    assert pars("color") == ([6] * 3, [65536, 95027, 124518])
    assert pars("color", 0.75) == ([6] * 3, [65536, 36045, 6554])
    # SolarizeAdd's cap: only a larger factor than 110 would reach it; l is clamped to [0, 1]
    _, _, ppar = _plan([[("solarize", 0.0, 0.0, 5.0)], [("solarize", 0.0, 0.0, -5.0)]], **LEVELS)
    assert ppar == [[0], [256]]


def test_plan_geometric_magnitudes_at_three_levels():
    Ho, Wo = 20, 30

    def affs(name, u2=0.0):
        aff, pops, ppar = _plan([[(name, 0.0, u2, z)] for z in (-1.0, 0.0, 1.0)], **LEVELS)
        assert pops == [[0]] * 3 and ppar == [[0]] * 3
        return aff

    # shear 0, 0.15, 0.3: 0.15 * 65536 = 9830.4, 0.3 * 65536 = 19660.8
    assert affs("shear_x") == [IDENTITY, [ONE, 9830, 0, 0, ONE, 0], [ONE, 19661, 0, 0, ONE, 0]]
    assert affs("shear_x", 0.5) == [IDENTITY, [ONE, -9830, 0, 0, ONE, 0],
                                    [ONE, -19661, 0, 0, ONE, 0]]
    assert affs("shear_y") == [IDENTITY, [ONE, 0, 0, 9830, ONE, 0], [ONE, 0, 0, 19661, ONE, 0]]
    # shifts 0.45 l of the side: 6.75 and 13.5 of 30 columns, 4.5 and 9 of 20 rows
    assert affs("translate_x") == [IDENTITY, [ONE, 0, 442368, 0, ONE, 0],
                                   [ONE, 0, 884736, 0, ONE, 0]]
    assert affs("translate_y", 0.9) == [IDENTITY, [ONE, 0, 0, 0, ONE, -294912],
                                        [ONE, 0, 0, 0, ONE, -589824]]
    # rotations by 0, 15 and 30 degrees about (15, 10), and by -30
    assert affs("rotate") == [IDENTITY, rotation(15.0, Ho, Wo), rotation(30.0, Ho, Wo)]
    assert affs("rotate", 0.5)[2] == rotation(-30.0, Ho, Wo)
    c30, s30 = math.sqrt(3) / 2, -0.5
    assert rotation(30.0, Ho, Wo) == q16(c30, s30, 15 - 15 * c30 - 10 * s30, -s30, c30,
                                         10 + 15 * s30 - 10 * c30)


def test_plan_thresholds_and_op_selection():
    # applied iff u1 < prob, strictly; sign = -1 iff u2 >= 0.5
    rows = [[("shear_x", 0.59, 0.4999, 1.0)], [("shear_x", 0.6, 0.0, 1.0)],
            [("shear_x", 0.0, 0.5, 1.0)], [("invert", 0.6, 0.0, 1.0)]]
    aff, pops, _ = _plan(rows, magnitude=5.0, mstd=5.0, prob=0.6)
    assert aff == [[ONE, 19661, 0, 0, ONE, 0], IDENTITY, [ONE, -19661, 0, 0, ONE, 0], IDENTITY]
    assert pops == [[0]] * 4
    # the op is ops[min(floor(u0 K), K - 1)]
    ra = ImageRandAugment(num_layers=1, magnitude=10.0, mstd=0.0, prob=1.0)
    below = math.nextafter(1.0, 0.0)
    u = torch.tensor([[[0.0, 0.0, 0.0]], [[below, 0.0, 0.0]], [[1.0, 0.0, 0.0]],
                      [[5 / 11 + 1e-9, 0.0, 0.0]], [[5 / 11 - 1e-9, 0.0, 0.0]]], dtype=F64)
    aff, pops, ppar = randaugment_plan(u, torch.zeros(5, 1, dtype=F64), (20, 30), ra)
    assert aff[0].tolist() == rotation(30.0, 20, 30) and pops[0].tolist() == [0]
    assert pops[1:].flatten().tolist() == [6, 6, 1, 0] and ppar[1].tolist() == [124518]
    assert aff[4].tolist() == [ONE, 0, 0, 0, ONE, 589824]         # translate_y, ops[4]
    # a shorter list of ops
    ra = ImageRandAugment(num_layers=1, magnitude=10.0, mstd=0.0, prob=1.0,
                          ops=("invert", "shear_y"))
    u = torch.tensor([[[0.49, 0.0, 0.0]], [[0.5, 0.0, 0.0]]], dtype=F64)
    aff, pops, _ = randaugment_plan(u, torch.zeros(2, 1, dtype=F64), (20, 30), ra)
    assert pops.tolist() == [[1], [0]] and aff[1].tolist() == [ONE, 0, 0, 19661, ONE, 0]
    with pytest.raises(ValueError):
        randaugment_plan(u, torch.zeros(2, 2, dtype=F64), (20, 30), ra)


def test_plan_composes_geometric_ops_in_layer_order():
    # M = M_g1 M_g2: a shear_x of 0.3 then a translate_y of 9 rows, and the other way round
    s, t = 0.3, 9.0
    rows = [[("shear_x", 0.0, 0.0, 1.0), ("translate_y", 0.0, 0.0, 1.0)],
            [("translate_y", 0.0, 0.0, 1.0), ("shear_x", 0.0, 0.0, 1.0)],
            [("shear_x", 0.0, 0.0, 1.0), ("posterize", 0.0, 0.0, 1.0)],
            [("solarize", 0.0, 0.0, 0.0), ("shear_x", 0.9, 0.0, 1.0)]]
    aff, pops, ppar = _plan(rows, magnitude=5.0, mstd=5.0, prob=0.8)
    assert aff[0] == q16(1, s, s * t, 0, 1, t)
    assert aff[1] == q16(1, s, 0, 0, 1, t)
    assert aff[2] == q16(1, s, 0, 0, 1, 0) and aff[3] == IDENTITY
    # geometric and unapplied layers hold code 0
    assert pops == [[0, 0], [0, 0], [0, 4], [2, 0]] and ppar == [[0, 0], [0, 0], [0, 0], [128, 0]]
    # three layers: rotate, shear_y, translate_x against the 3 x 3 product in float64
    rows = [[("rotate", 0.0, 0.0, 0.0), ("shear_y", 0.0, 0.5, 1.0), ("translate_x", 0.0, 0.0, 0.0)]]
    aff, _, _ = _plan(rows, **LEVELS)
    r = -15.0 * math.pi / 180
    cs, sn = math.cos(r), math.sin(r)
    m1 = np.array([[cs, sn, 15 - 15 * cs - 10 * sn], [-sn, cs, 10 + 15 * sn - 10 * cs], [0, 0, 1]])
    m2 = np.array([[1, 0, 0], [-0.3, 1, 0], [0, 0, 1.0]])
    m3 = np.array([[1, 0, 6.75], [0, 1, 0], [0, 0, 1.0]])
    m = m1 @ m2 @ m3
    want = q16(*m[0], *m[1])
    assert all(abs(g - w) <= 1 for g, w in zip(aff[0], want))     # the order of the sums differs
    assert abs(aff[0][2] - q16((m1 @ m3 @ m2)[0, 2])[0]) > 1000   # and the order of the ops shows


def test_plan_with_prob_zero_is_the_identity_and_draws_are_fixed():
    ra = ImageRandAugment(num_layers=3, prob=0.0)
    u, z = ra.draw(50, torch.Generator().manual_seed(4))
    assert u.shape == (50, 3, 3) and z.shape == (50, 3) and u.dtype == z.dtype == F64
    aff, pops, ppar = randaugment_plan(u, z, (20, 30), ra)
    assert aff.tolist() == [IDENTITY] * 50 and not pops.any() and not ppar.any()
    # the order of the draws: the uniforms, then the normals, whatever mstd is
    g = torch.Generator().manual_seed(4)
    assert torch.equal(u, torch.rand(50, 3, 3, generator=g, dtype=F64))
    assert torch.equal(z, torch.randn(50, 3, generator=g, dtype=F64))
    u0, z0 = ImageRandAugment(num_layers=3, mstd=0.0).draw(50, torch.Generator().manual_seed(4))
    assert torch.equal(u0, u) and torch.equal(z0, z)
    # a strategy scope sets a default device: the draws and the plan stay on the host
    with torch.device("meta"):
        d = ra.draw(50, torch.Generator(device="cpu").manual_seed(4))
        again = randaugment_plan(*d, (20, 30), ra)
    assert all(t.device.type == "cpu" for t in d + again)
    # the default settings produce every op and valid parameters: the CPU path accepts the plan
    ra = ImageRandAugment()
    aff, pops, ppar = randaugment_plan(*ra.draw(400, torch.Generator().manual_seed(1)), (8, 8), ra)
    assert set(pops.flatten().tolist()) == set(range(7))
    assert int((aff != torch.tensor(IDENTITY, dtype=I32)).any(1).sum()) > 100
    images = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    ops.augment_rand_images(images, torch.zeros(400, dtype=torch.int64),
                            torch.tensor([[0, 0, 4, 4]] * 400, dtype=I32),
                            torch.zeros(400, dtype=torch.uint8), lut_of(3), (8, 8), aff, pops, ppar)


# ----------------------------------------------------------------------------- against PIL

def _pil_case(side, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (1, side, side, 3), generator=g, dtype=torch.uint8)


def _ours(images, aff, pops, ppar):
    """The rule on one image: a box of the output's size, no flip, ra_fill 128, and a table that
    holds the value itself."""
    side = images.shape[1]
    lut = torch.arange(256, dtype=torch.float32).repeat(3, 1)
    out = ops.augment_rand_images(images, torch.zeros(1, dtype=torch.int64),
                                  torch.tensor([[0, 0, side, side]], dtype=I32),
                                  torch.zeros(1, dtype=torch.uint8), lut, (side, side),
                                  aff, pops, ppar, fill=0, ra_fill=128)
    return out[0].to(torch.int64).numpy()


def _single(name, sign_u, side, **kw):
    """The plan of one applied op at level 1."""
    ra = ImageRandAugment(num_layers=1, mstd=0.0, prob=1.0, ops=(name,), **kw)
    return randaugment_plan(torch.tensor([[[0.0, 0.0, sign_u]]], dtype=F64),
                            torch.zeros(1, 1, dtype=F64), (side, side), ra)


def test_pointwise_ops_equal_pil():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageOps
    images = _pil_case(32, 11)
    pil = Image.fromarray(images[0].numpy())
    aff = torch.tensor([IDENTITY], dtype=I32)

    def ours(code, m):
        return _ours(images, aff, torch.tensor([[code]], dtype=I32), torch.tensor([[m]], dtype=I32))

    assert np.array_equal(ours(1, 0), np.asarray(ImageOps.invert(pil)))
    for m in (0, 1, 77, 128, 255, 256):
        assert np.array_equal(ours(2, m), np.asarray(ImageOps.solarize(pil, m)))
    for m in (0, 1, 55, 110, 128):                        # timm's solarize_add
        table = [min(255, i + m) if i < 128 else i for i in range(256)]
        assert np.array_equal(ours(3, m), np.asarray(pil.point(table * 3)))
    for bits in (1, 2, 3, 4):
        assert np.array_equal(ours(4, 256 - (1 << (8 - bits))),
                              np.asarray(ImageOps.posterize(pil, bits)))
    # and through the plan: magnitude 10 is Solarize 0, magnitude 5 Posterize to 2 bits
    _, pops, ppar = _single("solarize", 0.0, 32, magnitude=10.0)
    assert np.array_equal(_ours(images, aff, pops, ppar), np.asarray(ImageOps.solarize(pil, 0)))
    _, pops, ppar = _single("posterize", 0.0, 32, magnitude=5.0)
    assert np.array_equal(_ours(images, aff, pops, ppar), np.asarray(ImageOps.posterize(pil, 2)))


def test_geometric_ops_match_pil():
    Image = pytest.importorskip("PIL.Image")
    side = 32
    images = _pil_case(side, 12)
    pil = Image.fromarray(images[0].numpy())
    grey = (128, 128, 128)

    def affine(*m):
        return pil.transform(pil.size, Image.AFFINE, m, resample=Image.NEAREST, fillcolor=grey)

    none = torch.zeros(1, 1, dtype=I32)
    table = [("shear_x 0.21", _single("shear_x", 0.0, side, magnitude=7.0)[0],
              affine(1, 0.21, 0, 0, 1, 0)),
             ("shear_y 0.21", _single("shear_y", 0.0, side, magnitude=7.0)[0],
              affine(1, 0, 0, 0.21, 1, 0)),
             ("translate_x 5.3", _single("translate_x", 0.0, side, magnitude=10.0,
                                         translate=5.3 / side)[0], affine(1, 0, 5.3, 0, 1, 0)),
             ("rotate 17", _single("rotate", 0.0, side, magnitude=17.0 / 3.0)[0],
              pil.rotate(17.0, resample=Image.NEAREST, fillcolor=grey)),
             ("rotate -29.5", _single("rotate", 0.5, side, magnitude=29.5 / 3.0)[0],
              pil.rotate(-29.5, resample=Image.NEAREST, fillcolor=grey))]
    for name, aff, want in table:
        got, want = _ours(images, aff, none, none), np.asarray(want).astype(np.int64)
        differ = float((got != want).any(axis=2).mean())
        print(f"{name}: {differ:.4%} of pixels differ from PIL")
        assert (got == 128).all(axis=2).any() and not (got == 128).all()   # some fill, not all
        assert differ <= 0.005, name


def test_brightness_and_color_match_pil():
    """Factors 0.10 .. 1.90 in steps of 0.01: every element within 1 of PIL, and at most 5 % of
    the elements, counted over all factors of an op, differ.  (Per factor the share can sit at
    the bound by construction: PIL multiplies by the float factor and truncates, the rule by the
    factor rounded to 1/65536, so with 0.15 -> 9830 / 65536 every x that is a multiple of 20
    lands just below its integer, 13 of 256 byte values = 5.08 %.  The per-factor worst is
    printed.)"""
    pytest.importorskip("PIL.Image")
    from PIL import Image, ImageEnhance
    images = _pil_case(64, 13)
    pil = Image.fromarray(images[0].numpy())
    aff = torch.tensor([IDENTITY], dtype=I32)
    worst, differing, total = {5: 0.0, 6: 0.0}, {5: 0, 6: 0}, {5: 0, 6: 0}
    for i in range(10, 191):
        factor = i / 100.0
        m = torch.tensor([[int(math.floor(65536 * factor + 0.5))]], dtype=I32)
        for code, enhance in ((5, ImageEnhance.Brightness), (6, ImageEnhance.Color)):
            got = _ours(images, aff, torch.tensor([[code]], dtype=I32), m)
            want = np.asarray(enhance(pil).enhance(factor)).astype(np.int64)
            assert int(np.abs(got - want).max()) <= 1, (code, factor)
            differing[code] += int((got != want).sum())
            total[code] += got.size
            worst[code] = max(worst[code], float((got != want).mean()))
    share = {k: differing[k] / total[k] for k in total}
    print(f"share of elements off by one over all factors: brightness {share[5]:.4%}, color "
          f"{share[6]:.4%}; the worst single factor: {worst[5]:.4%}, {worst[6]:.4%}")
    assert share[5] <= 0.05 and share[6] <= 0.05


# ----------------------------------------------------------------------------- the dataset

def _arrays(n=24, seed=3):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, 12, 10, 3)).astype(np.uint8), rng.randint(0, 10, n)


AUG = ImageAugment((8, 8), mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3), fill=7)
KW = dict(shuffle=True, seed=1, aug_seed=2)


def _states(ds):
    return [g.get_state() for g in (ds._gen, ds._aug_gen)] + \
        ([ds._mix_gen.get_state()] if ds.mix is not None else []) + \
        ([ds._rand_gen.get_state()] if ds.rand is not None else [])


def test_dataset_with_rand_keeps_order_labels_and_crops(monkeypatch):
    imgs, labels = _arrays()
    ra = ImageRandAugment(num_layers=2, magnitude=9.0, prob=0.7)
    plain = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, **KW)
    rand = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ra, rand_seed=5, **KW)
    twin = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ra, rand_seed=5, **KW)
    other = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ra, rand_seed=6, **KW)
    off = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ImageRandAugment(prob=0.0),
                             rand_seed=5, **KW)
    seen = []
    real = ops.augment_rand_images

    def spy(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, *mix, **kw):
        seen.append((idx.clone(), boxes.clone(), flip.clone(), aff.clone(), pops.clone(),
                     ppar.clone()))
        assert not mix and kw.get("ra_fill", 128) == 128 and kw["fill"] == 7
        return real(images, idx, boxes, flip, lut, out_hw, aff, pops, ppar, *mix, **kw)

    monkeypatch.setattr(ops, "augment_rand_images", spy)
    differs = changed = False
    for _ in range(6):                                     # over an epoch boundary
        xp, yp = next(plain)
        xr, yr = next(rand)
        idx, boxes, flip, aff, pops, ppar = seen[-1]
        xt, yt = next(twin)
        xo, yo = next(other)
        xf, yf = next(off)
        assert not isinstance(yr, MixedLabels) and torch.equal(yr, yp)
        assert xr.shape == xp.shape and xr.dtype == xp.dtype
        # the same examples under the same crops and flips
        assert torch.equal(reference.augment_images(plain.images, idx, boxes, flip, plain._lut,
                                                    (8, 8), 7), xp)
        assert aff.shape == (6, 6) and pops.shape == ppar.shape == (6, 2)
        assert torch.equal(reference.augment_rand_images(plain.images, idx, boxes, flip,
                                                         plain._lut, (8, 8), aff, pops, ppar,
                                                         fill=7), xr)
        # the same seeds agree; another rand_seed changes the plan alone; prob = 0 changes nothing
        assert torch.equal(xt, xr) and torch.equal(yt, yr)
        assert torch.equal(yo, yr)
        assert torch.equal(xf, xp) and torch.equal(yf, yp)
        differs |= not torch.equal(xo, xr)
        changed |= not torch.equal(xr, xp)
    assert differs and changed
    for a, b in zip(_states(plain), _states(rand)[:2]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand="m9")
    with pytest.raises(ValueError):
        DeviceImageDataset(imgs, labels, 6, "cpu", ImageAugment((8, 1025)), rand=ra)


def test_dataset_without_rand_is_unchanged():
    imgs, labels = _arrays()
    mix = ImageMix(mixup_alpha=0.4, cutmix_alpha=1.0)
    for kw in (dict(), dict(mix=mix, mix_seed=3)):
        old = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, **KW, **kw)
        new = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=None, rand_seed=9, **KW, **kw)
        for _ in range(5):
            (xo, yo), (xn, yn) = next(old), next(new)
            assert torch.equal(xo, xn)
            assert all(torch.equal(a, b) for a, b in zip(yo, yn)) if kw else torch.equal(yo, yn)
        for a, b in zip(_states(old), _states(new)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_dataset_with_rand_and_mix_yields_mixed_labels(mode):
    imgs, labels = _arrays()
    mix = ImageMix(mixup_alpha=0.4, cutmix_alpha=1.0, mode=mode)
    ra = ImageRandAugment(num_layers=3, prob=0.8)
    kw = dict(mix=mix, mix_seed=3, **KW)
    mixed = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, **kw)
    both = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ra, rand_seed=4, **kw)
    off = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ImageRandAugment(prob=0.0),
                             rand_seed=4, **kw)
    changed = False
    for _ in range(6):
        xm, ym = next(mixed)
        xb, yb = next(both)
        xf, yf = next(off)
        assert isinstance(yb, MixedLabels) and isinstance(yf, MixedLabels)
        # the mix plan and the labels are those of the dataset without rand
        assert all(torch.equal(a, b) for a, b in zip(yb, ym))
        assert all(torch.equal(a, b) for a, b in zip(yf, ym))
        assert yb.lam.dtype == torch.float32 and xb.shape == xm.shape
        assert torch.equal(xf, xm)
        changed |= not torch.equal(xb, xm)
    assert changed
    for a, b in zip(_states(mixed), _states(both)[:3]):
        assert torch.equal(a, b)


def test_single_pass_never_applies_it_and_touches_no_generator():
    imgs, labels = _arrays(n=23)
    ds = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ImageRandAugment(prob=1.0),
                            rand_seed=3, mix=ImageMix(mixup_alpha=1.0), mix_seed=4, **KW)
    twin = DeviceImageDataset(imgs, labels, 6, "cpu", AUG, rand=ImageRandAugment(prob=1.0),
                              rand_seed=3, mix=ImageMix(mixup_alpha=1.0), mix_seed=4, **KW)
    plain = DeviceImageDataset(imgs, labels, 6, "cpu", AUG)
    next(ds)
    next(twin)
    before = _states(ds)
    got = list(ds.single_pass())
    assert sum(len(y) for _, y in got) == 23
    for (x, y), (xp, yp) in zip(got, plain.single_pass()):
        assert not isinstance(y, MixedLabels)
        assert torch.equal(x, xp) and torch.equal(y, yp)
    assert len(before) == 4
    for a, b in zip(before, _states(ds)):
        assert torch.equal(a, b)
    # and the next training batch is what it would have been
    (xa, ya), (xb, yb) = next(ds), next(twin)
    assert torch.equal(xa, xb) and all(torch.equal(a, b) for a, b in zip(ya, yb))


# ----------------------------------------------------------------------------- CLI

def _env():
    e = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        e.pop(k, None)
    return e


def write_set(d, C=1, side=32):
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(0)
    for split, n in (("train", 40), ("val", 13)):
        np.save(os.path.join(d, f"{split}_images.npy"),
                rng.randint(0, 256, (n, side, side, C)).astype(np.uint8))
        np.save(os.path.join(d, f"{split}_labels.npy"), rng.randint(0, 10, n))


def _train(tmp_path, *flags):
    return subprocess.run([sys.executable, TRAIN, "--device", "cpu", "--train_steps", "3",
                           "--log_dir", str(tmp_path / "tb"), *flags],
                          capture_output=True, text=True, env=_env(), timeout=300)


def _result(r):
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_cli_randaugment_flags(tmp_path):
    d = str(tmp_path / "set")
    write_set(d)
    base = ("--model", "mnist_cnn", "--image_data", d, "--augment", "pad_crop", "--batch_size",
            "8")
    res = _result(_train(tmp_path, *base, "--randaugment", "2", "--eval"))
    assert res["global_step"] == 3 and math.isfinite(res["final_loss"])
    assert (res["randaugment"], res["ra_magnitude"], res["ra_mstd"], res["ra_prob"]) == \
        (2, 9.0, 0.5, 0.5)
    assert res["eval_count"] == 13                         # evaluation is complete and plain
    # with a mix and the other settings
    both = _result(_train(tmp_path, *base, "--randaugment", "3", "--ra_magnitude", "7",
                          "--ra_mstd", "0", "--ra_prob", "1", "--mixup_alpha", "0.2",
                          "--augment", "rrc"))
    assert (both["randaugment"], both["ra_magnitude"], both["ra_mstd"], both["ra_prob"]) == \
        (3, 7.0, 0.0, 1.0)
    assert both["mixup_alpha"] == 0.2 and math.isfinite(both["final_loss"])
    # without the flag the result is what it was: no new key, and the same loss twice
    plain = _result(_train(tmp_path, *base))
    again = _result(_train(tmp_path, *base, "--randaugment", "0", "--ra_magnitude", "3"))
    assert set(plain) == set(again) == {"model", "strategy", "replicas", "global_step",
                                        "elapsed_s", "final_loss", "examples_per_sec"}
    assert plain["final_loss"] == again["final_loss"] != res["final_loss"]


@pytest.mark.parametrize("flags,message", [
    (("--model", "mnist_cnn", "--randaugment", "2"), "needs --image_data"),
    (("--model", "bert_base", "--randaugment", "2"), "bert_base"),
    (("--model", "mnist_cnn", "--image_data", "SET", "--randaugment", "5"), "1 to 4"),
    (("--model", "mnist_cnn", "--image_data", "SET", "--randaugment", "2", "--ra_magnitude",
      "11"), "ra_magnitude"),
])
def test_cli_refusals(tmp_path, flags, message):
    d = str(tmp_path / "set")
    write_set(d)
    r = _train(tmp_path, *[d if f == "SET" else f for f in flags])
    assert r.returncode != 0 and message in r.stderr
