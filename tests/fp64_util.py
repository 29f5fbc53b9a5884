"""Helpers of the per-element fp64 comparison in tests/test_stream_kernels_gpu.py: the error
constants, the bf16 grid in fp64 (rounding, truncation, spacing, fragile elements), the exact and
bounded assertions with their ``MEASURE`` line, and sentinel-guarded buffers."""
import math

import torch

BF16 = torch.bfloat16
U16 = 2.0 ** -8             # bf16 spacing relative to the value (twice the unit roundoff)
U32 = 2.0 ** -24
FTZ = 2.0 ** -126
SENT = -1.7e38              # guard value (a bf16 / fp32 nobody computes)
GUARD = 4096                # margin elements each side (8 KB bf16, 16 KB fp32)


def gamma(n):
    assert n * U32 < 1
    return n * U32 / (1.0 - n * U32)


def bf(t):
    """Round to bf16 (nearest even), back as fp64: the value a kernel reads or stores."""
    return t.to(BF16).double()


def trunc_bf16(t32):
    """fp32 -> bf16 by dropping the low 16 bits (a damage)."""
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def ulp16(v):
    """Spacing of the bf16 grid in the binade of ``v`` (2^-8 at 0: never used there)."""
    _, e = torch.frexp(v.abs().double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def fragile_round(v, err):
    """An fp64 value ``v`` that a kernel evaluates in fp32 to within ``err`` and then rounds to
    bf16: (fragile, allowance).  ``fragile``: a rounding boundary (the midpoint of two bf16
    neighbours) lies within ``err`` of ``v``, so the kernel may land on either neighbour.  The
    allowance is what the kernel's rounded value may then differ by from ``bf(v)``: one spacing
    -- or, where ``err`` itself reaches half a spacing (cancellation: the linearisation in one
    spacing no longer holds), ``err`` plus one spacing at ``|v| + err``."""
    u = ulp16(v)
    q = v.abs() / u
    dist = ((q - q.floor()) - 0.5).abs() * u
    frag = dist <= err
    allow = torch.where(err < u / 2, u, err + ulp16(v.abs() + err))
    return frag, torch.where(frag, allow, torch.zeros_like(allow))


def assert_within(got, ref64, bound, what=""):
    g64 = got.detach().double().cpu()
    ref64, bound = ref64.detach().double().cpu(), bound.detach().double().cpu()
    bound = bound.expand_as(ref64) + FTZ
    assert g64.shape == ref64.shape, (what, g64.shape, ref64.shape)
    assert bool(torch.isfinite(g64).all()), f"{what}: non-finite result"
    err = (g64 - ref64).abs()
    bad = err > bound
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        flat = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), ratio.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at "
            f"{idx}: got {g64[idx].item()!r} ref {ref64[idx].item()!r} err {err[idx].item():.3e} "
            f"= {ratio[idx].item():.3g} x bound {bound[idx].item():.3e}")


def assert_exact(got, ref64, what=""):
    g64 = got.detach().double().cpu()
    ref64 = ref64.detach().double().cpu()
    assert g64.shape == ref64.shape, (what, g64.shape, ref64.shape)
    if not torch.equal(g64, ref64):
        bad = g64 != ref64
        idx = tuple(int(v[0]) for v in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at "
                             f"{idx}: got {g64[idx].item()!r} ref {ref64[idx].item()!r}")


def measure(name, got, ref64, bound):
    err = (got.detach().double().cpu() - ref64).abs()
    r = float((err / (bound.expand_as(ref64) + FTZ)).max()) if err.numel() else 0.0
    print(f"MEASURE {name} {r:.4f}")
    return r


def assert_normal_f32(got, what=""):
    """An fp32 result is the exact 0 or a normal number."""
    g = got.detach().double().cpu().abs()
    assert bool(((g == 0) | (g >= FTZ)).all()), f"{what}: denormal fp32 result"


def guarded(shape, dtype, fill=SENT, device="cuda"):
    """A tensor of ``shape`` inside a larger sentinel-filled allocation -> (view, whole)."""
    n = math.prod(shape)
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
    return whole[GUARD:GUARD + n].view(shape), whole


def assert_guards(whole, what, fill=SENT):
    s = torch.tensor(fill, dtype=whole.dtype).item()
    lo, hi = whole[:GUARD].cpu(), whole[-GUARD:].cpu()
    assert bool((lo == s).all()), f"{what}: wrote below the buffer"
    assert bool((hi == s).all()), f"{what}: wrote past the buffer"
