"""The convolution kernels of ``csrc/kernels/conv.hip``, ``conv_wgrad.hip`` and the implicit-GEMM
form in ``gemm.hip`` element by element against fp64, on every route of the two dispatchers.
The kernels are called through ``native.conv2d_forward`` / ``conv2d_dgrad`` / ``conv2d_wgrad``
and, where an epilogue has no public entry or the test owns the output buffer, through
``native._K.conv_igemm`` / ``_K.conv_wgrad`` the way ``_launch_fwd`` / ``conv2d_wgrad`` do.  Data
is made on the CPU with seeded generators; every ``*_set_*`` knob is restored in ``finally``.

Method
------
*References.*  ``torch.nn.functional.conv2d``, ``torch.nn.grad.conv2d_input`` and
``conv2d_weight`` in fp64 on the CPU, on the bf16-rounded operands, with the padding of
``reference.resolve_padding`` applied explicitly (so the asymmetric SAME padding of even kernels
is the reference's too).

*Routes.*  Every case names the kernel it is meant for and asserts it: the calls of
``_K.conv_igemm`` / ``_K.conv_wgrad`` are watched and their arguments handed to
``_K.conv_route`` / ``_K.conv_wgrad_route``, the functions the two dispatchers branch on
(conv.hip ``conv_route``, conv_wgrad.hip ``wgrad_route``).  The route functions are host code, so
``test_routes_dry`` checks the whole table without a GPU.

*Exact mode* (the main instrument, no tolerance).  x integer in [-2, 2], filters in {-1, 0, 1},
dy integer in [-2, 2], accumulate bases integer in [-8, 8].  Every product and partial sum is an
integer below 2^24 (asserted on the reference: ``sum |a b| < 2^24``), hence exact in fp32 in any
order and under any MFMA-internal rounding, and the kernel must return exactly
``ref64.to(bfloat16)`` (bf16 outputs) or ``ref64.float()`` (the fp32 weight gradient).  The
sums pass 256, so the bf16 store's round-to-nearest-even (ties included) is part of the check.

*Bound mode.*  The same cases on Gaussian data, filters scaled by ``(T C)^-1/2``:
``|got - ref64| <= k u |ref64| + F gamma(n + 8) mag`` per element, ``u = 2^-8``, ``k`` the bf16
roundings on the path, ``n`` the reduction length (``T C`` forward, the taps of the class times
``K`` for a data gradient -- bounded by ``T K``), ``mag = sum |a b|`` from the same fp64 conv on
``|x|``, ``|w|``.  The fp32 weight gradient: ``k = 0``, ``n = N P Q +`` the split count, and a
value is the exact 0 or at least ``FTZ``.  ``F = 1`` (see profiles/CONV_KERNELS.md for the
measured ratios; every ``MEASURE`` line is the largest ``err / bound`` of one call).

Rounding points (read from the epilogues)
    register / gather kernels (conv.hip conv_igemm_body l.395-450): ``v = acc + bias``,
        ``relu``, ``f2bf`` into the LDS tile (ONE rounding); the BN statistics sum the ROUNDED
        value; ``acc`` 1 / 2 then reads that bf16 tile back, adds the base (``acc_add8`` l.46-60)
        in fp32 and rounds AGAIN: the result is ``bf16(bf16(conv) + base)``, two roundings, and
        the reference does the same.  The DMA kernel (l.739) and the persistent GEMM
        (gemm.hip l.1238-1258, ``h = f2bf(bf2f(h) + src)``) round twice in the same way.
    bias / ReLU: ``bf16(relu(conv + bias))``, one rounding (l.403-405).
    halo kernels: one rounding; no ``acc`` (halo_family refuses ``g.acc``).  BN on load:
        ``ly = bf16(max(x lsc + lsh, 0))`` and y is the conv of that ROUNDED tensor.
    BN-backward sums (BnbAcc l.73-133): fp32 sums of the bf16 value just stored, so they are
        compared with fp64 sums of the kernel's own stored dx (the stage-wise rule).
    weight gradient: fp32 slabs summed in split order, the old dW added last (slab reduce).

Exact-mode side conditions (asserted on the reference in each case)
    stats     ``|y| <= 128`` (sparser filters), so a 256-row tile's ``sum y^2 < 2^24``
    BN sums   integer mean in {-1, 0, 1}, invstd in {0.5, 1, 2}, fsc in {-1, 1, 2},
              fsh = k + 0.5, so ``min |x fsc + fsh| >= 0.5`` and the mask-kind-2 decision never
              sits at zero; ``sum |dz (x - mean) invstd| < 2^23`` (half-integers)

Guard rows.  Where the test owns the output (direct ``_K`` calls, ``out=``, the weight
gradient's slab workspace) the buffer sits inside a larger allocation filled with a sentinel, and
both margins (8 KB bf16 / 16 KB fp32) must be unchanged afterwards; the output itself starts as
the sentinel, so an element the kernel never wrote differs from the reference.

Cases -> routes (shape tuples are ``(N, H, W, C, Kout, R, stride, pad)`` of the FORWARD conv)
    FWD        one entry per forward route; the comment at each entry says what it is for
    FWD_EPI    stats / bias / ReLU / BN on load / non-temporal stores, by direct launch
    DGRAD      stride-1 (register, halo, GEMM; plain, ``out=``, ``acc_from``), stride 2 grouped
               and per class, 1x1 stride 2 (``need_zero``), 7x7 / 2 at C = 8, 5x5 SAME
    DGRAD_BNB  the BN-backward sums on the register, DMA and halo kernels, mask kinds 0, 1, 2,
               and a stride-2 case where the grouped launch must not run
    WGRAD      generic, register, DMA 2x2 / narrow with pipes 0..3, dense, ping-pong forms,
               halo, stem, slab reduce with and without accumulate

*CPU self-tests* (unmarked).  A torch emulation (fp32 accumulation in two different orders, one
bf16 rounding) equals the reference bit for bit in exact mode and lies inside the bound in bound
mode on every shape, which also proves the side conditions before a GPU is touched; each listed
damage (``DAMAGES``) falls outside the check in both modes -- truncation instead of rounding on
the bf16 store in bound mode only: on integers below 2^8 times a power of two truncation and
rounding agree too often to rely on.

Measured on an MI355X with F = 1 (profiles/CONV_KERNELS.md): the fp32 weight gradient, whose
ratio is the fp32 term alone, reaches at most 0.048 of its bound on any route (at M = 35, one
split: gamma(44)), the fused sums 0.029; the bf16 outputs reach 0.99 of theirs, all of it
the ``k u |ref|`` term.  F stays 1.

Found by this file: ``native.conv2d_wgrad`` raised on a 56-wide conv of ONE strip (N = 1,
H = 4: the halo route reports one split and no slab workspace was allocated; ``test_wgrad`` at
``halo_n1``) -- fixed in ``conv2d_wgrad``.  ``wgrad_set_dense(3)`` selects a timing probe with
wrong results by design (conv_wgrad.hip, FORM 3), so it has no case here.  No kernel fault.
"""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from distributedtensorflow_amd.ops import reference as R

BF16 = torch.bfloat16
U16 = 2.0 ** -8
U32 = 2.0 ** -24
FTZ = 2.0 ** -126
FACTOR = 1.0                # F of the bound (profiles/CONV_KERNELS.md)
SENT = -1.7e38              # guard value (a bf16 / fp32 nobody computes)
GUARD = 4096                # margin elements each side (8 KB bf16, 16 KB fp32)
EXACT, BOUND = "exact", "bound"
MODES = [EXACT, BOUND]


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module", autouse=True)
def _leave_allocator_as_found():
    """This file allocates hundreds of small, odd-sized buffers (guard margins, slabs).  Left in
    torch's caching allocator they change which cached block later tests are handed, and with it
    the ``max_memory_allocated`` that test_resnet_gpu compares between steps to within 4 MB; so
    the cached blocks are released when the module is done."""
    yield
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _native():
    from distributedtensorflow_amd.ops import native
    return native


def _K():
    return _native()._K


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def gamma(n):
    assert n * U32 < 1
    return n * U32 / (1.0 - n * U32)


def _bf(t):
    """Round to bf16, back as fp64: the value a kernel reads (or stores)."""
    return t.to(BF16).double()


# ----------------------------------------------------------------------------- assertions
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


def _measure(name, got, ref64, bound):
    err = (got.detach().double().cpu() - ref64).abs()
    r = float((err / (bound.expand_as(ref64) + FTZ)).max()) if err.numel() else 0.0
    print(f"MEASURE {name} {r:.4f}")
    return r


def check(got, case, what, k=1):
    """The check of one bf16 output (``k`` roundings) or, ``k = 0``, one fp32 output, against the
    dict ``case`` (mode, ref, mag, n).  ``ref`` is the UNROUNDED fp64 value unless ``k = 2``
    (then the caller has applied the first rounding; see the docstring)."""
    ref, mode = case["ref"], case["mode"]
    if mode == EXACT:
        assert float(case["mag"].max()) < 2.0 ** 24, (what, float(case["mag"].max()))
        assert_exact(got, _bf(ref) if k else ref.float().double(), what)
        return
    # every rounding is relative to the value rounded: ``round_mag`` when they differ (acc)
    bound = U16 * case.get("round_mag", k * ref.abs()) + FACTOR * gamma(case["n"] + 8) * case["mag"]
    _measure(what, got, ref, bound)
    assert_within(got, ref, bound, what)
    if k == 0:      # an fp32 result is the exact 0 or a normal number
        g = got.detach().double().cpu().abs()
        assert bool(((g == 0) | (g >= FTZ)).all()), f"{what}: denormal fp32 result"


# ----------------------------------------------------------------------------- references
def _pads(shape):
    N, H, W, C, K, Rk, stride, pad = shape
    return R.resolve_padding(pad, H, W, Rk, Rk, stride)


def _out_hw(shape):
    N, H, W, C, K, Rk, stride, pad = shape
    sh, sw = _pair(stride)
    pt, pb, pl, pr = _pads(shape)
    return (H + pt + pb - Rk) // sh + 1, (W + pl + pr - Rk) // sw + 1


def ref_fwd(x, w, shape):
    """x [N,H,W,C], w [K,R,S,C] (any float dtype) -> y [N,P,Q,K]; explicit padding."""
    pt, pb, pl, pr = _pads(shape)
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xn, w.permute(0, 3, 1, 2), None, _pair(shape[6])).permute(0, 2, 3, 1)


def ref_dgrad(dy, w, shape):
    """dy [N,P,Q,K], w [K,R,S,C] -> dx [N,H,W,C]."""
    N, H, W, C, K, Rk, stride, pad = shape
    pt, pb, pl, pr = _pads(shape)
    full = torch.nn.grad.conv2d_input((N, C, H + pt + pb, W + pl + pr), w.permute(0, 3, 1, 2),
                                      dy.permute(0, 3, 1, 2), _pair(stride), 0)
    return full[:, :, pt:pt + H, pl:pl + W].permute(0, 2, 3, 1)


def ref_wgrad(x, dy, shape):
    """x [N,H,W,C], dy [N,P,Q,K] -> dw [K,R,S,C]."""
    N, H, W, C, K, Rk, stride, pad = shape
    pt, pb, pl, pr = _pads(shape)
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    dw = torch.nn.grad.conv2d_weight(xn, (K, C, Rk, Rk), dy.permute(0, 3, 1, 2), _pair(stride), 0)
    return dw.permute(0, 2, 3, 1)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _operands(shape, mode, salt=0, wdens=1.0):
    """(x, w, dy) as fp64 holding bf16-representable values."""
    N, H, W, C, K, Rk, stride, pad = shape
    P, Q = _out_hw(shape)
    s = sum(int(v) * 31 ** i for i, v in enumerate((N, H, W, C, K, Rk, P, Q))) + 7919 * salt
    g = _gen(s % (2 ** 31))
    if mode == EXACT:
        x = _ints(g, (N, H, W, C), -2, 2)
        w = _ints(g, (K, Rk, Rk, C), -1, 1)
        if wdens < 1.0:
            w = w * (torch.rand(w.shape, generator=g) < wdens)
        dy = _ints(g, (N, P, Q, K), -2, 2)
    else:
        x = _bf(torch.randn(N, H, W, C, generator=g))
        w = _bf(torch.randn(K, Rk, Rk, C, generator=g) / math.sqrt(Rk * Rk * C))
        dy = _bf(torch.randn(N, P, Q, K, generator=g))
    return x, w, dy


@functools.lru_cache(maxsize=None)
def fwd_case(shape, mode, wdens=1.0):
    x, w, _ = _operands(shape, mode, wdens=wdens)
    return {"mode": mode, "x": x, "w": w, "ref": ref_fwd(x, w, shape),
            "mag": ref_fwd(x.abs(), w.abs(), shape), "n": shape[5] ** 2 * shape[3]}


@functools.lru_cache(maxsize=None)
def dgrad_case(shape, mode):
    _, w, dy = _operands(shape, mode, salt=1)
    return {"mode": mode, "dy": dy, "w": w, "ref": ref_dgrad(dy, w, shape),
            "mag": ref_dgrad(dy.abs(), w.abs(), shape), "n": shape[5] ** 2 * shape[4]}


@functools.lru_cache(maxsize=None)
def wgrad_case(shape, mode):
    x, _, dy = _operands(shape, mode, salt=2)
    P, Q = _out_hw(shape)
    return {"mode": mode, "x": x, "dy": dy, "ref": ref_wgrad(x, dy, shape),
            "mag": ref_wgrad(x.abs(), dy.abs(), shape),
            "n": shape[0] * P * Q + 1}        # one split; with_splits() sets the launch's count


def with_splits(case, shape, splits):
    """The weight-gradient case with ``n = N P Q +`` the split count of the launch."""
    P, Q = _out_hw(shape)
    return dict(case, n=shape[0] * P * Q + splits)


# ----------------------------------------------------------------------------- knobs, spies
# (setter name, default) of every switch a case may move
_KNOBS = {
    "small_k": ("conv_set_small_k", 31), "dma_mode": ("conv_set_dma_mode", -1),
    "halo": ("conv_set_halo", 3), "halo_strips": ("conv_set_halo_strips", 0),
    "halo_freg": ("conv_set_halo_freg", 0), "halo_stages": ("conv_set_halo_stages", 0),
    "stem_halo": ("conv_set_stem_halo", 1), "halo_bnb": ("conv_set_halo_bnb", 1),
    "gemm": ("conv_set_gemm", 1), "nt": ("conv_set_nt", 0),
    "w_dma_mode": ("wgrad_set_dma_mode", -1), "w_pp": ("wgrad_set_pp", 1),
    "w_dense": ("wgrad_set_dense", 1), "w_direct": ("wgrad_set_direct", 0),
    "w_deep": ("wgrad_set_deep", 0), "w_pipe": ("wgrad_set_pipe", 3),
    "w_halo": ("wgrad_set_halo", 1), "w_stem": ("wgrad_set_stem", 1),
}


@contextlib.contextmanager
def knobs(kw):
    K = _K()
    try:
        for name, v in kw.items():
            getattr(K, _KNOBS[name][0])(v)
        yield
    finally:
        for name in kw:
            getattr(K, _KNOBS[name][0])(_KNOBS[name][1])


def _igemm_route(x, w, y, geom, dh, dw, bk, st, stats=0, bnb=(), acc_src=0, acc_mask=0, bias=0,
                 relu=0, bnl_sc=0, bnl_sh=0, bnl_y=0):
    return _K().conv_route(list(geom), list(dh), list(dw), bk, bool(stats), bool(len(bnb)),
                           bool(bias), int(relu), bool(bnl_y))


@contextlib.contextmanager
def watch(dry=False):
    """Record the route of every conv launch made through ``native`` (``dry``: launch nothing)."""
    nat = _native()
    K = nat._K
    seen = []
    orig = {n: getattr(K, n) for n in ("conv_igemm", "conv_igemm_grouped", "conv_wgrad", "gemm_nt")}
    orig_st, orig_chk = nat._st, nat._check_cuda_bf16

    def igemm(*a, **kw):
        seen.append(_igemm_route(*a, **kw))
        return None if dry else orig["conv_igemm"](*a, **kw)

    def grouped(*a, **kw):
        ok = False if dry else orig["conv_igemm_grouped"](*a, **kw)
        if ok:
            seen.append("grouped")
        return ok

    def wgrad(x, dy, dw_out, ws, geom, dh, dw, splits, st, tr_mode=1, accumulate=0):
        seen.append(K.conv_wgrad_route(list(geom), list(dh), list(dw), splits, tr_mode))
        return None if dry else orig["conv_wgrad"](x, dy, dw_out, ws, geom, dh, dw, splits, st,
                                                   tr_mode, accumulate)

    def gemm_nt(*a, **kw):
        seen.append("gemm_nt")
        return None if dry else orig["gemm_nt"](*a, **kw)

    try:
        K.conv_igemm, K.conv_igemm_grouped, K.conv_wgrad, K.gemm_nt = igemm, grouped, wgrad, gemm_nt
        if dry:
            nat._st = lambda: 0
            nat._check_cuda_bf16 = lambda *a: None
        yield seen
    finally:
        for n, f in orig.items():
            setattr(K, n, f)
        nat._st, nat._check_cuda_bf16 = orig_st, orig_chk


def _dev(t, dtype=BF16):
    return t.to("cuda", dtype).contiguous()


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


# ============================================================================= case tables
S, V = "SAME", "VALID"
# (id, forward shape, knobs, route)
FWD = [
    # element gather (C % 8 != 0): the two the issue names; M = 70 < one tile, 7x7 stride 2
    ("gather1_c1", (2, 5, 7, 1, 8, 5, 1, S), {}, "gather1_narrow"),
    ("gather1_c3", (1, 9, 6, 3, 72, 7, 2, 3), {}, "gather1_wide"),
    # chunk gather: T C = 72 -> Kpad 96; Q = 13; M = 182 below a tile
    ("gather8_c8", (2, 7, 13, 8, 8, 3, 1, 1), {}, "gather8_narrow"),
    # W = 1, Kout just past one tile width, 3 taps fall into the padding on every pixel
    ("gather8_c24", (1, 35, 1, 24, 72, 3, 1, S), {}, "gather8_wide"),
    # P Q = 9 (a tile spans 14 images), M = 261 = 2 x 128 + 5, Kout between the tile widths
    ("gather8_c40", (29, 3, 3, 40, 136, 3, 1, 1), {}, "gather8_wide"),
    # register BK 32 (default small_k): M = 234 < 256, Q = 13
    ("reg32_narrow", (2, 9, 13, 32, 8, 3, 1, 1), {}, "reg32_narrow"),
    # M = 129 = one tile + 1, Q = 3, Kout = 72
    ("reg32_k72", (1, 43, 3, 64, 72, 3, 1, 1), {}, "reg32_wide"),
    # 1 tap, stride 2, C < 128; Kout = 136; P Q = 16
    ("reg32_1tap_s2", (2, 7, 7, 96, 136, 1, 2, 0), {}, "reg32_wide"),
    ("reg32_5x5", (1, 6, 5, 64, 64, 5, 1, S), {}, "reg32_narrow"),            # 25 taps
    ("reg32_7x7", (1, 7, 9, 32, 16, 7, 1, 3), {}, "reg32_narrow"),            # 49 taps, Q = 9
    ("reg32_even", (1, 6, 7, 32, 24, 4, 1, S), {}, "reg32_narrow"),           # asymmetric SAME, Q = 7
    ("reg32_s12", (1, 5, 9, 64, 40, 3, (1, 2), 1), {}, "reg32_narrow"),       # stride (1, 2)
    ("reg32_q1", (3, 35, 1, 32, 72, 3, 1, 1), {}, "reg32_wide"),              # Q = 1, P Q = 35
    ("reg32_pq1", (130, 1, 1, 32, 8, 3, 1, 1), {}, "reg32_narrow"),           # P Q = 1, H = W = 1
    # register BK 64 (small_k 0): C in {64, 192}; C = 96 stays on BK 32; H = 1
    ("reg64_narrow", (2, 9, 13, 64, 8, 3, 1, 1), {"small_k": 0}, "reg64_narrow"),
    ("reg64_wide", (1, 43, 3, 192, 72, 3, 1, 1), {"small_k": 0}, "reg64_wide"),
    ("reg32_c96", (1, 1, 35, 96, 72, 3, 1, 1), {"small_k": 0}, "reg32_wide"),
    # DMA: automatic at C = 256 / Kout = 128 with M = 257; forced at C = 64 (P Q = 9, M = 18)
    ("dma_257", (1, 1, 257, 256, 128, 3, 1, 1), {}, "dma"),
    ("dma_c64", (2, 3, 3, 64, 128, 3, 1, 1), {"dma_mode": 1}, "dma"),
    # halo family 1: H = 4 (top and bottom padding in one strip); H = 12 (three strips, an odd
    # count under two strips per block); each form; Kout = 256 with the GEMM route off
    ("halo1", (1, 4, 56, 64, 64, 3, 1, 1), {}, "halo1"),
    ("halo1_h12", (1, 12, 56, 64, 128, 3, 1, 1), {}, "halo1"),
    ("halo1_k256", (1, 4, 56, 64, 256, 3, 1, 1), {"gemm": 0}, "halo1"),
    ("halo1_strips2", (1, 12, 56, 64, 64, 3, 1, 1), {"halo_strips": 1}, "halo1_strips2"),
    ("halo1_freg", (1, 12, 56, 64, 64, 3, 1, 1), {"halo_freg": 1}, "halo1_freg"),
    ("halo1_ring3", (1, 12, 56, 64, 64, 3, 1, 1), {"halo_stages": 3}, "halo1_ring3"),
    ("halo1_ring4", (2, 4, 56, 64, 64, 3, 1, 1), {"halo_stages": 4}, "halo1_ring4"),
    ("halo1_ring3_strips2", (1, 12, 56, 64, 64, 3, 1, 1), {"halo_stages": 3, "halo_strips": 1},
     "halo1_ring3_strips2"),
    # halo family 2
    ("halo2", (1, 4, 28, 128, 128, 3, 1, 1), {}, "halo2"),
    ("halo2_h12", (1, 12, 28, 128, 128, 3, 1, 1), {}, "halo2"),
    ("halo2_k256", (1, 4, 28, 128, 256, 3, 1, 1), {"gemm": 0}, "halo2"),
    ("halo2_strips2", (1, 12, 28, 128, 128, 3, 1, 1), {"halo_strips": 2}, "halo2_strips2"),
    ("halo2_freg", (1, 12, 28, 128, 128, 3, 1, 1), {"halo_freg": 2}, "halo2_freg"),
    ("halo2_ring3", (1, 12, 28, 128, 128, 3, 1, 1), {"halo_stages": 0x30}, "halo2_ring3"),
    ("halo2_ring4", (1, 12, 28, 128, 128, 3, 1, 1), {"halo_stages": 0x40}, "halo2_ring4"),
    ("halo2_ring4_strips2", (2, 4, 28, 128, 128, 3, 1, 1),
     {"halo_stages": 0x40, "halo_strips": 2}, "halo2_ring4_strips2"),
    # stem halo: the space-to-depth input (N, P + 3, 115, 16), 4x4 VALID
    ("stem_p4", (1, 7, 115, 16, 64, 4, 1, V), {}, "stem"),
    ("stem_p8", (2, 11, 115, 16, 64, 4, 1, V), {}, "stem"),
    # persistent GEMM: ONE_PARTIAL_TILE and CB_THREE of test_conv_gemm_issue_gpu.py
    ("gemm_partial", (3, 7, 7, 64, 256, 3, 1, 1), {}, "gemm"),
    ("gemm_cb3", (7, 5, 9, 192, 320, 3, 1, 1), {}, "gemm"),
    # the strided 1x1 projection (1 tap, C >= 128, Kout > 128) also runs on the persistent GEMM
    ("gemm_proj", (2, 7, 7, 128, 256, 1, 2, 0), {}, "gemm"),
    # 1x1 stride 1 through conv2d_forward: the stream GEMM with an M tail, the ping-pong GEMM,
    # and Kout = 72 at C = 512, which _gemm_1x1 leaves on the register kernel
    ("1x1_stream", (1, 5, 13, 64, 256, 1, 1, 0), {}, "gemm_nt"),
    ("1x1_c512", (2, 9, 7, 512, 256, 1, 1, 0), {}, "gemm_nt"),
    ("1x1_k72", (1, 3, 43, 512, 72, 1, 1, 0), {}, "reg32_wide"),
]

# (id, forward shape, knobs, route, epilogue, filter density in exact mode)
FWD_EPI = [
    ("stats_reg_narrow", (2, 9, 15, 32, 8, 3, 1, 1), {}, "reg32_narrow_stats", "stats", 0.25),
    ("stats_reg_wide", (3, 43, 3, 64, 72, 3, 1, 1), {}, "reg32_wide_stats", "stats", 0.1),
    ("stats_reg64", (3, 43, 3, 64, 72, 3, 1, 1), {"small_k": 0}, "reg64_wide_stats", "stats", 0.1),
    ("stats_gather8", (29, 3, 3, 40, 136, 3, 1, 1), {}, "gather8_wide_stats", "stats", 0.2),
    ("stats_dma", (2, 13, 11, 64, 128, 3, 1, 1), {"dma_mode": 1}, "dma_stats", "stats", 0.1),
    ("stats_halo1", (1, 8, 56, 64, 64, 3, 1, 1), {}, "halo1_stats", "stats", 0.1),
    ("stats_halo2", (2, 4, 28, 128, 128, 3, 1, 1), {}, "halo2_stats", "stats", 0.05),
    ("stats_stem", (2, 11, 115, 16, 64, 4, 1, V), {}, "stem_stats", "stats", 0.2),
    ("stats_gemm", (3, 7, 7, 64, 256, 3, 1, 1), {}, "gemm_stats", "stats", 0.1),
    ("bias_relu_reg", (1, 43, 3, 64, 72, 3, 1, 1), {}, "reg32_wide", "bias_relu", 1.0),
    ("bias_gather1", (2, 5, 7, 1, 8, 5, 1, S), {}, "gather1_narrow", "bias", 1.0),
    ("relu_gather8", (2, 7, 13, 8, 8, 3, 1, 1), {}, "gather8_narrow", "relu", 1.0),
    ("bnl_halo1", (1, 8, 56, 64, 64, 3, 1, 1), {}, "halo1_bnl", "bnl", 1.0),
    ("bnl_halo2", (2, 4, 28, 128, 128, 3, 1, 1), {}, "halo2_bnl", "bnl", 1.0),
    ("bnl_stats_halo1", (1, 4, 56, 64, 64, 3, 1, 1), {}, "halo1_bnl_stats", "bnl_stats", 0.03),
    # non-temporal stores, one per store path
    ("nt_reg", (1, 43, 3, 64, 72, 3, 1, 1), {"nt": 1}, "reg32_wide", "plain", 1.0),
    ("nt_gather", (2, 7, 13, 8, 8, 3, 1, 1), {"nt": 1}, "gather8_narrow", "plain", 1.0),
    ("nt_dma", (2, 3, 3, 64, 128, 3, 1, 1), {"nt": 1, "dma_mode": 1}, "dma", "plain", 1.0),
    ("nt_halo1", (1, 4, 56, 64, 64, 3, 1, 1), {"nt": 1}, "halo1", "plain", 1.0),
    ("nt_halo2", (1, 4, 28, 128, 128, 3, 1, 1), {"nt": 1}, "halo2", "plain", 1.0),
    ("nt_stem", (1, 7, 115, 16, 64, 4, 1, V), {"nt": 1}, "stem", "plain", 1.0),
    ("nt_gemm", (3, 7, 7, 64, 256, 3, 1, 1), {"nt": 1}, "gemm", "plain", 1.0),
]

# (id, forward shape, knobs, routes in launch order).  In a data gradient the kernel's C is the
# forward Kout and its Kout the forward C.
DGRAD = [
    ("s1_reg", (2, 7, 9, 32, 64, 3, 1, 1), {}, ["reg32_narrow"]),
    ("s1_halo", (1, 4, 56, 64, 64, 3, 1, 1), {}, ["halo1"]),
    ("s1_gemm", (3, 7, 7, 256, 64, 3, 1, 1), {}, ["gemm"]),
    # stride 2, pad 1, H and W even, K % 32 == 0: all four phase classes in one launch
    ("s2_grouped", (2, 8, 10, 32, 64, 3, 2, 1), {}, ["grouped"]),
    # odd H and W: unequal class grids -> one launch per class
    ("s2_odd", (1, 7, 9, 32, 64, 3, 2, 1), {}, ["reg32_narrow"] * 4),
    # K = 72: not a multiple of 32 -> per class, on the chunk gather (kernel C = 72)
    ("s2_k72", (1, 8, 8, 16, 72, 3, 2, 1), {}, ["gather8_narrow"] * 4),
    # R = 1, stride 2: three of four classes have no taps (need_zero)
    ("s2_1x1", (2, 6, 8, 64, 32, 1, 2, 0), {}, ["reg32_narrow"]),
    # the stem's shape family: 7x7 / 2 pad 3 with C = 8
    ("s2_7x7_c8", (1, 12, 10, 8, 16, 7, 2, 3), {}, ["gather8_narrow"] * 4),
    ("s1_5x5", (1, 6, 7, 32, 32, 5, 1, S), {}, ["reg32_narrow"]),
    ("s1_q13_k136", (1, 3, 13, 136, 32, 3, 1, 1), {}, ["reg32_wide"]),
    # the DMA kernel without the sums (kernel C = 256, Kout = 128), M = 35
    ("s1_dma", (1, 5, 7, 128, 256, 3, 1, 1), {}, ["dma"]),
    # stride-2 phase classes with 256 outputs: the grouped launch refuses (not the register
    # kernel) and each class runs on the persistent GEMM with a strided output placement
    ("s2_gemm", (1, 8, 8, 256, 64, 3, 2, 1), {}, ["gemm"] * 4),
]
# with ``out=`` / ``acc_from`` the halo kernel is not eligible (halo_family refuses g.acc)
DGRAD_ACC_ROUTE = {"s1_halo": ["reg32_narrow"]}
DGRAD_ACC = ["s1_reg", "s1_halo", "s1_gemm", "s1_dma", "s2_grouped", "s2_gemm", "s2_1x1"]
DGRAD_ACC_FROM = ["s1_reg", "s1_halo", "s1_gemm", "s1_dma"]

# (id, forward shape, knobs, routes, mask kind)
DGRAD_BNB = [
    ("bnb_reg_k0", (2, 7, 9, 32, 64, 3, 1, 1), {}, ["reg32_narrow_bnb"], 0),
    ("bnb_reg_k1", (1, 43, 3, 136, 32, 3, 1, 1), {}, ["reg32_wide_bnb"], 1),
    ("bnb_reg_k2", (2, 7, 9, 32, 64, 3, 1, 1), {}, ["reg32_narrow_bnb"], 2),
    ("bnb_dma_k1", (1, 5, 7, 128, 256, 3, 1, 1), {}, ["dma_bnb"], 1),
    ("bnb_dma_k2", (2, 13, 11, 128, 64, 3, 1, 1), {"dma_mode": 1}, ["dma_bnb"], 2),
    ("bnb_halo1_k2", (1, 8, 56, 64, 64, 3, 1, 1), {}, ["halo1_bnb"], 2),
    ("bnb_halo1_k1_freg", (1, 4, 56, 64, 64, 3, 1, 1), {"halo_freg": 1}, ["halo1_freg_bnb"], 1),
    ("bnb_halo1_ring3", (1, 8, 56, 64, 64, 3, 1, 1), {"halo_stages": 3}, ["halo1_ring3_bnb"], 0),
    ("bnb_halo1_ring4", (1, 4, 56, 64, 64, 3, 1, 1), {"halo_stages": 4}, ["halo1_ring4_bnb"], 2),
    ("bnb_halo2_k1", (1, 8, 28, 128, 128, 3, 1, 1), {}, ["halo2_bnb"], 1),
    ("bnb_halo2_freg", (1, 8, 28, 128, 128, 3, 1, 1), {"halo_freg": 2}, ["halo2_freg_bnb"], 2),
    ("bnb_halo2_ring3", (1, 4, 28, 128, 128, 3, 1, 1), {"halo_stages": 0x30}, ["halo2_ring3_bnb"], 0),
    ("bnb_halo2_ring4", (2, 4, 28, 128, 128, 3, 1, 1), {"halo_stages": 0x40}, ["halo2_ring4_bnb"], 1),
    ("bnb_halo_off", (1, 4, 56, 64, 64, 3, 1, 1), {"halo_bnb": 0}, ["reg32_narrow_bnb"], 2),
    # stride 2: the grouped launch must refuse the sums; one launch per class
    ("bnb_s2", (2, 8, 10, 32, 64, 3, 2, 1), {}, ["reg32_narrow_bnb"] * 4, 2),
]

# (id, forward shape, knobs, route)
WGRAD = [
    ("generic_5x5", (1, 9, 8, 1, 8, 5, 2, 2), {}, "generic"),
    ("generic_7x7", (2, 9, 11, 3, 16, 7, 2, 3), {}, "generic"),
    ("reg", (1, 5, 7, 8, 72, 3, 1, 1), {"w_dma_mode": 0}, "reg"),                  # Kout 72, TC 72
    # DMA 2x2: M = 35 (no multiple of 32, one split), Kout = TC = 72
    ("dma_2x2", (1, 5, 7, 8, 72, 3, 1, 1), {}, "dma_2x2_pipe3"),
    # DMA narrow: stride 2 with padding taps, TC = 200; M = 75; and TC = 576 with Q = 7
    ("dma_narrow_tc200", (3, 9, 9, 8, 64, 5, 2, 2), {}, "dma_narrow_pipe3"),
    ("dma_narrow_tc576", (2, 13, 7, 64, 8, 3, 1, 1), {}, "dma_narrow_pipe3"),
    ("dma_narrow_off", (3, 9, 9, 8, 64, 5, 2, 2), {"w_dma_mode": 2}, "dma_2x2_pipe3"),
    ("dma_2x2_q13", (2, 3, 13, 8, 72, 3, 1, 1), {}, "dma_2x2_pipe3"),              # Q = 13
    ("dma_narrow_q1", (4, 35, 1, 16, 8, 3, 1, 1), {}, "dma_narrow_pipe3"),         # Q = 1, W = 1
    # two splits that do not divide M = 315
    ("dma_2x2_splits", (5, 9, 7, 24, 72, 3, 1, 1), {}, "dma_2x2_pipe3"),
    ("dma_narrow_splits", (5, 9, 7, 24, 40, 3, 1, 1), {}, "dma_narrow_pipe3"),
    ("dma_2x2_pipe0", (5, 9, 7, 24, 72, 3, 1, 1), {"w_pipe": 0}, "dma_2x2_pipe0"),
    ("dma_2x2_pipe1", (5, 9, 7, 24, 72, 3, 1, 1), {"w_pipe": 1}, "dma_2x2_pipe1"),
    ("dma_2x2_pipe2", (5, 9, 7, 24, 72, 3, 1, 1), {"w_pipe": 2}, "dma_2x2_pipe2"),
    ("dma_narrow_pipe0", (3, 9, 9, 8, 64, 5, 2, 2), {"w_pipe": 0}, "dma_narrow_pipe0"),
    ("dma_narrow_pipe1", (3, 9, 9, 8, 64, 5, 2, 2), {"w_pipe": 1}, "dma_narrow_pipe1"),
    ("dma_narrow_pipe2", (3, 9, 9, 8, 64, 5, 2, 2), {"w_pipe": 2}, "dma_narrow_pipe2"),
    # the dense one-tap form: M = 8 x 13 x 7
    ("dense", (8, 13, 7, 64, 64, 1, 1, 0), {}, "dma_2x2_dense_pipe3"),
    ("dense_pipe0", (8, 13, 7, 64, 64, 1, 1, 0), {"w_pipe": 0}, "dma_2x2_dense_pipe0"),
    ("dense_pipe1", (8, 13, 7, 64, 64, 1, 1, 0), {"w_pipe": 1}, "dma_2x2_dense_pipe1"),
    ("dense_pipe2", (8, 13, 7, 64, 64, 1, 1, 0), {"w_pipe": 2}, "dma_2x2_dense_pipe2"),
    ("dense_off", (8, 13, 7, 64, 64, 1, 1, 0), {"w_dense": 0}, "dma_2x2_pipe3"),
    ("dense_q3_s2", (2, 5, 5, 64, 72, 1, 2, 0), {}, "dma_2x2_pipe3"),              # 1 tap, strided
    # ping-pong: Kout = 320, TC = 576; one split (M = 70) and two (M = 315)
    ("pp0", (2, 7, 5, 64, 320, 3, 1, 1), {}, "pp0"),
    ("pp0_splits", (5, 9, 7, 64, 320, 3, 1, 1), {}, "pp0"),
    ("pp2", (5, 9, 7, 64, 320, 3, 1, 1), {"w_direct": 1}, "pp2"),
    ("pp4", (5, 9, 7, 64, 320, 3, 1, 1), {"w_direct": 2}, "pp4"),
    ("pp0_deep", (5, 9, 7, 64, 320, 3, 1, 1), {"w_deep": 1}, "pp0_deep"),
    ("pp0_early", (5, 9, 7, 64, 320, 3, 1, 1), {"w_deep": 2}, "pp0_early"),
    # 1x1 with C = 256: the dense form 1, and the decode form with dense off (form 3, dense 3,
    # is a timing probe with wrong results by design: conv_wgrad.hip l.541)
    ("pp1", (3, 7, 6, 256, 256, 1, 1, 0), {}, "pp1"),
    ("pp1_splits", (5, 9, 7, 256, 256, 1, 1, 0), {}, "pp1"),
    ("pp1_early", (5, 9, 7, 256, 256, 1, 1, 0), {"w_deep": 2}, "pp1_early"),
    ("pp0_1x1", (5, 9, 7, 256, 256, 1, 1, 0), {"w_dense": 0}, "pp0"),
    ("pp_off", (2, 7, 5, 64, 320, 3, 1, 1), {"w_pp": 0}, "dma_2x2_pipe3"),
    ("halo_n1", (1, 4, 56, 64, 64, 3, 1, 1), {}, "halo"),
    ("halo_n3", (3, 8, 56, 64, 64, 3, 1, 1), {}, "halo"),
    ("halo_off", (1, 4, 56, 64, 64, 3, 1, 1), {"w_halo": 0}, "dma_narrow_pipe3"),
    ("stem_n1", (1, 115, 115, 16, 64, 4, 1, V), {}, "stem"),
    ("stem_n3", (3, 115, 115, 16, 64, 4, 1, V), {}, "stem"),
]
# accumulate into ``out=`` (the slab reduce with a base), one and several splits, each family
WGRAD_ACC = ["generic_5x5", "reg", "dma_2x2", "dma_2x2_splits", "dma_narrow_tc200", "dense",
             "pp0", "pp0_splits", "pp1_splits", "halo_n3", "stem_n1"]


def _ids(table):
    return [c[0] for c in table]


def _by_id(table, name):
    return next(c for c in table if c[0] == name)


# ============================================================================= launchers (GPU)
def _taps(shape):
    pt, pb, pl, pr = _pads(shape)
    Rk = shape[5]
    return [(r - pt, s - pl) for r in range(Rk) for s in range(Rk)]


def launch_fwd(case, shape, stats=False, bias=None, relu=False, bnl=None, out_guard=True):
    """``_K.conv_igemm`` the way ``native._launch_fwd`` calls it, into a guarded output.
    -> dict(y, stats, ly, route); ``bnl`` = (lsc, lsh) fp64 vectors."""
    nat, K = _native(), _K()
    N, H, W, C, Kout, Rk, stride, pad = shape
    sh, sw = _pair(stride)
    P, Q = _out_hw(shape)
    taps = _taps(shape)
    dh, dw = [t[0] for t in taps], [t[1] for t in taps]
    x = _dev(case["x"])
    kdim = Rk * Rk * C
    kpad = -(-kdim // 32) * 32
    wmat = torch.zeros(Kout, kpad, device="cuda", dtype=BF16)
    wmat[:, :kdim] = _dev(case["w"]).reshape(Kout, kdim)
    geom = nat._fwd_geom((N, H, W, C), Kout, taps, P, Q, sh, sw, P, Q)
    y, ywhole = guarded((N, P, Q, Kout), BF16)
    res = {"y": y}
    sbuf = swhole = ly = lywhole = None
    if stats:
        rows = K.conv_tile_rows(geom, dh, dw, 0)
        sbuf, swhole = guarded((rows, 2, Kout), torch.float32)
        res["stats"] = sbuf
    b32 = None if bias is None else _dev(bias, torch.float32)
    extra = [0, 0, _p(b32), int(relu)]
    if bnl is not None:
        lsc, lsh = _dev(bnl[0], torch.float32), _dev(bnl[1], torch.float32)
        ly, lywhole = guarded((N, H, W, C), BF16)
        res["ly"] = ly
        extra = [0, 0, 0, 0, lsc.data_ptr(), lsh.data_ptr(), ly.data_ptr()]
    args = (x.data_ptr(), wmat.data_ptr(), y.data_ptr(), geom, dh, dw, 64, _st(), _p(sbuf), [])
    res["route"] = _igemm_route(*args, *extra)
    K.conv_igemm(*args, *extra)
    torch.cuda.synchronize()
    assert_guards(ywhole, "y")
    if swhole is not None:
        assert_guards(swhole, "stats")
    if lywhole is not None:
        assert_guards(lywhole, "ly")
    return res


def launch_wgrad(case, shape, base=None, tr_mode=1):
    """``_K.conv_wgrad`` the way ``native.conv2d_wgrad`` calls it, dW and the slab workspace
    guarded.  ``base``: fp64 [K, R, S, C] to accumulate onto.  -> (dW, route, splits)."""
    nat, K = _native(), _K()
    N, H, W, C, Kout, Rk, stride, pad = shape
    sh, sw = _pair(stride)
    P, Q = _out_hw(shape)
    taps = _taps(shape)
    dhs, dws = [t[0] for t in taps], [t[1] for t in taps]
    tc = Rk * Rk * C
    geom = [N, H, W, C, P, Q, sh, sw, Kout, tc]
    slabbed = K.conv_wgrad_halo_splits(geom, dhs, dws)
    splits = slabbed or K.conv_wgrad_splits(N * P * Q, Kout, tc, nat._WGRAD_WS_CAP, Rk * Rk)
    acc = base is not None
    dW, dwhole = guarded((Kout, tc), torch.float32)
    if acc:
        dW.copy_(_dev(base, torch.float32).reshape(Kout, tc))
    ws = wswhole = None
    if splits > 1 or acc or slabbed:
        ws, wswhole = guarded((splits * Kout * tc,), torch.float32)
    x, dy = _dev(case["x"]), _dev(case["dy"])
    route = K.conv_wgrad_route(geom, dhs, dws, splits, tr_mode)
    K.conv_wgrad(x.data_ptr(), dy.data_ptr(), dW.data_ptr(), _p(ws), geom, dhs, dws, splits, _st(),
                 tr_mode, int(acc))
    torch.cuda.synchronize()
    assert_guards(dwhole, "dW")
    if wswhole is not None:
        assert_guards(wswhole, "wgrad slabs")
    return dW.reshape(Kout, Rk, Rk, C), route, splits


# ============================================================================= forward (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", _ids(FWD))
def test_forward(name, mode):
    _, shape, kn, route = _by_id(FWD, name)
    nat = _native()
    case = fwd_case(shape, mode)
    with knobs(kn), watch() as seen:
        y = nat.conv2d_forward(_dev(case["x"]), _dev(case["w"]), shape[6], shape[7])
        torch.cuda.synchronize()
    assert seen == [route], (name, seen)
    check(y, case, f"fwd/{route}/{name}")


def _tile_rows_of(route, M, tiles, shape):
    """M rows summed into one slab row on ``route``."""
    if route.startswith("halo") or route.startswith("stem"):
        assert M % tiles == 0
        return M // tiles
    return 256 if (route.startswith("dma") or route.startswith("gemm") or "_narrow" in route) else 128


def _check_stats(stats, y, route, shape, mode, what):
    """Each slab row against the fp64 sums of the STORED y over that tile's rows."""
    Kout = shape[4]
    y64 = y.detach().double().cpu().reshape(-1, Kout)
    M = y64.shape[0]
    tiles = stats.shape[0]
    bm = _tile_rows_of(route, M, tiles, shape)
    assert tiles == -(-M // bm), (what, tiles, M, bm)
    pad = torch.zeros(tiles * bm - M, Kout, dtype=torch.float64)
    yt = torch.cat([y64, pad]).reshape(tiles, bm, Kout)
    ref = torch.stack([yt.sum(1), (yt * yt).sum(1)], 1)
    mag = torch.stack([yt.abs().sum(1), (yt * yt).sum(1)], 1)
    got = stats.detach().double().cpu()
    if mode == EXACT:
        assert float(y64.abs().max()) <= 128.0, (what, float(y64.abs().max()))
        assert float(mag.max()) < 2.0 ** 24
        assert_exact(got, ref, what + " slab rows")
        assert_exact(got.sum(0), ref.sum(0), what + " total")
    else:
        bound = gamma(bm + 8) * mag
        _measure(what, got, ref, bound)
        assert_within(got, ref, bound, what + " slab rows")
        assert_within(got.sum(0), ref.sum(0), bound.sum(0), what + " total")


def epi_case(name, mode):
    """CPU side of one FWD_EPI entry -> (case, launch keywords, fp64 pre-rounding ly or None)."""
    _, shape, kn, route, epi, dens = _by_id(FWD_EPI, name)
    case = dict(fwd_case(shape, mode, dens))
    C, Kout = shape[3], shape[4]
    g = _gen(17 + C)
    kw, pre = {}, None
    if "bias" in epi:
        kw["bias"] = _ints(g, (Kout,), -8, 8) if mode == EXACT else \
            torch.randn(Kout, generator=g).float().double()
        case["ref"] = case["ref"] + kw["bias"]
        case["mag"] = case["mag"] + kw["bias"].abs()
    if "relu" in epi:
        kw["relu"] = True
        case["ref"] = case["ref"].clamp_min(0)
    if "bnl" in epi:
        lsc = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (C,), generator=g)].double()
        lsh = _ints(g, (C,), -2, 2)
        if mode == BOUND:
            lsc = lsc * torch.randn(C, generator=g).float().double()
            lsh = torch.randn(C, generator=g).float().double()
        kw["bnl"] = (lsc, lsh)
        pre = {"mode": mode, "ref": (case["x"] * lsc + lsh).clamp_min(0), "n": 2,
               "mag": (case["x"] * lsc).abs() + lsh.abs()}
        ly = _bf(pre["ref"])
        case["ref"] = ref_fwd(ly, case["w"], shape)
        case["mag"] = ref_fwd(ly.abs(), case["w"].abs(), shape)
    return case, kw, pre


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", _ids(FWD_EPI))
def test_forward_epilogue(name, mode):
    _, shape, kn, route, epi, dens = _by_id(FWD_EPI, name)
    case, kw, pre = epi_case(name, mode)
    with knobs(kn):
        res = launch_fwd(case, shape, stats="stats" in epi, **kw)
    assert res["route"] == route, (name, res["route"])
    what = f"fwd/{route}/{name}"
    if pre is not None:
        # ly: one rounding of the fp32 fma x lsc + lsh (2 u32 of |x lsc| + |lsh|)
        check(res["ly"], pre, what + " ly")
        if mode == BOUND:       # stage-wise: y is the conv of the STORED ly
            ly_got = res["ly"].detach().double().cpu()
            case["ref"] = ref_fwd(ly_got, case["w"], shape)
            case["mag"] = ref_fwd(ly_got.abs(), case["w"].abs(), shape)
    check(res["y"], case, what)
    if "stats" in epi:
        _check_stats(res["stats"], res["y"], route, shape, mode, what + " stats")


# ============================================================================= dgrad (GPU)
def _mask_bits(g, shape):
    """A random ReLU bit mask: (uint8 [numel / 8], fp64 0/1 tensor of ``shape``)."""
    bits = torch.randint(0, 2, shape, generator=g)
    packed = (bits.reshape(-1, 8) << torch.arange(8)).sum(1).to(torch.uint8)
    return packed, bits.double()


def _run_dgrad(name, mode, variant):
    _, shape, kn, routes = _by_id(DGRAD, name)
    nat = _native()
    N, H, W, C, Kout, Rk, stride, pad = shape
    case = dict(dgrad_case(shape, mode))
    g = _gen(23 + H * W)
    kw, k, whole = {}, 1, None
    if variant != "plain":
        routes = DGRAD_ACC_ROUTE.get(name, routes)
        if mode == EXACT:
            base = _ints(g, (N, H, W, C), -8, 8)
        else:
            base = _bf(torch.randn(N, H, W, C, generator=g))
        conv1 = _bf(case["ref"])          # the first rounding (docstring: rounding points)
        k = 2
        if variant == "out":
            out, whole = guarded((N, H, W, C), BF16)
            out.copy_(_dev(base))
            kw["out"] = out
            touched = torch.ones(N, H, W, C, dtype=torch.bool)
            if name == "s2_1x1":          # classes without taps leave the base untouched
                touched[:] = False
                touched[:, ::2, ::2] = True
            add = base
        else:
            packed, bits = _mask_bits(g, (N, H, W, C))
            kw["acc_from"] = nat._MaskedGrad(_dev(base), packed.cuda())
            touched = torch.ones(N, H, W, C, dtype=torch.bool)
            add = base * bits
        if mode == EXACT:
            case["ref"] = torch.where(touched, conv1 + add, add)
        else:
            # bound mode stays on the unrounded value; the two roundings are of conv and of the sum
            case["round_mag"] = torch.where(touched, case["ref"].abs(), torch.zeros_like(add)) + \
                (case["ref"] + add).abs()
            case["ref"] = case["ref"] + add
        case["mag"] = case["mag"] + add.abs()
    with knobs(kn), watch() as seen:
        dx = nat.conv2d_dgrad(_dev(case["dy"]), _dev(case["w"]), (N, H, W, C), stride, pad, **kw)
        torch.cuda.synchronize()
    assert seen == routes, (name, variant, seen)
    if whole is not None:
        assert_guards(whole, "dgrad out=")
    what = f"dgrad/{routes[0]}/{name}/{variant}"
    if name == "s2_1x1" and variant == "out":      # both modes: the base where no class has taps
        keep = dx.detach().double().cpu().clone()
        keep[:, ::2, ::2] = base[:, ::2, ::2]
        assert_exact(keep, base, what + " untouched base")
    if name == "s2_1x1" and variant == "plain":
        z = dx.detach().double().cpu().clone()
        z[:, ::2, ::2] = 0
        assert_exact(z, torch.zeros_like(z), what + " tapless classes")     # exact zeros, +0 or -0
    check(dx, case, what, k=k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", _ids(DGRAD))
def test_dgrad(name, mode):
    _run_dgrad(name, mode, "plain")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", DGRAD_ACC)
def test_dgrad_out(name, mode):
    _run_dgrad(name, mode, "out")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", DGRAD_ACC_FROM)
def test_dgrad_acc_from(name, mode):
    _run_dgrad(name, mode, "acc_from")


def bnb_operands(name):
    """The BatchNorm's operands of one DGRAD_BNB entry: the integer set in BOTH modes (bound mode
    is about dx; its sums are then fp32 sums of Gaussian dz times exact factors, and no mask
    decision is near 0).  -> xb, mean, invstd, fsc, fsh, packed mask, mask bits, x fsc + fsh."""
    _, shape, kn, routes, mkind = _by_id(DGRAD_BNB, name)
    N, H, W, C = shape[:4]
    g = _gen(31 + mkind + H)
    xb = _ints(g, (N, H, W, C), -2, 2)
    mean = _ints(g, (C,), -1, 1)
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)].double()
    fsc = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)].double()
    fsh = _ints(g, (C,), -3, 2) + 0.5
    packed, bits = _mask_bits(g, (N, H, W, C))
    pre = xb * fsc + fsh
    assert float(pre.abs().min()) >= 0.5
    return xb, mean, invstd, fsc, fsh, packed, bits, pre


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", _ids(DGRAD_BNB))
def test_dgrad_bnb(name, mode):
    """The data gradient with the BN-backward sums: dx as usual; each slab row against fp64 sums
    of the kernel's own stored dx over that tile's rows (stride 1), the total over rows always."""
    _, shape, kn, routes, mkind = _by_id(DGRAD_BNB, name)
    nat = _native()
    N, H, W, C, Kout, Rk, stride, pad = shape
    case = dgrad_case(shape, mode)
    M = N * H * W
    xb, mean, invstd, fsc, fsh, packed, bits, pre = bnb_operands(name)
    stats = tuple(_dev(t, torch.float32) for t in (mean, invstd, fsc, fsh))
    bnb = (_dev(xb), stats, packed.cuda() if mkind == 1 else None, mkind != 0, mkind == 1, object())
    spy_orig = nat._K.conv_igemm_grouped
    with knobs(kn), watch() as seen:
        dx = nat.conv2d_dgrad(_dev(case["dy"]), _dev(case["w"]), (N, H, W, C), stride, pad, bnb=bnb)
        torch.cuda.synchronize()
    assert nat._K.conv_igemm_grouped is spy_orig
    assert seen == routes and "grouped" not in seen, (name, seen)
    what = f"dgrad/{routes[0]}/{name}"
    check(dx, case, what)
    part, G, Mp, Cp, _, _ = dx._dtf_bnb_part
    assert (Mp, Cp) == (M, C)
    got = part[:G * 2 * C].reshape(G, 2, C).detach().double().cpu()
    dz = dx.detach().double().cpu()
    if mkind == 1:
        dz = dz * bits
    elif mkind == 2:
        dz = torch.where(pre > 0, dz, torch.zeros_like(dz))
    t1 = dz * (xb - mean) * invstd
    if mode == EXACT:
        assert float(t1.abs().reshape(M, C).sum(0).max()) < 2.0 ** 23
    tot = torch.stack([dz.reshape(M, C).sum(0), t1.reshape(M, C).sum(0)])
    tmag = torch.stack([dz.abs().reshape(M, C).sum(0), t1.abs().reshape(M, C).sum(0)])
    if len(routes) == 1:        # one launch: slab row tm sums the M rows of tile tm
        bm = _tile_rows_of(routes[0], M, G, shape)
        assert G == -(-M // bm), (G, M, bm)
        z = torch.zeros(G * bm - M, C, dtype=torch.float64)
        rows = [torch.cat([t.reshape(M, C), z]).reshape(G, bm, C) for t in (dz, t1)]
        ref = torch.stack([rows[0].sum(1), rows[1].sum(1)], 1)
        mag = torch.stack([rows[0].abs().sum(1), rows[1].abs().sum(1)], 1)
        if mode == EXACT:
            assert_exact(got, ref, what + " slab rows")
        else:
            bound = gamma(bm + 16) * mag
            _measure(what + " sums", got, ref, bound)
            assert_within(got, ref, bound, what + " slab rows")
    if mode == EXACT:
        assert_exact(got.sum(0), tot, what + " total")
    else:
        assert_within(got.sum(0), tot, gamma(M + 16) * tmag, what + " total")


# ============================================================================= wgrad (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", _ids(WGRAD))
def test_wgrad(name, mode):
    _, shape, kn, route = _by_id(WGRAD, name)
    nat = _native()
    N, H, W, C, Kout, Rk, stride, pad = shape
    case = wgrad_case(shape, mode)
    with knobs(kn), watch() as seen:
        dw = nat.conv2d_wgrad(_dev(case["x"]), _dev(case["dy"]), (Kout, Rk, Rk, C), stride, pad)
        torch.cuda.synchronize()
    assert seen == [route], (name, seen)
    with knobs(kn):             # the same launch into guarded dW and slabs
        dw2, route2, splits = launch_wgrad(case, shape)
    assert route2 == route
    check(dw, with_splits(case, shape, splits), f"wgrad/{route}/{name}", k=0)
    assert_exact(dw2, dw.detach().double().cpu(), f"wgrad/{route}/{name} guarded rerun")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", WGRAD_ACC)
def test_wgrad_accumulate(name, mode):
    """``out=``: the slab reduce adds the old dW last; in exact mode the base is preserved
    exactly (``ref + base`` is an integer below 2^24)."""
    _, shape, kn, route = _by_id(WGRAD, name)
    N, H, W, C, Kout, Rk, stride, pad = shape
    case = dict(wgrad_case(shape, mode))
    g = _gen(41 + Kout)
    if mode == EXACT:
        base = _ints(g, (Kout, Rk, Rk, C), -8, 8)
    else:
        base = torch.randn(Kout, Rk, Rk, C, generator=g).float().double()
    case["ref"] = case["ref"] + base
    case["mag"] = case["mag"] + base.abs()
    with knobs(kn):
        dw, got_route, splits = launch_wgrad(case, shape, base=base)
    assert got_route == route, (name, got_route)
    # the old dW is one more term of the sum
    check(dw, with_splits(case, shape, splits + 1), f"wgrad/{route}/{name}/acc splits={splits}", k=0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,route", [("reg", "reg_notr"), ("dma_2x2_splits", "reg_notr"),
                                        ("generic_7x7", "generic_notr")])
def test_wgrad_debug_reads(name, route, mode):
    """``tr_mode`` 0: the register kernels with element-wise LDS reads instead of the transposing
    ones (the debug path the DMA kernels are compared with elsewhere)."""
    _, shape, kn, _ = _by_id(WGRAD, name)
    case = wgrad_case(shape, mode)
    dw, got_route, splits = launch_wgrad(case, shape, tr_mode=0)
    assert got_route == route, (name, got_route)
    check(dw, with_splits(case, shape, splits), f"wgrad/{route}/{name}", k=0)


# ============================================================================= CPU self-tests
def test_routes_dry():
    """The route every table entry is named for, without a GPU: the launches are intercepted
    before anything runs and their arguments handed to the dispatchers' own route functions."""
    nat = _native()
    for name, shape, kn, route in FWD:
        N, H, W, C, Kout, Rk, stride, pad = shape
        with knobs(kn), watch(dry=True) as seen:
            nat.conv2d_forward(torch.zeros(N, H, W, C, dtype=BF16),
                               torch.zeros(Kout, Rk, Rk, C, dtype=BF16), stride, pad)
        assert seen == [route], (name, seen)
    K = nat._K
    for name, shape, kn, route, epi, _ in FWD_EPI:
        N, H, W, C, Kout, Rk, stride, pad = shape
        sh, sw = _pair(stride)
        P, Q = _out_hw(shape)
        taps = _taps(shape)
        geom = nat._fwd_geom((N, H, W, C), Kout, taps, P, Q, sh, sw, P, Q)
        with knobs(kn):
            got = K.conv_route(geom, [t[0] for t in taps], [t[1] for t in taps], 64,
                               "stats" in epi, False, "bias" in epi, int("relu" in epi),
                               "bnl" in epi)
        assert got == route, (name, got)
    for table in (DGRAD, DGRAD_BNB):
        for entry in table:
            name, shape, kn, routes = entry[:4]
            N, H, W, C, Kout, Rk, stride, pad = shape
            P, Q = _out_hw(shape)
            kw = {}
            if table is DGRAD_BNB:
                v = torch.zeros(C)
                kw["bnb"] = (torch.zeros(N, H, W, C, dtype=BF16), (v, v, v, v),
                             torch.zeros(N * H * W * C // 8, dtype=torch.uint8), entry[4] != 0,
                             entry[4] == 1, None)
            with knobs(kn), watch(dry=True) as seen:
                nat.conv2d_dgrad(torch.zeros(N, P, Q, Kout, dtype=BF16),
                                 torch.zeros(Kout, Rk, Rk, C, dtype=BF16), (N, H, W, C), stride,
                                 pad, **kw)
            # dry: the grouped launch (a device decision) reports "not taken"
            want = routes if routes != ["grouped"] else ["reg32_narrow"] * 4
            assert seen == want, (name, seen)
    for name, shape, kn, route in WGRAD:
        N, H, W, C, Kout, Rk, stride, pad = shape
        P, Q = _out_hw(shape)
        with knobs(kn), watch(dry=True) as seen:
            nat.conv2d_wgrad(torch.zeros(N, H, W, C, dtype=BF16),
                             torch.zeros(N, P, Q, Kout, dtype=BF16), (Kout, Rk, Rk, C), stride, pad)
        assert seen == [route], (name, seen)


def tap_conv(x, w, shape, dh, dw, order=1, last_c_shift=0):
    """The kernels' own formulation in torch: per tap ``t`` the input shifted by ``(dh, dw)``
    (zero outside the image) times ``w[:, t, :]``, accumulated in ``x.dtype`` over the taps in
    ``order`` (1 forward, -1 reversed).  ``last_c_shift``: read the last tap's last 32 channels
    at this channel offset (a damage)."""
    N, H, W, C, Kout, Rk, stride, pad = shape
    sh, sw = _pair(stride)
    P, Q = _out_hw(shape)
    T = len(dh)
    m = max(max(abs(v) for v in dh), max(abs(v) for v in dw)) + 1
    xp = F.pad(x, (0, 0, m, m + sw * Q, m, m + sh * P))
    wt = w.reshape(Kout, T, C)
    acc = torch.zeros(N, P, Q, Kout, dtype=x.dtype)
    for t in (range(T) if order > 0 else reversed(range(T))):
        xs = xp[:, m + dh[t]: m + dh[t] + sh * P: sh, m + dw[t]: m + dw[t] + sw * Q: sw, :]
        if last_c_shift and t == T - 1:
            xs = xs.clone()
            c0 = max(C - 32, 0)
            xs[..., c0:] = torch.roll(xs, -last_c_shift, -1)[..., c0:]
        acc = acc + xs @ wt[:, t, :].T
    return acc


def _emulate_fwd(case, shape):
    """fp32 accumulation in two orders (torch's conv and the reversed tap loop), one rounding."""
    x32, w32 = case["x"].float(), case["w"].float()
    taps = _taps(shape)
    a = ref_fwd(x32, w32, shape)
    b = tap_conv(x32, w32, shape, [t[0] for t in taps], [t[1] for t in taps], order=-1)
    return a.to(BF16), b.to(BF16)


_ALL_FWD_SHAPES = sorted({c[1] for c in FWD} | {c[1] for c in FWD_EPI}, key=str)
_ALL_DGRAD_SHAPES = sorted({c[1] for c in DGRAD} | {c[1] for c in DGRAD_BNB}, key=str)
_ALL_WGRAD_SHAPES = sorted({c[1] for c in WGRAD}, key=str)


@pytest.mark.parametrize("mode", MODES)
def test_emulated_forward(mode):
    for shape in _ALL_FWD_SHAPES:
        case = fwd_case(shape, mode)
        for got in _emulate_fwd(case, shape):
            check(got, case, f"emulated fwd {shape}")


@pytest.mark.parametrize("mode", MODES)
def test_emulated_dgrad(mode):
    for shape in _ALL_DGRAD_SHAPES:
        case = dgrad_case(shape, mode)
        dy32, w32 = case["dy"].float(), case["w"].float()
        h = shape[4] // 2                      # second order: the two halves of K, high first
        a = ref_dgrad(dy32, w32, shape)
        b = ref_dgrad(dy32[..., h:], w32[h:], shape[:4] + (shape[4] - h,) + shape[5:]) + \
            ref_dgrad(dy32[..., :h], w32[:h], shape[:4] + (h,) + shape[5:])
        for got in (a.to(BF16), b.to(BF16)):
            check(got, case, f"emulated dgrad {shape}")


@pytest.mark.parametrize("mode", MODES)
def test_emulated_wgrad(mode):
    for shape in _ALL_WGRAD_SHAPES:
        case = wgrad_case(shape, mode)
        x32, dy32 = case["x"].float(), case["dy"].float()
        a = ref_wgrad(x32, dy32, shape)
        b = torch.zeros_like(a)                # second order: one image at a time, last first
        for n in reversed(range(shape[0])):
            b = b + ref_wgrad(x32[n:n + 1], dy32[n:n + 1], (1,) + shape[1:])
        for got in (a, b):
            check(got, case, f"emulated wgrad {shape}", k=0)


def test_exactness_conditions():
    """The side conditions of the exact-mode epilogue cases, on the reference."""
    for name, shape, kn, route, epi, dens in FWD_EPI:
        case, _, _ = epi_case(name, EXACT)
        assert float(case["mag"].max()) < 2.0 ** 24
        if "stats" in epi:
            assert float(case["ref"].abs().max()) <= 128.0, (name, float(case["ref"].abs().max()))


def test_bnb_exactness_conditions():
    """The BN-backward side conditions for the chosen inputs, on the reference: the mask-kind-2
    decision is at least 0.5 from zero, and with dz = the bf16-rounded reference dx (what the
    kernel stores when it is right) every channel's ``sum |dz (x - mean) invstd|`` and
    ``sum |dz|`` stay below 2^23, so the half-integer sums are exact in fp32."""
    for name, shape, kn, routes, mkind in DGRAD_BNB:
        xb, mean, invstd, fsc, fsh, _, _, pre = bnb_operands(name)
        assert float(pre.abs().min()) >= 0.5, name
        C = shape[3]
        dz = _bf(dgrad_case(shape, EXACT)["ref"]).abs()
        t1 = (dz * (xb - mean).abs() * invstd).reshape(-1, C).sum(0)
        assert float(t1.max()) < 2.0 ** 23, (name, float(t1.max()))
        assert float(dz.reshape(-1, C).sum(0).max()) < 2.0 ** 23, name


def _trunc_bf16(t32):
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def _damaged(kind, mode):
    """(got, case, k) of one listed damage on the smallest case of its family."""
    if kind in ("pad_tap", "swap_tap", "c_off8", "drop_row", "trunc"):
        shape = (2, 7, 13, 8, 8, 3, 1, 1) if kind != "c_off8" else (2, 9, 13, 32, 8, 3, 1, 1)
        case = fwd_case(shape, mode)
        x32, w32 = case["x"].float(), case["w"].float()
        taps = _taps(shape)
        dh, dw = [t[0] for t in taps], [t[1] for t in taps]
        if kind == "swap_tap":          # tap (r, s) = (0, 1) read at (dh, dw) swapped
            dh[1], dw[1] = dw[1], dh[1]
        got = tap_conv(x32, w32, shape, dh, dw, last_c_shift=8 if kind == "c_off8" else 0)
        if kind == "pad_tap":           # output pixel (0, 0, 0): tap (0, 0) lies in the padding;
            got[0, 0, 0] += w32[:, 0, 0, :] @ x32[0, 0, 0]      # read the pixel's own data there
        if kind == "drop_row":          # the last row of the last tile never stored
            got.reshape(-1, shape[4])[-1] = 0
        return (_trunc_bf16(got) if kind == "trunc" else got.to(BF16)), case, 1
    if kind == "k72_alias":             # channels 64..71 of Kout = 72 written from 0..7
        shape = (1, 9, 6, 3, 72, 7, 2, 3)
        case = fwd_case(shape, mode)
        got = ref_fwd(case["x"].float(), case["w"].float(), shape).to(BF16).clone()
        got[..., 64:72] = got[..., 0:8]
        return got, case, 1
    if kind == "phase_oh0":             # class (1, 0) of a stride-2 dgrad written at oh0 = 0
        shape = (2, 8, 10, 32, 64, 3, 2, 1)
        case = dgrad_case(shape, mode)
        got = ref_dgrad(case["dy"].float(), case["w"].float(), shape).to(BF16).clone()
        got[:, 0::2, 0::2] = got[:, 1::2, 0::2].clone()
        return got, case, 1
    if kind == "lost_slab":             # one split's slab left out of the reduce
        shape = (5, 9, 7, 24, 72, 3, 1, 1)
        case = wgrad_case(shape, mode)
        x32, dy32 = case["x"].float(), case["dy"].float()
        got = ref_wgrad(x32[:3], dy32[:3], (3,) + shape[1:])      # the images of the last 2 lost
        return got, case, 0
    raise KeyError(kind)


DAMAGES = ["pad_tap", "swap_tap", "c_off8", "drop_row", "k72_alias", "phase_oh0", "lost_slab"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", DAMAGES)
def test_damage_detected(kind, mode):
    got, case, k = _damaged(kind, mode)
    with pytest.raises(AssertionError):
        check(got, case, kind, k=k)


def test_truncation_detected():
    """Truncating instead of rounding the bf16 store: outside the bound in bound mode (in exact
    mode the integers are too often representable for this damage to be reliable)."""
    got, case, k = _damaged("trunc", BOUND)
    with pytest.raises(AssertionError):
        check(got, case, "trunc", k=k)
