"""The fused 1x1 backward (``csrc/kernels/conv1x1_bwd.hip``) and every epilogue of the
row-streaming GEMM (``csrc/kernels/gemm_stream.hip``) element by element against fp64.  The
kernels are called directly through ``native._K.*`` with the argument lists of
``native._conv1x1_bwd_fused``, ``_dgrad_1x1_bnb[_dual]``, the ``gemm_stream_apply`` /
``gemm_stream_pre`` call sites and ``tools/c1_bench.py``; the plain, ``cin``, masked and ``stats``
forms of ``gemm_stream`` run through ``native.gemm_nt`` under ``gemm_set_variant(13)`` (a strided
``cin``, which ``native.gemm_nt`` refuses, through ``_K.gemm_nt``, the call it makes).  Data is made
on the CPU with seeded generators; ``conv1x1_bwd_set_grid`` / ``_set_w16``, ``gemm_set_variant``
and ``gemm_set_nt`` are restored in ``finally``.  The method and vocabulary are those of
tests/test_conv_kernels_gpu.py.

References (fp64 on the CPU, on the bf16-rounded operands, from the kernel headers' formulas)
    conv1x1_bwd   ``dY[m,c] = sum_k dO[m,k] W[k,c]`` (bf16), ``dW[k,c] = sum_m dO[m,k] Y[m,c]``
        (fp32: one ``[K][C]`` slab per block, reduced by ``slab_reduce``; the reduced result is
        checked and every one of the ``G = conv1x1_bwd[_lazy]_blocks(M, C)`` sentinel-prefilled
        slabs must be fully written), ``bpart[g][0][c] = sum dz``, ``bpart[g][1][c] = sum dz
        (x - mean) invstd`` with ``dz = dY_stored [fma(x, sc, sh) > 0]``.  The kernel sums the
        rounded dY it stored (conv1x1_bwd.hip l.438-449), so by the stage-wise rule the sums are
        compared with fp64 sums of the kernel's OWN stored dY: each block's row over exactly the
        tiles it walks (``tile % G == g``) and the total over ``g``.
        LZ: ``dO = bf16(fma(A[k], dz3, B[k] x3) + C[k])``, ``dz3 = dy3 * mask bit`` (``bn_bwd_dx``
        in common.h; bit ``e`` of byte ``j`` is channel ``8 j + e``).  RC (stage 0 lazy):
        ``x3 = bf16(sum_c Y[m,c] W[k,c])``; the kernel gets an ``x3`` buffer full of NaN and must
        return finite, correct results.
    gemm_stream   ``C = bf16(A B^T)``, one rounding (gemm_stream.hip l.352).  ``cin`` / masked
        ``acc_from``: the staged bf16 tile is read back and the addend added in fp32 and rounded
        AGAIN (l.464-475): ``bf16(bf16(A B^T) + Cin)`` resp. ``+ acc_src * bit``.  ``stats``:
        ``[ceil(M/256)][2][N]`` sums of ``y``, ``y^2`` of the STORED y per 256-row block
        (l.355-359, ``q = bf2f(h)``).  ``bnb`` kinds 0 / 1 / 2, plain / ``cin`` / masked: the two
        BN-backward sums per block row of the gradient as stored (l.477-493); with ``y2, w3, k3``
        (RC) ``x = bf16(y2 w3^T)`` (l.390-417) and ``bx`` a NaN buffer or 0; ``bnb_dual``: a second
        slab with ``(xp, meanp, invp)`` and the same dz.  ``pre``: ``y = bf16(max(fma(x, sc, sh),
        0))`` written to ``pre_y`` (l.286-297), ``C = y B^T``, statistics; ``nostore=1``: C stays
        all sentinel and the statistics equal the storing form's bit for bit.  ``apply``:
        ``Y = bf16(relu(fma(bf16(A W^T), sc, sh) + res))`` (l.444-456), mask bit = ``Y_stored >
        0`` exactly, mask bytes past row M untouched.

*Exact mode* (the main instrument, no tolerance).  Integer operands -- dO in [-40, 40] (so dY
passes 256 and the store's round-to-nearest-even, ties included, is exercised), dy3 in [-2, 2],
W / w3 in {-1, 0, 1}, Y / y2 in [0, 3], x in [-3, 3], mean in {-1, 0, 1}, invstd in {0.5, 1, 2},
sc in {-1, 1, 2}, sh = k + 0.5 (no ReLU decision at zero), A in {-1, 1, 2}, B in {-1, 0, 1}
sparse, C in [-4, 4] -- make every product and partial sum an integer (half-integer: BN sums,
``pre``, ``apply``) below 2^24 (2^23, 2^22 for sums of squares of half-integers); ``|x3| < 256``
and ``|dO| < 256`` keep the unstored intermediates exact in bf16.  All of it is asserted on the
reference in the case builders.  The kernel must return exactly ``ref64.to(bfloat16)`` resp.
``ref64.float()``.

*Bound mode.*  The same cases on Gaussian data, filters scaled by ``K^-1/2`` (``C^-1/2`` where
the filter's recomputed product is the intermediate): per element ``|got - ref64| <= k u |ref| +
F gamma(n + 8) sum|a b| + allowance``, ``u = 2^-8``, ``F = 1``; ``n = K`` for dY, (rows the block
walks) ``+ G`` for dW, (rows of the block) ``+ 8`` for the sums (3 roundings per term, the lane's
chain, 4 cross-lane adds, the waves), ``K`` / ``K3`` for the stream forms.  fp32 outputs are the
exact 0 or at least 2^-126.  Two roundings (``cin``, masked): every rounding is relative to the
value rounded, ``u (1 + u) (|A B^T| + |ref|)`` with ``ref = A B^T + addend`` unrounded (the first
rounding is of the kernel's fp32 product, which may sit across a boundary from the fp64 one) and
the addend joins ``sum|a b|`` for the fp32 add.

Unstored intermediates.  ``dO`` (LZ), ``x3`` (RC, K3, and the conv output inside ``apply``) and
``y`` inside ``pre`` are rounded, and the ReLU decisions ``fma(x, sc, sh) > 0`` decided, by the
kernel from an fp32 value the test never sees; the reference rounds / decides from fp64.  An
element whose fp64 value lies within the fp32 evaluation error of a rounding boundary (of zero:
a decision) is FRAGILE: either neighbour (decision) is right.  Evaluation errors: ``3 2^-24 (|A
dz| + |B x| + |C|)`` for dO, ``gamma(n + 8) sum|a b|`` for x3, ``2^-23 (|x sc| + |sh|)`` for y and
a decision.  Propagation, all linear: a fragile dO[m,k] may be off by one bf16 spacing ``s`` and
adds ``s |W[k,c]|`` to dY[m,c]'s bound and ``s |Y[m,c]|`` to dW[k,c]'s; a fragile x3[m,k] moves
dO64 by ``|B[k]| s(x3)`` and, the rounding being monotone, dO by at most that plus one spacing of
dO; a fragile decision adds ``|dz|`` resp. ``|dz (x - mean) invstd|`` of that element to its two
sums; a fragile RC x adds ``|dz| s(x) invstd`` to the second sum; a fragile ``pre`` y adds
``s |B[n,k]|`` to C; a fragile ``apply`` conv output adds ``s |sc[n]|``.  (Where the evaluation
error itself reaches half a spacing -- cancellation -- the allowance is the error plus one spacing:
``fp64_util.fragile_round``.)  The fragile share of each intermediate is asserted <= 5 % on the
reference in every case; to keep it there at K = 256 the recomputed products use non-negative
activations (they are ReLU outputs in the model) and filters of mean = their deviation, so that
``sum|a b| / |x|`` stays near 1.

Guard rows.  Every output (dy, wpart, bpart, the reduced dW, C, pre_y, the apply mask, part,
part_p) sits inside a larger sentinel-filled allocation and starts as the sentinel; both margins
(8 KB bf16 / 16 KB fp32 / 4 KB mask) and, for a strided C, the columns between N and ldc must be
unchanged afterwards.

Cases.  conv1x1_bwd: the six configurations (stage 0 / 1, plain / lazy, stage 0 also as 16
waves) x the walks ``C1_WALKS`` -- 1..5 tiles on one block (below, at and past the ring depth),
5 tiles on 2 blocks, 7 on 3, and 3 tiles on the default grid; the largest is 448 x 256.
gemm_stream: ``ST_SHAPES`` per K covers M in {1, 33, 255, 256, 257, 513} and N in {64, 192, 256,
320}; every (K, form) sees a wave-interior tail, a block tail and a multi-chunk N; strided
lda / ldb / ldc for plain / cin / stats, lda / ldb for three bnb forms; non-temporal stores off
for the four ``gemm_nt`` forms (on is the default everywhere else).

*CPU self-tests* (unmarked).  A torch emulation of each family (fp32 accumulation in two orders,
the bf16 roundings at the lines named above) goes through the SAME ``*_verify`` as the kernels:
bit-exact in exact mode, inside the bound in bound mode, on every listed case -- which proves the
side conditions and the fragile cap before a GPU is touched.  Every entry of ``DAMAGES`` falls
outside the check in both modes; ``trunc`` (truncation instead of rounding) and ``x3_unrounded``
in bound mode only: with ``|x3| < 256`` integer, as exact mode demands, the rounding that damage
skips is the identity.  ``conv1x1_bwd[_lazy]_ok`` is host code and checked without a GPU; for
the 16-row lazy tile ``M = TM + 16`` IS a multiple of the tile, so that configuration is refused
at ``M = TM + 8`` instead.

Measured on an MI355X with F = 1 (profiles/STREAM_KERNELS.md): the fp32 outputs without a
recomputed intermediate reach at most 0.064 (dW), 0.11 (``bpart``, 16-row tiles), 0.057
(statistics) and 0.25 (``part`` at M = 1: three roundings of one term against gamma(9)) of their
bounds; with one (RC) 0.60 (dW) and 0.74 (``part``), where the kernel took the other neighbour of
a fragile x3 and the allowance is most of the bound; the bf16 outputs reach 0.996, all of it the
``k u |ref|`` term.  The largest fragile share is 3.1 % (2 of 64 conv outputs in the M = 1
``apply`` case at K = 256), otherwise below 0.4 %.

Found by this file: no kernel fault.  The first run failed ``apply`` in exact mode through a test
error -- ``data_ptr()`` of two temporaries, the second of which the allocator placed where the
first had been, so the kernel read the shift as the scale; the launch keeps them alive now.
"""
import functools
import math
import zlib

import pytest
import torch

import fp64_util as U
from fp64_util import BF16, SENT, U16, U32, bf, gamma

FACTOR = 1.0                # F of the bound (profiles/STREAM_KERNELS.md)
FRAGILE_CAP = 0.05
MASK_FILL = 0xA5            # sentinel of the uint8 mask buffer
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


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _pick(g, shape, values):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _f32(t):
    """An fp32 per-channel parameter as the fp64 value the kernel reads."""
    return t.float().double()


def _dev(t, dtype=BF16):
    return t.to(dtype).to("cuda").contiguous()


def _bits(mask, reverse=False):
    """[M, N/8] uint8 -> [M, N] of 0 / 1: bit e of byte j is channel 8 j + e."""
    sh = torch.arange(8)
    if reverse:
        sh = 7 - sh
    return ((mask.int().unsqueeze(-1) >> sh) & 1).reshape(mask.shape[0], -1).double()


def _pack(b):
    """[M, N] bool -> [M, N/8] uint8, bit e of byte j = channel 8 j + e."""
    w = (1 << torch.arange(8)).int()
    return (b.reshape(b.shape[0], -1, 8).int() * w).sum(-1).to(torch.uint8)


def _mm32(a, b, order):
    """fp32 product a [m, k] . b [k, n] in one of two accumulation orders."""
    if order == 0:
        return a @ b
    h = a.shape[1] // 2
    return a[:, h:] @ b[h:] + a[:, :h] @ b[:h]


def _sum32(t, order):
    if order == 0 or t.shape[0] < 2:
        return t.sum(0)
    h = t.shape[0] // 2
    return t[h:].sum(0) + t[:h].sum(0)


def _share(name, what, frag):
    s = float(frag.double().mean()) if frag.numel() else 0.0
    assert s <= FRAGILE_CAP, f"{name}: fragile share of {what} {s:.4f} > {FRAGILE_CAP}"
    return s


def _check_bf16(got, ref, mode, name, bound=None):
    """One bf16 output: exact mode ``got == bf16(ref)``; bound mode within ``bound``."""
    if mode == EXACT:
        U.assert_exact(got, bf(ref), name)
    else:
        U.measure(name, got, ref, bound)
        U.assert_within(got, ref, bound, name)


def _check_f32(got, ref, mode, name, bound=None):
    if mode == EXACT:
        U.assert_exact(got, ref.float().double(), name)
    else:
        U.measure(name, got, ref, bound)
        U.assert_within(got, ref, bound, name)
        U.assert_normal_f32(got, name)


# ============================================================================= conv1x1_bwd
# configuration -> (C, K, TM, lazy, rc, w16)
C1 = {"s0": (64, 256, 64, False, False, 0), "s0w": (64, 256, 64, False, False, 1),
      "s1": (128, 512, 32, False, False, 0), "s0l": (64, 256, 64, True, True, 0),
      "s0lw": (64, 256, 64, True, True, 1), "s1l": (128, 512, 16, True, False, 0)}
# (tiles, set_grid): trips per block below / at / past the ring depth of 3 on ONE block; uneven
# walks (3 + 2, 3 + 2 + 2 tiles); the default grid with fewer tiles than CUs
C1_WALKS = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (5, 2), (7, 3), (3, 0)]
C1_CASES = [(cfg, t, g) for cfg in C1 for t, g in C1_WALKS]


@functools.lru_cache(maxsize=None)
def c1_case(cfg, tiles, grid, mode):
    """Operands (fp64 holding bf16 / fp32 values) and the references that do not depend on the
    kernel's output; the side conditions and the fragile cap are asserted here."""
    C, K, TM, lazy, rc, w16 = C1[cfg]
    M = tiles * TM
    G = min(tiles, grid) if grid else tiles           # tiles < CUs on the default grid
    name = f"c1/{cfg}/{tiles}x{TM}g{grid}/{mode}"
    g = _gen("c1", C, lazy, tiles, grid, mode)
    c = {"name": name, "cfg": cfg, "mode": mode, "M": M, "G": G, "grid": grid, "tiles": tiles}
    if mode == EXACT:
        W = _ints(g, (K, C), -1, 1)
        Y, x = _ints(g, (M, C), 0, 3), _ints(g, (M, C), -3, 3)
        mean, inv = _ints(g, (C,), -1, 1), _pick(g, (C,), [0.5, 1.0, 2.0])
        sc, sh = _pick(g, (C,), [-1.0, 1.0, 2.0]), _ints(g, (C,), -2, 1) + 0.5
        if lazy:
            dy3 = _ints(g, (M, K), -2, 2)
            cA = _pick(g, (K,), [-1.0, 1.0, 2.0])
            cB = _ints(g, (K,), -1, 1) * (torch.rand(K, generator=g) < 0.15)
            cC = _ints(g, (K,), -4, 4)
            x3 = None if rc else _ints(g, (M, K), -3, 3)
        else:
            dO = _ints(g, (M, K), -40, 40)
    else:
        # RC: x3 = Y W^T is the intermediate -> C^-1/2 and a filter of mean = deviation
        W = bf((torch.randn(K, C, generator=g) + 1.0) / math.sqrt(C)) if rc else \
            bf(torch.randn(K, C, generator=g) / math.sqrt(K))
        Y, x = bf(torch.randn(M, C, generator=g).abs()), bf(torch.randn(M, C, generator=g))
        mean, inv = _f32(0.1 * torch.randn(C, generator=g)), _f32(torch.rand(C, generator=g) + 0.5)
        sc, sh = _f32(torch.rand(C, generator=g) + 0.5), _f32(0.2 * torch.randn(C, generator=g))
        if lazy:
            dy3 = bf(torch.randn(M, K, generator=g))
            cA = _f32(torch.rand(K, generator=g) + 0.5)
            cB = _f32(0.3 * torch.randn(K, generator=g))
            cC = _f32(0.1 * torch.randn(K, generator=g))
            x3 = None if rc else bf(torch.randn(M, K, generator=g))
        else:
            dO = bf(torch.randn(M, K, generator=g))
    c.update(W=W, Y=Y, x=x, mean=mean, inv=inv, sc=sc, sh=sh)
    al_dO = torch.zeros(M, K, dtype=torch.float64)
    shares = {}
    if lazy:
        mask = torch.randint(0, 256, (M, K // 8), generator=g).to(torch.uint8)
        c.update(dy3=dy3, mask=mask, cA=cA, cB=cB, cC=cC, x3=x3)
        al_x3 = torch.zeros(M, K, dtype=torch.float64)
        if rc:
            x364 = Y @ W.T
            if mode == EXACT:
                assert float(x364.abs().max()) < 256, name
            else:
                fr, al_x3 = U.fragile_round(x364, gamma(C + 8) * (Y.abs() @ W.abs().T))
                shares["x3"] = _share(name, "x3", fr)
            x3 = bf(x364)
        dz3 = dy3 * _bits(mask)
        dO64 = cA * dz3 + cB * x3 + cC
        if mode == EXACT:
            assert float(dO64.abs().max()) < 256, name
        else:
            err = 3 * U32 * ((cA * dz3).abs() + (cB * x3).abs() + cC.abs())
            fr, al_dO = U.fragile_round(dO64, err)
            shares["dO"] = _share(name, "dO", fr)
            # a fragile x3 moves dO64 by |B| s(x3), and dO by at most that plus one spacing
            mv = cB.abs() * al_x3
            al_dO = al_dO + torch.where(mv > 0, mv + U.ulp16(dO64.abs() + mv), torch.zeros_like(mv))
        dO = bf(dO64)
    c["dO"] = dO
    c["dY"], c["magY"] = dO @ W, dO.abs() @ W.abs()
    c["dW"], c["magW"] = dO.T @ Y, dO.abs().T @ Y.abs()
    c["alY"], c["alW"] = al_dO @ W.abs(), al_dO.T @ Y.abs()
    v = x * sc + sh
    c["dec"] = (v > 0).double()
    c["xhat"] = (x - mean) * inv
    if mode == EXACT:
        assert float(v.abs().min()) >= 0.5, name
        assert float(c["magY"].max()) < 2.0 ** 24 and float(c["magW"].max()) < 2.0 ** 24, name
        dz = bf(c["dY"]).abs()                        # what a right kernel stores
        assert float((dz * c["xhat"].abs()).sum(0).max()) < 2.0 ** 23, name
        assert float(dz.sum(0).max()) < 2.0 ** 23, name
        c["fr_dec"] = torch.zeros(M, C, dtype=torch.float64)
    else:
        fr = v.abs() <= 2 * U32 * ((x * sc).abs() + sh.abs())
        shares["decision"] = _share(name, "ReLU decision", fr)
        c["fr_dec"] = fr.double()
    c["shares"] = shares
    return c


def _c1_rows(case, g):
    """The rows block ``g`` walks: tiles g, g + G, ..."""
    TM = C1[case["cfg"]][2]
    return torch.cat([torch.arange(t * TM, (t + 1) * TM) for t in range(g, case["tiles"], case["G"])])


def c1_verify(case, out):
    """The whole check of one launch (or one emulation): ``out`` holds dy [M, C] bf16, wpart
    [G, K, C], bpart [G, 2, C] and the reduced dw [K, C], on the CPU."""
    C, K, TM = C1[case["cfg"]][:3]
    mode, name, G = case["mode"], case["name"], case["G"]
    _check_bf16(out["dy"], case["dY"], mode, name + "/dy",
                U16 * case["dY"].abs() + FACTOR * gamma(K + 8) * case["magY"] + case["alY"])
    assert out["wpart"].shape == (G, K, C) and out["bpart"].shape == (G, 2, C), name
    assert bool((out["wpart"] != SENT).all()), f"{name}: a dW slab element was never written"
    assert bool((out["bpart"] != SENT).all()), f"{name}: a BN slab element was never written"
    rows_max = -(-case["tiles"] // G) * TM
    _check_f32(out["dw"], case["dW"], mode, name + "/dw",
               FACTOR * gamma(rows_max + G + 8) * case["magW"] + case["alW"])
    # the BN sums, stage-wise: from the kernel's own stored dY
    dyk = out["dy"].double()
    dz = dyk * case["dec"]
    t1, t2 = dz, dz * case["xhat"]
    a1, a2 = case["fr_dec"] * dyk.abs(), case["fr_dec"] * (dyk * case["xhat"]).abs()
    ref = torch.zeros(G, 2, C, dtype=torch.float64)
    bound = torch.zeros(G, 2, C, dtype=torch.float64)
    for g in range(G):
        r = _c1_rows(case, g)
        ref[g, 0], ref[g, 1] = t1[r].sum(0), t2[r].sum(0)
        gm = FACTOR * gamma(len(r) + 8)
        bound[g, 0] = gm * t1[r].abs().sum(0) + a1[r].sum(0)
        bound[g, 1] = gm * t2[r].abs().sum(0) + a2[r].sum(0)
    if mode == EXACT:
        assert float(t2.abs().sum(0).max()) < 2.0 ** 23 and float(t1.abs().sum(0).max()) < 2.0 ** 23
    _check_f32(out["bpart"], ref, mode, name + "/bpart", bound)
    tot = out["bpart"].double().sum(0)
    if mode == EXACT:
        U.assert_exact(tot, ref.sum(0), name + "/bsum")
    else:
        U.measure(name + "/bsum", tot, ref.sum(0), bound.sum(0))
        U.assert_within(tot, ref.sum(0), bound.sum(0), name + "/bsum")


def c1_emulate(case, order=0, damage=None):
    """The kernel in torch: fp32 accumulation in one of two orders, bf16 roundings where the
    kernel has them (x3, dO, the dY store), per-block slabs over the tiles the block walks."""
    C, K, TM, lazy, rc, _ = C1[case["cfg"]]
    G, tiles = case["G"], case["tiles"]
    W, Y, x = case["W"].float(), case["Y"].float(), case["x"].float()
    mean, inv, sc, sh = (case[n].float() for n in ("mean", "inv", "sc", "sh"))
    if lazy:
        if rc:
            x3 = _mm32(Y, W.T.contiguous(), order)
            if damage != "x3_unrounded":
                x3 = x3.to(BF16).float()
        else:
            x3 = case["x3"].float()
        bits = _bits(case["mask"], reverse=damage == "mask_bit_reversed").float()
        if damage == "dz3_ignores_mask":
            bits = torch.ones_like(bits)
        dz3 = case["dy3"].float() * bits
        cA, cB, cC = (case[n].float() for n in ("cA", "cB", "cC"))
        dO = cA * dz3 if damage == "dO_drops_BC" else (cA * dz3 + cB * x3) + cC
        dO = dO.to(BF16).float()
    else:
        dO = case["dO"].float()
    dY32 = _mm32(dO, W, order)
    dy = U.trunc_bf16(dY32) if damage == "trunc" else dY32.to(BF16)
    if damage == "swap_channels":       # channels 1 and 2 of the lane's group 4..7
        dy[:, [5, 6]] = dy[:, [6, 5]]
    dys = dY32 if damage == "sums_unrounded" else dy.float()
    dz = dys * (x * sc + sh > 0).float()
    t2 = dz * (x - mean) * inv
    wpart = torch.zeros(G, K, C)
    bpart = torch.zeros(G, 2, C)
    for g in range(G):
        mine = list(range(g, tiles, G))
        if damage == "tile_twice" and g == 0:
            mine = mine + mine[-1:]     # a ring slot re-read
        for t in (mine if order == 0 else reversed(mine)):
            r = slice(t * TM, (t + 1) * TM)
            wpart[g] += _mm32(dO[r].T.contiguous(), Y[r], order)
        r = _c1_rows(case, g)
        bpart[g, 0], bpart[g, 1] = _sum32(dz[r], order), _sum32(t2[r], order)
    if damage == "s1s2_swapped":
        bpart = bpart.flip(1)
    if damage == "last_row":            # the last row of the last tile never stored
        dy[-1] = SENT
    dw = torch.zeros(K, C)
    for g in (range(G) if order == 0 else reversed(range(G))):
        dw = dw + wpart[g]
    return {"dy": dy, "wpart": wpart, "bpart": bpart, "dw": dw}


def c1_launch(case):
    C, K, TM, lazy, rc, w16 = C1[case["cfg"]]
    M, G, name = case["M"], case["G"], case["name"]
    Kn = _K()
    w = _dev(case["W"])
    wt = _dev(case["W"].T)
    y, x = _dev(case["Y"]), _dev(case["x"])
    prm = [_dev(case[n], torch.float32) for n in ("mean", "inv", "sc", "sh")]
    dy, dy_w = U.guarded((M, C), BF16)
    wpart, wpart_w = U.guarded((G, K, C), torch.float32)
    bpart, bpart_w = U.guarded((G, 2, C), torch.float32)
    dw, dw_w = U.guarded((K, C), torch.float32)
    common = (wt.data_ptr(), y.data_ptr(), x.data_ptr(), *[p.data_ptr() for p in prm],
              dy.data_ptr(), wpart.data_ptr(), bpart.data_ptr(), M, C, K)
    try:
        Kn.conv1x1_bwd_set_grid(case["grid"])
        Kn.conv1x1_bwd_set_w16(w16)
        if lazy:
            assert Kn.conv1x1_bwd_lazy_ok(M, C, K) and Kn.conv1x1_bwd_lazy_blocks(M, C) == G, name
            dy3, mask = _dev(case["dy3"]), case["mask"].to("cuda").contiguous()
            x3 = torch.full((M, K), float("nan"), dtype=BF16, device="cuda") if rc \
                else _dev(case["x3"])
            coef = [_dev(case[n], torch.float32) for n in ("cA", "cB", "cC")]
            Kn.conv1x1_bwd_lazy(dy3.data_ptr(), x3.data_ptr(), mask.data_ptr(),
                                *[p.data_ptr() for p in coef], *common, w.data_ptr(), _st())
        else:
            assert Kn.conv1x1_bwd_ok(M, C, K) and Kn.conv1x1_bwd_blocks(M, C) == G, name
            dO = _dev(case["dO"])
            Kn.conv1x1_bwd(dO.data_ptr(), *common, _st())
        Kn.slab_reduce(wpart.data_ptr(), dw.data_ptr(), K * C, G, 0, _st())
        torch.cuda.synchronize()
    finally:
        Kn.conv1x1_bwd_set_grid(0)
        Kn.conv1x1_bwd_set_w16(0)
    for whole, what in ((dy_w, "dy"), (wpart_w, "wpart"), (bpart_w, "bpart"), (dw_w, "dw")):
        U.assert_guards(whole, f"{name}/{what}")
    return {"dy": dy.cpu(), "wpart": wpart.cpu(), "bpart": bpart.cpu(), "dw": dw.cpu()}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg,tiles,grid", C1_CASES, ids=lambda v: str(v))
def test_conv1x1_bwd(cfg, tiles, grid, mode):
    case = c1_case(cfg, tiles, grid, mode)
    c1_verify(case, c1_launch(case))


# ============================================================================= gemm_stream
# per K: (M, N); the first two give every form a wave-interior tail, a block tail and a
# multi-chunk N; together M covers {1, 33, 255, 256, 257, 513}, N {64, 192, 256, 320}
ST_SHAPES = {64: [(33, 320), (255, 192), (1, 64), (513, 256)],
             128: [(1, 192), (257, 256), (33, 64), (256, 320)],
             256: [(33, 256), (513, 192), (257, 64), (1, 320)]}
ACCS = ["plain", "cin", "masked"]
BNB_FORMS = [f"bnb{k}_{a}" for k in (0, 1, 2) for a in ACCS]
GEMM_NT_FORMS = ["plain", "cin", "masked", "stats"]
PAD3 = (8, 16, 24)          # lda - K, ldb - K, ldc - N
PAD2 = (8, 16, 0)           # forms that need a dense C


def _st_cases():
    out = []
    for K, shapes in ST_SHAPES.items():
        for form in GEMM_NT_FORMS + ["dual", "pre", "pre0", "pre_nostore", "apply"]:
            out += [(form, K, M, N, (0, 0, 0), 1) for M, N in shapes]
        for form in BNB_FORMS:
            out += [(form, K, M, N, (0, 0, 0), 1) for M, N in shapes[:2]]
        if K <= 128:
            for k3 in (64, 128):
                out += [(f"rc{k3}", K, M, N, (0, 0, 0), 1) for M, N in shapes[:3]]
        if (1, 64) not in shapes:
            out.append(("apply", K, 1, 64, (0, 0, 0), 1))
        M, N = shapes[1]
        out += [(form, K, M, N, PAD3, 1) for form in ("plain", "cin", "stats")]
        out += [(form, K, M, N, PAD2, 1) for form in ("bnb1_plain", "bnb2_cin", "bnb0_masked")]
        M, N = shapes[0]
        out += [(form, K, M, N, (0, 0, 0), 0) for form in GEMM_NT_FORMS]
    return out


ST_CASES = _st_cases()


def _st_form(form):
    """form -> (acc, kind, k3, dual): the accumulate epilogue, the BN-backward kind (-1: none),
    the RC depth, the dual slab."""
    if form.startswith("bnb"):
        return form[5:], int(form[3]), 0, False
    if form.startswith("rc"):
        return "plain", 1, int(form[2:]), False
    if form == "dual":
        return "plain", 1, 0, True
    return (form if form in ("cin", "masked") else "plain"), -1, 0, False


@functools.lru_cache(maxsize=None)
def st_case(form, K, M, N, mode):
    acc, kind, k3, dual = _st_form(form)
    pre = form.startswith("pre")
    name = f"stream/{form}/K{K}_{M}x{N}/{mode}"
    g = _gen("st", form, K, M, N, mode)
    ex = mode == EXACT
    c = {"name": name, "form": form, "mode": mode, "K": K, "M": M, "N": N, "shares": {}}
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)      # noqa: E731
    if ex:
        Bw = _ints(g, (N, K), -1, 1)
    elif form == "apply":   # the conv output is the intermediate: mean = deviation (docstring)
        Bw = bf((torch.randn(N, K, generator=g) + 1.0) / math.sqrt(K))
    else:
        Bw = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    c["B"] = Bw
    alA = z(M, K)
    if pre:
        xa = _ints(g, (M, K), -3, 3) if ex else bf(torch.randn(M, K, generator=g))
        psc = _pick(g, (K,), [-1.0, 1.0, 2.0]) if ex else _f32(torch.rand(K, generator=g) + 0.5)
        psh = _ints(g, (K,), -2, 1) + 0.5 if ex else _f32(0.3 * torch.randn(K, generator=g))
        v = xa * psc + psh
        c.update(xa=xa, psc=psc, psh=psh, y64=v.clamp_min(0), yerr=2 * U32 * ((xa * psc).abs() + psh.abs()))
        if ex:
            assert float(v.abs().min()) >= 0.5, name
        else:
            fr, alA = U.fragile_round(v, c["yerr"])
            fr = fr & (v > -c["yerr"])                       # below zero by more: y = 0 either way
            alA = torch.where(fr, alA, z(M, K))
            c["shares"]["y"] = _share(name, "pre y", fr)
        A = bf(c["y64"])
    elif ex:
        A = _ints(g, (M, K), 0, 3) if form == "apply" else _ints(g, (M, K), -2, 2)
    else:
        A = bf(torch.randn(M, K, generator=g))
        if form == "apply":
            A = A.abs()
    c["A"] = A
    y, mag = A @ Bw.T, A.abs() @ Bw.abs().T
    c["alC"] = alA @ Bw.abs().T
    c["y"], c["mag"] = y, mag
    if ex:
        assert float(mag.max()) < 2.0 ** 23, name
    add = None
    if form == "apply":     # a residual wide enough to switch the ReLU both ways
        c["cin"] = add = _ints(g, (M, N), -40, 40) if ex else bf(8.0 * torch.randn(M, N, generator=g))
    elif acc == "cin":
        c["cin"] = add = _ints(g, (M, N), -8, 8) if ex else bf(torch.randn(M, N, generator=g))
    elif acc == "masked":
        c["src"] = _ints(g, (M, N), -8, 8) if ex else bf(torch.randn(M, N, generator=g))
        c["amask"] = torch.randint(0, 256, (M, N // 8), generator=g).to(torch.uint8)
        add = c["src"] * _bits(c["amask"])
    if form == "apply":
        c["asc"] = asc = _pick(g, (N,), [-1.0, 1.0, 2.0]) if ex else _f32(torch.rand(N, generator=g) + 0.5)
        c["ash"] = ash = _ints(g, (N,), -2, 1) + 0.5 if ex else _f32(0.2 * torch.randn(N, generator=g))
        xr, alx = bf(y), z(M, N)
        if not ex:
            fr, alx = U.fragile_round(y, gamma(K + 8) * mag)
            c["shares"]["conv"] = _share(name, "apply conv output", fr)
        c["refC"] = (xr * asc + ash + add).clamp_min(0)
        # fma, add: two fp32 roundings on three terms -> gamma(3 + 8)
        c["boundC"] = U16 * c["refC"].abs() + FACTOR * gamma(3 + 8) * (
            (xr * asc).abs() + ash.abs() + add.abs()) + alx * asc.abs()
    elif add is None:
        c["refC"] = y
        c["boundC"] = U16 * y.abs() + FACTOR * gamma(K + 8) * mag + c["alC"]
    else:
        # exact mode: both roundings are deterministic, ref = bf16(bf16(y) + add).  Bound mode:
        # the first rounding is of the kernel's fp32 y, which may sit across a boundary from
        # the fp64 y, so the reference stays unrounded and each rounding counts u of the value
        # it rounds; the fp32 add is one more rounding of (y + add)
        c["refC"] = (bf(y) if ex else y) + add
        c["boundC"] = U16 * (1 + U16) * (y.abs() + c["refC"].abs()) + \
            FACTOR * gamma(K + 8) * (mag + add.abs()) + c["alC"]
    if ex and (form in ("stats", "pre", "pre_nostore")):
        # sums of squares of half-integers (pre) over a 256-row block
        sq = bf(c["refC"]) ** 2
        worst = max(float(sq[r:r + 256].sum(0).max()) for r in range(0, M, 256))
        assert worst < 2.0 ** 22, (name, worst)
    if kind >= 0:
        c["kind"] = kind
        c["mean"] = _ints(g, (N,), -1, 1) if ex else _f32(0.1 * torch.randn(N, generator=g))
        c["inv"] = _pick(g, (N,), [0.5, 1.0, 2.0]) if ex else _f32(torch.rand(N, generator=g) + 0.5)
        c["fr_dec"], c["alx"] = z(M, N), z(M, N)
        if k3:
            c["y2"] = y2 = _ints(g, (M, k3), 0, 3) if ex else bf(torch.randn(M, k3, generator=g).abs())
            c["w3"] = w3 = _ints(g, (N, k3), -1, 1) if ex else \
                bf((torch.randn(N, k3, generator=g) + 1.0) / math.sqrt(k3))
            x64 = y2 @ w3.T
            if ex:
                assert float(x64.abs().max()) < 256, name
            else:
                fr, c["alx"] = U.fragile_round(x64, gamma(k3 + 8) * (y2.abs() @ w3.abs().T))
                c["shares"]["x3"] = _share(name, "RC x", fr)
            c["bx"] = bf(x64)
        else:
            c["bx"] = _ints(g, (M, N), -3, 3) if ex else bf(torch.randn(M, N, generator=g))
        if kind == 1:
            c["bmask"] = torch.randint(0, 256, (M, N // 8), generator=g).to(torch.uint8)
            c["bit"] = _bits(c["bmask"])
        elif kind == 2:
            c["bsc"] = _pick(g, (N,), [-1.0, 1.0, 2.0]) if ex else _f32(torch.rand(N, generator=g) + 0.5)
            c["bsh"] = _ints(g, (N,), -2, 1) + 0.5 if ex else _f32(0.2 * torch.randn(N, generator=g))
            v = c["bx"] * c["bsc"] + c["bsh"]
            c["bit"] = (v > 0).double()
            if ex:
                assert float(v.abs().min()) >= 0.5, name
            else:
                fr = v.abs() <= 2 * U32 * ((c["bx"] * c["bsc"]).abs() + c["bsh"].abs())
                c["shares"]["decision"] = _share(name, "ReLU decision", fr)
                c["fr_dec"] = fr.double()
        else:
            c["bit"] = torch.ones(M, N, dtype=torch.float64)
        if dual:
            c["bxp"] = _ints(g, (M, N), -3, 3) if ex else bf(torch.randn(M, N, generator=g))
            c["meanp"] = _ints(g, (N,), -1, 1) if ex else _f32(0.1 * torch.randn(N, generator=g))
            c["invp"] = _pick(g, (N,), [0.5, 1.0, 2.0]) if ex else _f32(torch.rand(N, generator=g) + 0.5)
        if ex:                                              # with what a right kernel stores
            dz = (bf(c["refC"]) * c["bit"]).abs()
            xh = (c["bx"] - c["mean"]).abs() * c["inv"]
            for r in range(0, M, 256):
                assert float((dz * xh)[r:r + 256].sum(0).max()) < 2.0 ** 23, name
    return c


def _block_sums(terms, allow, M, mode):
    """Per 256-row block: (fp64 sums [Gb, N], bound [Gb, N]) of ``terms`` [M, N]."""
    Gb = (M + 255) // 256
    ref = torch.stack([terms[b * 256:(b + 1) * 256].sum(0) for b in range(Gb)])
    bnd = torch.stack([FACTOR * gamma(min(256, M - b * 256) + 8) * terms[b * 256:(b + 1) * 256].abs().sum(0)
                       + allow[b * 256:(b + 1) * 256].sum(0) for b in range(Gb)])
    if mode == EXACT:
        assert float(torch.stack([terms[b * 256:(b + 1) * 256].abs().sum(0)
                                  for b in range(Gb)]).max()) < 2.0 ** 23
    return ref, bnd


def st_verify(case, out):
    """The whole check of one launch (or emulation).  ``out``: C [M, N] bf16 and, by form, stats
    / part [Gb, 2, N], part_p, pre_y [M, K], mask [M, N/8]; ``pre_nostore`` adds the second
    launch's C_nost (must be all sentinel), stats_nost, pre_y_nost."""
    form, mode, name, M, N, K = (case[k] for k in ("form", "mode", "name", "M", "N", "K"))
    acc, kind, k3, dual = _st_form(form)
    C = out["C"]
    _check_bf16(C, case["refC"], mode, name + "/C", case["boundC"])
    Ck = C.double()
    zero = torch.zeros(M, N, dtype=torch.float64)
    if form.startswith("pre"):
        yb = U16 * case["y64"] + case["yerr"]
        for key in ("pre_y",) + (("pre_y_nost",) if form == "pre_nostore" else ()):
            _check_bf16(out[key], case["y64"], mode, f"{name}/{key}", yb)
    if form in ("stats", "pre", "pre_nostore"):
        r1, b1 = _block_sums(Ck, zero, M, mode)
        r2, b2 = _block_sums(Ck * Ck, zero, M, mode)
        _check_f32(out["stats"], torch.stack([r1, r2], 1), mode, name + "/stats", torch.stack([b1, b2], 1))
    if form == "pre_nostore":
        assert bool((out["C_nost"].float() == torch.tensor(SENT, dtype=BF16).float()).all()), \
            f"{name}: the no-store form wrote C"
        assert torch.equal(out["stats_nost"], out["stats"]), \
            f"{name}: the no-store form's statistics differ from the storing form's"
    if form == "apply":
        want = _pack(C.float() > 0)
        assert torch.equal(out["mask"], want), \
            f"{name}: {int((out['mask'] != want).sum())} mask bytes differ from Y_stored > 0"
    if kind >= 0:
        dz = Ck * case["bit"]
        xh = (case["bx"] - case["mean"]) * case["inv"]
        # a fragile decision: either dz; a fragile RC x: x off by one spacing
        a1 = case["fr_dec"] * Ck.abs()
        a2 = case["fr_dec"] * (Ck * xh).abs() + dz.abs() * case["alx"] * case["inv"]
        r1, b1 = _block_sums(dz, a1, M, mode)
        r2, b2 = _block_sums(dz * xh, a2, M, mode)
        _check_f32(out["part"], torch.stack([r1, r2], 1), mode, name + "/part", torch.stack([b1, b2], 1))
        if dual:
            xp = (case["bxp"] - case["meanp"]) * case["invp"]
            r3, b3 = _block_sums(dz * xp, zero, M, mode)
            _check_f32(out["part_p"], torch.stack([r1, r3], 1), mode, name + "/part_p",
                       torch.stack([b1, b3], 1))


def _slabs(terms, order):
    return torch.stack([_sum32(terms[b * 256:(b + 1) * 256], order)
                        for b in range((terms.shape[0] + 255) // 256)])


def st_emulate(case, order=0, damage=None):
    form, M, N, K = (case[k] for k in ("form", "M", "N", "K"))
    acc, kind, k3, dual = _st_form(form)
    rnd = U.trunc_bf16 if damage == "trunc" else (lambda t: t.to(BF16))
    Bw = case["B"].float()
    out = {}
    if form.startswith("pre"):
        v = case["xa"].float() * case["psc"].float() + case["psh"].float()
        out["pre_y"] = v.clamp_min(0).to(BF16)
        A = out["pre_y"].float()
    else:
        A = case["A"].float()
    acc32 = _mm32(A, Bw.T.contiguous(), order)
    if form == "apply":
        o = acc32.to(BF16).float() * case["asc"].float() + case["ash"].float()
        pre_res = o
        o = (o + case["cin"].float()).clamp_min(0)
        out["C"] = rnd(o)
        src = pre_res if damage == "apply_mask_pre_residual" else out["C"].float()
        out["mask"] = _pack(src > 0)
        return out
    if acc == "cin":
        c = rnd(acc32.to(BF16).float() + case["cin"].float())
    elif acc == "masked":
        bits = _bits(case["amask"], reverse=damage == "mask_bit_reversed").float()
        c = rnd(acc32.to(BF16).float() + case["src"].float() * bits)
    else:
        c = rnd(acc32)
    out["C"] = c
    cf = c.float()
    if form in ("stats", "pre", "pre_nostore"):
        out["stats"] = torch.stack([_slabs(cf, order), _slabs(cf * cf, order)], 1)
    if form == "pre_nostore":
        out["C_nost"] = c.clone() if damage == "nostore_writes_C" else torch.full_like(c, SENT)
        out["stats_nost"], out["pre_y_nost"] = out["stats"].clone(), out["pre_y"].clone()
    if kind >= 0:
        if k3:
            bx = _mm32(case["y2"].float(), case["w3"].float().T.contiguous(), order).to(BF16).float()
        else:
            bx = case["bx"].float()
        if kind == 1:
            bit = case["bit"].float()
        elif kind == 2:
            bit = (bx * case["bsc"].float() + case["bsh"].float() > 0).float()
        else:
            bit = torch.ones_like(cf)
        dz = cf * bit
        s1 = _slabs(dz, order)
        s2 = _slabs(dz * (bx - case["mean"].float()) * case["inv"].float(), order)
        out["part"] = torch.stack([s1, s2], 1)
        if dual:
            s3 = _slabs(dz * (case["bxp"].float() - case["meanp"].float()) * case["invp"].float(), order)
            out["part_p"] = out["part"].clone() if damage == "dual_copies_first" \
                else torch.stack([s1, s3], 1)
    return out


def _rows(t64, ld, dtype=BF16):
    """[M, n] -> a device tensor [M, ld] holding it in its first n columns (the rest zero)."""
    full = torch.zeros(t64.shape[0], ld, dtype=dtype)
    full[:, :t64.shape[1]] = t64.to(dtype)
    return full.to("cuda")


def _p(t):
    return 0 if t is None else t.data_ptr()


def st_launch(case, pads=(0, 0, 0), nt=1):
    form, M, N, K, name = (case[k] for k in ("form", "M", "N", "K", "name"))
    acc, kind, k3, dual = _st_form(form)
    nat, Kn = _native(), _K()
    lda, ldb, ldc = K + pads[0], K + pads[1], N + pads[2]
    assert Kn.gemm_stream_ok(M, N, K, lda, ldb, ldc), name
    Gb = (M + 255) // 256
    f32 = torch.float32
    a = _rows(case["xa"] if form.startswith("pre") else case["A"], lda)
    b = _rows(case["B"], ldb)
    cbuf, c_w = U.guarded((M, ldc), BF16)
    whole = [(c_w, "C")]
    cin = _rows(case["cin"], ldc) if "cin" in case else None
    src = _dev(case["src"]) if acc == "masked" else None
    amask = case["amask"].to("cuda").contiguous() if acc == "masked" else None
    stats = part = part_p = pre_y = mask = None
    if form in ("stats", "pre", "pre_nostore"):
        stats, w_ = U.guarded((Gb, 2, N), f32)
        whole.append((w_, "stats"))
    if kind >= 0:
        part, w_ = U.guarded((Gb, 2, N), f32)
        whole.append((w_, "part"))
    if dual:
        part_p, w_ = U.guarded((Gb, 2, N), f32)
        whole.append((w_, "part_p"))
    if form.startswith("pre"):
        pre_y, w_ = U.guarded((M, K), BF16)
        whole.append((w_, "pre_y"))
    out = {}
    try:
        Kn.gemm_set_variant(13)
        Kn.gemm_set_nt(nt)
        if form in GEMM_NT_FORMS:
            av, bv, cv = a[:, :K], b[:, :K], cbuf[:, :N]
            if cin is not None and ldc != N:
                Kn.gemm_nt(a.data_ptr(), b.data_ptr(), cbuf.data_ptr(), M, N, K, lda, ldb, ldc, 0,
                           cin.data_ptr(), 0, _st(), 0, 0, 0)
            else:
                nat.gemm_nt(av, bv, out=cv, cin=cin, stats=stats,
                            acc_from=nat._MaskedGrad(src, amask.view(-1)) if acc == "masked" else None)
        elif form == "apply":
            mask, mask_w = U.guarded((M, N // 8), torch.uint8, fill=MASK_FILL)
            keep = [_dev(case["asc"], f32), _dev(case["ash"], f32)]
            Kn.gemm_stream_apply(a.data_ptr(), b.data_ptr(), cbuf.data_ptr(), M, N, K,
                                 cin.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(),
                                 mask.data_ptr(), _st())
        elif form.startswith("pre"):
            keep = [_dev(case["psc"], f32), _dev(case["psh"], f32)]
            Kn.gemm_stream_pre(a.data_ptr(), b.data_ptr(), cbuf.data_ptr(), M, N, K,
                               keep[0].data_ptr(), keep[1].data_ptr(), pre_y.data_ptr(),
                               _p(stats), _st(), 0)
            if form == "pre_nostore":
                c2, c2_w = U.guarded((M, N), BF16)
                s2, s2_w = U.guarded((Gb, 2, N), f32)
                y2, y2_w = U.guarded((M, K), BF16)
                whole += [(c2_w, "C_nost"), (s2_w, "stats_nost"), (y2_w, "pre_y_nost")]
                Kn.gemm_stream_pre(a.data_ptr(), b.data_ptr(), c2.data_ptr(), M, N, K,
                                   keep[0].data_ptr(), keep[1].data_ptr(), y2.data_ptr(),
                                   s2.data_ptr(), _st(), 1)
                torch.cuda.synchronize()
                out.update(C_nost=c2.cpu(), stats_nost=s2.cpu(), pre_y_nost=y2.cpu())
        else:
            prm = {n: _dev(case[n], f32) for n in ("mean", "inv", "bsc", "bsh", "meanp", "invp")
                   if n in case}
            bmask = case["bmask"].to("cuda").contiguous() if kind == 1 else None
            if k3:      # the launcher's own check is (!bx && !rc): a NaN buffer or 0
                bx = torch.full((M, N), float("nan"), dtype=BF16, device="cuda") \
                    if N in (192, 320) else None
                y2d, w3d = _dev(case["y2"]), _dev(case["w3"])
            else:
                bx, y2d, w3d = _dev(case["bx"]), None, None
            head = (a.data_ptr(), b.data_ptr(), cbuf.data_ptr(), M, N, K, lda, ldb, ldc,
                    _p(cin) if acc == "cin" else 0, _p(src), _p(amask), _p(bx),
                    prm["mean"].data_ptr(), prm["inv"].data_ptr())
            if dual:
                bxp = _dev(case["bxp"])
                Kn.gemm_stream_bnb_dual(*head, bmask.data_ptr(), part.data_ptr(), bxp.data_ptr(),
                                        prm["meanp"].data_ptr(), prm["invp"].data_ptr(),
                                        part_p.data_ptr(), _st())
            else:
                Kn.gemm_stream_bnb(*head, _p(prm.get("bsc")), _p(prm.get("bsh")), _p(bmask), kind,
                                   part.data_ptr(), _st(), _p(y2d), _p(w3d), k3)
        torch.cuda.synchronize()
    finally:
        Kn.gemm_set_variant(-1)
        Kn.gemm_set_nt(1)
    for w_, what in whole:
        U.assert_guards(w_, f"{name}/{what}")
    ch = cbuf.cpu()
    if ldc != N:
        assert bool((ch[:, N:].float() == torch.tensor(SENT, dtype=BF16).float()).all()), \
            f"{name}: wrote between N and ldc"
    out["C"] = ch[:, :N].contiguous()
    if mask is not None:
        U.assert_guards(mask_w, f"{name}/mask", fill=MASK_FILL)
        out["mask"] = mask.cpu()
    for key, t in (("stats", stats), ("part", part), ("part_p", part_p), ("pre_y", pre_y)):
        if t is not None:
            out[key] = t.cpu()
    return out


def _st_id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form,K,M,N,pads,nt", ST_CASES, ids=_st_id)
def test_gemm_stream(form, K, M, N, pads, nt, mode):
    case = st_case(form, K, M, N, mode)
    st_verify(case, st_launch(case, pads, nt))


# ============================================================================= CPU self-tests
def test_ok_refusals_dry():
    """``conv1x1_bwd_ok`` / ``_lazy_ok`` are host code: every listed case is accepted; a row count
    that is no multiple of the tile, (64, 512) and M = 0 are refused."""
    Kn = _K()
    for cfg, (C, K, TM, lazy, rc, w16) in C1.items():
        ok = Kn.conv1x1_bwd_lazy_ok if lazy else Kn.conv1x1_bwd_ok
        for tiles, _ in C1_WALKS:
            assert ok(tiles * TM, C, K), (cfg, tiles)
        if TM == 16:        # TM + 16 is two whole tiles here
            assert ok(TM + 16, C, K) and not ok(TM + 8, C, K), cfg
        else:
            assert not ok(TM + 16, C, K), cfg
        assert not ok(0, C, K) and not ok(4 * TM, 64, 512), cfg


@pytest.mark.parametrize("mode", MODES)
def test_emulated_conv1x1_bwd(mode):
    """Both accumulation orders pass the kernels' check on every case; building the cases proves
    the side conditions (exact) and the fragile cap (bound) on the reference."""
    for cfg, tiles, grid in C1_CASES:
        case = c1_case(cfg, tiles, grid, mode)
        for order in (0, 1):
            c1_verify(case, c1_emulate(case, order))
        for what, s in case["shares"].items():
            print(f"FRAGILE {case['name']} {what} {s:.5f}")


@pytest.mark.parametrize("mode", MODES)
def test_emulated_gemm_stream(mode):
    for form, K, M, N in sorted({c[:4] for c in ST_CASES}):
        case = st_case(form, K, M, N, mode)
        for order in (0, 1):
            st_verify(case, st_emulate(case, order))
        for what, s in case["shares"].items():
            print(f"FRAGILE {case['name']} {what} {s:.5f}")


# damage -> (family, case key): the smallest case on which the damaged code path runs
DAMAGES = {
    "last_row": ("c1", ("s0", 2, 1)),
    "tile_twice": ("c1", ("s1", 4, 1)),
    "swap_channels": ("c1", ("s0w", 1, 1)),
    "s1s2_swapped": ("c1", ("s1", 1, 1)),
    "sums_unrounded": ("c1", ("s0", 1, 1)),
    "mask_bit_reversed": ("c1", ("s1l", 1, 1)),
    "dz3_ignores_mask": ("c1", ("s0l", 1, 1)),
    "dO_drops_BC": ("c1", ("s0l", 2, 1)),
    "apply_mask_pre_residual": ("st", ("apply", 64, 33, 320)),
    "nostore_writes_C": ("st", ("pre_nostore", 64, 33, 320)),
    "dual_copies_first": ("st", ("dual", 128, 1, 192)),
}
BOUND_ONLY_DAMAGES = {"trunc": ("c1", ("s0", 1, 1)), "x3_unrounded": ("c1", ("s0l", 1, 1))}


def _run_damage(kind, where, mode):
    fam, key = where
    if fam == "c1":
        case = c1_case(*key, mode)
        c1_verify(case, c1_emulate(case, 0))            # the undamaged emulation passes
        return lambda: c1_verify(case, c1_emulate(case, 0, damage=kind))
    case = st_case(*key, mode)
    st_verify(case, st_emulate(case, 0))
    return lambda: st_verify(case, st_emulate(case, 0, damage=kind))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", list(DAMAGES))
def test_damage_detected(kind, mode):
    check = _run_damage(kind, DAMAGES[kind], mode)
    with pytest.raises(AssertionError):
        check()


@pytest.mark.parametrize("kind", list(BOUND_ONLY_DAMAGES))
def test_bound_only_damage_detected(kind):
    """Truncation instead of rounding, and an unrounded x3: outside the bound in bound mode (in
    exact mode the values are representable and the rounding skipped is the identity)."""
    check = _run_damage(kind, BOUND_ONLY_DAMAGES[kind], BOUND)
    with pytest.raises(AssertionError):
        check()


def test_truncation_detected_on_stream_store():
    case = st_case("plain", 64, 33, 320, BOUND)
    with pytest.raises(AssertionError):
        st_verify(case, st_emulate(case, 0, damage="trunc"))
