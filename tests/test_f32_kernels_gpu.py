"""The fp32 kernels of ``csrc/kernels/f32.hip`` (``ops/native_f32.py``) element by element against
fp64, at the shapes where they can go wrong: tile / K tails, every operand orientation, the
epilogue (alpha, bias, ReLU, accumulate), split-K with fewer launched slabs than planned, odd
conv / pool geometries, grids that make more than one trip, and the clipped cross-entropy with
its clip active.

Two comparison modes:

* bound mode: ``|got - ref64| <= gamma(terms) * mag64`` per element, the standard a-priori bound
  of an fp32 fma chain in ANY summation order (so it holds for split-K too), with
  ``gamma(n) = n u / (1 - n u)``, ``u = 2^-24`` and ``mag64`` the fp64 sum of absolute products;
* exact mode: small-integer inputs and a power-of-two ``alpha``; every partial sum stays below
  2^24, the result is exact in any order and must ``torch.equal`` the fp64 one.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TRIP = 65536 * 256          # grid_for() caps at 65536 blocks of 256 threads


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _nf():
    from distributedtensorflow_amd.ops import native_f32
    return native_f32


def _K():
    from distributedtensorflow_amd.ops import native
    return native._K


def _st():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------- helpers
def gamma(n):
    assert n * U < 1
    return n * U / (1.0 - n * U)


def assert_within_fma_bound(got, ref64, mag64, terms, what=""):
    """Element-wise ``|got - ref64| <= gamma(terms) * mag64``; reports the worst element."""
    g64 = got.detach().double().cpu()
    ref64, mag64 = ref64.detach().double().cpu(), mag64.detach().double().cpu()
    assert g64.shape == ref64.shape == mag64.shape, (what, g64.shape, ref64.shape, mag64.shape)
    assert bool(torch.isfinite(g64).all()), f"{what}: non-finite result"
    err = (g64 - ref64).abs()
    bound = gamma(terms) * mag64
    bad = err > bound
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        flat = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), ratio.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the fma bound "
            f"(terms={terms}); worst at {idx}: got {g64[idx].item()!r} ref {ref64[idx].item()!r} "
            f"err {err[idx].item():.3e} = {ratio[idx].item():.3g} x bound {bound[idx].item():.3e}")


def assert_exact(got, ref64, what=""):
    g64 = got.detach().double().cpu()
    ref64 = ref64.detach().double().cpu()
    assert g64.shape == ref64.shape, (what, g64.shape, ref64.shape)
    if not torch.equal(g64, ref64):
        bad = g64 != ref64
        idx = tuple(int(v[0]) for v in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at "
                             f"{idx}: got {g64[idx].item()!r} ref {ref64[idx].item()!r}")


def _check(got, ref64, mag64, terms, exact, what=""):
    if exact:
        assert_exact(got, ref64, what)
    else:
        assert_within_fma_bound(got, ref64, mag64, terms, what)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _vals(shape, g, exact):
    """fp32 test data made on the CPU: integers in [-3, 3] (exact mode) or randn."""
    if exact:
        return torch.randint(-3, 4, shape, generator=g).float()
    return torch.randn(shape, generator=g)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- 0. helper tests
@pytest.mark.parametrize("signs", ["randn", "positive"])
@pytest.mark.parametrize("K", [17, 2048])
def test_fma_bound_accepts_fp32_matmul_and_rejects_damage(K, signs):
    """A plain fp32 matmul is inside the bound; one element off by 1e-3 relative, or one zeroed
    row, is outside: the GPU tests below can fail.

    The bound is relative to the sum of ABSOLUTE products.  At K = 2048 it is 1.2e-4 of that sum;
    randn operands cancel down to ~3 % of it, so a 1e-3 relative change of one such element
    (3e-5 of the sum) is within what fp32 itself may do at that K, while a zeroed row is not.
    With operands of one sign nothing cancels and the 1e-3 change is caught at both K; exact
    mode (below) catches a single wrong product at any K."""
    g = _gen(K)
    a, b = torch.randn(37, K, generator=g), torch.randn(29, K, generator=g)
    if signs == "positive":
        a, b = a.abs(), b.abs()
    out = a @ b.t()
    ref = a.double() @ b.double().t()
    mag = a.double().abs() @ b.double().abs().t()
    assert_within_fma_bound(out, ref, mag, K + 4)
    if signs == "positive" or K == 17:
        i, j = divmod(int(ref.abs().argmax()), 29)
        one = out.clone()
        one[i, j] *= 1 + 1e-3
        with pytest.raises(AssertionError, match=rf"1 of 1073 .* worst at \({i}, {j}\)"):
            assert_within_fma_bound(one, ref, mag, K + 4)
    row = out.clone()
    row[36] = 0
    with pytest.raises(AssertionError, match="outside the fma bound"):
        assert_within_fma_bound(row, ref, mag, K + 4)
    nan = out.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_within_fma_bound(nan, ref, mag, K + 4)


def test_exact_mode_is_exact_on_the_cpu():
    """Integer inputs in [-3, 3] and a power-of-two alpha: fp32 matmul == fp64, at the longest K
    the GPU tests use (9 * 51300 < 2^24); one dropped product is caught."""
    g = _gen(1)
    a, b = _vals((8, 51300), g, True), _vals((8, 51300), g, True)
    out = -0.5 * (a @ b.t())
    ref = -0.5 * (a.double() @ b.double().t())
    assert float(ref.abs().max()) < 2 ** 24
    assert_exact(out, ref)
    k = int((a[3] * b[5]).abs().argmax())
    a2 = a.clone()
    a2[3, k] = 0
    with pytest.raises(AssertionError, match="differ"):
        assert_exact(-0.5 * (a2 @ b.t()), ref)


# ----------------------------------------------------------------------------- 1. gemm_f32
NAN = float("nan")
SENTINEL = -7.0625e11


def _strided(vals, inner_fast, pad=3):
    """A CUDA view ``v`` with ``v[r, c] == vals[r, c]`` inside a larger NaN-filled buffer (real
    offset, padded leading dimension); ``inner_fast``: the second index is the contiguous one.
    A read outside the view poisons the result."""
    rows, cols = vals.shape
    if inner_fast:
        v = torch.full((rows + 2, cols + 2 + pad), NAN, device="cuda")[1:rows + 1, 2:cols + 2]
    else:
        v = torch.full((cols + 2, rows + 2 + pad), NAN, device="cuda")[1:cols + 1, 2:rows + 2].t()
    v.copy_(vals)
    assert v.shape == vals.shape
    return v


def _c_buffer(M, N, colmajor, padded):
    """(buffer pre-filled with a sentinel, function taking a buffer-shaped tensor to its M x N
    view).  ``padded``: a 2-D window with a padded leading dimension; else a dense M x N block
    (what split-K needs) with guard elements on both sides."""
    if padded:
        shape = (N + 2, M + 5) if colmajor else (M + 2, N + 5)
        sel = (lambda t: t[1:N + 1, 2:M + 2].t()) if colmajor else (lambda t: t[1:M + 1, 2:N + 2])
    else:
        shape = (M * N + 64,)
        sel = (lambda t: t[32:32 + M * N].view(N, M).t()) if colmajor else \
            (lambda t: t[32:32 + M * N].view(M, N))
    return torch.full(shape, SENTINEL, device="cuda"), sel


def _assert_outside_untouched(buf, before, sel, what=""):
    outside = torch.ones_like(buf, dtype=torch.bool)
    sel(outside).fill_(False)
    assert torch.equal(_bits(buf)[outside], _bits(before)[outside]), f"{what}: wrote outside C"


def _gemm_case(M, N, K, a_kfast=True, b_kfast=True, colmajor=False, padded=True, exact=False,
               alpha=1.0, bias=False, relu=False, accumulate=False, seed=0, ws="auto", pad=3):
    g = _gen(seed * 1000003 + M * 131 + N * 17 + K)
    A, B = _vals((M, K), g, exact), _vals((N, K), g, exact)
    bv = _vals((N,), g, exact) if bias else None
    C0 = _vals((M, N), g, exact)
    if exact:
        C0 = C0 * 5                      # so relu-then-add differs from add-then-relu often
    a, b = _strided(A, a_kfast, pad), _strided(B, b_kfast, pad)
    buf, sel = _c_buffer(M, N, colmajor, padded)
    c = sel(buf)
    assert c.shape == (M, N)
    if accumulate:
        c.copy_(C0)
    before = buf.clone()
    bd = bv.cuda() if bias else None
    args = (M, N, K, a, a.stride(0), a.stride(1), b, b.stride(0), b.stride(1), c, c.stride(0),
            c.stride(1))
    if isinstance(ws, str):
        _nf().gemm_f32(*args, bias=bd, relu=relu, accumulate=accumulate, alpha=alpha)
    else:
        _K().gemm_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), 0 if bd is None else bd.data_ptr(),
                      M, N, K, *args[4:6], *args[7:9], *args[10:12], float(alpha), int(relu),
                      int(accumulate), ws.data_ptr(), _st())
    torch.cuda.synchronize()
    prod = A.double() @ B.double().t()
    ref = alpha * prod + (bv.double() if bias else 0)
    mag = abs(alpha) * (A.double().abs() @ B.double().abs().t()) + (bv.double().abs() if bias else 0)
    if relu:
        ref = torch.relu(ref)
    if accumulate:
        if relu:                         # the case must tell relu(x) + c from relu(x + c)
            assert bool((torch.relu(ref + C0.double()) != ref + C0.double()).any()) or M * N < 4
        ref = ref + C0.double()
        mag = mag + C0.double().abs()
    what = (f"gemm {M}x{N}x{K} a_k={a_kfast} b_k={b_kfast} col={colmajor} pad={padded} "
            f"alpha={alpha} bias={bias} relu={relu} acc={accumulate} exact={exact}")
    _check(c, ref, mag, K + 4, exact, what)
    _assert_outside_untouched(buf, before, sel, what)


TILE_SHAPES = [(1, 1, 1), (64, 64, 16), (65, 63, 17), (130, 70, 33), (33, 129, 15)]


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["bound", "exact"])
@pytest.mark.parametrize("M,N,K", TILE_SHAPES)
def test_gemm_f32_tiles_and_tails(M, N, K, exact):
    assert _K().gemm_f32_splits(M, N, K) == 1
    _gemm_case(M, N, K, exact=exact, seed=1)
    _gemm_case(M, N, K, exact=exact, alpha=-2.0 if exact else -0.5, bias=True, relu=True,
               accumulate=True, seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("a_kfast,b_kfast,colmajor",
                         list(itertools.product([True, False], repeat=3)))
def test_gemm_f32_orientations(a_kfast, b_kfast, colmajor):
    """All 8 operand orientations at (65, 63, 17); every operand has a padded leading dimension
    (``sam = K + 5`` ...), C a padded row / column stride, and the bias follows the GEMM's n
    whichever way C is stored."""
    for exact in (False, True):
        _gemm_case(65, 63, 17, a_kfast, b_kfast, colmajor, padded=True, exact=exact, bias=True,
                   seed=3)
        _gemm_case(65, 63, 17, a_kfast, b_kfast, colmajor, padded=False, exact=exact,
                   alpha=0.5, accumulate=True, seed=4, pad=0)


@pytest.mark.gpu
@pytest.mark.parametrize("bias,relu,accumulate", list(itertools.product([False, True], repeat=3)))
def test_gemm_f32_epilogue(bias, relu, accumulate):
    """C_new = C_old [accumulate] + act(alpha AB + bias): the ReLU applies before the add."""
    _gemm_case(65, 63, 17, alpha=-0.5, bias=bias, relu=relu, accumulate=accumulate, seed=5)
    _gemm_case(65, 63, 17, exact=True, alpha=-0.5, bias=bias, relu=relu, accumulate=accumulate,
               seed=6)
    _gemm_case(33, 129, 15, colmajor=True, exact=True, alpha=4.0, bias=bias, relu=relu,
               accumulate=accumulate, seed=7)


SPLIT_SHAPES = [(8, 8, 2048), (70, 25, 6272), (8, 8, 51300)]


@pytest.mark.gpu
@pytest.mark.parametrize("mfast", [False, True], ids=["kfast", "wgrad"])
@pytest.mark.parametrize("colmajor", [False, True], ids=["rowC", "colC"])
@pytest.mark.parametrize("M,N,K", SPLIT_SHAPES)
def test_gemm_f32_split_k(M, N, K, colmajor, mfast):
    """Split-K (slab workspace + in-order sum), plain and with bias + ReLU + accumulate, in both
    modes; ``mfast`` = A and B contiguous along m / n, the weight-gradient orientation."""
    S = _K().gemm_f32_splits(M, N, K)
    assert S > 1
    if K == 51300:
        assert S == 100
    for exact in (False, True):
        kw = dict(a_kfast=not mfast, b_kfast=not mfast, colmajor=colmajor, padded=False,
                  exact=exact)
        _gemm_case(M, N, K, seed=8, **kw)
        _gemm_case(M, N, K, alpha=-2.0 if exact else -0.5, bias=True, relu=True, accumulate=True,
                   seed=9, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("colmajor", [False, True], ids=["rowC", "colC"])
def test_gemm_f32_split_k_fewer_slabs_than_planned(colmajor):
    """K = 51300: the plan is S = 100 splits, the 16-aligned chunk is 528, so only 98 slabs are
    launched.  The workspace is NaN: summing a never-written slab shows, and so does a write past
    the S * M * N floats the caller is asked for."""
    M, N, K = 8, 8, 51300
    S = _K().gemm_f32_splits(M, N, K)
    assert S == 100
    chunk = -(-(-(-K // S)) // 16) * 16
    assert chunk == 528 and -(-K // chunk) == 98
    for exact, mfast in itertools.product((True, False), (False, True)):
        ws = torch.full((S * M * N + 4096,), NAN, device="cuda")
        before = ws[S * M * N:].clone()
        _gemm_case(M, N, K, a_kfast=not mfast, b_kfast=not mfast, colmajor=colmajor, padded=False,
                   exact=exact, alpha=-2.0 if exact else -0.5, bias=True, relu=True,
                   accumulate=True, seed=10, ws=ws)
        assert torch.equal(_bits(ws[S * M * N:]), _bits(before))
        assert bool(torch.isnan(ws[98 * M * N:S * M * N]).all())      # slabs 98, 99: not launched
        assert bool(torch.isfinite(ws[:98 * M * N]).all())


@pytest.mark.gpu
def test_gemm_f32_split_k_rejects_strided_c_and_missing_workspace():
    M, N, K = 8, 8, 2048
    assert _K().gemm_f32_splits(M, N, K) > 1
    g = _gen(11)
    a, b = _vals((M, K), g, False).cuda(), _vals((N, K), g, False).cuda()
    buf, sel = _c_buffer(M, N, False, True)          # padded row stride: not a dense block
    c = sel(buf)
    before = buf.clone()
    with pytest.raises(RuntimeError, match="contiguous"):
        _nf().gemm_f32(M, N, K, a, K, 1, b, K, 1, c, c.stride(0), c.stride(1))
    dense = torch.full((M, N), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="workspace"):
        _K().gemm_f32(a.data_ptr(), b.data_ptr(), dense.data_ptr(), 0, M, N, K, K, 1, K, 1, N, 1,
                      1.0, 0, 0, 0, _st())
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(before))
    assert bool((dense == SENTINEL).all())


# ----------------------------------------------------------------------------- 2. im2col / conv
# (H, W, R, S, stride, padding)
GEOMS = {
    "3x3s2same8x8": (8, 8, 3, 3, 2, "same"),            # asymmetric padding 0 / 1
    "7x7s2same9x12": (9, 12, 7, 7, 2, "same"),
    "1x1s2valid7x7": (7, 7, 1, 1, 2, "valid"),
    "2x3s21pad1_6x5": (6, 5, 2, 3, (2, 1), 1),
    "5x5s1same6x7": (6, 7, 5, 5, 1, "same"),
}


def _geom(name):
    from distributedtensorflow_amd.ops.reference import resolve_padding
    H, W, R, S, stride, padding = GEOMS[name]
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    pt, pb, pl, pr = resolve_padding(padding, H, W, R, S, stride)
    P, Q = (H + pt + pb - R) // sh + 1, (W + pl + pr - S) // sw + 1
    return H, W, R, S, sh, sw, pt, pb, pl, pr, P, Q


def _unfold_ref(x, name):
    """im2col of NHWC ``x`` by F.unfold on the padded NCHW input, columns in (r, s, c) order."""
    H, W, R, S, sh, sw, pt, pb, pl, pr, P, Q = _geom(name)
    n, c = x.shape[0], x.shape[3]
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    u = F.unfold(xn, (R, S), stride=(sh, sw))                  # [n, c * R * S, P * Q], c-major
    assert u.shape == (n, c * R * S, P * Q)
    return u.view(n, c, R, S, P * Q).permute(0, 4, 2, 3, 1).reshape(n * P * Q, R * S * c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMS))
def test_im2col_col2im_f32(name):
    H, W, R, S, sh, sw, pt, pb, pl, pr, P, Q = _geom(name)
    n, c = 2, 3
    g = _gen(20 + H * W)
    x = torch.randn(n, H, W, c, generator=g)
    ref = _unfold_ref(x, name)
    M, TC = n * P * Q, R * S * c
    cols = torch.full((M * TC + 64,), NAN, device="cuda")
    xg = x.cuda()
    _K().im2col_f32(xg.data_ptr(), cols.data_ptr(), n, H, W, c, P, Q, sh, sw, R, S, pt, pl,
                    _st())
    torch.cuda.synchronize()
    assert torch.equal(cols[:M * TC].view(M, TC).cpu(), ref)          # a pure copy
    assert bool(torch.isnan(cols[M * TC:]).all())
    for exact in (True, False):
        dcols = _vals((M, TC), g, exact)
        xr = x.double().requires_grad_()
        (dref,) = torch.autograd.grad(_unfold_ref(xr, name), xr, dcols.double())
        (dmag,) = torch.autograd.grad(_unfold_ref(xr, name), xr, dcols.double().abs())
        dx = torch.full((n * H * W * c + 64,), NAN, device="cuda")
        dcg = dcols.cuda()
        _K().col2im_f32(dcg.data_ptr(), dx.data_ptr(), n, H, W, c, P, Q, sh, sw, R, S,
                        pt, pl, _st())
        torch.cuda.synchronize()
        _check(dx[:n * H * W * c].view(n, H, W, c), dref, dmag, R * S, exact, f"col2im {name}")
        assert bool(torch.isnan(dx[n * H * W * c:]).all())


def _relu_mask(z, mag_y, terms, y_got):
    """The ReLU mask the gradients are judged with.  Wherever the fp64 pre-activation is clear of
    zero by more than the forward bound, it is the fp64 one, and the kernel's own mask (its
    output > 0) must agree: asserted.  Only where rounding may legitimately decide the sign is
    the kernel's own mask taken."""
    clear = z.abs() > gamma(terms) * mag_y
    got = y_got.detach().double().cpu().reshape(z.shape) > 0
    assert torch.equal(got[clear], (z > 0)[clear]), "ReLU mask differs from fp64 away from zero"
    return torch.where(clear, z > 0, got).double()


def _conv_reference(x, w, b, dy, stride, padding, relu, y_got=None):
    """fp64 conv (+bias)(+ReLU) forward and gradients, with the magnitude of every sum (the same
    linear maps applied to absolute values) for the element-wise bound.  ``y_got``: the kernel's
    forward output (see :func:`_relu_mask`)."""
    from distributedtensorflow_amd.ops import reference
    K, R, S, C = w.shape
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if b is not None else None
    xa, wa = x.double().abs().requires_grad_(), w.double().abs().requires_grad_()
    za = reference.conv2d(xa, wa, stride, padding)
    mag_y = za.detach() + (b.double().abs() if b is not None else 0)
    z = reference.conv2d(xr, wr, stride, padding)
    if br is not None:
        z = z + br
    mask = _relu_mask(z.detach(), mag_y, R * S * C + 4, y_got) if relu else torch.ones_like(z)
    y = z * mask
    dy = dy.double()
    y.backward(dy)
    dz = dy * mask
    mag_dx, mag_dw = torch.autograd.grad(za, (xa, wa), dz.abs())
    return dict(y=y.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if br is not None else None,
                mag_y=mag_y, mag_dx=mag_dx, mag_dw=mag_dw, mag_db=dz.abs().sum((0, 1, 2)))


def _conv_inputs(name, C, K, n=2):
    H, W, R, S = GEOMS[name][:4]
    g = _gen(31 * C + K + H * W)
    x = torch.randn(n, H, W, C, generator=g)
    w = torch.randn(K, R, S, C, generator=g) / (R * S * C) ** 0.5
    b = torch.randn(K, generator=g)
    P, Q = _geom(name)[-2:]
    dy = torch.randn(n, P, Q, K, generator=g)
    return x, w, b, dy


@pytest.mark.gpu
@pytest.mark.parametrize("C,K", [(3, 5), (1, 32), (16, 70)])
@pytest.mark.parametrize("name", list(GEOMS))
def test_conv2d_f32_elementwise(name, C, K):
    """y, dx, dW, db of the fp32 conv op against ``reference.conv2d`` on doubles, for the four
    bias / ReLU combinations (no bias + no ReLU: the ``return dy, None`` shortcut; bias without
    ReLU: the backward kernel runs in place on dy, which must come back unchanged)."""
    R, S, stride, padding = GEOMS[name][2:]
    x, w, b, dy = _conv_inputs(name, C, K)
    M = dy.numel() // K
    for bias, relu in itertools.product((False, True), repeat=2):
        what = f"conv {name} C={C} K={K} bias={bias} relu={relu}"
        xg, wg = x.cuda().requires_grad_(), w.cuda().requires_grad_()
        bg = b.cuda().requires_grad_() if bias else None
        dyg = dy.cuda()
        if not bias and not relu:
            y = _nf().conv2d(xg, wg, stride, padding)
        else:
            y = _nf().conv2d_bias_relu(xg, wg, bg, stride, padding, relu)
        y.backward(dyg)
        torch.cuda.synchronize()
        ref = _conv_reference(x, w, b if bias else None, dy, stride, padding, relu, y)
        assert torch.equal(dyg.cpu(), dy), f"{what}: backward changed dy"
        assert_within_fma_bound(y, ref["y"], ref["mag_y"], R * S * C + 4, what + " y")
        assert_within_fma_bound(xg.grad, ref["dx"], ref["mag_dx"], K + R * S, what + " dx")
        assert_within_fma_bound(wg.grad, ref["dw"], ref["mag_dw"], M + 4, what + " dW")
        if bias:
            assert_within_fma_bound(bg.grad, ref["db"], ref["mag_db"], M + 4, what + " db")


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
def test_conv2d_f32_direct_gradient_split_k(relu):
    """The path every training step takes: dW / db accumulated by the kernels straight into a
    non-zero flat fp32 gradient (``_dtf_flat``), dW through split-K."""
    n, H, C, K = 2, 32, 3, 5
    assert _K().gemm_f32_splits(K, 9 * C, n * H * H) > 1
    g = _gen(40)
    x = torch.randn(n, H, H, C, generator=g)
    w = torch.randn(K, 3, 3, C, generator=g) / (9 * C) ** 0.5
    b = torch.randn(K, generator=g)
    dy = torch.randn(n, H, H, K, generator=g)
    w0, b0 = torch.randn(w.shape, generator=g), torch.randn(b.shape, generator=g)
    xg, wg, bg = (t.cuda().requires_grad_() for t in (x, w, b))
    wg.grad, bg.grad = w0.cuda(), b0.cuda()
    wg._dtf_flat = bg._dtf_flat = True
    gw, gb = wg.grad, bg.grad
    y = _nf().conv2d_bias_relu(xg, wg, bg, 1, "same", relu)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert wg.grad is gw and bg.grad is gb
    ref = _conv_reference(x, w, b, dy, 1, "same", relu, y)
    M = n * H * H
    assert_within_fma_bound(y, ref["y"], ref["mag_y"], 9 * C + 4, "y")
    assert_within_fma_bound(gw, ref["dw"] + w0.double(), ref["mag_dw"] + w0.double().abs(), M + 4,
                            "direct dW")
    assert_within_fma_bound(gb, ref["db"] + b0.double(), ref["mag_db"] + b0.double().abs(), M + 4,
                            "direct db")
    assert_within_fma_bound(xg.grad, ref["dx"], ref["mag_dx"], K + 9, "dx")


@pytest.mark.gpu
def test_im2col_f32_more_than_one_grid_trip():
    n, H, C, R = 108, 14, 32, 5
    total = n * H * H * R * R * C
    assert total > TRIP
    g = torch.Generator(device="cuda").manual_seed(50)
    x = torch.randn(n, H, H, C, device="cuda", generator=g)
    cols = torch.full((n * H * H, R * R * C), NAN, device="cuda")
    _K().im2col_f32(x.data_ptr(), cols.data_ptr(), n, H, H, C, H, H, 1, 1, R, R, 2, 2, _st())
    u = F.unfold(x.permute(0, 3, 1, 2), (R, R), padding=2)            # [n, C * 25, H * H]
    ref = u.view(n, C, R, R, H * H).permute(0, 4, 2, 3, 1).reshape(n * H * H, R * R * C)
    assert torch.equal(cols, ref)


@pytest.mark.gpu
def test_col2im_f32_more_than_one_grid_trip():
    """2x2 stride 2 VALID: every pixel has exactly one tap, so dx is a permutation of dcols."""
    n, H, C = 4, 64, 1025
    assert n * H * H * C > TRIP
    P = H // 2
    g = torch.Generator(device="cuda").manual_seed(51)
    dcols = torch.randn(n * P * P, 4 * C, device="cuda", generator=g)
    dx = torch.full((n, H, H, C), NAN, device="cuda")
    _K().col2im_f32(dcols.data_ptr(), dx.data_ptr(), n, H, H, C, P, P, 2, 2, 2, 2, 0, 0, _st())
    ref = dcols.view(n, P, P, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(n, H, H, C)
    assert torch.equal(dx, ref)


# ----------------------------------------------------------------------------- 3. max-pool
def _pool_reference(x, k, s, dy):
    """F.max_pool2d on doubles: (y, arg = window index i * k + j of the max, dx)."""
    n, H, W, c = x.shape
    xr = x.double().permute(0, 3, 1, 2).requires_grad_()
    y, idx = F.max_pool2d(xr, k, s, return_indices=True)
    P, Q = y.shape[2], y.shape[3]
    h, w = idx // W, idx % W
    i = h - torch.arange(P).view(1, 1, P, 1) * s
    j = w - torch.arange(Q).view(1, 1, 1, Q) * s
    assert bool(((i >= 0) & (i < k) & (j >= 0) & (j < k)).all())
    arg = (i * k + j).permute(0, 2, 3, 1).to(torch.uint8)
    (dx,) = torch.autograd.grad(y, xr, dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), arg, dx.permute(0, 2, 3, 1)


def _pool_direct(x, k, s, dy):
    """The two pool kernels through the binding, every output pre-filled with a sentinel."""
    n, H, W, c = x.shape
    P, Q = (H - k) // s + 1, (W - k) // s + 1
    xg, dyg = x.cuda(), dy.cuda()
    y = torch.full((n, P, Q, c), NAN, device="cuda")
    arg = torch.full((n, P, Q, c), 0xFF, device="cuda", dtype=torch.uint8)
    dx = torch.full((n, H, W, c), NAN, device="cuda")
    _K().maxpool_f32_fwd(xg.data_ptr(), y.data_ptr(), arg.data_ptr(), n, H, W, c, P, Q, k, s,
                         _st())
    _K().maxpool_f32_bwd(dyg.data_ptr(), arg.data_ptr(), dx.data_ptr(), n, H, W, c, P, Q, k, s,
                         _st())
    torch.cuda.synchronize()
    return y.cpu(), arg.cpu(), dx.cpu()


def _pool_check(x, k, s, dy, what):
    yr, ar, dxr = _pool_reference(x, k, s, dy)
    y, arg, dx = _pool_direct(x, k, s, dy)
    assert bool((arg < k * k).all()), f"{what}: arg not written everywhere"
    assert torch.equal(y.double(), yr), f"{what}: y"
    assert torch.equal(arg, ar), f"{what}: arg"
    assert torch.equal(dx.double(), dxr), f"{what}: dx"
    # pixels in a dropped edge row / column or in the gaps of s > k: exactly zero
    n, H, W, c = x.shape
    P, Q = y.shape[1], y.shape[2]
    hh, ww = torch.arange(H), torch.arange(W)
    inh = (hh // s < P) & (hh % s < k)
    inw = (ww // s < Q) & (ww % s < k)
    covered = (inh.view(H, 1) & inw.view(1, W)).view(1, H, W, 1).expand_as(dx)
    assert bool((dx[~covered] == 0).all()), f"{what}: gradient outside every window"
    # and the op (autograd.Function) gives the same
    xg = x.cuda().requires_grad_()
    yo = _nf().max_pool2d(xg, k, s)
    yo.backward(dy.cuda())
    assert torch.equal(yo.detach().cpu(), y) and torch.equal(xg.grad.cpu(), dx), f"{what}: op"


POOL_CASES = [(k, s, hw) for (k, s) in [(2, 2), (2, 3), (1, 2)]
              for hw in [(7, 9), (8, 8), (5, 11)]] + [(3, 3, (7, 9))]


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 33])
@pytest.mark.parametrize("k,s,hw", POOL_CASES)
def test_max_pool_f32(k, s, hw, C):
    H, W = hw
    g = _gen(60 + k * 7 + s + H + C)
    x = torch.randn(2, H, W, C, generator=g)
    P, Q = (H - k) // s + 1, (W - k) // s + 1
    dy = torch.randn(2, P, Q, C, generator=g)
    _pool_check(x, k, s, dy, f"pool k={k} s={s} {H}x{W} C={C}")


@pytest.mark.gpu
@pytest.mark.parametrize("k,s", [(2, 2), (3, 3)])
def test_max_pool_f32_ties_and_infinities(k, s):
    g = _gen(70 + k)
    H, W, C = 7, 9, 33
    P, Q = (H - k) // s + 1, (W - k) // s + 1
    dy = torch.randn(2, P, Q, C, generator=g)
    # constant input: every window's first element wins
    const = torch.full((2, H, W, C), 1.5)
    y, arg, dx = _pool_direct(const, k, s, dy)
    assert bool((arg == 0).all()) and bool((y == 1.5).all())
    first = torch.zeros(2, H, W, C)
    first[:, 0:P * s:s, 0:Q * s:s, :] = dy
    assert torch.equal(dx, first)
    # mixed ties (few distinct values) against torch
    mixed = torch.randint(0, 3, (2, H, W, C), generator=g).float()
    _pool_check(mixed, k, s, dy, f"pool ties k={k}")
    # infinities: a window of -inf only, -inf beside finite values, +inf in a window
    x = torch.randn(2, H, W, C, generator=g)
    x[0, 0:k, 0:k, :] = float("-inf")
    x[0, s, s, :] = float("-inf")
    x[1, s + k - 1, k - 1, :] = float("inf")
    x[1, 0, s:s + k, 0] = float("-inf")
    _pool_check(x, k, s, dy, f"pool inf k={k}")


@pytest.mark.gpu
def test_max_pool_f32_rejects_overlapping_windows():
    x = torch.zeros(1, 8, 8, 4, device="cuda")
    with pytest.raises(ValueError, match="non-overlapping"):
        _nf().max_pool2d(x, 3, 2)
    y = torch.full((1, 3, 3, 4), SENTINEL, device="cuda")
    arg = torch.zeros(1, 3, 3, 4, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="overlapping"):
        _K().maxpool_f32_fwd(x.data_ptr(), y.data_ptr(), arg.data_ptr(), 1, 8, 8, 4, 3, 3, 3, 2,
                             _st())
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


@pytest.mark.gpu
def test_max_pool_f32_fwd_more_than_one_grid_trip():
    n, H, C = 4, 128, 1025                                   # input: 4 x the outputs, 269 MB
    P = H // 2
    assert n * P * P * C > TRIP
    g = torch.Generator(device="cuda").manual_seed(80)
    x = torch.randn(n, H, H, C, device="cuda", generator=g)
    y = torch.full((n, P, P, C), NAN, device="cuda")
    arg = torch.full((n, P, P, C), 0xFF, device="cuda", dtype=torch.uint8)
    _K().maxpool_f32_fwd(x.data_ptr(), y.data_ptr(), arg.data_ptr(), n, H, H, C, P, P, 2, 2, _st())
    assert torch.equal(y, x.view(n, P, 2, P, 2, C).amax(dim=(2, 4)))
    assert bool((arg < 4).all())
    win = x.view(n, P, 2, P, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(n, P, P, C, 4)
    del x
    assert torch.equal(win.gather(-1, arg.long().unsqueeze(-1)).squeeze(-1), y)


@pytest.mark.gpu
def test_max_pool_f32_bwd_more_than_one_grid_trip():
    n, H, C = 4, 64, 1025
    P = H // 2
    assert n * H * H * C > TRIP
    g = torch.Generator(device="cuda").manual_seed(81)
    dy = torch.randn(n, P, P, C, device="cuda", generator=g)
    arg = torch.randint(0, 4, (n, P, P, C), device="cuda", generator=g, dtype=torch.uint8)
    dx = torch.full((n, H, H, C), NAN, device="cuda")
    _K().maxpool_f32_bwd(dy.data_ptr(), arg.data_ptr(), dx.data_ptr(), n, H, H, C, P, P, 2, 2,
                         _st())
    win = torch.zeros(n, P, P, C, 4, device="cuda")
    win.scatter_(-1, arg.long().unsqueeze(-1), dy.unsqueeze(-1))
    ref = win.view(n, P, P, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, H, H, C)
    assert torch.equal(dx, ref)


# ----------------------------------------------------------------------------- 4. bias_relu_bwd
def _bias_relu_bwd(dy, y, relu, db0=None, want_db=True, inplace=False):
    """One call through the binding; returns (dz, db) on the CPU.  The workspace has exactly the
    floats the kernel asks for, followed by a sentinel tail that must stay untouched."""
    T, N = dy.shape
    need = _K().bias_relu_bwd_f32_ws_floats(N)
    ws = torch.full((need + 1024,), NAN, device="cuda")
    dyg = dy.cuda()
    dz = dyg if inplace else torch.full((T, N), NAN, device="cuda")
    db = None
    if want_db:
        db = db0.cuda() if db0 is not None else torch.full((N,), NAN, device="cuda")
    yg = y.cuda() if relu else dyg
    _K().bias_relu_bwd_f32(dyg.data_ptr(), yg.data_ptr(), dz.data_ptr(), T, N, ws.data_ptr(),
                           0 if db is None else db.data_ptr(), int(db0 is not None), int(relu),
                           _st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[need:]).all()), "wrote past the workspace"
    if not inplace:
        assert torch.equal(dyg.cpu(), dy)
    return dz.cpu(), None if db is None else db.cpu()


def _relu_outputs(T, N, g):
    """A forward output with +0.0, -0.0, the smallest subnormal and normal positives, and
    ordinary values of both signs: the mask is y > 0."""
    pool = torch.tensor([0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 1.0, 3.5, -1.0, -2.0 ** -126])
    return pool[torch.randint(0, len(pool), (T, N), generator=g)]


BRB_SHAPES = [(1, 1), (3, 65), (33, 64), (31, 130), (8200, 10)]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("T,N", BRB_SHAPES)
def test_bias_relu_bwd_f32(T, N, relu):
    """(8200, 10): 256 slices of 33 rows, the last of which start past T."""
    g = _gen(90 + T + N)
    y = _relu_outputs(T, N, g)
    mask = (y > 0).double() if relu else torch.ones(T, N, dtype=torch.float64)
    # exact: integer dy, column sums exact in any order
    dy = _vals((T, N), g, True)
    ref_dz = dy.double() * mask
    dz, db = _bias_relu_bwd(dy, y, relu)
    assert_exact(dz, ref_dz, "dz")
    assert_exact(db, ref_dz.sum(0), "db")
    db0 = _vals((N,), g, True) * 7
    dz, db = _bias_relu_bwd(dy, y, relu, db0=db0)
    assert_exact(dz, ref_dz, "dz (accumulate)")
    assert_exact(db, ref_dz.sum(0) + db0.double(), "db (accumulate)")
    dz, db = _bias_relu_bwd(dy, y, relu, want_db=False)
    assert_exact(dz, ref_dz, "dz (db = None)")
    if not relu:
        dz, db = _bias_relu_bwd(dy, y, relu, inplace=True)
        assert_exact(dz, ref_dz, "dz (in place)")
        assert_exact(db, ref_dz.sum(0), "db (in place)")
    # bound: randn dy, T terms per column
    dy = _vals((T, N), g, False)
    db0 = _vals((N,), g, False)
    ref_dz = dy.double() * mask
    dz, db = _bias_relu_bwd(dy, y, relu, db0=db0)
    assert_exact(dz, ref_dz, "dz (randn)")
    assert_within_fma_bound(db, ref_dz.sum(0) + db0.double(),
                            ref_dz.abs().sum(0) + db0.double().abs(), T + 1, "db (randn)")


# ----------------------------------------------------------------------------- 5. clipped xent
XENT_B = 40


def _xent_inputs(V, seed):
    """z = randn; in every second row one logit sits 35 below the row's maximum, so its
    probability (< 1e-13) is clipped and every other one (> 1e-7) is not."""
    g = _gen(seed)
    z = torch.randn(XENT_B, V, generator=g)
    cls = torch.randint(0, V, (XENT_B,), generator=g)
    clipped = torch.zeros(XENT_B, V, dtype=torch.bool)
    for r in range(0, XENT_B, 2):
        others = z[r].clone()
        others[cls[r]] = float("-inf")
        z[r, cls[r]] = others.max() - 35
        clipped[r, cls[r]] = True
    return z, cls, clipped, g


def _xent_targets(kind, V, cls, clipped, g):
    if kind == "soft":
        return torch.softmax(torch.randn(XENT_B, V, generator=g), -1)
    other = (cls + 1 + torch.randint(0, V - 1, (XENT_B,), generator=g)) % V
    hot = torch.where(clipped.any(1), cls if kind == "onehot_clipped" else other, other)
    return F.one_hot(hot, V).float()


def _xent_reference(z, t):
    zr = z.double().requires_grad_()
    y = torch.softmax(zr, -1)
    rows = -(t.double() * torch.log(y.clamp(1e-10, 1.0))).sum(-1)
    rows.sum().backward()
    return y.detach(), rows.detach(), zr.grad


def _xent_margin(y, clipped):
    """No entry near the clip: fast-exp error cannot move one across it."""
    assert bool(((y > 1e-7) | (y < 1e-13)).all())
    assert torch.equal(y < 1e-10, clipped)


@pytest.mark.parametrize("V", [10, 64, 65, 130, 1000])
def test_clipped_xent_inputs_keep_their_margin(V):
    z, cls, clipped, g = _xent_inputs(V, 100 + V)
    _xent_margin(torch.softmax(z.double(), -1), clipped)
    assert int(clipped.sum()) == XENT_B // 2


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["onehot_clipped", "onehot_other", "soft"])
@pytest.mark.parametrize("V", [10, 64, 65, 130, 1000])
def test_clipped_xent_f32_with_the_clip_active(V, kind):
    """Per row: loss within 1e-4 relative, gradient within 1e-5 norm-relative of fp64 (the
    project's tolerances, applied to every row on its own); a row whose one-hot target sits on
    the clipped class has loss -log(1e-10) and a gradient of exactly zero."""
    z, cls, clipped, g = _xent_inputs(V, 100 + V)
    t = _xent_targets(kind, V, cls, clipped, g)
    y, rows_ref, dz_ref = _xent_reference(z, t)
    _xent_margin(y, clipped)
    zg, tg = z.cuda(), t.cuda()
    rows = torch.full((XENT_B,), NAN, device="cuda")
    dz = torch.full((XENT_B, V), NAN, device="cuda")
    _K().clipped_xent(zg.data_ptr(), tg.data_ptr(), XENT_B, V, rows.data_ptr(), dz.data_ptr(),
                      1.0, _st())
    torch.cuda.synchronize()
    rows, dz = rows.cpu().double(), dz.cpu().double()
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(dz).all())
    loss_rel = (rows - rows_ref).abs() / rows_ref.abs()
    zero = dz_ref.abs().amax(1) == 0
    grad_rel = (dz - dz_ref).norm(dim=1) / dz_ref.norm(dim=1).clamp_min(1e-300)
    print(f"clipped_xent V={V} {kind}: worst row loss rel {float(loss_rel.max()):.3e}, worst row "
          f"grad rel {float(grad_rel[~zero].max()) if bool((~zero).any()) else 0.0:.3e}, "
          f"{int(zero.sum())} all-zero rows")
    if kind == "onehot_clipped":
        assert torch.equal(zero, clipped.any(1))
        assert bool(((rows_ref[zero] - 23.025850929940457).abs() < 1e-12).all())
    else:
        assert not bool(zero.any())
    assert bool((dz[zero] == 0).all())
    assert bool((loss_rel < 1e-4).all()), (int(loss_rel.argmax()), float(loss_rel.max()))
    assert bool((grad_rel[~zero] < 1e-5).all()), (int(grad_rel.argmax()), float(grad_rel.max()))
    # scale: dz scales (exactly, by a power of two), the row loss does not
    rows_q = torch.full((XENT_B,), NAN, device="cuda")
    dz_q = torch.full((XENT_B, V), NAN, device="cuda")
    _K().clipped_xent(zg.data_ptr(), tg.data_ptr(), XENT_B, V, rows_q.data_ptr(), dz_q.data_ptr(),
                      0.25, _st())
    torch.cuda.synchronize()
    assert torch.equal(rows_q.cpu().double(), rows)
    assert torch.equal(dz_q.cpu().double(), 0.25 * dz)
    # the op: batch sum, and an upstream gradient of 3
    zo = zg.clone().requires_grad_()
    loss = _nf().softmax_cross_entropy_clipped_sum(zo, tg)
    (loss * 3).backward()
    assert abs(float(loss.detach()) - float(rows_ref.sum())) < 1e-4 * abs(float(rows_ref.sum()))
    assert torch.equal(zo.grad.cpu().double(), (dz.float() * 3).double())


# ----------------------------------------------------------------------------- 6. dense op
def _dense_reference(x, w, b, dy, relu, layout, y_got=None):
    """fp64 dense forward and gradients with their magnitudes; ``y_got`` as for the conv."""
    i = x.shape[-1]
    x2, dy2 = x.double().reshape(-1, i), dy.double().reshape(-1, dy.shape[-1])
    xr, wr = x2.clone().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if b is not None else None
    wt = (lambda t: t.t()) if layout == "OI" else (lambda t: t)
    wa = w.double().abs()
    mag_y = x2.abs() @ wt(wa) + (b.double().abs() if b is not None else 0)
    z = xr @ wt(wr)
    if br is not None:
        z = z + br
    mask = _relu_mask(z.detach(), mag_y, i + 4, y_got) if relu else torch.ones_like(z)
    y = z * mask
    y.backward(dy2)
    dz = dy2 * mask
    mag_dw = dz.abs().t() @ x2.abs()
    return dict(y=y.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if br is not None else None,
                mag_y=mag_y, mag_dx=dz.abs() @ wt(wa).t(),
                mag_dw=mag_dw if layout == "OI" else mag_dw.t(), mag_db=dz.abs().sum(0))


def _dense_inputs(mshape, i, o, layout, seed=0):
    g = _gen(seed * 7919 + 7 * i + o + sum(mshape))
    x = torch.randn(*mshape, i, generator=g)
    w = torch.randn(*((o, i) if layout == "OI" else (i, o)), generator=g) / i ** 0.5
    b = torch.randn(o, generator=g)
    dy = torch.randn(*mshape, o, generator=g)
    return x, w, b, dy, g


@pytest.mark.gpu
@pytest.mark.parametrize("i", [17, 784])
@pytest.mark.parametrize("o", [1, 10, 100])
@pytest.mark.parametrize("mshape", [(1,), (65,), (4, 33)], ids=["M1", "M65", "M4x33"])
@pytest.mark.parametrize("layout", ["OI", "IO"])
def test_dense_f32_elementwise(layout, mshape, o, i):
    x, w, b, dy, _ = _dense_inputs(mshape, i, o, layout)
    M = dy.numel() // o
    for bias, relu in itertools.product((False, True), repeat=2):
        what = f"dense {layout} M={mshape} i={i} o={o} bias={bias} relu={relu}"
        xg, wg = x.cuda().requires_grad_(), w.cuda().requires_grad_()
        bg = b.cuda().requires_grad_() if bias else None
        y = _nf().dense(xg, wg, bg, relu, layout)
        assert y.shape == (*mshape, o)
        y.backward(dy.cuda())
        torch.cuda.synchronize()
        ref = _dense_reference(x, w, b if bias else None, dy, relu, layout, y)
        assert_within_fma_bound(y.reshape(M, o), ref["y"], ref["mag_y"], i + 4, what + " y")
        assert_within_fma_bound(xg.grad.reshape(M, i), ref["dx"], ref["mag_dx"], o + 4,
                                what + " dx")
        assert_within_fma_bound(wg.grad, ref["dw"], ref["mag_dw"], M + 4, what + " dW")
        if bias:
            assert_within_fma_bound(bg.grad, ref["db"], ref["mag_db"], M + 4, what + " db")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["OI", "IO"])
def test_dense_f32_direct_gradient_split_k(layout):
    """dW accumulated straight into a non-zero flat gradient through split-K; for ``IO`` the
    GEMM's C is column-major."""
    M, i, o = 4096, 40, 10
    assert _K().gemm_f32_splits(o, i, M) > 1
    x, w, b, dy, g = _dense_inputs((M,), i, o, layout, seed=1)
    w0, b0 = torch.randn(w.shape, generator=g), torch.randn(b.shape, generator=g)
    xg, wg, bg = (t.cuda().requires_grad_() for t in (x, w, b))
    wg.grad, bg.grad = w0.cuda(), b0.cuda()
    wg._dtf_flat = bg._dtf_flat = True
    gw, gb = wg.grad, bg.grad
    y = _nf().dense(xg, wg, bg, True, layout)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert wg.grad is gw and bg.grad is gb
    ref = _dense_reference(x, w, b, dy, True, layout, y)
    assert_within_fma_bound(y, ref["y"], ref["mag_y"], i + 4, "y")
    assert_within_fma_bound(gw, ref["dw"] + w0.double(), ref["mag_dw"] + w0.double().abs(), M + 4,
                            "direct dW")
    assert_within_fma_bound(gb, ref["db"] + b0.double(), ref["mag_db"] + b0.double().abs(), M + 4,
                            "direct db")
    assert_within_fma_bound(xg.grad, ref["dx"], ref["mag_dx"], o + 4, "dx")


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["transposed", "column_slice"])
@pytest.mark.parametrize("layout", ["OI", "IO"])
def test_dense_f32_non_contiguous_weight(layout, view):
    """A weight that is a ``.t()`` view or a column slice of a larger parameter gives bit for bit
    what its contiguous copy gives, and the gradient reaches the parameter behind the view."""
    M, i, o = 65, 17, 10
    x, w, b, dy, g = _dense_inputs((M,), i, o, layout, seed=2)
    r, c = w.shape
    if view == "transposed":
        base = w.t().contiguous().cuda().requires_grad_()
        wv = base.t()
    else:
        big = torch.randn(r, c + 5, generator=g)
        big[:, 2:c + 2] = w
        base = big.cuda().requires_grad_()
        wv = base[:, 2:c + 2]
    assert not wv.is_contiguous() and torch.equal(wv.detach().cpu(), w)
    outs = []
    for wt in (w.cuda().requires_grad_(), wv):
        xg, bg = x.cuda().requires_grad_(), b.cuda().requires_grad_()
        y = _nf().dense(xg, wt, bg, True, layout)
        y.backward(dy.cuda())
        outs.append((y.detach(), xg.grad, bg.grad))
        if wt is not wv:
            dw = wt.grad
    for got, want in zip(outs[1], outs[0]):
        assert torch.equal(got, want)
    assert base.grad is not None
    if view == "transposed":
        assert torch.equal(base.grad.t(), dw)
    else:
        assert torch.equal(base.grad[:, 2:c + 2], dw)
        assert bool((base.grad[:, :2] == 0).all()) and bool((base.grad[:, c + 2:] == 0).all())
    ref = _dense_reference(x, w, b, dy, True, layout, outs[1][0])
    assert_within_fma_bound(outs[1][0], ref["y"], ref["mag_y"], i + 4, "y")
    assert_within_fma_bound(dw, ref["dw"], ref["mag_dw"], M + 4, "dW")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16])
def test_f32_ops_reject_a_bias_of_another_dtype(dtype):
    """A bias that is not fp32 would be read as raw fp32 bits: dense and conv refuse it, as they
    refuse a non-fp32 input or weight."""
    x = torch.randn(4, 17, device="cuda")
    w = torch.randn(10, 17, device="cuda")
    b = torch.randn(10, device="cuda").to(dtype)
    with pytest.raises(TypeError, match="fp32"):
        _nf().dense(x, w, b)
    with pytest.raises(TypeError, match="fp32"):
        _nf().dense(x, w.t().contiguous(), b, True, "IO")
    xc = torch.randn(2, 6, 6, 3, device="cuda")
    wc = torch.randn(10, 3, 3, 3, device="cuda")
    with pytest.raises(TypeError, match="fp32"):
        _nf().conv2d_bias_relu(xc, wc, b, 1, "same", True)
    with pytest.raises(TypeError, match="fp32"):
        _nf().conv2d_bias_relu(xc, wc, torch.randn(10), 1, "same", False)      # a CPU bias
