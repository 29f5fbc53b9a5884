"""The persistent GEMM's implicit-GEMM conv form (csrc/kernels/gemm.hip gemm_pp2_kernel<1, *>)
issues its A pieces from carried state: a (tap, channel block) cursor per look-ahead distance,
stepped once per K-step, and per-row corner offsets / validity bits computed once per tile for the
current and the next tile.  The shapes here are the smallest at which that path can go wrong: the
tap changing every K-step (C = 64), a channel-block count that is no power of two, tiles ending
inside an image, partial last tiles, blocks that walk several tiles (current / next sets swap,
the cursor wraps into the next tile, the last "next" tile is invalid), the 1- / 2- / 4-tap tables
of the strided data-gradient phase classes and the one-tap strided projection.

Every case is compared bit for bit with the same call on the register / halo kernels
(conv_set_gemm(0)) and per element with an fp64 CPU reference on the bf16-rounded operands."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from distributedtensorflow_amd.ops import native  # noqa: E402

# N, H, W, C, K_out of the stride-1 pad-1 3x3 cases
ONE_PARTIAL_TILE = (3, 7, 7, 64, 256)
TILES_WITH_TAIL = (5, 14, 14, 128, 256)
CB_THREE = (7, 5, 9, 192, 320)
MANY_TILES = (1004, 14, 14, 64, 256)
SMALL = [ONE_PARTIAL_TILE, TILES_WITH_TAIL, CB_THREE]


def _assert_close64(got, ref):
    torch.testing.assert_close(got.double().cpu(), ref, rtol=1e-2, atol=1e-2)


@functools.lru_cache(maxsize=None)
def _fwd_case(N, H, W, C, K):
    """Operands of a 3x3 forward case and its fp64 CPU reference (computed once, never written)."""
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + C)
    x = torch.randn(N, H, W, C, device="cuda", generator=g).bfloat16()
    w = (torch.randn(K, 3, 3, C, device="cuda", generator=g) / (9 * C) ** 0.5).bfloat16()
    ref = torch.nn.functional.conv2d(x.double().cpu().permute(0, 3, 1, 2),
                                     w.double().cpu().permute(0, 3, 1, 2), padding=1)
    return x, w, ref.permute(0, 2, 3, 1).contiguous()


def _forward(x, w, stride, pad, gemm, stats):
    """conv2d_forward on the GEMM route (the default) or the register / halo kernels; with
    stats also the BatchNorm sums [2][K] of its statistics slab."""
    N, H, W, C = x.shape
    K, R = w.shape[0], w.shape[1]
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    taps = [(r - pad, s - pad) for r in range(R) for s in range(R)]
    geom = native._fwd_geom(x.shape, K, taps, P, Q, stride, stride, P, Q)
    try:
        native._K.conv_set_gemm(1 if gemm else 0)
        rows = native._K.conv_tile_rows(geom, [t[0] for t in taps], [t[1] for t in taps], 0)
        if gemm:
            assert native._K.gemm_get_pp2() & 2               # the persistent kernel takes convs
            assert rows == (N * P * Q + 255) // 256           # ... and this one is on the GEMM
        ws = torch.zeros(native._K.bn_workspace_floats_g(rows, K), device="cuda") if stats else None
        y = native.conv2d_forward(x, w, stride, pad, stats=ws)
        torch.cuda.synchronize()
    finally:
        native._K.conv_set_gemm(1)
    return y, (ws[: rows * 2 * K].view(rows, 2, K).sum(0) if stats else None)


def _check_forward(x, w, ref, stride, pad, stats):
    yg, sg = _forward(x, w, stride, pad, True, stats)
    yr, _ = _forward(x, w, stride, pad, False, stats)
    assert torch.equal(yg, yr)
    _assert_close64(yg, ref)
    if stats:      # the slab holds the sums of the bf16 outputs (tests/test_conv_r6_gpu.py's bounds)
        yf = yg.float()
        torch.testing.assert_close(sg[0], yf.sum((0, 1, 2)), rtol=1e-3, atol=1.0)
        torch.testing.assert_close(sg[1], (yf * yf).sum((0, 1, 2)), rtol=1e-3, atol=1.0)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("case", SMALL + [MANY_TILES], ids=["one_partial_tile", "tiles_with_tail",
                                                          "cb3", "many_tiles"])
def test_conv3x3_forward_on_the_persistent_gemm(case, stats):
    x, w, ref = _fwd_case(*case)
    _check_forward(x, w, ref, 1, 1, stats)


@functools.lru_cache(maxsize=None)
def _dgrad_case(N, H, W, C, K, R, stride):
    """dy [N, H/stride, W/stride, K], filter [K, R, R, C], an accumulate base and the fp64 CPU
    data gradient of shape [N, H, W, C]."""
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + C + R)
    pad = R // 2
    dy = torch.randn(N, H // stride, W // stride, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(K, R, R, C, device="cuda", generator=g) / (R * R * K) ** 0.5).bfloat16()
    base = torch.randn(N, H, W, C, device="cuda", generator=g).bfloat16()
    ref = torch.nn.grad.conv2d_input((N, C, H, W), w.double().cpu().permute(0, 3, 1, 2),
                                     dy.double().cpu().permute(0, 3, 1, 2), stride=stride,
                                     padding=pad)
    return dy, w, base, ref.permute(0, 2, 3, 1).contiguous()


def _dgrad(dy, w, base, shape, stride, acc, gemm=1, pp2_strided=1):
    try:
        native._K.conv_set_gemm(gemm)
        native._K.gemm_set_pp2_strided(pp2_strided)
        out = base.clone() if acc else None
        dx = native.conv2d_dgrad(dy, w, shape, stride, w.shape[1] // 2, out=out).clone()
        torch.cuda.synchronize()
    finally:
        native._K.conv_set_gemm(1)
        native._K.gemm_set_pp2_strided(1)
    return dx


@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
@pytest.mark.parametrize("case", SMALL, ids=["one_partial_tile", "tiles_with_tail", "cb3"])
def test_conv3x3_dgrad_on_the_persistent_gemm(case, acc):
    """The stride-1 data gradient of the same geometry with the channel roles swapped (its GEMM
    reduces over 9 x C and writes K_out >= 256 columns): the mirrored tap table, plain and with
    the accumulate epilogue."""
    N, H, W, C, K = case
    dy, w, base, ref = _dgrad_case(N, H, W, K, C, 3, 1)     # dy has C channels, dx K_out
    dg = _dgrad(dy, w, base, (N, H, W, K), 1, acc)
    dr = _dgrad(dy, w, base, (N, H, W, K), 1, acc, gemm=0)
    assert torch.equal(dg, dr)
    _assert_close64(dg, ref + base.double().cpu() if acc else ref)


@pytest.mark.parametrize("acc", [False, True], ids=["plain", "acc"])
def test_strided_dgrad_phase_classes_on_the_persistent_gemm(acc):
    """Stride-2 3x3 data gradient, N=2, 28x28, C=256, K=256: the four phase classes carry 1-,
    2- and 4-tap tables with their own offsets; plain and with the accumulate epilogue.  Bit for
    bit against the round-5 ping-pong kernel and against the register kernels."""
    N, H, C, K = 2, 28, 256, 256
    dy, w, base, ref = _dgrad_case(N, H, H, C, K, 3, 2)
    dg = _dgrad(dy, w, base, (N, H, H, C), 2, acc)
    dp = _dgrad(dy, w, base, (N, H, H, C), 2, acc, pp2_strided=0)
    dr = _dgrad(dy, w, base, (N, H, H, C), 2, acc, gemm=0)
    assert torch.equal(dg, dp)
    assert torch.equal(dg, dr)
    _assert_close64(dg, ref + base.double().cpu() if acc else ref)


def test_projection_shortcut_one_tap_strided_rows():
    """1x1 stride-2 forward, N=3, 28x28, C=128, K_out=256: one tap, strided input rows."""
    N, H, C, K = 3, 28, 128, 256
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(N, H, H, C, device="cuda", generator=g).bfloat16()
    w = (torch.randn(K, 1, 1, C, device="cuda", generator=g) / C ** 0.5).bfloat16()
    ref = torch.nn.functional.conv2d(x.double().cpu().permute(0, 3, 1, 2),
                                     w.double().cpu().permute(0, 3, 1, 2), stride=2)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    for stats in (False, True):
        _check_forward(x, w, ref, 2, 0, stats)
