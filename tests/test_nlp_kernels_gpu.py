"""The transformer kernels of ``csrc/kernels/nlp.hip`` element by element against fp64, at the
shapes, modes and rows where they can go wrong.  The kernels are called through ``native._K``
with explicit seeds on CPU-made data; every ``*_set_*`` switch is restored in ``finally``.

Method
------
*Stage-wise references.*  Every output is compared with the fp64 value of the same function of
what that stage READS: the LayerNorm statistics and ``y`` are functions of the kernel's own
stored ``s``, the attention backward of the stored bf16 ``O`` and fp32 ``lse``.  Each bound then
covers the roundings of one stage only.

*Bound mode.*  Per element ``|got - ref64| <= k u |.| + fp32 term`` with ``u = 2^-8`` (bf16),
``u32 = 2^-24``, ``gamma(n) = n u32 / (1 - n u32)`` and ``k`` the number of bf16 roundings on
the output's path.  Intrinsics (``exp2f``, ``__expf``, ``rsqrtf``, ``rcp``) that feed a bf16
output get 16 u32 (``INTR``), a condition: 2^-12 of ``u``.  Line numbers are those of nlp.hip.

  LayerNorm forward (ln_fwd_kernel 84-164, ln_fwd_wide_kernel 274-355)
    s      k = 1 (round_bf, l.121/313).  fp32: a + bias, * inv_keep, + res: gamma(3) of
           |a| + |bias| (scaled) + |res|; embedding mode w + p + t: gamma(2).
    mean   fp32 sum of H stored values in any order times fl(1/H) (l.123-132): gamma(H + 2) of
           mean|s|.  No intrinsic: derived, not measured.
    rstd   rsqrtf(var + eps) (l.142).  var is a sum of H squares of d = s - mean, each d with one
           rounding, plus the error D of the fp32 mean squared: relative
           gamma(H + 6) + D^2 / (var + eps), halved by the square root, plus the rsqrtf allowance
           ``ALLOW['rstd']`` (measured, below).
    y      k = 1 (store4 l.158).  fp32 (l.153): (|xhat g| + |beta|) (gamma(H + 8) +
           ALLOW['rstd'] u32) + D rstd |g| + D^2 / (2 (var + eps)) |xhat g|, all times inv_keep
           under the post-dropout.
  LayerNorm backward (ln_bwd_kernel 183-259, ln_bwd_wide_kernel 358-434, col_sum 448-518)
    ds,da  k = 1 each (both are rounded from the fp32 dx, l.240-241).  fp32: gamma(H + 10) of
           rstd (|gy| + mean|gy| + |xhat| mean|gy xhat|) (l.216-230).
    dgamma fp32 sum over M rows of dy' xhat: gamma(M + 6) of sum |dy' xhat|.
    dbeta  gamma(M + 2) of sum |dy'|;  exact for integer dy.
    dbias  sums the UNROUNDED da (l.238): the rows' fp32 terms plus gamma(M + 2) of sum |da|.
    ``accumulate``: + |old| in the magnitude, one more term.
  bias + GELU (kernels 648-714, gelu_f / gelu_grad in common.h: r = rcp(1 + exp2(y)),
  gelu = x - x r, gelu' = (1 - r)(1 + x r q))
    y      k = 1.  fp32: u32 |x| (4 + 33 r): the a + bias rounding through |gelu'| <= 1.13 and
           the final fma (4), and x r's relative error: rcp and exp2 allowances (16 + 16), the
           1 + e add (1), and the exponent's 3 roundings, at most 0.67 after the r (1 - r) factor.
    da     k = 1.  fp32: u32 |dy| (40 (1 + |x| r q) + 2 |x|) by the same count on both factors.
    dbias  the rows' fp32 terms plus gamma(M + 4) of sum |dy gelu'| (unrounded da is summed).
  mlm_xent (1364-1433)
    loss   fp32 output, ``ALLOW['loss_rows']`` u32 of wsc (|lse| + |x_label|) (measured).
    grad   k = 1.  fp32: wsc p (u32 (2 (|x| + |lse|) + ALLOW['loss_rows'] |lse|) + INTR)
           + 2 u32 wsc (p + onehot) (l.1423).
  attention forward (789-876), log2 domain, c = scale log2(e)
    out    k = 2: the dropped probabilities are rounded for the MFMA operand (pack_frag l.856)
           and the output on store (l.872).  fp32: (gamma(S + 8) + 2 ln2 gamma(70) smag + 2 INTR)
           of mag = sum_k |Pd v|, smag = max_k sum_d |q k| c (64-term MFMA score sums, l.823-832,
           numerator and denominator).
    lse    gamma(70) smag + gamma(S) / ln2 + ``ALLOW['lse']`` u32 (|m| + log2 l) (measured).
  attention backward (880-1045 split, 1090-1249 fused)
    delta  fp32 sum of 64 products of stored bf16 values (l.990-996 / 1115-1121): gamma(66) of
           sum |O dO|.  Derived, not measured.
    dV     k = 2: bf16(Pd) (l.939 / 1155) and the store.  fp32: (gamma(S + 4) + relP) magV with
           relP = ln2 gamma(72) max(smag + |lse|) + INTR the relative error of P = exp2(s - lse).
    dQ,dK  k = 2: bf16(dS) (l.940 / 1035 / 1156) and the store, of scale sum |dS| |K or Q|;
           fp32: (gamma(S + 72) + relP + 2 u32) of the same sum with |dS| replaced by
           P (|dPd| + |delta|), since dS = P (dPd - delta) cancels.
    colpart  fp32 column sums of the STORED dqkv over 128 tokens: gamma(128) of sum |dqkv|.
  pos_type_grad (1657-1730): integer ds, exact.

*Exact mode.*  Integer ``dy`` in [-3, 3] (``dbeta``, ``dbias`` at pre-activation 40 where
gelu' == 1, ``accumulate`` onto an integer buffer); attention with Q = 0 (every row the mean of
the 64 unmasked integer V rows) and the gather construction (one key leads by 16 nats, so
``O[q] == V[pi(q)]`` and ``dV[k] == dO[pi^-1(k)]`` after bf16 rounding, and with dropout each
row shows the keep decision of its one element); exact zeros at dropped positions.

*CPU self-tests* (unmarked): a torch emulation of each kernel's rounding points lies inside its
bound and each listed damage outside.

fp32 outputs whose error is dominated by an intrinsic (measured on an MI355X over this file's
shapes, allowance = 4 x measured rounded up to a power of two; see profiles/NLP_KERNELS.md):
    rstd       measured 2.21 u32 of rstd                    -> ALLOW 16
    lse        measured 2.76 u32 of |m| + log2 l            -> ALLOW 16
    loss_rows  measured 1.63 u32 of wsc (|lse| + |x_label|) -> ALLOW 8
mean and delta need no allowance: measured 0.0009 and 0.011 of their derived bounds.

Found by this file and fixed in nlp.hip: ``mlm_xent`` read the last logit of the last row as 0
when N * ld is odd (``test_mlm_xent`` at V = ld in {1, 5, 9, 77, 511}), and ``ln_fwd`` subtracted
the unrounded mean where the compiler fused ``sum * (1 / H)`` into ``v - mean`` (the constant row
of ``test_ln_fwd`` at H = 768).
"""
import math

import pytest
import torch

from distributedtensorflow_amd.ops import reference as R

BF16 = torch.bfloat16
U16 = 2.0 ** -8
U32 = 2.0 ** -24
INTR = 16 * U32
LN2 = math.log(2.0)
LOG2E = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
# allowances of the intrinsic-dominated fp32 outputs, in u32 of the magnitude named above
ALLOW = {"rstd": 16, "lse": 16, "loss_rows": 8}
FTZ = 2.0 ** -126           # below the fp32 normal range a result may flush to zero
SENT = -1.7e38              # guard value (a bf16 / fp32 nobody computes)


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _K():
    from distributedtensorflow_amd.ops import native
    return native._K


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _dev(t, dtype=None):
    return None if t is None else t.to("cuda", dtype or t.dtype).contiguous()


def gamma(n):
    assert n * U32 < 1
    return n * U32 / (1.0 - n * U32)


def _bf(t):
    """Round to bf16, back as fp64: the value a kernel reads."""
    return t.to(BF16).double()


def _inv_keep(p):
    """The kernels' fp32 ``1 / (1 - p)``."""
    if p <= 0:
        return 1.0
    one = torch.tensor(1.0)
    return float(one / (one - torch.tensor(p, dtype=torch.float32)))


def _keep(seed, idx, p):
    if p <= 0:
        return torch.ones(idx.shape, dtype=torch.bool)
    return R.keep_mask(seed, idx, p)


# ----------------------------------------------------------------------------- assertions
def assert_within(got, ref64, bound, what=""):
    """Element-wise ``|got - ref64| <= bound`` (+ ``FTZ``); reports the worst element."""
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


def _measure(name, got, ref64, unit):
    """Print the largest error of an fp32 output in units of ``unit`` (kept by the measuring
    job; the assertion follows)."""
    err = (got.detach().double().cpu() - ref64).abs()
    r = float((err / unit.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"MEASURE {name} {r:.4f}")
    return r


def _ratio(got, ref64, bound):
    err = (got.detach().double().cpu() - ref64).abs()
    return float((err / bound.expand_as(ref64).clamp_min(1e-300)).max())


# ============================================================================= LayerNorm
def ln_fwd_oracle(s, g, b, eps, keep_post=None, ik_post=1.0):
    """fp64 LayerNorm of the stored rows ``s`` [M, H] (fp64) -> dict of (ref, bound)."""
    H = s.shape[1]
    mean = s.mean(1, keepdim=True)
    mabs = s.abs().mean(1, keepdim=True)
    var = ((s - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    D = gamma(H + 2) * mabs                           # error of the fp32 mean
    rel_var = gamma(H + 6) + D * D / (var + eps)
    xg = ((s - mean) * rstd * g).abs()
    y = (s - mean) * rstd * g + b
    f32 = (xg + b.abs()) * (gamma(H + 8) + ALLOW["rstd"] * U32) + D * rstd * g.abs() \
        + 0.5 * D * D / (var + eps) * xg
    if keep_post is not None:
        y = torch.where(keep_post, y * ik_post, torch.zeros_like(y))
        f32 = f32 * ik_post
    return {
        "mean": (mean[:, 0], D[:, 0]),
        "rstd": (rstd[:, 0], (rstd * (0.5 * rel_var + ALLOW["rstd"] * U32))[:, 0]),
        "rstd_unit": (rstd * U32)[:, 0],
        "y": (y, U16 * y.abs() + f32),
    }


def ln_s_oracle(a, bias, res, keep_pre, ik_pre):
    """fp64 ``dropout(a + bias) + res`` and its bound (one bf16 rounding)."""
    x = a.clone()
    mag = a.abs()
    if bias is not None:
        x = x + bias
        mag = mag + bias.abs()
    if keep_pre is not None:
        x = torch.where(keep_pre, x * ik_pre, torch.zeros_like(x))
        mag = torch.where(keep_pre, mag * ik_pre, torch.zeros_like(x))
    if res is not None:
        x = x + res
        mag = mag + res.abs()
    return x, U16 * x.abs() + gamma(3) * mag


def ln_fwd_emulate(s32, g, b, eps):
    """fp32 arithmetic at the kernel's rounding points (stats of the stored bf16 row)."""
    H = s32.shape[1]
    mean = s32.sum(1, keepdim=True) * torch.tensor(1.0 / H, dtype=torch.float32)
    d = s32 - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) * torch.tensor(1.0 / H, dtype=torch.float32)
                       + torch.tensor(eps, dtype=torch.float32))
    return (d * rstd * g + b).to(BF16), mean[:, 0], rstd[:, 0]


def ln_bwd_oracle(dy, s, mean, rstd, g, keep_pre=None, ik_pre=1.0, keep_post=None, ik_post=1.0):
    """fp64 LayerNorm backward of what the kernel reads (bf16 dy, s; fp32 mean, rstd, gamma)."""
    M, H = s.shape
    mean, rstd = mean[:, None], rstd[:, None]
    if keep_post is not None:
        dy = torch.where(keep_post, dy * ik_post, torch.zeros_like(dy))
    xh = (s - mean) * rstd
    gy = dy * g
    s1 = gy.mean(1, keepdim=True)
    s2 = (gy * xh).mean(1, keepdim=True)
    dx = rstd * (gy - s1 - xh * s2)
    mdx = rstd * (gy.abs() + gy.abs().mean(1, keepdim=True)
                  + xh.abs() * (gy * xh).abs().mean(1, keepdim=True))
    fdx = gamma(H + 10) * mdx
    if keep_pre is not None:
        da = torch.where(keep_pre, dx * ik_pre, torch.zeros_like(dx))
        fda = torch.where(keep_pre, fdx * ik_pre, torch.zeros_like(dx))
    else:
        da, fda = dx, fdx
    return {
        "ds": (dx, U16 * dx.abs() + fdx),
        "da": (da, U16 * da.abs() + fda),
        "dgamma": ((dy * xh).sum(0), gamma(M + 6) * (dy * xh).abs().sum(0)),
        "dbeta": (dy.sum(0), gamma(M + 2) * dy.abs().sum(0)),
        "dbias": (da.sum(0), fda.sum(0) + gamma(M + 2) * da.abs().sum(0)),
    }


def ln_bwd_emulate(dy, s, mean, rstd, g):
    """fp32 twin of ln_bwd_kernel without dropout: (ds bf16, dgamma, dbeta)."""
    H = s.shape[1]
    invH = torch.tensor(1.0 / H, dtype=torch.float32)
    xh = (s - mean[:, None]) * rstd[:, None]
    gy = dy * g
    s1 = gy.sum(1, keepdim=True) * invH
    s2 = (gy * xh).sum(1, keepdim=True) * invH
    dx = rstd[:, None] * (gy - s1 - xh * s2)
    return dx.to(BF16), (dy * xh).sum(0), dy.sum(0)


def _ln_rows(M, H, g, special):
    """[M, H] fp32 rows ~ randn * 1.4; ``special``: rows 1..3 become a constant row (0.5: every
    partial sum and 384 * fl(1/768) are exact, so mean == 0.5 and var == 0 in any order), a row of
    +-2^-20 (var ~ 9e-13, next to eps = 1e-12) and a row of mean 4096 with spread 32."""
    a = torch.randn(M, H, generator=g) * 1.4
    if special and M >= 4:
        a[1] = 0.5
        a[2] = (torch.randint(0, 2, (H,), generator=g).float() * 2 - 1) * 2.0 ** -20
        a[3] = 4096 + 32 * torch.randn(H, generator=g)
    return a.to(BF16)


def _ln_params(H, g):
    return (1 + 0.1 * torch.randn(H, generator=g)), 0.1 * torch.randn(H, generator=g)


def _run_ln_fwd(M, H, gam, bet, eps, a=None, bias=None, res=None, p_pre=0.0, seed_pre=0,
                p_post=0.0, seed_post=0, emb=None, save_s=True):
    """ln_fwd on the GPU; outputs sit in buffers with 8 guard rows behind them."""
    K = _K()

    def out(dtype, *shape):
        return torch.full(shape, SENT, device="cuda", dtype=dtype)

    y, s = out(BF16, M + 8, H), out(BF16, M + 8, H) if save_s else None
    mean, rstd = out(torch.float32, M + 8), out(torch.float32, M + 8)
    ad, bd, rd = _dev(a), _dev(bias), _dev(res)
    gd, btd = _dev(gam), _dev(bet)
    ids = tt = word = pos = typ = None
    S = 1
    if emb is not None:
        ids, tt, word, pos, typ, S = emb
        ids, tt, word, pos, typ = (_dev(t) for t in (ids, tt, word, pos, typ))
    K.ln_fwd(_p(ad), _p(bd), _p(rd), gd.data_ptr(), btd.data_ptr(), y.data_ptr(), _p(s),
             mean.data_ptr(), rstd.data_ptr(), M, H, float(eps), float(p_pre), seed_pre,
             float(p_post), seed_post, _p(ids), _p(tt), _p(word), _p(pos), _p(typ), S, _st())
    torch.cuda.synchronize()
    res_ = {}
    for name, t in (("y", y), ("s", s), ("mean", mean), ("rstd", rstd)):
        if t is None:
            continue
        t = t.cpu()
        assert bool((t[M:].float() == SENT).all() if t.dtype == torch.float32
                    else (t[M:] == torch.tensor(SENT).to(BF16)).all()), f"{name}: wrote past row M"
        res_[name] = t[:M]
    return res_


def _check_ln_fwd(tag, r, s64, gam, bet, eps, keep_post=None, ik_post=1.0):
    o = ln_fwd_oracle(s64, gam.double(), bet.double(), eps, keep_post, ik_post)
    _measure("mean/bound", r["mean"], o["mean"][0], o["mean"][1])
    _measure("rstd", r["rstd"], o["rstd"][0], o["rstd_unit"])
    assert_within(r["mean"], *o["mean"], f"{tag} mean")
    assert_within(r["rstd"], *o["rstd"], f"{tag} rstd")
    assert_within(r["y"], *o["y"], f"{tag} y")
    if keep_post is not None:
        assert bool((r["y"][~keep_post] == 0).all()), f"{tag}: non-zero at a dropped position"
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_ln_fwd(H, wide):
    """Every mode of ln_fwd at M in {1, 7, 9, 37} (partial last blocks at 4 and at 8 rows per
    block), with the special rows in the plain mode."""
    eps = 1e-12
    _K().ln_set_wide(wide)
    try:
        for M in (1, 7, 9, 37):
            g = _gen(H * 100 + M)
            gam, bet = _ln_params(H, g)
            idx = torch.arange(M * H).view(M, H)
            # plain: s is not saved, the row read is a itself
            a = _ln_rows(M, H, g, special=True)
            r = _run_ln_fwd(M, H, gam, bet, eps, a=a, save_s=False)
            tag = f"ln_fwd plain H={H} M={M} wide={wide}"
            o = _check_ln_fwd(tag, r, a.double(), gam, bet, eps)
            if M >= 4:
                assert_exact(r["y"][1], bet.to(BF16).double(), f"{tag} constant row")
                assert_exact(r["mean"][1], torch.tensor(0.5, dtype=torch.float64))
                want = torch.tensor(eps, dtype=torch.float32).double() ** -0.5
                assert abs(float(r["rstd"][1]) - float(want)) <= ALLOW["rstd"] * U32 * float(want)
            # plain with the post-dropout
            r = _run_ln_fwd(M, H, gam, bet, eps, a=a, p_post=0.1, seed_post=5 + M, save_s=False)
            _check_ln_fwd(f"{tag} post-dropout", r, a.double(), gam, bet, eps,
                          _keep(5 + M, idx, 0.1), _inv_keep(0.1))
            # bias + pre-dropout + residual, s saved
            a, res = _ln_rows(M, H, g, False), _ln_rows(M, H, g, False)
            bias = 0.1 * torch.randn(H, generator=g)
            for p_pre, seed in ((0.0, 0), (0.1, 1234 + M)):
                r = _run_ln_fwd(M, H, gam, bet, eps, a=a, bias=bias, res=res, p_pre=p_pre,
                                seed_pre=seed)
                tag = f"ln_fwd fused H={H} M={M} wide={wide} p={p_pre}"
                kp = _keep(seed, idx, p_pre) if p_pre else None
                assert_within(r["s"], *ln_s_oracle(a.double(), bias.double(), res.double(), kp,
                                                   _inv_keep(p_pre)), f"{tag} s")
                if kp is not None:
                    assert torch.equal(r["s"][~kp], res[~kp]), f"{tag}: s != residual where dropped"
                _check_ln_fwd(tag, r, r["s"].double(), gam, bet, eps)
            # embedding mode with repeated ids and the post-dropout; tt given and null
            S, nv = 5, 11
            word, pos, typ = (0.05 * torch.randn(n, H, generator=g) for n in (nv, S, 2))
            word, pos, typ = word.to(BF16), pos.to(BF16), typ.to(BF16)
            ids = torch.randint(0, 4, (M,), generator=g) * 3
            for tt in (torch.randint(0, 2, (M,), generator=g), None):
                for p_post, seed in ((0.0, 0), (0.1, 77 + M)):
                    r = _run_ln_fwd(M, H, gam, bet, eps, emb=(ids, tt, word, pos, typ, S),
                                    p_post=p_post, seed_post=seed)
                    tag = f"ln_fwd emb H={H} M={M} wide={wide} tt={tt is not None} p={p_post}"
                    parts = [word.double()[ids], pos.double()[torch.arange(M) % S],
                             typ.double()[tt if tt is not None else torch.zeros(M, dtype=torch.long)]]
                    s64 = sum(parts)
                    assert_within(r["s"], s64, U16 * s64.abs()
                                  + gamma(2) * sum(t.abs() for t in parts), f"{tag} s")
                    kp = _keep(seed, idx, p_post) if p_post else None
                    _check_ln_fwd(tag, r, r["s"].double(), gam, bet, eps, kp, _inv_keep(p_post))
    finally:
        _K().ln_set_wide(1)


def _run_ln_bwd(M, H, dy, s, mean, rstd, gam, want_da, want_dbias, p_pre=0.0, seed_pre=0,
                p_post=0.0, seed_post=0, old=None):
    K = _K()
    ds = torch.full((M + 8, H), SENT, device="cuda", dtype=BF16)
    da = torch.full((M + 8, H), SENT, device="cuda", dtype=BF16) if want_da else None
    part = torch.empty(3 * K.ln_bwd_blocks(M) * H, device="cuda", dtype=torch.float32)
    outs = []
    for i in range(3):
        if i == 2 and not want_dbias:
            outs.append(None)
        elif old is not None:
            outs.append(_dev(old[i]).clone())
        else:
            outs.append(torch.full((H,), SENT, device="cuda", dtype=torch.float32))
    ins = [_dev(t) for t in (dy, s, mean, rstd, gam)]      # held until the kernels are done
    K.ln_bwd(*(t.data_ptr() for t in ins), ds.data_ptr(), _p(da), part.data_ptr(),
             outs[0].data_ptr(), outs[1].data_ptr(), _p(outs[2]), M, H, float(p_pre), seed_pre,
             float(p_post), seed_post, _st(), int(old is not None))
    torch.cuda.synchronize()
    guard = torch.tensor(SENT).to(BF16)
    assert bool((ds[M:] == guard).all()) and (da is None or bool((da[M:] == guard).all()))
    return {"ds": ds[:M].cpu(), "da": None if da is None else da[:M].cpu(),
            "dgamma": outs[0].cpu(), "dbeta": outs[1].cpu(),
            "dbias": None if outs[2] is None else outs[2].cpu()}


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [1, 3])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_ln_bwd(H, wide):
    """ln_bwd on host-made s / mean / rstd at M in {1, 33, 1100} (1100: 35 partial rows, 2
    col_sum slices of 18 and 17), with and without da / dbias and either dropout, accumulate
    0 / 1; integer dy makes dbeta (and its accumulation) exact."""
    _K().ln_set_wide(wide)
    try:
        for M in (1, 33, 1100):
            g = _gen(H * 7 + M)
            gam, _ = _ln_params(H, g)
            s = _ln_rows(M, H, g, False)
            s64 = s.double()
            mean = s64.mean(1).float()
            rstd = (1.0 / torch.sqrt(s64.var(1, unbiased=False) + 1e-12)).float()
            idx = torch.arange(M * H).view(M, H)
            old = [torch.randint(-5, 6, (H,), generator=g).float() for _ in range(3)]
            modes = [("plain", False, False, 0.0, 0.0), ("pre", True, True, 0.1, 0.0),
                     ("bias", True, True, 0.0, 0.0), ("post", False, False, 0.0, 0.1)]
            for name, want_da, want_dbias, p_pre, p_post in modes:
                for integer in (False, True):
                    for acc in (False, True):
                        dy = (torch.randint(-3, 4, (M, H), generator=g).float() if integer
                              else torch.randn(M, H, generator=g)).to(BF16)
                        r = _run_ln_bwd(M, H, dy, s, mean, rstd, gam, want_da, want_dbias, p_pre,
                                        11 + M, p_post, 13 + M, old if acc else None)
                        kpre = _keep(11 + M, idx, p_pre) if p_pre else None
                        kpost = _keep(13 + M, idx, p_post) if p_post else None
                        o = ln_bwd_oracle(dy.double(), s64, mean.double(), rstd.double(),
                                          gam.double(), kpre, _inv_keep(p_pre), kpost,
                                          _inv_keep(p_post))
                        tag = f"ln_bwd {name} H={H} M={M} wide={wide} int={integer} acc={acc}"
                        assert_within(r["ds"], *o["ds"], f"{tag} ds")
                        if want_da:
                            assert_within(r["da"], *o["da"], f"{tag} da")
                            if kpre is not None:
                                assert bool((r["da"][~kpre] == 0).all()), f"{tag}: da at a drop"
                        for i, q in enumerate(("dgamma", "dbeta", "dbias")):
                            if r[q] is None:
                                continue
                            ref, bnd = o[q]
                            if acc:
                                bnd = bnd + U32 * (ref.abs() + old[i].double().abs())
                                ref = ref + old[i].double()
                            if q == "dbeta" and integer and not p_post:
                                assert_exact(r[q], ref, f"{tag} dbeta")
                            else:
                                assert_within(r[q], ref, bnd, f"{tag} {q}")
    finally:
        _K().ln_set_wide(1)


def test_ln_bounds_accept_emulation_and_reject_damage():
    """fp32 emulations of ln_fwd / ln_bwd lie inside their bounds; eps = 1e-5 for 1e-12 on the
    small-variance row, y or ds 1 % off and one row missing from dgamma lie outside."""
    H, M, eps = 768, 37, 1e-12
    g = _gen(5)
    gam, bet = _ln_params(H, g)
    a = _ln_rows(M, H, g, special=True)
    o = ln_fwd_oracle(a.double(), gam.double(), bet.double(), eps)
    y, mean, rstd = ln_fwd_emulate(a.float(), gam, bet, eps)
    assert_within(y, *o["y"], "emulated y")
    assert_within(mean, *o["mean"], "emulated mean")
    assert_within(rstd, *o["rstd"], "emulated rstd")
    assert_exact(y[1], bet.to(BF16).double(), "constant row")
    y5, _, rstd5 = ln_fwd_emulate(a.float(), gam, bet, 1e-5)
    with pytest.raises(AssertionError, match=r"worst at \(2, "):
        assert_within(y5, *o["y"], "eps 1e-5")
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within(rstd5, *o["rstd"], "eps 1e-5")
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within((y.float() * 1.01).to(BF16), *o["y"], "y 1 % off")
    # backward
    M = 1100
    s = _ln_rows(M, H, g, False)
    s64 = s.double()
    mean = s64.mean(1).float()
    rstd = (1.0 / torch.sqrt(s64.var(1, unbiased=False) + eps)).float()
    dy = torch.randn(M, H, generator=g).to(BF16)
    ob = ln_bwd_oracle(dy.double(), s64, mean.double(), rstd.double(), gam.double())
    ds, dg, db = ln_bwd_emulate(dy.float(), s.float(), mean, rstd, gam)
    assert_within(ds, *ob["ds"], "emulated ds")
    assert_within(dg, *ob["dgamma"], "emulated dgamma")
    assert_within(db, *ob["dbeta"], "emulated dbeta")
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within((ds.float() * 1.01).to(BF16), *ob["ds"], "ds 1 % off")
    _, dg1, _ = ln_bwd_emulate(dy.float()[:-1], s.float()[:-1], mean[:-1], rstd[:-1], gam)
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within(dg1, *ob["dgamma"], "row missing from dgamma")
    dyi = torch.randint(-3, 4, (M, H), generator=g).float()
    assert_exact(ln_bwd_emulate(dyi, s.float(), mean, rstd, gam)[2], dyi.double().sum(0))


# ============================================================================= bias + GELU
K0 = float(torch.tensor(0.7978845608028654, dtype=torch.float32))
K1 = float(torch.tensor(0.044715, dtype=torch.float32))
EXTREME = [-3e4, -200.0, -40.0, -9.5, -4.0, -1e-3, 0.0, 1e-3, 4.0, 9.5, 40.0, 200.0, 3e4]


def gelu_oracle(x):
    """tanh-GELU in fp64 as x sigmoid(2u) (no cancellation): (gelu, gelu', r, q)."""
    u2 = 2.0 * K0 * (x + K1 * x ** 3)
    sig, r = torch.sigmoid(u2), torch.sigmoid(-u2)
    q = 2.0 * K0 + 6.0 * K0 * K1 * x * x
    return x * sig, sig * (1.0 + x * r * q), r, q


def gelu_fwd_bound(x):
    y, _, r, _ = gelu_oracle(x)
    return y, U16 * y.abs() + U32 * x.abs() * (4 + 33 * r)


def gelu_bwd_bound(x, dy):
    _, gp, r, q = gelu_oracle(x)
    f32 = U32 * dy.abs() * (40 * (1 + x.abs() * r * q) + 2 * x.abs())
    return dy * gp, U16 * (dy * gp).abs() + f32, f32


def gelu_emulate(x32):
    """fp32 twin of gelu_f / gelu_grad (common.h)."""
    x2 = x32 * x32
    e0 = torch.tensor(2.0 * K0, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    e1 = e0 * torch.tensor(K1, dtype=torch.float32)
    r = 1.0 / (1.0 + torch.exp2(x32 * (x2 * e1 + e0)))
    q = x2 * torch.tensor(6.0 * K0 * K1, dtype=torch.float32) + torch.tensor(2.0 * K0, dtype=torch.float32)
    return x32 - x32 * r, (1.0 - r) * (x32 * r * q + 1.0)


def _gelu_inputs(M, N, g):
    """Pre-activations a + bias dense over [-12, 12] (bias within +-0.5)."""
    a = (torch.rand(M, N, generator=g) * 24 - 12).to(BF16)
    bias = torch.rand(N, generator=g) - 0.5
    return a, bias


@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 264, 2056])
def test_bias_gelu_fwd(N):
    """M in {1, 3, 5, 8195} (8195: R = 8 rows per block, the last block has 3, so the 4-row unroll
    is partial twice); N = 2056 has 257 column vectors (a second trip of the column loop); bias
    given and null; the extreme values exactly."""
    K = _K()
    for M in (1, 3, 5, 8195):
        g = _gen(N * 10 + M)
        a, bias = _gelu_inputs(M, N, g)
        for bv in (bias, None):
            y = torch.full((M + 4, N), SENT, device="cuda", dtype=BF16)
            ad, bd = _dev(a), _dev(bv)
            K.bias_gelu_fwd(ad.data_ptr(), _p(bd), y.data_ptr(), M, N, _st())
            torch.cuda.synchronize()
            assert bool((y[M:] == torch.tensor(SENT).to(BF16)).all()), "wrote past row M"
            x = a.double() + (bv.double() if bv is not None else 0)
            assert_within(y[:M], *gelu_fwd_bound(x), f"bias_gelu_fwd M={M} N={N} bias={bv is not None}")
    ext = torch.tensor(EXTREME).repeat(5, 8)[:, :N if N == 8 else 104].contiguous().to(BF16)
    M, Ne = ext.shape
    y, ed = torch.empty_like(ext, device="cuda"), _dev(ext)
    K.bias_gelu_fwd(ed.data_ptr(), 0, y.data_ptr(), M, Ne, _st())
    torch.cuda.synchronize()
    big = ext.double().abs() >= 40
    want = torch.where(ext.double() >= 40, ext.double(), torch.zeros_like(ext.double()))
    assert_exact(y.cpu()[big], want[big], "gelu at |x| >= 40")
    ref, bnd = gelu_fwd_bound(ext.double())
    assert_within(y.cpu()[~big], ref[~big], bnd[~big], "gelu at the small extremes")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 264, 2056])
def test_bias_gelu_bwd(N):
    """M in {1, 17, 530} (530: 34 partial rows, 2 col_sum slices); bias / dbias given and null,
    accumulate 0 / 1; at pre-activation 40 gelu' == 1: da == dy and dbias the exact integer
    column sums (also accumulated onto an integer buffer)."""
    K = _K()
    for M in (1, 17, 530):
        g = _gen(N * 20 + M)
        a, bias = _gelu_inputs(M, N, g)
        old = torch.randint(-5, 6, (N,), generator=g).float()
        for mode in ("bound", "bound_acc", "nobias", "exact", "exact_acc"):
            exact, acc = mode.startswith("exact"), mode.endswith("acc")
            if exact:
                a_, b_ = torch.full((M, N), 38.0).to(BF16), torch.full((N,), 2.0)
                dy = torch.randint(-3, 4, (M, N), generator=g).float().to(BF16)
            else:
                a_, b_ = a, (None if mode == "nobias" else bias)
                dy = torch.randn(M, N, generator=g).to(BF16)
            da = torch.full((M + 4, N), SENT, device="cuda", dtype=BF16)
            part = torch.empty(K.bias_gelu_bwd_blocks(M) * N, device="cuda", dtype=torch.float32)
            dbias = None
            if b_ is not None:
                dbias = _dev(old).clone() if acc else torch.full((N,), SENT, device="cuda")
            dyd, ad, bd = _dev(dy), _dev(a_), _dev(b_)
            K.bias_gelu_bwd(dyd.data_ptr(), ad.data_ptr(), _p(bd), da.data_ptr(),
                            part.data_ptr(), _p(dbias), M, N, _st(), int(acc))
            torch.cuda.synchronize()
            assert bool((da[M:] == torch.tensor(SENT).to(BF16)).all()), "wrote past row M"
            tag = f"bias_gelu_bwd M={M} N={N} {mode}"
            x = a_.double() + (b_.double() if b_ is not None else 0)
            ref, bnd, f32 = gelu_bwd_bound(x, dy.double())
            if exact:
                assert_exact(da[:M], dy.double(), f"{tag} da")
                assert_exact(dbias, dy.double().sum(0) + (old.double() if acc else 0), f"{tag} dbias")
                continue
            assert_within(da[:M], ref, bnd, f"{tag} da")
            if dbias is not None:
                want = ref.sum(0)
                b2 = f32.sum(0) + gamma(M + 4) * ref.abs().sum(0)
                if acc:
                    b2 = b2 + U32 * (want.abs() + old.double().abs())
                    want = want + old.double()
                assert_within(dbias, want, b2, f"{tag} dbias")
    ext = torch.tensor(EXTREME).repeat(5, 8)[:, :104].contiguous().to(BF16)
    M, Ne = ext.shape
    dy = torch.randn(M, Ne, generator=_gen(3)).to(BF16)
    da = torch.empty_like(ext, device="cuda")
    dyd, ed = _dev(dy), _dev(ext)
    K.bias_gelu_bwd(dyd.data_ptr(), ed.data_ptr(), 0, da.data_ptr(), 0, 0, M, Ne, _st(), 0)
    torch.cuda.synchronize()
    big = ext.double().abs() >= 40
    want = torch.where(ext.double() >= 40, dy.double(), torch.zeros_like(dy.double()))
    assert_exact(da.cpu()[big], want[big], "gelu' at |x| >= 40")
    ref, bnd, _ = gelu_bwd_bound(ext.double(), dy.double())
    assert_within(da.cpu()[~big], ref[~big], bnd[~big], "gelu' at the small extremes")


def test_gelu_bounds_accept_emulation_and_reject_damage():
    g = _gen(9)
    a, bias = _gelu_inputs(64, 264, g)
    a = torch.cat([a, torch.tensor(EXTREME[3:-3]).repeat(40)[:264].view(1, 264).to(BF16)])
    x32 = a.float() + bias
    dy = torch.randn(65, 264, generator=g).to(BF16)
    y, gp = gelu_emulate(x32)
    ref, bnd = gelu_fwd_bound(a.double() + bias.double())
    assert_within(y.to(BF16), ref, bnd, "emulated gelu")
    refb, bndb, _ = gelu_bwd_bound(a.double() + bias.double(), dy.double())
    assert_within((dy.float() * gp).to(BF16), refb, bndb, "emulated gelu'")
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within((y * 1.01).to(BF16), ref, bnd, "gelu 1 % off")
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within((dy.float() * gp * 1.01).to(BF16), refb, bndb, "gelu' 1 % off")
    y_erf = torch.nn.functional.gelu(x32)            # the erf form is not the tanh form
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within(y_erf.to(BF16), ref, bnd, "erf gelu")


# ============================================================================= mlm_xent
PAD = 1e4
MLM_SHAPES = [(1, 1), (5, 5), (8, 8), (9, 9), (77, 77), (77, 80), (511, 511), (513, 576),
              (30522, 30522)]


def mlm_oracle(x, V, labels, w, denom):
    """x [N, ld] fp64 stored logits; w fp32 weights or None; denom the fp32 value the kernel
    reads.  Returns dict of (ref, bound) for loss_rows and grad [N, ld]."""
    N, ld = x.shape
    xv = x[:, :V]
    lse = torch.logsumexp(xv, 1)
    wsc = (w.double() if w is not None else torch.ones(N, dtype=torch.float64)) / max(float(denom), 1e-5)
    xl = xv[torch.arange(N), labels]
    loss = wsc * (lse - xl)
    lunit = U32 * wsc.abs() * (lse.abs() + xl.abs())
    p = torch.exp(xv - lse[:, None])
    onehot = torch.zeros_like(xv)
    onehot[torch.arange(N), labels] = 1.0
    grad = torch.zeros_like(x)
    grad[:, :V] = wsc[:, None] * (p - onehot)
    relp = U32 * (2 * (xv.abs() + lse.abs()[:, None]) + ALLOW["loss_rows"] * lse.abs()[:, None]) + INTR
    bnd = torch.zeros_like(x)
    bnd[:, :V] = U16 * grad[:, :V].abs() + wsc.abs()[:, None] * (p * relp + 2 * U32 * (p + onehot))
    return {"loss": (loss, ALLOW["loss_rows"] * lunit), "loss_unit": lunit, "grad": (grad, bnd)}


def mlm_emulate(x32, V, labels, w, denom):
    N = x32.shape[0]
    xv = x32[:, :V]
    lse = torch.logsumexp(xv, 1)
    wsc = (w if w is not None else torch.ones(N)) / max(float(denom), 1e-5)
    onehot = torch.zeros_like(xv)
    onehot[torch.arange(N), labels] = 1.0
    grad = torch.zeros_like(x32)
    grad[:, :V] = wsc[:, None] * (torch.exp(xv - lse[:, None]) - onehot)
    return wsc * (lse - xv[torch.arange(N), labels]), grad.to(BF16)


def _mlm_inputs(N, V, ld, g, special):
    x = torch.full((N, ld), PAD)
    x[:, :V] = torch.randn(N, V, generator=g) * 3
    labels = torch.randint(0, V, (N,), generator=g)
    w = torch.rand(N, generator=g) + 0.5
    labels[0] = 0
    if N >= 3:
        labels[1] = V - 1
        if special:
            x[1, :V] = 0.75                                   # equal logits
            x[2, :V] = (torch.randint(0, 2, (V,), generator=g).float() * 2 - 1) * 80
    if N >= 6:
        w[4] = 0.0                                            # a zero-weight row
    return x.to(BF16), labels, w


def _run_mlm(x, V, labels, w, denom, want_grad=True):
    """mlm_xent with the gradient in a guarded buffer: 16 B before it and 128 B behind it hold a
    sentinel that must survive (the base stays 16-B aligned)."""
    K = _K()
    N, ld = x.shape
    rows = torch.full((N + 2,), SENT, device="cuda")
    buf = torch.full((8 + N * ld + 64,), SENT, device="cuda", dtype=BF16)
    gptr = buf.data_ptr() + 16
    assert gptr % 16 == 0
    xd = _dev(x)
    assert xd.data_ptr() % 16 == 0
    ld_, wd = _dev(labels), _dev(w)
    dd = torch.tensor([denom], dtype=torch.float32, device="cuda")
    K.mlm_xent(xd.data_ptr(), ld_.data_ptr(), _p(wd), dd.data_ptr(), N, V, ld,
               rows.data_ptr(), gptr if want_grad else 0, _st())
    torch.cuda.synchronize()
    buf, rows = buf.cpu(), rows.cpu()
    guard = torch.tensor(SENT).to(BF16)
    assert bool((buf[:8] == guard).all()) and bool((buf[8 + N * ld:] == guard).all()), \
        "mlm_xent wrote outside the gradient"
    assert bool((rows[N:] == SENT).all())
    if not want_grad:
        assert bool((buf == guard).all()), "mlm_xent wrote a gradient it was not asked for"
    return rows[:N], buf[8:8 + N * ld].view(N, ld)


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld", MLM_SHAPES)
def test_mlm_xent(V, ld):
    """Every row-head offset (odd V with ld == V), V below one chunk and below 512 (lanes
    without a chunk), N in {1, 3, 6} (N % 4 != 0), labels at 0 and V - 1, the equal and the +-80
    rows, a zero-weight row, all weights zero, null weights and a null gradient; padding columns
    hold 1e4 on input and +0 bits in the gradient."""
    for N in (1, 3, 6):
        g = _gen(V * 10 + N)
        x, labels, w = _mlm_inputs(N, V, ld, g, special=True)
        for wmode in ("weights", "none", "zero", "nograd"):
            wv = {"weights": w, "none": None, "zero": torch.zeros(N), "nograd": w}[wmode]
            denom = float(wv.sum()) if wv is not None else float(N)
            rows, grad = _run_mlm(x, V, labels, wv, denom, want_grad=wmode != "nograd")
            tag = f"mlm_xent V={V} ld={ld} N={N} {wmode}"
            o = mlm_oracle(x.double(), V, labels, wv, torch.tensor(denom, dtype=torch.float32))
            if wmode != "zero":
                _measure("loss_rows", rows, o["loss"][0], o["loss_unit"])
            assert_within(rows, *o["loss"], f"{tag} loss_rows")
            if wmode == "nograd":
                continue
            assert_within(grad, *o["grad"], f"{tag} grad")
            assert bool((grad[:, V:].contiguous().view(torch.int16) == 0).all()), \
                f"{tag}: padding gradient is not +0"
            zero = torch.ones(N, dtype=torch.bool) if wmode == "zero" else \
                (wv == 0 if wv is not None else torch.zeros(N, dtype=torch.bool))
            assert bool((rows[zero] == 0).all()) and bool((grad[zero] == 0).all()), \
                f"{tag}: zero weight, non-zero result"


def test_mlm_bounds_accept_emulation_and_reject_damage():
    g = _gen(4)
    N, V, ld = 6, 513, 576
    x, labels, w = _mlm_inputs(N, V, ld, g, special=True)
    denom = torch.tensor(float(w.sum()), dtype=torch.float32)
    o = mlm_oracle(x.double(), V, labels, w, denom)
    rows, grad = mlm_emulate(x.float(), V, labels, w, denom)
    assert_within(rows, *o["loss"], "emulated loss_rows")
    assert_within(grad, *o["grad"], "emulated grad")
    col = int(torch.where(torch.arange(V) == labels[0], torch.zeros(V),
                          grad[0, :V].float().abs()).argmax())
    bad = grad.clone()
    bad[0, col] = (bad[0, col].float() * 1.02).to(BF16)
    with pytest.raises(AssertionError, match=rf"1 of {N * ld} .* worst at \(0, {col}\)"):
        assert_within(bad, *o["grad"], "column 2 % off")
    bad = grad.clone()
    bad[3, V + 2] = 1e-6
    with pytest.raises(AssertionError, match=rf"worst at \(3, {V + 2}\)"):
        assert_within(bad, *o["grad"], "padding column non-zero")
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within(rows * (1 + 1e-5), *o["loss"], "loss 1e-5 off")


# ============================================================================= pos_type_grad
@pytest.mark.gpu
@pytest.mark.parametrize("H", [8, 520, 768])
def test_pos_type_grad(H):
    """Integer ds: position sums over the batch and per-type sums, exact; NT in {1, 2, 4},
    B in {1, 3, 6} (4 row groups: fewer, partial and more than one trip), tt null for NT = 1."""
    K, S = _K(), 5
    for NT in (1, 2, 4):
        for B in (1, 3, 6):
            g = _gen(H + 10 * NT + B)
            ds = torch.randint(-3, 4, (B * S, H), generator=g).float().to(BF16)
            tt = torch.randint(0, NT, (B * S,), generator=g) if NT > 1 else None
            dpos = torch.full((S + 1, H), SENT, device="cuda")
            dtyp = torch.full((NT + 1, H), SENT, device="cuda")
            ws = torch.empty(K.pos_type_grad_ws_floats(S, H, NT), device="cuda")
            dsd, ttd = _dev(ds), _dev(tt)
            K.pos_type_grad(dsd.data_ptr(), _p(ttd), B, S, H, NT, dpos.data_ptr(),
                            dtyp.data_ptr(), ws.data_ptr(), _st())
            torch.cuda.synchronize()
            tag = f"pos_type_grad H={H} NT={NT} B={B}"
            d64 = ds.double()
            assert_exact(dpos[:S], d64.view(B, S, H).sum(0), f"{tag} dpos")
            t = tt if tt is not None else torch.zeros(B * S, dtype=torch.long)
            want = torch.stack([d64[t == k].sum(0) for k in range(NT)])
            assert_exact(dtyp[:NT], want, f"{tag} dtyp")
            assert bool((dpos[S:] == SENT).all()) and bool((dtyp[NT:] == SENT).all())


# ============================================================================= attention
AD = 64


def _heads(t, B, S, H):
    """[B*S, H*64] -> [B, H, S, 64] fp64."""
    return t.double().view(B, S, H, AD).permute(0, 2, 1, 3)


def _rows(t, B, S, H):
    """[B, H, S, 64] -> [B*S, H*64]."""
    return t.permute(0, 2, 1, 3).reshape(B * S, H * AD)


def _split_qkv(qkv, B, S, H):
    x = qkv.double().view(B, S, 3, H, AD)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def _scores(q, k, mask, B, S, scale):
    """log2-domain scores and the magnitude of their 64-term sums; c = fl(scale) fl(log2 e)."""
    c = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    s2 = q @ k.transpose(-1, -2) * c
    smag = (q.abs() @ k.abs().transpose(-1, -2) * c)
    if mask is not None:
        s2 = s2 + (mask.double() * LOG2E).view(B, 1, 1, S)
    return s2, smag


def _attn_idx(B, H, S):
    return torch.arange(B * H * S * S, dtype=torch.int64).view(B, H, S, S)


def attn_fwd_oracle(qkv, mask, B, S, H, scale, p, seed):
    q, k, v = _split_qkv(qkv, B, S, H)
    s2, smag = _scores(q, k, mask, B, S, scale)
    smax = smag.max(-1, keepdim=True).values
    m = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    keep = _keep(seed, _attn_idx(B, H, S), p)
    Pd = torch.where(keep, P * _inv_keep(p), torch.zeros_like(P))
    out, mag = Pd @ v, Pd @ v.abs()
    rel32 = gamma(S + 8) + 2 * LN2 * gamma(70) * smax + 2 * INTR
    lse = (m + torch.log2(l))[..., 0]
    lunit = U32 * (m.abs() + torch.log2(l))[..., 0]
    lb = gamma(70) * smax[..., 0] + gamma(S) / LN2 + ALLOW["lse"] * lunit
    return {"out": (_rows(out, B, S, H), _rows((2 * U16 + rel32) * mag, B, S, H)),
            "lse": (lse.reshape(-1), lb.reshape(-1)), "lse_unit": lunit.reshape(-1),
            "mag": _rows(mag, B, S, H)}


def attn_fwd_emulate(qkv, mask, B, S, H, scale, p, seed, rescale=True):
    """fp32 arithmetic with bf16 where attn_fwd_kernel rounds (dropped probabilities, output)."""
    x = qkv.float().view(B, S, 3, H, AD)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s2 = q @ k.transpose(-1, -2) * c
    if mask is not None:
        s2 = s2 + (mask.float() * torch.tensor(LOG2E, dtype=torch.float32)).view(B, 1, 1, S)
    e = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    keep = _keep(seed, _attn_idx(B, H, S), p)
    ik = torch.tensor(_inv_keep(p) if rescale else 1.0, dtype=torch.float32)
    pd = torch.where(keep, e * ik, torch.zeros_like(e)).to(BF16).float()
    return _rows((pd @ v) * (1.0 / l), B, S, H).to(BF16)


def attn_bwd_oracle(qkv, mask, dO, O, lse, B, S, H, scale, p, seed):
    """fp64 backward of what the kernels read: bf16 qkv, dO and the STORED O, fp32 stored lse."""
    q, k, v = _split_qkv(qkv, B, S, H)
    s2, smag = _scores(q, k, mask, B, S, scale)
    L = lse.double().view(B, H, S, 1)
    P = torch.exp2(s2 - L)
    dOh, Oh = _heads(dO, B, S, H), _heads(O, B, S, H)
    delta = (Oh * dOh).sum(-1, keepdim=True)
    dmag = (Oh * dOh).abs().sum(-1, keepdim=True)
    keep = _keep(seed, _attn_idx(B, H, S), p)
    ik = _inv_keep(p)
    zero = torch.zeros_like(P)
    Pd = torch.where(keep, P * ik, zero)
    dPd = torch.where(keep, dOh @ v.transpose(-1, -2) * ik, zero)
    dPm = torch.where(keep, dOh.abs() @ v.abs().transpose(-1, -2) * ik, zero)
    dS, dSm = P * (dPd - delta), P * (dPm + dmag)
    sc = float(torch.tensor(scale, dtype=torch.float32))
    # P of a masked key is exactly 0 on both sides: its score magnitude does not count
    live = P > 0
    relP = LN2 * gamma(72) * float((smag + L.abs())[live].max()) + INTR
    T = lambda t: t.transpose(-1, -2)
    dV, mV = T(Pd) @ dOh, T(Pd) @ dOh.abs()
    dK, mK, mK2 = sc * T(dS) @ q, sc * T(dS.abs()) @ q.abs(), sc * T(dSm) @ q.abs()
    dQ, mQ, mQ2 = sc * dS @ k, sc * dS.abs() @ k.abs(), sc * dSm @ k.abs()
    r2 = gamma(S + 72) + relP + 2 * U32
    ref = torch.cat([_rows(t, B, S, H) for t in (dQ, dK, dV)], 1)
    bnd = torch.cat([_rows(t, B, S, H) for t in
                     (2 * U16 * mQ + r2 * mQ2, 2 * U16 * mK + r2 * mK2,
                      (2 * U16 + gamma(S + 4) + relP) * mV)], 1)
    return {"dqkv": (ref, bnd), "delta": (delta.reshape(-1), gamma(66) * dmag.reshape(-1))}


def _run_attn(qkv, mask, dO, B, S, H, scale, p, seed, colpart=False):
    """attn_fwd then attn_bwd on the GPU -> dict of CPU tensors."""
    K = _K()
    qd, md, dod = _dev(qkv), _dev(mask), _dev(dO)
    out = torch.full((B * S, H * AD), SENT, device="cuda", dtype=BF16)
    lse = torch.full((B * H * S,), SENT, device="cuda")
    nk = K.attn_keep_words(B, S, H, float(p))
    keep = torch.zeros(nk, device="cuda", dtype=torch.int32) if nk else None
    K.attn_fwd(qd.data_ptr(), _p(md), out.data_ptr(), lse.data_ptr(), B, S, H, float(scale),
               float(p), seed, _st(), _p(keep))
    torch.cuda.synchronize()
    r = {"out": out.cpu(), "lse": lse.cpu()}
    if dO is None:
        return r
    dqkv = torch.full_like(qd, SENT)
    delta = torch.full_like(lse, SENT)
    part = torch.full((B, 3 * H * AD), SENT, device="cuda") if colpart else None
    K.attn_bwd(qd.data_ptr(), _p(md), out.data_ptr(), dod.data_ptr(), lse.data_ptr(),
               delta.data_ptr(), dqkv.data_ptr(), B, S, H, float(scale), float(p), seed, _st(),
               _p(part), _p(keep))
    torch.cuda.synchronize()
    r.update(dqkv=dqkv.cpu(), delta=delta.cpu(), colpart=None if part is None else part.cpu())
    return r


def _attn_inputs(B, S, H, g, masked):
    """Q, K = randn * 2, V = |randn| + 0.5 (nothing cancels in O: mag64 == |O|), dO = randn."""
    x = torch.randn(B * S, 3, H, AD, generator=g) * 2
    x[:, 2] = x[:, 2].abs() / 2 + 0.5
    qkv = x.view(B * S, 3 * H * AD).to(BF16)
    dO = torch.randn(B * S, H * AD, generator=g).to(BF16)
    mask = None
    if masked:
        mask = torch.zeros(B, S)
        mask[1, S - 37:] = -10000.0
    return qkv, dO, mask


# (S, wide, fused, keep): every combination at which the launchers take another kernel
ATTN_PATHS = [(64, 1, 1, 1), (192, 1, 1, 1),
              (128, 1, 1, 1), (128, 1, 1, 0), (128, 1, 0, 1), (128, 0, 1, 1), (128, 0, 0, 1),
              (256, 1, 1, 1), (256, 0, 1, 1)]


def _attn_switches(wide, fused, keep):
    K = _K()
    K.attn_set_wide(wide)
    K.attn_set_fused(fused)
    K.attn_set_keep(keep)


@pytest.mark.gpu
@pytest.mark.parametrize("S,wide,fused,keep", ATTN_PATHS)
def test_attention_bound(S, wide, fused, keep):
    """out, lse, delta and the three thirds of dqkv against fp64 on every kernel path, with
    p in {0, 0.1} and the mask null or masking the tail of one batch entry; on the fused path
    the column partials against the fp64 column sums of the stored dqkv."""
    B, H, scale = 2, 3, AD ** -0.5
    _attn_switches(wide, fused, keep)
    try:
        use_part = bool(_K().attn_bwd_fused(S))
        for p, seed in ((0.0, 0), (0.1, 4242 + S)):
            for masked in (False, True):
                g = _gen(S * 10 + int(p * 10) + masked)
                qkv, dO, mask = _attn_inputs(B, S, H, g, masked)
                r = _run_attn(qkv, mask, dO, B, S, H, scale, p, seed, colpart=use_part)
                tag = f"attention S={S} wide={wide} fused={fused} keep={keep} p={p} mask={masked}"
                of = attn_fwd_oracle(qkv, mask, B, S, H, scale, p, seed)
                _measure("lse", r["lse"], of["lse"][0], of["lse_unit"])
                assert_within(r["out"], *of["out"], f"{tag} out")
                assert_within(r["lse"], *of["lse"], f"{tag} lse")
                ob = attn_bwd_oracle(qkv, mask, dO, r["out"], r["lse"], B, S, H, scale, p, seed)
                _measure("delta/bound", r["delta"], *ob["delta"])
                assert_within(r["delta"], *ob["delta"], f"{tag} delta")
                ref, bnd = ob["dqkv"]
                for i, name in enumerate(("dQ", "dK", "dV")):
                    sl = slice(i * H * AD, (i + 1) * H * AD)
                    assert_within(r["dqkv"][:, sl], ref[:, sl], bnd[:, sl], f"{tag} {name}")
                if use_part:
                    d64 = r["dqkv"].double().view(B, S, 3 * H * AD)
                    assert_within(r["colpart"], d64.sum(1), gamma(128) * d64.abs().sum(1),
                                  f"{tag} colpart")
    finally:
        _attn_switches(1, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("S,wide,fused,keep", ATTN_PATHS)
def test_attention_uniform_exact(S, wide, fused, keep):
    """Q = 0, integer V in [-3, 3] and a -10000 mask that leaves 64 scattered keys: every output
    row is exactly the mean of the unmasked V rows (sums below 256 over 64: bf16 holds them), and
    lse is exactly log2(64) = 6."""
    B, H = 2, 3
    g = _gen(S)
    x = torch.randint(-3, 4, (B * S, 3, H, AD), generator=g).float()
    x[:, 0] = 0
    qkv = x.view(B * S, 3 * H * AD).to(BF16)
    mask = torch.full((B, S), -10000.0)
    for b in range(B):
        mask[b, torch.randperm(S, generator=g)[:64]] = 0.0
    _attn_switches(wide, fused, keep)
    try:
        r = _run_attn(qkv, mask, None, B, S, H, AD ** -0.5, 0.0, 0)
    finally:
        _attn_switches(1, 1, 1)
    v = x[:, 2].double().view(B, S, H * AD)
    want = torch.stack([v[b][mask[b] == 0].sum(0) / 64 for b in range(B)])     # [B, H*64]
    assert_exact(want.to(BF16), want, "the mean is not a bf16 value")
    assert_exact(r["out"].view(B, S, H * AD), want[:, None].expand(B, S, H * AD), f"uniform S={S}")
    six = torch.full((B * H * S,), 6.0, dtype=torch.float64)
    assert_within(r["lse"], six, ALLOW["lse"] * U32 * six, "lse")


def _gather_inputs(B, S, H, g):
    """Key k carries the +-8 code of k in its first 9 dims, query q the code of pi(q): the score
    of (q, pi(q)) is 72 scale = 9 (x 8), every other at least 16 below.  V, dO: non-zero integers
    of magnitude 1..7."""
    bits = ((torch.arange(S)[:, None] >> torch.arange(9)[None]) & 1).float() * 16 - 8   # [S, 9]
    x = torch.zeros(B, S, 3, H, AD)
    pi = torch.stack([torch.stack([torch.randperm(S, generator=g) for _ in range(H)])
                      for _ in range(B)])                                                 # [B,H,S]
    for b in range(B):
        for h in range(H):
            x[b, :, 1, h, :9] = bits
            x[b, :, 0, h, :9] = bits[pi[b, h]]

    def ints(*shape):
        return torch.randint(1, 8, shape, generator=g).float() * \
            (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    x[:, :, 2] = ints(B, S, H, AD)
    dO = ints(B * S, H * AD)
    return x.view(B * S, 3 * H * AD).to(BF16), dO.to(BF16), pi


@pytest.mark.gpu
@pytest.mark.parametrize("S,wide,fused,keep", ATTN_PATHS)
def test_attention_gather_exact(S, wide, fused, keep):
    """One key per query leads by 16 nats: O[q] == V[pi(q)], dV[k] == dO[pi^-1(k)] exactly and
    |dQ|, |dK| < 1e-2 -- the key order shared by the two MFMA operands, checked against indices
    made here.  For S > 64 most pi(q) lie in a later key chunk than larger earlier scores, so the
    online rescale runs.  With p = 0.1 each row shows the keep decision of (q, pi(q)) taken from
    ``reference.keep_mask``: V[pi(q)] / (1 - p) within one bf16 ulp, or below 1e-4."""
    B, H, scale = 2, 3, AD ** -0.5
    g = _gen(1000 + S)
    qkv, dO, pi = _gather_inputs(B, S, H, g)
    v = _split_qkv(qkv, B, S, H)[2]                                   # [B, H, S, 64]
    dOh = _heads(dO, B, S, H)
    gat = pi[..., None].expand(B, H, S, AD)
    want_o = torch.gather(v, 2, gat)                                  # V[pi(q)]
    want_dv = torch.zeros_like(dOh).scatter_(2, gat, dOh)             # dO[pi^-1(k)]
    if S > 64:
        assert int((pi >= 64).sum()) > B * H * S // 4
    _attn_switches(wide, fused, keep)
    try:
        r = _run_attn(qkv, None, dO, B, S, H, scale, 0.0, 0)
        seed = 99 + S
        rd = _run_attn(qkv, None, dO, B, S, H, scale, 0.1, seed)
    finally:
        _attn_switches(1, 1, 1)
    tag = f"gather S={S} wide={wide} fused={fused} keep={keep}"
    assert_exact(r["out"], _rows(want_o, B, S, H), f"{tag} O")
    n = H * AD
    assert_exact(r["dqkv"][:, 2 * n:], _rows(want_dv, B, S, H), f"{tag} dV")
    assert float(r["dqkv"][:, :2 * n].float().abs().max()) < 1e-2, f"{tag}: dQ / dK not small"
    # dropout: the decision of element (q, pi(q)) of every row, and of its column in dV
    idx = (_attn_idx(B, H, S).gather(3, pi[..., None]))[..., 0]       # [B, H, S]
    kept = R.keep_mask(seed, idx, 0.1)
    ik = _inv_keep(0.1)
    for name, got, want, kk in (
            ("O", _heads(rd["out"], B, S, H), want_o, kept),
            ("dV", _heads(rd["dqkv"][:, 2 * n:], B, S, H), want_dv,
             torch.zeros_like(kept).scatter_(2, pi, kept))):
        k4 = kk[..., None].expand_as(want)
        assert_within(got[k4], want[k4] * ik, 2 * U16 * (want[k4] * ik).abs(), f"{tag} p=0.1 kept {name}")
        assert float(got[~k4].abs().max()) < 1e-4, f"{tag} p=0.1: dropped {name} row not ~0"
    assert 0.05 < 1 - float(kept.float().mean()) < 0.15


def test_attention_bound_accepts_emulation_and_rejects_damage():
    """The emulation of the forward's rounding points lies inside the bound; the softmax scale
    x 1.01, one more key masked, the missing 1 / (1 - p) and one output row 2 % low lie outside."""
    B, H, S, scale = 2, 3, 192, AD ** -0.5
    g = _gen(6)
    qkv, _, mask = _attn_inputs(B, S, H, g, masked=True)
    for p, seed in ((0.0, 0), (0.1, 31)):
        o = attn_fwd_oracle(qkv, mask, B, S, H, scale, p, seed)
        out = attn_fwd_emulate(qkv, mask, B, S, H, scale, p, seed)
        assert_within(out, *o["out"], f"emulated forward p={p}")
        print(f"emulation / bound p={p}: {_ratio(out, *o['out']):.3f}")
        with pytest.raises(AssertionError, match="outside the bound"):
            assert_within(attn_fwd_emulate(qkv, mask, B, S, H, scale * 1.01, p, seed), *o["out"])
        m2 = mask.clone()
        m2[0, 17] = -10000.0
        with pytest.raises(AssertionError, match="outside the bound"):
            assert_within(attn_fwd_emulate(qkv, m2, B, S, H, scale, p, seed), *o["out"])
        low = out.clone()
        low[S + 5] = (low[S + 5].float() * 0.98).to(BF16)
        with pytest.raises(AssertionError, match=rf"{H * AD} of {B * S * H * AD} "):
            assert_within(low, *o["out"], "row 2 % low")
    norescale = attn_fwd_emulate(qkv, mask, B, S, H, scale, 0.1, 31, rescale=False)
    err = (norescale.double() - o["out"][0]).abs()
    assert bool((err > o["out"][1]).all()), "a missing 1 / (1 - p) must fail every element"


def test_attention_exact_constructions_on_the_cpu():
    """The gather and uniform inputs give exact results under the emulation too (the margins of
    16 nats and of sums below 256 hold), and a swapped key pair is seen."""
    B, H, S = 2, 3, 192
    g = _gen(2)
    qkv, _, pi = _gather_inputs(B, S, H, g)
    out = attn_fwd_emulate(qkv, None, B, S, H, AD ** -0.5, 0.0, 0)
    v = _split_qkv(qkv, B, S, H)[2]
    want = _rows(torch.gather(v, 2, pi[..., None].expand(B, H, S, AD)), B, S, H)
    assert_exact(out, want, "gather")
    pi2 = pi.clone()
    pi2[1, 2, [3, 4]] = pi[1, 2, [4, 3]]
    with pytest.raises(AssertionError, match="differ"):
        assert_exact(out, _rows(torch.gather(v, 2, pi2[..., None].expand(B, H, S, AD)), B, S, H))
