"""The deferred LayerNorm of the skinny-M dense kernel off the device: the reference rule, the
refusals, the CLI value and a CPU decode step (the kernel: tests/test_skinny_ln_gpu.py)."""
import copy

import pytest
import torch

from distributedtensorflow_amd import cli, ops
from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining, KVCache
from distributedtensorflow_amd.ops import reference
from test_dense_skinny import TINY


def _operands(dtype):
    g = torch.Generator().manual_seed(0)
    x, r = (3 + torch.randn(5, 64, generator=g)).to(dtype), torch.randn(5, 48, generator=g).to(dtype)
    w1, b1 = torch.randn(48, 64, generator=g), torch.randn(48, generator=g)
    w2, b2 = torch.randn(64, 48, generator=g), torch.randn(64, generator=g)
    ln = lambda n: (1 + 0.1 * torch.randn(n, generator=g), torch.randn(n, generator=g), 1e-12)
    return x, r, w1, b1, w2, b2, ln(64), ln(48)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_ops_are_the_composition(dtype):
    """lnb = layer_norm rounded to the activation dtype; the residual joins the fp32 sum, so the
    result rounds once."""
    x, r, w1, b1, w2, b2, ln_x, ln_r = _operands(dtype)
    lnx, lnr = reference.layer_norm(x, *ln_x), reference.layer_norm(r, *ln_r)
    assert torch.equal(ops.dense(x, w1, b1, impl="skinny", pre_ln=ln_x), reference.dense(lnx, w1, b1))
    acc = torch.nn.functional.linear(x.float(), w1.to(dtype).float(), b1)
    assert torch.equal(ops.dense(x, w1, b1, impl="skinny", residual=r), (acc + r.float()).to(dtype))
    assert torch.equal(ops.dense(x, w1, b1, impl="skinny", residual=r, residual_ln=ln_r),
                       (acc + lnr.float()).to(dtype))
    h = reference.bias_gelu(reference.dense(lnx, w1), b1)
    want = (torch.nn.functional.linear(h.float(), w2.to(dtype).float(), b2) + lnx.float()).to(dtype)
    got = ops.dense_gelu_dense(x, w1, b1, w2, impl="skinny", pre_ln=ln_x, b2=b2, residual=x,
                               residual_ln=ln_x)
    assert torch.equal(got, want)


def test_refusals():
    x, r, w1, b1, _, _, ln_x, ln_r = _operands(torch.float32)
    with pytest.raises(ValueError, match="both"):
        ops.dense(x, w1, b1, impl="skinny", pre_ln=ln_x, residual=r, residual_ln=ln_r)
    with pytest.raises(ValueError, match="activation"):             # residual with GELU
        reference.deferred_ln_check(None, r, None, gelu=True)
    with pytest.raises(ValueError, match="needs the residual"):
        ops.dense(x, w1, b1, impl="skinny", residual_ln=ln_r)
    native = pytest.importorskip("distributedtensorflow_amd.ops.native")
    with pytest.raises(ValueError, match="impl='skinny'"):
        native.dense(x, w1, b1, impl="library", pre_ln=ln_x)
    with pytest.raises(ValueError, match="impl='skinny'"):
        native.dense_gelu_dense(x, w1, b1, w1, residual=r)


def test_cli_value():
    p = cli.build_parser()
    args = p.parse_args(["--model", "bert_base", "--generate_decode_gemm", "skinny_ln"])
    assert args.generate_decode_gemm == "skinny_ln"
    with pytest.raises(SystemExit):
        p.parse_args(["--model", "bert_base", "--generate_decode_gemm", "thin"])


def test_cpu_decode_and_extend_with_deferred_layer_norms_match_the_default():
    torch.manual_seed(0)
    model = BertForPreTraining(BertConfig(**TINY)).eval()
    with torch.no_grad():                         # LayerNorms that are not the identity
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    prompt = torch.randint(1, 256, (2, 12), generator=torch.Generator().manual_seed(1))
    lens = torch.tensor([5, 12])
    cache = KVCache(model.cfg, 2, 32, "cpu", torch.float32)
    model.prefill(prompt, lens, cache)
    for ids in (torch.tensor([7, 9]), torch.tensor([[3, 4, 5], [6, 7, 8]])):
        step = model.decode_step if ids.dim() == 1 else model.extend
        twin = copy.deepcopy(cache)
        want, got = step(ids, cache), step(ids, twin, gemm="skinny_ln")
        assert float((got - want).abs().max()) <= 1e-5
    assert torch.equal(model.generate(prompt, lens, 4, decode_gemm="skinny_ln", prefill_chunk=4),
                       model.generate(prompt, lens, 4, prefill_chunk=4))
    with pytest.raises(ValueError, match="gemm"):
        model.generate(prompt, lens, 4, decode_gemm="thin")
