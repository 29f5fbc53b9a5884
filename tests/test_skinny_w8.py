"""FP8 weights for the skinny-M dense kernel off the device: the rule, the reference path of a
decode step, the refusals that need no device (the kernels: tests/test_skinny_w8_gpu.py)."""
import copy

import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining, KVCache
from distributedtensorflow_amd.ops import reference
from test_dense_skinny import TINY


def test_weight_quantize_fp8_is_the_rule_on_the_bf16_weight():
    w = torch.randn(16, 128, generator=torch.Generator().manual_seed(0))
    q, s = ops.weight_quantize_fp8(w)
    want_q, want_s = reference.kv_quantize_rows(w.to(torch.bfloat16).view(16, 2, 64))
    assert q.shape == (16, 128) and q.dtype == torch.float8_e4m3fn and s.shape == (16, 2)
    assert torch.equal(q.view(torch.int8), want_q.view(16, 128).view(torch.int8))
    assert torch.equal(s, want_s)
    x = torch.randn(3, 128)
    assert torch.equal(ops.dense(x, (q, s)), reference.dense(x, reference.weight_dequantize((q, s))))


@pytest.mark.parametrize("case", ["scale_shape", "scale_dtype", "q_strided", "k_not_64"])
def test_refusals(case):
    q, s = ops.weight_quantize_fp8(torch.randn(16, 128))
    with pytest.raises(ValueError):
        if case == "k_not_64":
            ops.weight_quantize_fp8(torch.randn(16, 96))
        pair = {"scale_shape": (q, s[:, :1].contiguous()), "scale_dtype": (q, s.double()),
                "q_strided": (q.t().contiguous().t(), s)}[case]
        ops.dense(torch.randn(3, 128), pair, impl="skinny")


def test_cpu_decode_step_on_fp8_weights_equals_the_step_on_the_dequantised_weights():
    torch.manual_seed(0)
    model = BertForPreTraining(BertConfig(**TINY)).eval()
    cache = KVCache(model.cfg, 2, 32, "cpu", torch.float32)
    ids = torch.tensor([7, 9])
    with pytest.raises(ValueError, match="quantize_weights"):
        model.decode_step(ids, cache, gemm="skinny_w8")
    with torch.no_grad():      # the tied table is also the lookup's: one that FP8 holds exactly
        model.word_embeddings.copy_(reference.weight_dequantize(
            ops.weight_quantize_fp8(model.word_embeddings)))
    twin = copy.deepcopy(model.quantize_weights())
    with torch.no_grad():
        for p, p2 in zip(model._w8_params(), twin._w8_params()):
            p2.copy_(reference.weight_dequantize(p._dtf_w8))
    prompt = torch.randint(1, 256, (2, 12), generator=torch.Generator().manual_seed(1))
    model.prefill(prompt, torch.tensor([5, 12]), cache)
    for g in ("skinny", "skinny_ln"):
        got = model.decode_step(ids, copy.deepcopy(cache), gemm=g + "_w8")
        assert torch.equal(got, twin.decode_step(ids, copy.deepcopy(cache), gemm=g))
    assert model.generate(prompt, torch.tensor([5, 12]), 3, decode_gemm="skinny_w8").shape == (2, 3)
