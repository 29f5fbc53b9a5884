"""The skinny-M dense option off the device: the reference path ignores ``impl="skinny"``,
``generate(decode_gemm=...)`` on the CPU, and the CLI flag."""
import pytest
import torch

from distributedtensorflow_amd import cli, ops
from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
from distributedtensorflow_amd.ops import reference

TINY = dict(vocab_size=256, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
            intermediate_size=512, max_position_embeddings=128, causal=True)


def test_reference_path_ignores_the_skinny_impl():
    g = torch.Generator().manual_seed(0)
    x, w1, b1 = torch.randn(5, 64, generator=g), torch.randn(48, 64, generator=g), torch.randn(48)
    w2 = torch.randn(16, 48, generator=g)
    assert torch.equal(ops.dense(x, w1, b1, impl="skinny"), reference.dense(x, w1, b1))
    want = reference.dense(reference.bias_gelu(reference.dense(x, w1), b1), w2)
    assert torch.equal(ops.dense_gelu_dense(x, w1, b1, w2, impl="skinny"), want)


def test_generate_on_the_cpu_returns_the_same_tokens_with_decode_gemm():
    torch.manual_seed(0)
    model = BertForPreTraining(BertConfig(**TINY)).eval()
    prompt = torch.randint(1, 256, (2, 12), generator=torch.Generator().manual_seed(1))
    lens = torch.tensor([5, 12])
    want = model.generate(prompt, lens, 6)
    assert torch.equal(model.generate(prompt, lens, 6, decode_gemm="skinny"), want)
    assert torch.equal(model.generate(prompt, lens, 6, decode_gemm="skinny", prefill_chunk=4),
                       model.generate(prompt, lens, 6, prefill_chunk=4))
    with pytest.raises(ValueError, match="gemm"):
        model.generate(prompt, lens, 6, decode_gemm="thin")


def test_cli_flag():
    p = cli.build_parser()
    assert p.parse_args(["--model", "bert_base"]).generate_decode_gemm == "default"
    args = p.parse_args(["--model", "bert_base", "--generate_decode_gemm", "skinny"])
    assert args.generate_decode_gemm == "skinny"
    with pytest.raises(SystemExit):
        p.parse_args(["--model", "bert_base", "--generate_decode_gemm", "thin"])
