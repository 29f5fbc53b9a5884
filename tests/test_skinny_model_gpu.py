"""A decode step of the model on the skinny-M dense kernel (csrc/kernels/dense_skinny.hip) against
the default step.  The kernel's own tests are in tests/test_skinny_dense_gpu.py.  Both files are
named to sort after tests/test_resnet_gpu.py, whose ``test_no_record_outlives_its_step`` compares
``max_memory_allocated`` between steps to within 8 MB and measured 8.4 MB with these tests ahead
of it in the process.

Measured on an MI355X: see profiles/SKINNY.md.
"""
import copy

import pytest
import torch

from test_decode_gpu import TINY
from test_nlp_kernels_gpu import _gen


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.gpu
def test_decode_steps_with_skinny_gemms_match_the_default_steps():
    """Teacher-forced decode steps with gemm="skinny" against decode_step() on the same cache
    contents, under the tolerance rule of tests/test_decode_gpu.py: twice the bf16 forward's own
    distance to the fp32 CPU result."""
    from distributedtensorflow_amd.models import KVCache
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    cpu = BertForPreTraining(BertConfig(**TINY)).eval()
    gpu = copy.deepcopy(cpu).cuda().eval()
    lens, steps = torch.tensor([5, 64]), 4
    prompt = torch.randint(1, 256, (2, 64), generator=_gen(3))
    prompt = prompt * (torch.arange(64).view(1, 64) < lens.view(2, 1))
    gen = gpu.generate(prompt.cuda(), lens, steps).cpu()
    assert torch.equal(gpu.generate(prompt.cuda(), lens, steps, decode_gemm="default").cpu(), gen)
    seq = torch.zeros(2, 128, dtype=torch.int64)
    seq[:, :64] = prompt
    for r in range(2):
        seq[r, lens[r]:lens[r] + steps] = gen[r]
    at = lens.view(2, 1) + torch.arange(steps).view(1, -1)            # positions of the steps
    with torch.no_grad():
        diff = (gpu(seq.cuda()).float().cpu() - cpu(seq)).view(2, 128, -1)
        tol = 2 * float(diff[torch.arange(2).view(2, 1), at].abs().max())
    cache = KVCache(gpu.cfg, 2, 128, "cuda")
    gpu.prefill(prompt.cuda(), lens, cache)
    err = 0.0
    for t in range(steps):
        twin = copy.deepcopy(cache)                                   # the same cache contents
        ref = gpu.decode_step(gen[:, t].cuda(), cache)
        got = gpu.decode_step(gen[:, t].cuda(), twin, gemm="skinny")
        assert got.shape == ref.shape
        err = max(err, float((got.float() - ref.float()).abs().max()))
    print(f"MEASURE skinny-vs-default decode / tolerance {err / tol:.4f} (tolerance {tol:.4f})")
    assert err <= tol
    # the whole loop through generate, and a chunked prefill whose 2 x 16 rows qualify
    out = gpu.generate(prompt.cuda(), lens, steps, decode_gemm="skinny", prefill_chunk=16)
    assert out.shape == (2, steps)
