"""The masked-LM example kernel (csrc/kernels/mlm_mask.hip) against ops/reference.py on the CPU,
bit for bit on all six outputs: both storage widths, every sequence-length path (one partial
group, whole groups, a partial last group, all eight groups), blocks that take several trips,
row offsets past 2 GiB, the DeviceTokenDataset on the device against the same dataset on the
host, a tiny BERT trained and evaluated from it, the word-embedding gradient on the long runs of
equal ids that real batches hold, and train.py --text_data."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distributedtensorflow_amd as dtf
from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import DeviceTokenDataset, TokenMasking
from distributedtensorflow_amd.metrics import ClassificationMetrics
from distributedtensorflow_amd.ops import native, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")
KEYS = ("input_ids", "segment_ids", "input_mask", "masked_lm_positions", "masked_lm_ids",
        "masked_lm_weights")
PAD, CLS, SEP = 0, 101, 102


def _rows(S, vocab=30522, seed=0):
    """Rows that hit every branch of the rule -> int64 [9, S]: 0 full, 1 padded, 2 [CLS] [SEP]
    pad... (nc = 0), 3 nc = 1, 4 nc = 3, 5 no sep, 6 two sep, 7 ids from the top of the
    vocabulary, 8 specials and a pad inside the row."""
    g = torch.Generator().manual_seed(1000 + S + seed)

    def words(k):
        return torch.randint(1000, vocab, (k,), generator=g).tolist()

    def fit(body):
        body = body[:S]
        return body + [PAD] * (S - len(body))

    half = max(1, S // 2 - 2)
    return torch.tensor([
        fit([CLS] + words(half) + [SEP] + words(S)[:S - half - 3] + [SEP]),
        fit([CLS] + words(max(1, S // 3)) + [SEP] + words(1) + [SEP]),
        fit([CLS, SEP]),
        fit([CLS] + words(1) + [SEP]),
        fit([CLS] + words(3) + [SEP]),
        fit([CLS] + words(S - 2)),
        fit([CLS] + words(1) + [SEP] + words(2) + [SEP]),
        fit([CLS] + [vocab - 1, vocab - 2] * S),
        fit([CLS, SEP, CLS] + words(2) + [PAD] + words(2) + [SEP]),
    ], dtype=torch.int64)


def _store(rows, dtype):
    if dtype == torch.int32:
        return rows.to(torch.int32)
    u16 = rows.numpy().astype(np.uint16)
    return torch.from_numpy(u16 if dtype == torch.uint16 else u16.view(np.int16))


def _run_gpu(tokens, idx, seed, P, m, *extra, **kw):
    fn = native.mlm_mask_tokens if kw else ops.mlm_mask_tokens
    out = fn(tokens.cuda(), idx.cuda(), seed, P, m, *extra, **kw)
    for k in KEYS:
        assert out[k].is_cuda and out[k].is_contiguous(), k
    return {k: v.cpu() for k, v in out.items()}


def _assert_same(got, want):
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int16, torch.int32],
                         ids=["uint16", "int16", "int32"])
@pytest.mark.parametrize("S", [8, 64, 72, 128, 512])
def test_kernel_equals_reference(S, dtype):
    m = TokenMasking(vocab_size=50000, random_low=999)          # ids of 32768 and more
    tokens = _store(_rows(S, vocab=50000), dtype)
    assert int(_rows(S, vocab=50000).max()) >= 32768
    for idx in (torch.tensor([8, 0, 3, 2, 3]),                  # B = 5, repeated, unordered
                torch.tensor([1, 7, 9, 4, 6]),                  # 9: outside the set
                torch.tensor([5, -1, 6, 2, 0])):
        for P in (1, 20, 76):
            if P > S:
                continue
            want = reference.mlm_mask_tokens(tokens, idx, 12345, P, m)
            _assert_same(_run_gpu(tokens, idx, 12345, P, m), want)
    # T = P on a long row; a shard's example numbers; a high masking rate
    P = min(S, 76)
    dense = TokenMasking(vocab_size=50000, prob=0.9)
    idx = torch.arange(9)
    want = reference.mlm_mask_tokens(tokens, idx, 4000000000, P, dense, 3, 2)
    _assert_same(_run_gpu(tokens, idx, 4000000000, P, dense, 3, 2), want)
    nc = S - 2                                                   # row 5: [CLS], S - 2 words, a pad
    assert want["masked_lm_weights"][5].sum() == min(P, nc, max(1, (58982 * nc + 32768) >> 16))


def _random_rows(N, S, seed, shortest=6):
    rng = np.random.RandomState(seed)
    rows = np.zeros((N, S), dtype=np.uint16)
    for r in range(N):
        L = rng.randint(shortest, S + 1)
        rows[r, :L] = rng.randint(1000, 30522, L)
        rows[r, 0], rows[r, rng.randint(2, L - 2)], rows[r, L - 1] = CLS, SEP, SEP
    return rows


@pytest.mark.parametrize("S,P", [(128, 20), (72, 11), (512, 76)])
def test_several_trips_equal_the_default_launch(S, P):
    m = TokenMasking()
    tokens = torch.from_numpy(_random_rows(40, S, seed=S))
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 40, (64,), generator=g)               # B = 64: 16 blocks of 4 rows
    want = reference.mlm_mask_tokens(tokens, idx, 777, P, m)
    _assert_same(_run_gpu(tokens, idx, 777, P, m), want)
    _assert_same(_run_gpu(tokens, idx, 777, P, m, max_blocks=2), want)
    _assert_same(_run_gpu(tokens, idx, 777, P, m, max_blocks=1), want)


def test_addressing_past_2_gib():
    S = 512
    N = (1 << 21) + 4096                                         # x 512 x 2 B = 2 GiB + 4 MiB
    tokens = torch.empty(N, S, dtype=torch.int16, device="cuda")
    assert tokens.numel() * 2 > (1 << 31) and (N - 1) * S * 2 > (1 << 31)
    small = torch.from_numpy(_random_rows(2, S, seed=9).view(np.int16))
    tokens[0].copy_(small[0])
    tokens[N - 1].copy_(small[1])
    m = TokenMasking()
    idx = torch.tensor([N - 1, 0, N, N - 1])                     # N: one past the set
    got = {k: v.cpu() for k, v in ops.mlm_mask_tokens(tokens, idx.cuda(), 31337, 76, m).items()}
    # the same rows in a 2-row set, the example numbers carried over: local row 1 is example N - 1
    want = reference.mlm_mask_tokens(small, torch.tensor([1, 0, 2, 1]), 31337, 76, m, N - 1, 0)
    _assert_same(got, want)
    assert want["masked_lm_weights"][2].sum() == 0 and want["masked_lm_weights"][0].sum() > 0
    del tokens
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [np.uint16, np.int32], ids=["uint16", "int32"])
def test_device_dataset_equals_the_cpu_dataset(dtype):
    toks = _random_rows(23, 64, seed=3).astype(dtype)
    kw = dict(max_predictions=9, seed=1, mask_seed=2, eval_seed=5, num_shards=2, shard_index=1)
    cpu = DeviceTokenDataset(toks, 5, "cpu", **kw)
    gpu = DeviceTokenDataset(toks, 5, "cuda", chunk_bytes=3 * 64 * toks.itemsize, **kw)
    assert gpu.tokens.is_cuda and torch.equal(gpu.tokens.cpu(), cpu.tokens) and gpu.n == 11
    for _ in range(5):                                           # over two epoch boundaries
        bc, bg = next(cpu), next(gpu)
        assert bg["input_ids"].is_cuda and bg["input_ids"].shape == (5, 64)
        _assert_same({k: v.cpu() for k, v in bg.items()}, bc)
    assert cpu.epoch == gpu.epoch == 2
    passes = list(zip(cpu.single_pass(), gpu.single_pass()))
    assert [len(c["input_ids"]) for c, _ in passes] == [5, 5, 1]
    for bc, bg in passes:
        _assert_same({k: v.cpu() for k, v in bg.items()}, bc)


@pytest.fixture(scope="module")
def tiny_bert_runs(tmp_path_factory):
    """Two LAMB steps of a tiny BERT from a DeviceTokenDataset and two evaluations after them,
    once with a further evaluation between the steps and once without ->
    {between: (parameters, training batches, evaluation results, sum of validation weights)}."""
    from distributedtensorflow_amd.data import load_token_arrays
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    from distributedtensorflow_amd.optimizers import LAMBOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    tmp_path = tmp_path_factory.mktemp("tokens")
    tiny = dict(vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                intermediate_size=512, max_position_embeddings=128)
    rng = np.random.RandomState(0)
    for split, n in (("train", 24), ("val", 10)):
        rows = _random_rows(n, 64, seed=n, shortest=20)
        body = (rows != PAD) & (rows != CLS) & (rows != SEP)
        rows[body] = rng.randint(200, 1000, int(body.sum()))     # inside the tiny vocabulary
        np.save(tmp_path / f"{split}_tokens.npy", rows)
    with open(tmp_path / "meta.json", "w") as f:
        json.dump({"vocab_size": 1000}, f)

    def run(evaluate_between):
        toks, masking = load_token_arrays(str(tmp_path), "train")
        train = DeviceTokenDataset(toks, 8, "cuda", masking, max_predictions=10, shuffle=True,
                                   mask_seed=1)
        toks, masking = load_token_arrays(str(tmp_path), "val")
        val = DeviceTokenDataset(toks, 4, "cuda", masking, max_predictions=10, eval_seed=3)
        assert train.masking.vocab_size == 1000
        torch.manual_seed(0)
        results, batches = [], []
        with OneDeviceStrategy("cuda").scope():
            model = BertForPreTraining(BertConfig(**tiny)).cuda()
            opt = LAMBOptimizer(1e-3)
            opt.build(list(model.parameters()))
            for step in range(2):
                b = next(train)
                batches.append({k: v.clone() for k, v in b.items()})
                loss = model(b["input_ids"], b["segment_ids"], b["input_mask"],
                             b["masked_lm_positions"], b["masked_lm_ids"], b["masked_lm_weights"])
                opt.minimize(loss)
                assert math.isfinite(float(loss))
                if step == 0 and evaluate_between:
                    results.append(dtf.train.evaluate(model, val.single_pass(),
                                                      ClassificationMetrics(k=5), optimizer=opt))
            for _ in range(2):
                results.append(dtf.train.evaluate(model, val.single_pass(),
                                                  ClassificationMetrics(k=5), optimizer=opt))
        weights = sum(float(b["masked_lm_weights"].sum()) for b in val.single_pass())
        return [p.detach().clone() for p in model.parameters()], batches, results, weights

    return {between: run(between) for between in (True, False)}


def test_tiny_bert_trains_and_evaluates_on_a_token_set(tiny_bert_runs):
    for between, (_, batches, results, weights) in tiny_bert_runs.items():
        assert weights > 0 and len(results) == (3 if between else 2)
        for r in results:
            assert math.isfinite(r["loss"]) and r["count"] == weights
            assert 0.0 <= r["top_1"] <= r["top_k"] <= 1.0
        assert results[-1] == results[-2]                         # a second evaluation repeats
    # the evaluation between the steps took nothing from the training stream
    for ba, bb in zip(tiny_bert_runs[True][1], tiny_bert_runs[False][1]):
        _assert_same(ba, bb)


def test_an_evaluation_between_two_lamb_steps_leaves_the_parameters_bit_identical(tiny_bert_runs):
    """The evaluation takes nothing from the training stream and draws no dropout seed, and the
    LAMB update sums its trust-ratio norms in a fixed order (csrc/kernels/optim.hip), so the two
    runs end with the same bits.  (With float atomics in those norms 7 to 9 of the 34 tensors
    differed by one fp32 ulp, 3.725e-09, between any two runs.)"""
    for pa, pb in zip(tiny_bert_runs[True][0], tiny_bert_runs[False][0]):
        assert torch.equal(pa, pb)


def test_word_embedding_gradient_sums_long_runs_in_run_order():
    """A token set repeats [MASK], [PAD] and [SEP] thousands of times per batch; the segment sum
    keeps many rows of such a run in flight and still adds them in run order: equal, bit for bit,
    to a sequential fp32 sum, for runs on both sides of its look-ahead of 16 rows."""
    H = 260                                                      # a second, partial column chunk
    runs = [1, 15, 16, 17, 2, 33, 1, 2500, 48, 5]
    ids = torch.cat([torch.full((n,), 7 * k + 3) for k, n in enumerate(runs)])
    T, V = len(ids), 7 * len(runs)
    g = torch.Generator().manual_seed(0)
    ids = ids[torch.randperm(T, generator=g)]
    src = torch.randn(T, H, generator=g).bfloat16()
    sorted_ids, perm = torch.sort(ids, stable=True)
    want = torch.zeros(V, H)
    rows = src.float()
    for j in range(T):                                           # one fp32 add per row, in order
        want[sorted_ids[j]] += rows[perm[j]]
    out = torch.zeros(V, H, device="cuda")
    src_gpu, sorted_gpu, perm_gpu = src.cuda(), sorted_ids.cuda(), perm.cuda()
    native.kernels().segment_sum(sorted_gpu.data_ptr(), perm_gpu.data_ptr(), src_gpu.data_ptr(),
                                 out.data_ptr(), T, H, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(out.cpu(), want)


def _env():
    e = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        e.pop(k, None)
    return e


def test_cli_text_data_bert_base(tmp_path):
    d = tmp_path / "set"
    d.mkdir()
    np.save(d / "train_tokens.npy", _random_rows(16, 64, seed=1, shortest=20))
    np.save(d / "val_tokens.npy", _random_rows(16, 64, seed=2, shortest=20))
    r = subprocess.run([sys.executable, TRAIN, "--model", "bert_base", "--text_data", str(d),
                        "--batch_size", "4", "--max_steps", "2", "--log_dir", str(tmp_path / "tb"),
                        "--eval"], capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["global_step"] == 2 and math.isfinite(res["final_loss"])
    assert math.isfinite(res["eval_loss"]) and 0.0 <= res["eval_top_1"] <= 1.0
    val = DeviceTokenDataset(_random_rows(16, 64, seed=2, shortest=20), 16, "cpu")
    assert res["eval_count"] == int(next(iter(val.single_pass()))["masked_lm_weights"].sum())
    # a sequence length the attention kernel cannot take is refused with a message
    from distributedtensorflow_amd import cli
    np.save(d / "train_tokens.npy", _random_rows(16, 72, seed=1, shortest=20))
    args = cli.build_parser().parse_args(["--model", "bert_base", "--text_data", str(d)])
    with pytest.raises(SystemExit, match="multiple of 64"):
        cli._token_dataset(args, "train", 4, torch.device("cuda"), 1, 0)
    assert cli._token_dataset(args, "train", 4, torch.device("cpu"), 1, 0).seq_len == 72
