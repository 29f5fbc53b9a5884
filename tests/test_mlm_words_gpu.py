"""The whole-word instantiation of the masked-LM example kernel (csrc/kernels/mlm_mask.hip)
against ops/reference.py on the CPU, bit for bit on all six outputs: the rows built for every
branch of the rule at every sequence-length path and storage width, the all-zero table against
the token kernel, blocks that take several trips (the per-wave LDS slices carry nothing from row
to row), the DeviceTokenDataset on the device against the same dataset on the host, and
train.py --text_data --whole_word_mask --eval.  The whole-word kernel shares the token kernel's
row addressing and output stage, which test_mlm_data_gpu.py covers past 2 GiB."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import ops
from distributedtensorflow_amd.data import DeviceTokenDataset, TokenMasking
from distributedtensorflow_amd.ops import native, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "train.py")
KEYS = ("input_ids", "segment_ids", "input_mask", "masked_lm_positions", "masked_lm_ids",
        "masked_lm_weights")
PAD, CLS, SEP = 0, 101, 102
VOCAB, FIRST_PIECE = 50000, 40000     # ids of 40000 and more are continuation pieces
FLAGGED_FROM = 24722                   # of a vocabulary of 30522: 19 %


def _table(vocab=VOCAB, first_piece=FIRST_PIECE):
    t = torch.zeros(vocab, dtype=torch.uint8)
    t[first_piece:] = 1
    return t


def _rows(S):
    """Rows that hit every branch of the whole-word rule -> int64 [9, S]:
    0 a full row of one-token words with a word over positions 62..65 (S > 65), one over
      126..128 (S > 128) and one that ends at S - 1
    1 a continuation piece at j = 0 of a row with no [CLS], and one right after [SEP]
    2 a continuation piece right after [CLS]
    3 one word of nc pieces, nc > T: nothing fits
    4 three words of 4 pieces and 8 of one: T = 3 at prob 0.15, the long words are skipped
    5 [CLS] [SEP] pad...: no candidate
    6 a word of 2 pieces in the second segment
    7 specials and a pad inside the row; the piece after the pad starts a word
    8 words of 3 pieces only: a word fits a budget of 3 exactly"""
    g = torch.Generator().manual_seed(2000 + S)

    def head(k=1):
        return torch.randint(1000, FIRST_PIECE, (k,), generator=g).tolist()

    def piece(k=1):
        return torch.randint(FIRST_PIECE, VOCAB, (k,), generator=g).tolist()

    def word(k):
        return head() + piece(k - 1)

    def fit(body):
        body = body[:S]
        return body + [PAD] * (S - len(body))

    full = [CLS] + head(S - 1)
    full[S // 4 + 1] = SEP
    runs = [(S - 2, S)] + ([(63, 66)] if S > 65 else []) + ([(127, 129)] if S > 128 else [])
    for lo, hi in runs:
        full[lo:hi] = piece(hi - lo)
    return torch.tensor([
        full,
        fit(piece(2) + head() + piece() + [SEP] + piece() + head() + [SEP]),
        fit([CLS] + piece(2) + head() + [SEP] + head() + piece() + [SEP]),
        fit([CLS] + word(min(S - 2, 40)) + [SEP]),
        fit([CLS] + word(4) + head(3) + word(4) + head(2) + [SEP] + head(3) + word(4) + [SEP]),
        fit([CLS, SEP]),
        fit([CLS] + head() + [SEP] + word(2) + [SEP]),
        fit([CLS, SEP, CLS] + word(2) + [PAD] + piece() + head() + [SEP]),
        fit([CLS] + word(3) + word(3) + [SEP] + word(3) * (S // 8) + [SEP]),
    ], dtype=torch.int64)


def _store(rows, dtype):
    if dtype == torch.int32:
        return rows.to(torch.int32)
    u16 = rows.numpy().astype(np.uint16)
    return torch.from_numpy(u16 if dtype == torch.uint16 else u16.view(np.int16))


def _run_gpu(tokens, idx, seed, P, m, *extra, continuation=None, **kw):
    fn = native.mlm_mask_tokens if kw else ops.mlm_mask_tokens
    table = None if continuation is None else continuation.cuda()
    out = fn(tokens.cuda(), idx.cuda(), seed, P, m, *extra, continuation=table, **kw)
    for k in KEYS:
        assert out[k].is_cuda and out[k].is_contiguous(), k
    return {k: v.cpu() for k, v in out.items()}


def _assert_same(got, want):
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


IDX = torch.tensor([8, 0, 3, 2, 3, 1, 7, 4, 6, 5, 9, -1, 2])     # repeated, unordered, 2 outside


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int16, torch.int32],
                         ids=["uint16", "int16", "int32"])
@pytest.mark.parametrize("S", [8, 64, 72, 128, 512])
def test_kernel_equals_reference(S, dtype):
    m = TokenMasking(vocab_size=VOCAB, random_low=999)
    rows = _rows(S)
    assert int(rows.max()) >= 32768
    tokens, cont = _store(rows, dtype), _table()
    for P, seed, mm, stride, offset in (
            (min(20, S), 12345, m, 1, 0), (2, 7, m, 3, 2), (1, 0, m, 1, 0),
            (min(20, S), 99, m.replace(prob=0.5), 1 << 33, 5),
            (min(76, S), 8, m.replace(prob=0.9), 1, 0),
            (S, 4000000000, m.replace(prob=1.0), 1, 0),           # T == nc
            (2, 31, m.replace(prob=1.0), 1, 0),                   # P below the budget
            (3, 5, m.replace(prob=0.4), 1, 0)):
        want = reference.mlm_mask_tokens(tokens, IDX, seed, P, mm, stride, offset,
                                         continuation=cont)
        _assert_same(_run_gpu(tokens, IDX, seed, P, mm, stride, offset, continuation=cont), want)
    # a bool table is the same table
    _assert_same(_run_gpu(tokens, IDX, 5, 3, m.replace(prob=0.4), continuation=cont.bool()), want)
    # row 3 is one word longer than its budget: nothing to predict, the row is a copy
    out = _run_gpu(tokens, torch.tensor([3]), 12345, min(20, S), m, continuation=cont)
    assert out["masked_lm_weights"].sum() == 0 and torch.equal(out["input_ids"][0], rows[3])


def _word_rows(N, S, seed, shortest=6, vocab=30522, flagged_from=FLAGGED_FROM):
    """[CLS] a [SEP] b [SEP] pad... rows whose text is words of 1 / 2 / 3 / 4 pieces with
    probability .7 / .2 / .07 / .03 -> uint16 numpy [N, S]."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((N, S), dtype=np.uint16)
    for r in range(N):
        L = rng.randint(shortest, S + 1)
        body = []
        while len(body) < L:
            k = rng.choice(4, p=[.7, .2, .07, .03]) + 1
            body += [rng.randint(1000, flagged_from)] + list(rng.randint(flagged_from, vocab, k - 1))
        rows[r, :L] = body[:L]
        rows[r, 0], rows[r, rng.randint(2, L - 2)], rows[r, L - 1] = CLS, SEP, SEP
    return rows


def test_all_zero_table_is_the_token_kernel():
    m = TokenMasking()
    zero = torch.zeros(30522, dtype=torch.uint8)
    for S, P in ((128, 20), (72, 11)):
        tokens = torch.from_numpy(_word_rows(64, S, seed=S))
        idx = torch.arange(64)
        want = _run_gpu(tokens, idx, 777, P, m)
        _assert_same(_run_gpu(tokens, idx, 777, P, m, continuation=zero), want)
        some = _run_gpu(tokens, idx, 777, P, m, continuation=_table(30522, FLAGGED_FROM))
        assert not torch.equal(some["masked_lm_positions"], want["masked_lm_positions"])


@pytest.mark.parametrize("S,P", [(128, 20), (72, 11), (512, 76)])
def test_several_trips_equal_the_default_launch(S, P):
    m = TokenMasking()
    cont = _table(30522, FLAGGED_FROM)
    tokens = torch.from_numpy(_word_rows(40, S, seed=S))
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 40, (300,), generator=g)              # B = 300: 75 blocks of 4 rows
    want = reference.mlm_mask_tokens(tokens, idx, 777, P, m, continuation=cont)
    assert 0 < float((want["masked_lm_weights"].sum(1) < P).float().mean())   # rows differ in T'
    default = _run_gpu(tokens, idx, 777, P, m, continuation=cont)
    _assert_same(default, want)
    _assert_same(_run_gpu(tokens, idx, 777, P, m, continuation=cont, max_blocks=3), default)
    _assert_same(_run_gpu(tokens, idx, 777, P, m, continuation=cont, max_blocks=1), default)


@pytest.mark.parametrize("dtype", [np.uint16, np.int32], ids=["uint16", "int32"])
def test_device_dataset_equals_the_cpu_dataset(dtype):
    toks = _word_rows(23, 64, seed=3).astype(dtype)
    cont = _table(30522, FLAGGED_FROM).numpy()
    kw = dict(max_predictions=9, seed=1, mask_seed=2, eval_seed=5, num_shards=2, shard_index=1,
              continuation=cont)
    cpu = DeviceTokenDataset(toks, 5, "cpu", **kw)
    gpu = DeviceTokenDataset(toks, 5, "cuda", chunk_bytes=3 * 64 * toks.itemsize, **kw)
    assert gpu.continuation.is_cuda and torch.equal(gpu.continuation.cpu(), cpu.continuation)
    plain = DeviceTokenDataset(toks, 5, "cuda", **dict(kw, continuation=None))
    differs = False
    for _ in range(5):                                           # over two epoch boundaries
        bc, bg, bp = next(cpu), next(gpu), next(plain)
        assert bg["input_ids"].is_cuda and bg["input_ids"].shape == (5, 64)
        _assert_same({k: v.cpu() for k, v in bg.items()}, bc)
        differs |= not torch.equal(bg["masked_lm_positions"], bp["masked_lm_positions"])
    assert differs and cpu.epoch == gpu.epoch == 2
    passes = list(zip(cpu.single_pass(), gpu.single_pass()))
    assert [len(c["input_ids"]) for c, _ in passes] == [5, 5, 1]
    for bc, bg in passes:
        _assert_same({k: v.cpu() for k, v in bg.items()}, bc)


def _env():
    e = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        e.pop(k, None)
    return e


def test_cli_whole_word_mask_bert_base(tmp_path):
    d = tmp_path / "set"
    d.mkdir()
    val = _word_rows(16, 64, seed=2, shortest=20)
    np.save(d / "train_tokens.npy", _word_rows(16, 64, seed=1, shortest=20))
    np.save(d / "val_tokens.npy", val)
    cont = _table(30522, FLAGGED_FROM).numpy()
    np.save(d / "continuation.npy", cont)
    r = subprocess.run([sys.executable, TRAIN, "--model", "bert_base", "--text_data", str(d),
                        "--batch_size", "4", "--max_steps", "2", "--log_dir", str(tmp_path / "tb"),
                        "--whole_word_mask", "--eval"], capture_output=True, text=True,
                       env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["global_step"] == 2 and math.isfinite(res["final_loss"])
    assert res["whole_word_mask"] is True
    assert math.isfinite(res["eval_loss"]) and 0.0 <= res["eval_top_1"] <= 1.0
    # the evaluation masks are the CPU rule's under the CLI's evaluation seed, 0
    want = reference.mlm_mask_tokens(torch.from_numpy(val), torch.arange(16), 0, 20,
                                     TokenMasking(), continuation=torch.from_numpy(cont))
    plain = reference.mlm_mask_tokens(torch.from_numpy(val), torch.arange(16), 0, 20,
                                      TokenMasking())
    assert res["eval_count"] == int(want["masked_lm_weights"].sum())
    assert not torch.equal(want["masked_lm_positions"], plain["masked_lm_positions"])
