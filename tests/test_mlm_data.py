"""Masked-LM example creation on the CPU path: the integer rule of ops.mlm_mask_tokens against a
pure-Python per-row oracle written from the rule's text, its invariants and 80 / 10 / 10 shares
on random rows, the DeviceTokenDataset (determinism, dynamic masks, single_pass, sharding,
evaluation masks that depend on the example alone), the .npy loader and the CLI's validation."""
import json
import math
import os

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import cli, ops
from distributedtensorflow_amd.data import DeviceTokenDataset, TokenMasking, load_token_arrays
from distributedtensorflow_amd.ops import reference

KEYS = ("input_ids", "segment_ids", "input_mask", "masked_lm_positions", "masked_lm_ids",
        "masked_lm_weights")
M32 = 0xFFFFFFFF
PAD, CLS, SEP, MASK = 0, 101, 102, 103


# ----------------------------------------------------------------------------- the oracle

def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def oracle_row(t, n, seed, P, m):
    """One row of the rule, in plain Python integers.  ``t``: the stored tokens (unsigned), or
    None for an example outside the set; ``n``: the example number."""
    S = len(t)
    n &= (1 << 64) - 1
    row_seed = fmix32(((n & M32) * 0x9E3779B1 + seed) & M32) ^ (n >> 32)
    key = [fmix32((j * 0x9E3779B1 + row_seed) & M32) for j in range(S)]
    mask = [int(v != m.pad_id) for v in t]
    first = t.index(m.sep_id) if m.sep_id in t else None
    seg = [int(bool(mask[j]) and first is not None and j > first) for j in range(S)]
    cands = [j for j in range(S) if t[j] not in (m.pad_id, m.cls_id, m.sep_id)]
    nc = len(cands)
    T = 0 if nc == 0 else min(P, nc, max(1, (nc * m.prob_q16 + 32768) >> 16))
    chosen = sorted(sorted(cands, key=lambda j: (key[j], j))[:T])
    out = list(t)
    for j in chosen:
        h2 = fmix32((key[j] + 0x85EBCA6B) & M32)
        d = ((h2 & 0xFFFF) * 10) >> 16
        if d < 8:
            out[j] = m.mask_id
        elif d == 9:
            out[j] = m.random_low + ((fmix32((h2 + 0x9E3779B1) & M32) *
                                      (m.vocab_size - m.random_low)) >> 32)
    pad = [0] * (P - T)
    return (out, seg, mask, chosen + pad, [t[j] for j in chosen] + pad, [1.0] * T + [0.0] * (P - T))


def oracle(tokens, idx, seed, P, m, stride=1, offset=0):
    width = 8 * tokens.element_size()
    store = tokens.view(torch.int16) if tokens.dtype == torch.uint16 else tokens
    rows = []
    for i in idx.tolist():
        if 0 <= i < len(tokens):
            t = [int(v) & ((1 << width) - 1) for v in store[i].tolist()]
        else:
            t = [m.pad_id] * tokens.shape[1]
        rows.append(oracle_row(t, offset + i * stride, seed, P, m))
    cols = list(zip(*rows))
    out = {k: torch.tensor(c, dtype=torch.int64) for k, c in zip(KEYS[:5], cols[:5])}
    out[KEYS[5]] = torch.tensor(cols[5], dtype=torch.float32).reshape(len(rows), P)
    return out


def assert_same(got, want):
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


# ----------------------------------------------------------------------------- the rows

def branch_rows(S, vocab=30522, seed=0):
    """Rows that hit every branch of the rule -> int64 [9, S]:
    0 full, 1 padded, 2 [CLS] [SEP] pad... (nc = 0), 3 nc = 1, 4 nc = 3, 5 no sep, 6 two sep,
    7 ids from the top of the vocabulary, 8 specials scattered through the row."""
    g = torch.Generator().manual_seed(1000 + S + seed)

    def words(k):
        return torch.randint(1000, vocab, (k,), generator=g).tolist()

    def fit(body):
        body = body[:S]
        return body + [PAD] * (S - len(body))

    half = max(1, S // 2 - 2)
    rows = [
        fit([CLS] + words(half) + [SEP] + words(S)[:S - half - 3] + [SEP]),
        fit([CLS] + words(max(1, S // 3)) + [SEP] + words(1) + [SEP]),
        fit([CLS, SEP]),
        fit([CLS] + words(1) + [SEP]),
        fit([CLS] + words(3) + [SEP]),
        fit([CLS] + words(S - 2)),
        fit([CLS] + words(1) + [SEP] + words(2) + [SEP]),
        fit([CLS] + [vocab - 1, vocab - 2] * S),
        fit([CLS, SEP, CLS] + words(2) + [PAD] + words(2) + [SEP]),
    ]
    return torch.tensor(rows, dtype=torch.int64)


def store(rows, dtype):
    """int64 ids -> the storage dtype (uint16 values of 32768 and more wrap into int16)."""
    if dtype == torch.int32:
        return rows.to(torch.int32)
    return torch.from_numpy(rows.numpy().astype(np.uint16)) if dtype == torch.uint16 else \
        torch.from_numpy(rows.numpy().astype(np.uint16).view(np.int16))


IDX = torch.tensor([8, 0, 3, 2, 3, 1, 7, 4, 6, 5, 9, -1, 2])     # repeated, unordered, 2 outside


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int16, torch.int32],
                         ids=["uint16", "int16", "int32"])
@pytest.mark.parametrize("S", [8, 64, 72, 128])
def test_rule_equals_the_python_oracle(S, dtype):
    m = TokenMasking()
    tokens = store(branch_rows(S), dtype)
    for P, seed in ((min(20, S), 12345), (2, 7), (S, 4000000000), (1, 0)):
        want = oracle(tokens, IDX, seed, P, m)
        got = reference.mlm_mask_tokens(tokens, IDX, seed, P, m)
        assert_same(got, want)
        assert_same(ops.mlm_mask_tokens(tokens, IDX, seed, P, m), want)
    # the branches the rows were built for (P = 20 or S)
    P = min(20, S)
    out = reference.mlm_mask_tokens(tokens, torch.arange(9), 12345, P, m)
    T = out["masked_lm_weights"].sum(1).tolist()
    assert T[2] == 0 and T[3] == 1 and T[4] == 1                  # nc = 0, 1, 3
    assert out["segment_ids"][5].sum() == 0 and out["segment_ids"][0].sum() > 0
    assert out["segment_ids"][6].tolist()[:6] == [0, 0, 0, 1, 1, 1]      # after the FIRST sep
    two = reference.mlm_mask_tokens(tokens, torch.arange(9), 12345, 2, m)
    assert two["masked_lm_weights"][5].tolist() == [1.0, 1.0] or S == 8   # nc large, T = P
    # outside the set: all pad, nothing to predict
    assert got["input_ids"][-2].eq(PAD).all() and got["input_mask"][-2].sum() == 0
    assert got["masked_lm_weights"][-2].sum() == 0 and got["masked_lm_weights"][-3].sum() == 0


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int32], ids=["uint16", "int32"])
def test_ids_from_the_top_half_of_16_bits_and_example_numbers(dtype):
    m = TokenMasking(vocab_size=50000, random_low=999, prob=0.5)
    tokens = store(branch_rows(72, vocab=50000), dtype)
    assert int(branch_rows(72, vocab=50000).max()) >= 32768
    for stride, offset in ((1, 0), (3, 2), (1 << 33, 5)):         # example numbers past 2^32
        want = oracle(tokens, IDX, 99, 30, m, stride, offset)
        assert_same(reference.mlm_mask_tokens(tokens, IDX, 99, 30, m, stride, offset), want)
    # the example number, not the row, keys the masks
    a = reference.mlm_mask_tokens(tokens, torch.tensor([0]), 99, 30, m, 1, 0)
    b = reference.mlm_mask_tokens(tokens, torch.tensor([0]), 99, 30, m, 1, 1)
    assert not torch.equal(a["masked_lm_positions"], b["masked_lm_positions"])
    full = TokenMasking(vocab_size=65536)
    top = store(torch.tensor([[CLS, 65535, 65534, 40000, SEP, PAD, PAD, PAD]]), dtype)
    assert_same(reference.mlm_mask_tokens(top, torch.tensor([0]), 1, 3, full),
                oracle(top, torch.tensor([0]), 1, 3, full))


def test_argument_errors():
    m = TokenMasking()
    tokens = store(branch_rows(8), torch.uint16)
    idx = torch.tensor([0])
    bad = [
        lambda: reference.mlm_mask_tokens(torch.zeros(2, 513, dtype=torch.int32), idx, 0, 20, m),
        lambda: reference.mlm_mask_tokens(torch.zeros(2, 0, dtype=torch.int32), idx, 0, 1, m),
        lambda: reference.mlm_mask_tokens(tokens, idx, 0, 0, m),
        lambda: reference.mlm_mask_tokens(tokens, idx, 0, 9, m),             # P > S
        lambda: reference.mlm_mask_tokens(tokens, idx, 0, 2, TokenMasking(vocab_size=70000)),
        lambda: reference.mlm_mask_tokens(tokens, idx, 1 << 32, 2, m),
        lambda: reference.mlm_mask_tokens(tokens, idx, -1, 2, m),
        lambda: reference.mlm_mask_tokens(tokens.long(), idx, 0, 2, m),
        lambda: reference.mlm_mask_tokens(tokens, idx.int(), 0, 2, m),
        lambda: TokenMasking(vocab_size=100),                                # cls_id outside
        lambda: TokenMasking(mask_id=30522),
        lambda: TokenMasking(prob=1.5),
    ]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
    reference.mlm_mask_tokens(tokens.view(torch.int16).to(torch.int32), idx, 0, 2,
                              TokenMasking(vocab_size=70000))                # fine in 32 bits
    assert TokenMasking().prob_q16 == 9830 and TokenMasking(prob=1.0).prob_q16 == 65536


# ----------------------------------------------------------------------------- invariants

def random_rows(N=1500, S=128, seed=12345, vocab=30522, shortest=20):
    """[CLS] a [SEP] b [SEP] pad... rows of random lengths shortest..S -> uint16 numpy [N, S]."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((N, S), dtype=np.uint16)
    for r in range(N):
        L = rng.randint(shortest, S + 1)
        rows[r, :L] = rng.randint(1000, vocab, L)
        rows[r, 0], rows[r, rng.randint(2, L - 2)], rows[r, L - 1] = CLS, SEP, SEP
    return rows


@pytest.fixture(scope="module")
def random_set():
    rows = random_rows()
    tokens = torch.from_numpy(rows)
    out = reference.mlm_mask_tokens(tokens, torch.arange(len(rows)), 12345, 20, TokenMasking())
    return torch.from_numpy(rows.astype(np.int64)), out


def test_invariants_on_random_rows(random_set):
    t, out = random_set
    N, S = t.shape
    P, m = 20, TokenMasking()
    pos, ids, w = out["masked_lm_positions"], out["masked_lm_ids"], out["masked_lm_weights"]
    cand = (t != PAD) & (t != CLS) & (t != SEP)
    nc = cand.sum(1)
    T = torch.minimum(torch.clamp((nc * m.prob_q16 + 32768) >> 16, min=1), nc).clamp(max=P)
    assert torch.equal(w.sum(1).long(), T)
    live = torch.arange(P).unsqueeze(0) < T.unsqueeze(1)
    assert torch.equal(w, live.float())
    assert (pos[~live] == 0).all() and (ids[~live] == 0).all()
    # strictly ascending candidates, labelled with the originals
    assert ((pos[:, 1:] > pos[:, :-1]) | ~live[:, 1:]).all()
    assert cand.gather(1, pos)[live].all()
    assert torch.equal(ids[live], t.gather(1, pos)[live])
    # everything else is untouched
    sel = torch.zeros(N, S + 1, dtype=torch.bool)
    sel.scatter_(1, torch.where(live, pos, torch.full_like(pos, S)), True)
    sel = sel[:, :S]
    assert torch.equal(out["input_ids"][~sel], t[~sel])
    assert torch.equal(out["input_mask"], (t != PAD).long())
    assert set(out["segment_ids"].unique().tolist()) == {0, 1}


def test_mask_keep_random_shares(random_set):
    """80 / 10 / 10 within 4 binomial standard deviations (a cap, not a measurement: a
    prototype of the rule sat within 1.2; beyond 4 the hash chain is a different one)."""
    t, out = random_set
    live = out["masked_lm_weights"] > 0
    new = out["input_ids"].gather(1, out["masked_lm_positions"])[live]
    old = out["masked_lm_ids"][live]
    n = live.sum().item()
    masked = (new == MASK).sum().item()
    kept = (new == old).sum().item()
    # a random draw equals the original with probability 1 / vocab: 0.5 of 15.8k draws on
    # average, far inside the band
    for share, count in ((0.8, masked), (0.1, kept), (0.1, n - masked - kept)):
        sd = math.sqrt(share * (1 - share) / n)
        print(f"share {share}: {count / n:.4f} ({(count / n - share) / sd:+.2f} sd of {n})")
        assert abs(count / n - share) <= 4 * sd
    # positions are spread evenly: columns 1..19 are candidates in every row
    hist = torch.bincount(out["masked_lm_positions"][live], minlength=128)[1:20].float()
    assert hist.min() > 0.7 * hist.mean() and hist.max() < 1.3 * hist.mean()
    # another seed moves every row's positions
    rows = torch.from_numpy(random_rows()[:50])
    a = reference.mlm_mask_tokens(rows, torch.arange(50), 12345, 20, TokenMasking())
    b = reference.mlm_mask_tokens(rows, torch.arange(50), 54321, 20, TokenMasking())
    assert (a["masked_lm_positions"] != b["masked_lm_positions"]).any(1).all()


# ----------------------------------------------------------------------------- the dataset

def _set(N=23, S=16, dtype=np.uint16):
    return random_rows(N, S, seed=3, shortest=6).astype(dtype)


def _eq(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


def test_dataset_is_deterministic_and_masks_dynamically():
    toks = _set()
    kw = dict(max_predictions=4, shuffle=True, seed=1, mask_seed=2)
    a = DeviceTokenDataset(toks, 5, "cpu", **kw)
    b = DeviceTokenDataset(toks, 5, "cpu", **kw)
    c = DeviceTokenDataset(toks, 5, "cpu", **dict(kw, mask_seed=3))
    differs = False
    for _ in range(6):                                     # over an epoch boundary
        xa, xb, xc = next(a), next(b), next(c)
        assert set(xa) == set(KEYS) and xa["input_ids"].shape == (5, 16)
        assert xa["masked_lm_positions"].shape == (5, 4)
        assert xa["masked_lm_weights"].dtype == torch.float32
        assert _eq(xa, xb)
        assert torch.equal(xa["input_mask"], xc["input_mask"])          # the same examples
        differs |= not torch.equal(xa["masked_lm_positions"], xc["masked_lm_positions"])
    assert differs and a.epoch == 1
    # int32 storage gives the same batches as uint16
    d = DeviceTokenDataset(toks.astype(np.int32), 5, "cpu", **kw)
    e = DeviceTokenDataset(toks, 5, "cpu", **kw)
    assert d.tokens.dtype == torch.int32 and e.tokens.dtype == torch.int16
    assert _eq(next(d), next(e))
    # successive epochs over one example differ (no shuffle: batch k of each epoch is the same)
    f = DeviceTokenDataset(toks, 23, "cpu", max_predictions=4, mask_seed=5)
    e0, e1 = next(f), next(f)
    assert f.epoch == 1 and torch.equal(e0["masked_lm_ids"].eq(0), e1["masked_lm_ids"].eq(0))
    assert not torch.equal(e0["masked_lm_positions"], e1["masked_lm_positions"])


def _single(toks, bs, shards, **kw):
    """-> {global example: row of every output} over the shards' single passes, + batch sizes."""
    seen, sizes = {}, []
    for shard in range(shards):
        d = DeviceTokenDataset(toks, bs, "cpu", max_predictions=4, eval_seed=77,
                               num_shards=shards, shard_index=shard, **kw)
        k = 0
        for batch in d.single_pass():
            sizes.append(len(batch["input_ids"]))
            for r in range(sizes[-1]):
                n = shard + k * shards
                assert n not in seen
                seen[n] = {key: batch[key][r].clone() for key in KEYS}
                k += 1
    return seen, sizes


def test_single_pass_covers_every_example_once_whatever_the_batch_and_sharding():
    toks = _set(N=23)
    one, sizes = _single(toks, 4, 1)
    assert sizes == [4, 4, 4, 4, 4, 3] and sorted(one) == list(range(23))
    seven, _ = _single(toks, 7, 1, chunk_bytes=5 * 32)
    three, sizes3 = _single(toks, 4, 3, chunk_bytes=3 * 32)
    assert sizes3 == [4, 4, 4, 4, 4, 3] and sorted(three) == list(range(23))   # 8 + 8 + 7 rows
    want = reference.mlm_mask_tokens(torch.from_numpy(toks), torch.arange(23), 77, 4,
                                     TokenMasking())
    for n in range(23):
        for key in KEYS:
            assert torch.equal(one[n][key], want[key][n]), (n, key)
            assert torch.equal(seven[n][key], want[key][n]), (n, key)
            assert torch.equal(three[n][key], want[key][n]), (n, key)


def test_an_evaluation_between_two_steps_leaves_training_alone():
    toks = _set()
    kw = dict(max_predictions=4, shuffle=True, seed=4, mask_seed=9, num_shards=2, shard_index=1)
    d = DeviceTokenDataset(toks, 5, "cpu", **kw)
    ref = DeviceTokenDataset(toks, 5, "cpu", **kw)
    assert _eq(next(d), next(ref))
    first = list(d.single_pass())
    again = list(d.single_pass(3))
    assert [len(b["input_ids"]) for b in first] == [5, 5, 1]
    cat = {k: torch.cat([b[k] for b in first]) for k in KEYS}
    assert _eq(cat, {k: torch.cat([b[k] for b in again]) for k in KEYS})
    assert _eq(next(d), next(ref))
    with pytest.raises(ValueError):
        DeviceTokenDataset(toks, 24, "cpu")                              # batch > set
    with pytest.raises(ValueError):
        DeviceTokenDataset(toks, 4, "cpu", max_predictions=17)           # P > S
    with pytest.raises(ValueError):
        DeviceTokenDataset(toks.astype(np.int64), 4, "cpu")
    with pytest.raises(ValueError):
        DeviceTokenDataset(toks, 4, "cpu", num_shards=2, shard_index=2)


# ----------------------------------------------------------------------------- loader

def test_load_token_arrays_and_its_errors(tmp_path):
    toks = _set(N=6)
    d = str(tmp_path / "ok")
    os.makedirs(d)
    np.save(os.path.join(d, "train_tokens.npy"), toks)
    got, m = load_token_arrays(d, "train")
    assert isinstance(got, np.memmap) and np.array_equal(got, toks)
    assert (m.vocab_size, m.pad_id, m.cls_id, m.sep_id, m.mask_id) == (30522, 0, 101, 102, 103)
    np.save(os.path.join(d, "val_tokens.npy"), toks.astype(np.int32))
    assert load_token_arrays(d, "val")[0].dtype == np.int32
    # meta.json overrides the defaults and keeps the caller's prob
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump({"vocab_size": 40000, "mask_id": 4}, f)
    _, m = load_token_arrays(d, "train", TokenMasking(prob=0.3))
    assert (m.vocab_size, m.mask_id, m.cls_id, m.prob) == (40000, 4, 101, 0.3)
    bad = {
        "dtype": toks.astype(np.int64),
        "rank": toks[0],
        "range": np.full((2, 8), 30522, dtype=np.uint16),
        "negative": np.full((2, 8), -1, dtype=np.int32),
    }
    for name, arr in bad.items():
        sub = str(tmp_path / name)
        os.makedirs(sub)
        np.save(os.path.join(sub, "train_tokens.npy"), arr)
        with pytest.raises(ValueError):
            load_token_arrays(sub, "train")
    for name, meta in (("meta_key", {"vocab": 5}), ("meta_vocab", {"vocab_size": 20000}),
                       ("meta_wide", {"vocab_size": 70000}), ("meta_id", {"sep_id": 30522})):
        sub = str(tmp_path / name)
        os.makedirs(sub)
        np.save(os.path.join(sub, "train_tokens.npy"), toks)
        with open(os.path.join(sub, "meta.json"), "w") as f:
            json.dump(meta, f)
        with pytest.raises(ValueError):
            load_token_arrays(sub, "train")
    with pytest.raises(FileNotFoundError):
        load_token_arrays(str(tmp_path / "dtype"), "val")


# ----------------------------------------------------------------------------- CLI

@pytest.mark.parametrize("argv,message", [
    (["--model", "resnet50", "--text_data", "D"], "needs a BERT model"),
    (["--model", "mnist_cnn", "--text_data", "D"], "needs a BERT model"),
    (["--model", "bert_base", "--text_data", "D", "--image_data", "E"], "cannot be combined"),
    (["--model", "bert_base", "--text_data", "D", "--mlm_prob", "1.5"], "--mlm_prob"),
    (["--model", "bert_large", "--text_data", "D", "--max_predictions", "0"], "--max_predictions"),
])
def test_cli_rejects_flag_combinations(argv, message):
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert message in str(e.value)


def test_cli_flags_and_defaults():
    args = cli.build_parser().parse_args(["--model", "bert_base", "--text_data", "D"])
    assert (args.text_data, args.mlm_prob, args.max_predictions) == ("D", 0.15, 20)
    cli.check_data_args(args)
    assert cli.build_parser().parse_args([]).text_data is None
