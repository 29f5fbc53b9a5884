"""Whole-word masking on the CPU path: ops.mlm_mask_tokens(..., continuation=) against a
pure-Python per-row oracle written from the rule's text (plain ints and lists, no call into
ops/reference.py), the all-zero table against the token rule, the rule's invariants and
80 / 10 / 10 shares on random rows of words, the DeviceTokenDataset with a table, the helpers
that make and load the table, and the CLI flag."""
import json
import math
import os

import numpy as np
import pytest
import torch

from distributedtensorflow_amd import cli, ops
from distributedtensorflow_amd.data import (DeviceTokenDataset, TokenMasking, load_continuation,
                                            wordpiece_continuation)
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


def oracle_row(t, n, seed, P, m, cont, events=None):
    """One row of the whole-word rule in plain Python integers -> the six outputs and (T, T').
    ``t``: the stored tokens (unsigned); ``n``: the example number; ``cont``: the table as a
    list.  ``events`` collects the branches of the greedy fill the row went through."""
    S = len(t)
    n &= (1 << 64) - 1
    row_seed = fmix32(((n & M32) * 0x9E3779B1 + seed) & M32) ^ (n >> 32)
    key = [fmix32((j * 0x9E3779B1 + row_seed) & M32) for j in range(S)]
    mask = [int(v != m.pad_id) for v in t]
    first = t.index(m.sep_id) if m.sep_id in t else None
    seg = [int(bool(mask[j]) and first is not None and j > first) for j in range(S)]
    cand = [t[j] not in (m.pad_id, m.cls_id, m.sep_id) for j in range(S)]
    nc = sum(cand)
    T = 0 if nc == 0 else min(P, nc, max(1, (nc * m.prob_q16 + 32768) >> 16))
    words = []
    for j in range(S):
        if not cand[j]:
            continue
        if cont[t[j]] == 0 or j == 0 or not cand[j - 1]:
            words.append([j])
        else:
            words[-1].append(j)
    taken, chosen, skipped = 0, [], False
    ev = set()
    for w in sorted(words, key=lambda w: (key[w[0]], w[0])):
        if taken >= T:
            ev.add("stopped_before_the_last_word")
            break
        if taken + len(w) > T:
            skipped = True
            continue
        if skipped:
            ev.add("taken_after_a_skip")
        if taken + len(w) == T and len(w) > 1:
            ev.add("a_word_fits_exactly")
        chosen += w
        taken += len(w)
    chosen.sort()
    if nc and taken == 0:
        ev.add("nothing_fits")
    if nc and taken < T:
        ev.add("budget_not_filled")
    if nc > 1 and T == nc:
        ev.add("budget_is_every_candidate")
    if nc and T == P and P < max(1, (nc * m.prob_q16 + 32768) >> 16):
        ev.add("budget_capped_by_P")
    if events is not None:
        events |= ev
    out = list(t)
    for j in chosen:
        h2 = fmix32((key[j] + 0x85EBCA6B) & M32)
        d = ((h2 & 0xFFFF) * 10) >> 16
        if d < 8:
            out[j] = m.mask_id
        elif d == 9:
            out[j] = m.random_low + ((fmix32((h2 + 0x9E3779B1) & M32) *
                                      (m.vocab_size - m.random_low)) >> 32)
    pad = [0] * (P - taken)
    return (out, seg, mask, chosen + pad, [t[j] for j in chosen] + pad,
            [1.0] * taken + [0.0] * (P - taken)), (T, taken), words


def oracle(tokens, idx, seed, P, m, cont, stride=1, offset=0, events=None):
    """-> (the six outputs as tensors, [(T, T')] per row)."""
    width = 8 * tokens.element_size()
    store = tokens.view(torch.int16) if tokens.dtype == torch.uint16 else tokens
    cont = [int(v) for v in cont.tolist()]
    rows, budgets = [], []
    for i in idx.tolist():
        if 0 <= i < len(tokens):
            t = [int(v) & ((1 << width) - 1) for v in store[i].tolist()]
        else:
            t = [m.pad_id] * tokens.shape[1]
        row, budget, _ = oracle_row(t, offset + i * stride, seed, P, m, cont, events)
        rows.append(row)
        budgets.append(budget)
    cols = list(zip(*rows))
    out = {k: torch.tensor(c, dtype=torch.int64) for k, c in zip(KEYS[:5], cols[:5])}
    out[KEYS[5]] = torch.tensor(cols[5], dtype=torch.float32).reshape(len(rows), P)
    return out, budgets


def assert_same(got, want):
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


# ----------------------------------------------------------------------------- the rows

VOCAB, FIRST_PIECE = 50000, 40000     # ids of 40000 and more are continuation pieces: all of
                                      # them in the top half of 16 bits


def table(vocab=VOCAB, first_piece=FIRST_PIECE):
    t = torch.zeros(vocab, dtype=torch.uint8)
    t[first_piece:] = 1
    return t


def branch_rows(S):
    """Rows that hit every branch of the whole-word rule -> int64 [9, S]:
    0 a full row of one-token words with a word over positions 62..65 (S > 65), one over
      126..128 (S > 128) and one that ends at S - 1
    1 a continuation piece at j = 0 of a row with no [CLS], and one right after [SEP]
    2 a continuation piece right after [CLS]
    3 one word of nc pieces, nc > T: nothing fits
    4 three words of 4 pieces and 8 of one: T = 3 at prob 0.15, the long words are skipped
    5 [CLS] [SEP] pad...: no candidate
    6 one word of 2 pieces (T == nc at prob 1.0) after a lone one-piece row part
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
    k = min(S - 2, 40)
    rows = [
        full,
        fit(piece(2) + head() + piece() + [SEP] + piece() + head() + [SEP]),
        fit([CLS] + piece(2) + head() + [SEP] + head() + piece() + [SEP]),
        fit([CLS] + word(k) + [SEP]),
        fit([CLS] + word(4) + head(3) + word(4) + head(2) + [SEP] + head(3) + word(4) + [SEP]),
        fit([CLS, SEP]),
        fit([CLS] + head() + [SEP] + word(2) + [SEP]),
        fit([CLS, SEP, CLS] + word(2) + [PAD] + piece() + head() + [SEP]),
        fit([CLS] + word(3) + word(3) + [SEP] + word(3) * (S // 8) + [SEP]),
    ]
    return torch.tensor(rows, dtype=torch.int64)


def store(rows, dtype):
    """int64 ids -> the storage dtype (uint16 values of 32768 and more wrap into int16)."""
    if dtype == torch.int32:
        return rows.to(torch.int32)
    u16 = rows.numpy().astype(np.uint16)
    return torch.from_numpy(u16 if dtype == torch.uint16 else u16.view(np.int16))


IDX = torch.tensor([8, 0, 3, 2, 3, 1, 7, 4, 6, 5, 9, -1, 2])     # repeated, unordered, 2 outside


def cases(S):
    """(P, seed, masking, example_stride, example_offset) of every run over the branch rows."""
    m = TokenMasking(vocab_size=VOCAB, random_low=999)
    return [(min(20, S), 12345, m, 1, 0), (2, 7, m, 3, 2), (1, 0, m, 1, 0),
            (min(20, S), 99, m.replace(prob=0.5), 1 << 33, 5),
            (S, 4000000000, m.replace(prob=1.0), 1, 0),           # T == nc
            (2, 31, m.replace(prob=1.0), 1, 0),                   # P below the budget
            (3, 5, m.replace(prob=0.4), 1, 0)]


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int16, torch.int32],
                         ids=["uint16", "int16", "int32"])
@pytest.mark.parametrize("S", [8, 64, 72, 128, 512])
def test_rule_equals_the_python_oracle(S, dtype):
    rows = branch_rows(S)
    assert int(rows.max()) >= 32768
    tokens, cont = store(rows, dtype), table()
    for P, seed, m, stride, offset in cases(S):
        want, budgets = oracle(tokens, IDX, seed, P, m, cont, stride, offset)
        got = reference.mlm_mask_tokens(tokens, IDX, seed, P, m, stride, offset, continuation=cont)
        assert_same(got, want)
        assert_same(ops.mlm_mask_tokens(tokens, IDX, seed, P, m, stride, offset,
                                        continuation=cont.bool()), want)
        # outside the set: all pad, nothing to predict
        assert got["input_ids"][-2].eq(PAD).all() and got["input_mask"][-2].sum() == 0
        assert got["masked_lm_weights"][-2].sum() == 0 and got["masked_lm_weights"][-3].sum() == 0
        assert budgets[-2] == (0, 0)


def test_the_branch_rows_hit_every_branch():
    """What the rows were built for, read off the oracle: its words and the path it took."""
    m = TokenMasking(vocab_size=VOCAB, random_low=999)
    cont = table().tolist()
    seen = set()
    for S in (8, 64, 72, 128, 512):
        rows = branch_rows(S)
        words = [oracle_row(r.tolist(), 0, 1, 1, m, cont)[2] for r in rows]
        assert [S - 3, S - 2, S - 1] in words[0]                  # ends at S - 1
        assert S <= 65 or [62, 63, 64, 65] in words[0]            # over 63 | 64
        assert S <= 128 or [126, 127, 128] in words[0]            # over 127 | 128
        assert words[1][:3] == [[0, 1], [2, 3], [5]]              # j = 0; right after [SEP]
        assert words[2][:2] == [[1, 2], [3]]                      # right after [CLS]
        assert len(words[3]) == 1 and len(words[3][0]) == min(S - 2, 40)
        assert words[5] == [] and words[7][:3] == [[3, 4], [6], [7]]     # after a pad
        for P, seed, mm, stride, offset in cases(S):
            for r in range(9):
                out, (T, taken), _ = oracle_row(rows[r].tolist(), offset + r * stride, seed, P,
                                                mm, cont, seen)
                assert taken <= T <= P
                if r == 3 and T < len(words[3][0]):
                    assert taken == 0 and sum(out[5]) == 0        # nothing fits: all weights 0
                if r == 5:
                    assert T == 0
                if mm.prob == 1.0 and P == S:
                    assert taken == T == sum(len(w) for w in words[r])
    assert seen == {"stopped_before_the_last_word", "taken_after_a_skip", "a_word_fits_exactly",
                    "nothing_fits", "budget_not_filled", "budget_is_every_candidate",
                    "budget_capped_by_P"}


# ----------------------------------------------------------------------------- random rows

FLAGGED_FROM = 24722                   # 5800 of 30522 ids are pieces: 19 %, as in BERT's vocabulary


def word_rows(N=1500, S=128, seed=12345, vocab=30522, shortest=20):
    """[CLS] a [SEP] b [SEP] pad... rows of random lengths shortest..S whose text is words of
    1 / 2 / 3 / 4 pieces with probability .7 / .2 / .07 / .03 -> uint16 numpy [N, S].  A word
    is a head (an unflagged id) and pieces (flagged ids); a word cut by a [SEP] stays a word."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((N, S), dtype=np.uint16)
    for r in range(N):
        L = rng.randint(shortest, S + 1)
        body = []
        while len(body) < L:
            k = rng.choice(4, p=[.7, .2, .07, .03]) + 1
            body += [rng.randint(1000, FLAGGED_FROM)] + list(rng.randint(FLAGGED_FROM, vocab, k - 1))
        rows[r, :L] = body[:L]
        rows[r, 0], rows[r, rng.randint(2, L - 2)], rows[r, L - 1] = CLS, SEP, SEP
    return rows


@pytest.fixture(scope="module")
def word_set():
    """-> (rows int64 [1500, 128], table, reference outputs, the oracle's (T, T') per row and
    its words per row), computed once."""
    rows = word_rows()
    cont = table(30522, FLAGGED_FROM)
    m = TokenMasking()
    out = reference.mlm_mask_tokens(torch.from_numpy(rows), torch.arange(len(rows)), 12345, 20, m,
                                    continuation=cont)
    lst = cont.tolist()
    per_row = [oracle_row([int(v) for v in rows[r]], r, 12345, 20, m, lst)
               for r in range(len(rows))]
    return (torch.from_numpy(rows.astype(np.int64)), cont, out, [p[1] for p in per_row],
            [p[2] for p in per_row])


def test_all_zero_table_is_the_token_rule():
    m = TokenMasking()
    rows = torch.from_numpy(word_rows(N=200, seed=7))
    idx = torch.arange(200)
    zero = torch.zeros(30522, dtype=torch.uint8)
    for seed in (12345, 1):
        want = reference.mlm_mask_tokens(rows, idx, seed, 20, m)
        assert_same(reference.mlm_mask_tokens(rows, idx, seed, 20, m, continuation=zero), want)
        assert_same(ops.mlm_mask_tokens(rows, idx, seed, 20, m, continuation=zero), want)
    # and a table makes a difference on these rows
    some = reference.mlm_mask_tokens(rows, idx, 1, 20, m, continuation=table(30522, FLAGGED_FROM))
    assert not torch.equal(some["masked_lm_positions"], want["masked_lm_positions"])


def test_invariants_on_random_rows(word_set):
    t, cont, out, budgets, words = word_set
    N, S = t.shape
    P = 20
    pos, ids, w = out["masked_lm_positions"], out["masked_lm_ids"], out["masked_lm_weights"]
    flagged = cont[t].bool() & (t != PAD)
    print(f"flagged tokens: {flagged.float().sum() / (t != PAD).sum():.3f} of the real ones")
    T = torch.tensor([b[0] for b in budgets])
    taken = torch.tensor([b[1] for b in budgets])
    # the weights sum to T' <= T, and the reference's T' is the oracle's, row by row
    assert torch.equal(w.sum(1).long(), taken) and (taken <= T).all()
    live = torch.arange(P).unsqueeze(0) < taken.unsqueeze(1)
    assert torch.equal(w, live.float())
    assert (pos[~live] == 0).all() and (ids[~live] == 0).all()
    share = float((taken == T).float().mean())
    print(f"rows with T' == T: {share:.4f}")
    assert share >= 0.99
    assert float((w.sum(1).long() == T).float().mean()) == share
    # ascending positions, labelled with the stored tokens
    assert ((pos[:, 1:] > pos[:, :-1]) | ~live[:, 1:]).all()
    assert torch.equal(ids[live], t.gather(1, pos)[live])
    sel = torch.zeros(N, S + 1, dtype=torch.bool)
    sel.scatter_(1, torch.where(live, pos, torch.full_like(pos, S)), True)
    sel = sel[:, :S]
    # every word is wholly selected or wholly untouched
    for r in range(N):
        row = sel[r].tolist()
        for word in words[r]:
            assert len({row[j] for j in word}) == 1, (r, word)
        assert sum(row) == sum(len(word) for word in words[r] if row[word[0]])
    # everything else is a copy
    assert torch.equal(out["input_ids"][~sel], t[~sel])
    assert torch.equal(out["input_mask"], (t != PAD).long())
    lengths = [len(word) for ws in words for word in ws]
    assert max(lengths) >= 4 and min(lengths) == 1


def test_mask_keep_random_shares(word_set):
    """80 / 10 / 10 over the selected tokens within 4 binomial standard deviations, the bound
    the token rule's test uses: the draws are per token and unchanged."""
    t, cont, out, _, _ = word_set
    live = out["masked_lm_weights"] > 0
    new = out["input_ids"].gather(1, out["masked_lm_positions"])[live]
    old = out["masked_lm_ids"][live]
    n = live.sum().item()
    masked = (new == MASK).sum().item()
    kept = (new == old).sum().item()
    for share, count in ((0.8, masked), (0.1, kept), (0.1, n - masked - kept)):
        sd = math.sqrt(share * (1 - share) / n)
        print(f"share {share}: {count / n:.4f} ({(count / n - share) / sd:+.2f} sd of {n})")
        assert abs(count / n - share) <= 4 * sd


# ----------------------------------------------------------------------------- the dataset

def _set(N=23, S=16):
    return word_rows(N, S, seed=3, shortest=6)


def _eq(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


CONT = table(30522, FLAGGED_FROM).numpy()


def test_dataset_with_a_table_is_deterministic_and_masks_dynamically():
    toks = _set()
    kw = dict(max_predictions=4, shuffle=True, seed=1, mask_seed=2, continuation=CONT)
    a = DeviceTokenDataset(toks, 5, "cpu", **kw)
    b = DeviceTokenDataset(toks, 5, "cpu", **kw)
    plain = DeviceTokenDataset(toks, 5, "cpu", **dict(kw, continuation=None))
    assert a.continuation.dtype == torch.uint8 and plain.continuation is None
    differs = False
    for _ in range(6):                                     # over an epoch boundary
        xa, xb, xp = next(a), next(b), next(plain)
        assert _eq(xa, xb)
        assert torch.equal(xa["input_mask"], xp["input_mask"])          # the same examples
        differs |= not torch.equal(xa["masked_lm_positions"], xp["masked_lm_positions"])
    assert differs and a.epoch == 1
    # the batches are the op's under the dataset's seeds: whole words
    c = DeviceTokenDataset(toks, 23, "cpu", max_predictions=4, mask_seed=5,
                           continuation=CONT.astype(bool))
    e0, e1 = next(c), next(c)
    assert c.epoch == 1 and not torch.equal(e0["masked_lm_positions"], e1["masked_lm_positions"])
    g = torch.Generator(device="cpu").manual_seed(5)
    seed = int(torch.randint(0, 1 << 32, (1,), generator=g, dtype=torch.int64))
    want, _ = oracle(torch.from_numpy(toks), torch.arange(23), seed, 4, TokenMasking(),
                     torch.from_numpy(CONT))
    assert_same(e0, want)
    for bad in (CONT[:-1], CONT.astype(np.int32), CONT * 2):
        with pytest.raises(ValueError):
            DeviceTokenDataset(toks, 5, "cpu", continuation=bad)
    flagged = CONT.copy()
    flagged[SEP] = 1
    with pytest.raises(ValueError):
        DeviceTokenDataset(toks, 5, "cpu", continuation=flagged)


def _single(toks, bs, shards, **kw):
    seen = {}
    for shard in range(shards):
        d = DeviceTokenDataset(toks, bs, "cpu", max_predictions=4, eval_seed=77,
                               num_shards=shards, shard_index=shard, continuation=CONT, **kw)
        k = 0
        for batch in d.single_pass():
            for r in range(len(batch["input_ids"])):
                n = shard + k * shards
                assert n not in seen
                seen[n] = {key: batch[key][r].clone() for key in KEYS}
                k += 1
    return seen


def test_single_pass_with_a_table_is_the_same_whatever_the_batch_and_sharding():
    toks = _set(N=23)
    one, seven = _single(toks, 4, 1), _single(toks, 7, 1, chunk_bytes=5 * 32)
    three = _single(toks, 4, 3, chunk_bytes=3 * 32)
    want, _ = oracle(torch.from_numpy(toks), torch.arange(23), 77, 4, TokenMasking(),
                     torch.from_numpy(CONT))
    assert sorted(one) == sorted(seven) == sorted(three) == list(range(23))
    for n in range(23):
        for key in KEYS:
            assert torch.equal(one[n][key], want[key][n]), (n, key)
            assert torch.equal(seven[n][key], want[key][n]), (n, key)
            assert torch.equal(three[n][key], want[key][n]), (n, key)


def test_an_evaluation_between_two_steps_leaves_training_alone():
    toks = _set()
    kw = dict(max_predictions=4, shuffle=True, seed=4, mask_seed=9, num_shards=2, shard_index=1,
              continuation=CONT)
    d = DeviceTokenDataset(toks, 5, "cpu", **kw)
    ref = DeviceTokenDataset(toks, 5, "cpu", **kw)
    assert _eq(next(d), next(ref))
    first = list(d.single_pass())
    again = list(d.single_pass(3))
    cat = {k: torch.cat([b[k] for b in first]) for k in KEYS}
    assert _eq(cat, {k: torch.cat([b[k] for b in again]) for k in KEYS})
    assert _eq(next(d), next(ref))


# ----------------------------------------------------------------------------- table helpers

VOCAB_TXT = ["[PAD]", "[unused0]", "[CLS]", "[SEP]", "[MASK]", "the", "##s", "play", "##ing",
             "#", "##", "a##b"]


def test_wordpiece_continuation(tmp_path):
    path = tmp_path / "vocab.txt"
    path.write_text("\n".join(VOCAB_TXT) + "\n", encoding="utf-8")
    want = [0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0]
    for got in (wordpiece_continuation(str(path)), wordpiece_continuation(path),
                wordpiece_continuation(VOCAB_TXT), wordpiece_continuation(tuple(VOCAB_TXT))):
        assert got.dtype == np.uint8 and got.shape == (12,) and got.tolist() == want


def test_load_continuation_and_its_errors(tmp_path):
    m = TokenMasking(vocab_size=12, pad_id=0, cls_id=2, sep_id=3, mask_id=4)
    good = wordpiece_continuation(VOCAB_TXT)

    def saved(name, arr):
        d = tmp_path / name
        d.mkdir()
        np.save(d / "continuation.npy", arr)
        return str(d)

    got = load_continuation(saved("ok", good), m)
    assert got.dtype == np.uint8 and got.tolist() == good.tolist()
    got = load_continuation(saved("bool", good.astype(bool)), m)
    assert got.dtype == np.uint8 and got.tolist() == good.tolist()
    special = good.copy()
    special[3] = 1
    bad = {"dtype": good.astype(np.int32), "short": good[:-1], "rank": good.reshape(3, 4),
           "value": good * 2, "special": special}
    for name, arr in bad.items():
        with pytest.raises(ValueError):
            load_continuation(saved(name, arr), m)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="continuation.npy"):
        load_continuation(str(empty), m)


def test_argument_errors():
    m = TokenMasking()
    tokens = torch.from_numpy(_set(N=4))
    idx = torch.tensor([0])
    good = torch.from_numpy(CONT)
    two = good * 2
    special = good.clone()
    special[MASK] = 1
    bad = [good.int(), good.float(), good[:-1], good.view(1, -1), two, special,
           torch.stack([good, good], 1)[:, 0],                     # not contiguous
           good.to("meta"),                                         # another device
           CONT]                                                    # not a tensor
    for fn in (reference.mlm_mask_tokens, ops.mlm_mask_tokens):
        for c in bad:
            with pytest.raises(ValueError):
                fn(tokens, idx, 0, 2, m, continuation=c)
        fn(tokens, idx, 0, 2, m, continuation=good)
        fn(tokens, idx, 0, 2, m, continuation=good.bool())
    # a table that passed is checked again once it has been written to
    t = good.clone()
    reference.mlm_mask_tokens(tokens, idx, 0, 2, m, continuation=t)
    t[CLS] = 1
    with pytest.raises(ValueError):
        reference.mlm_mask_tokens(tokens, idx, 0, 2, m, continuation=t)


# ----------------------------------------------------------------------------- CLI

def test_cli_rejects_the_flag_without_its_inputs(tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["--model", "bert_base", "--whole_word_mask"])
    assert "--whole_word_mask needs --text_data" in str(e.value)
    np.save(tmp_path / "train_tokens.npy", _set())
    with pytest.raises(SystemExit) as e:
        cli.main(["--model", "bert_base", "--text_data", str(tmp_path), "--whole_word_mask"])
    assert "--whole_word_mask needs" in str(e.value)
    assert os.path.join(str(tmp_path), "continuation.npy") in str(e.value)
    args = cli.build_parser().parse_args(["--model", "bert_base", "--text_data", "D"])
    assert args.whole_word_mask is False
    args = cli.build_parser().parse_args(["--model", "bert_base", "--text_data", "D",
                                          "--whole_word_mask"])
    assert args.whole_word_mask is True


def test_cli_trains_and_evaluates_a_tiny_bert_with_the_flag(tmp_path, monkeypatch, capsys):
    from distributedtensorflow_amd.models import bert
    tiny = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                intermediate_size=128, max_position_embeddings=16)       # head_dim 64
    monkeypatch.setattr(bert, "bert_base",
                        lambda **kw: bert.BertForPreTraining(bert.BertConfig(**tiny, **kw)))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TF_CONFIG"):
        monkeypatch.delenv(k, raising=False)
    vocab = 1200
    cont = np.zeros(vocab, dtype=np.uint8)
    cont[700:] = 1
    d = tmp_path / "set"
    d.mkdir()
    rng = np.random.RandomState(0)
    for split, n in (("train", 12), ("val", 7)):
        rows = word_rows(n, 16, seed=n, shortest=8)
        body = (rows != PAD) & (rows != CLS) & (rows != SEP)
        rows[body] = rng.randint(200, vocab, int(body.sum()))     # inside the tiny vocabulary
        np.save(d / f"{split}_tokens.npy", rows)
    val = np.load(d / "val_tokens.npy")
    np.save(d / "continuation.npy", cont)
    with open(d / "meta.json", "w") as f:
        json.dump({"vocab_size": vocab}, f)
    base = ["--model", "bert_base", "--device", "cpu", "--text_data", str(d), "--batch_size", "4",
            "--max_steps", "2", "--max_predictions", "4", "--log_dir", "", "--eval"]
    m = TokenMasking(vocab_size=vocab)
    counts = {}
    from distributedtensorflow_amd.train.global_step import reset_global_step
    for flag in (["--whole_word_mask"], []):
        reset_global_step()                                       # each run counts from 0
        assert cli.main(base + flag) == 0
        res = json.loads([l for l in capsys.readouterr().out.splitlines()
                          if l.startswith("{")][-1])
        assert res["global_step"] == 2 and math.isfinite(res["final_loss"])
        assert math.isfinite(res["eval_loss"])
        assert ("whole_word_mask" in res) == bool(flag)
        if flag:
            assert res["whole_word_mask"] is True
        counts[bool(flag)] = res["eval_count"]
    reset_global_step()
    want, _ = oracle(torch.from_numpy(val), torch.arange(7), 0, 4, m, torch.from_numpy(cont))
    assert counts[True] == int(want["masked_lm_weights"].sum())
    plain = reference.mlm_mask_tokens(torch.from_numpy(val), torch.arange(7), 0, 4, m)
    assert counts[False] == int(plain["masked_lm_weights"].sum())
