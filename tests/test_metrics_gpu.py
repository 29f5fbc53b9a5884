"""The evaluation kernels (csrc/kernels/metrics.hip) against ops/reference.py: eval_rows ranks
exactly and loss rows within the training loss kernels' own error, metrics_accumulate exactly and
bit-reproducibly, and train.evaluate end to end on MnistCNN, BERT and ResNet-50.

Loss rows (measured on an MI355X, max |kernel - fp64 oracle| over all rows of the listed shapes;
see profiles/EVAL.md):  fp32: eval_rows 6.56e-7, softmax_xent 1.25e-6;  bf16: eval_rows 9.27e-7,
mlm_xent 1.20e-6."""
import pytest
import torch

import distributedtensorflow_amd as dtf
from distributedtensorflow_amd import ops
from distributedtensorflow_amd.metrics import ClassificationMetrics
from distributedtensorflow_amd.ops import native, records, reference

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
PAD = 1e4                       # what the padding columns V .. ld-1 hold: must change nothing

FP32_SHAPES = [(1, 10, 10), (7, 10, 10), (5, 1000, 1000), (9, 1003, 1003), (4, 30522, 30522)]
BF16_SHAPES = [(2, 8, 8), (6, 77, 80), (3, 30522, 30528), (5, 30522, 30522)]


def _draw(dtype, N, V, ld, seed):
    """[N, ld] of ``dtype`` on the CPU: randn * 3 rounded to the input type (ties occur) in the
    class columns, PAD in the padding columns; labels in [0, V)."""
    g = torch.Generator().manual_seed(seed)
    full = torch.full((N, ld), PAD)
    full[:, :V] = torch.randn(N, V, generator=g) * 3
    return full.to(dtype), torch.randint(0, V, (N,), generator=g)


def _forced(dtype, V, ld, seed, ignored):
    """Five rows of the same geometry: the label at column 0, at V-1, an all-equal row, an
    ignored label and a NaN label logit."""
    x, y = _draw(dtype, 5, V, ld, seed + 1000)
    y[0], y[1] = 0, V - 1
    x[2, :V] = 0.75
    y[3] = ignored
    x[4, int(y[4])] = float("nan")
    return x, y


def _check_ranks(x, y, V, label_dtype, view=False):
    """eval_rows on the GPU copy of (x, y) vs the oracle; returns (loss fp32 GPU->CPU, oracle
    loss fp64, rank)."""
    want_loss, want_rank = reference.eval_rows(x, y, vocab=V, loss_dtype=torch.float64)
    xg, yg = x.cuda(), y.to(label_dtype).cuda()
    if view:
        loss, rank = ops.eval_rows(xg[:, :V], yg)
    else:
        loss, rank = ops.eval_rows(xg, yg, vocab=V)
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.equal(rank.cpu(), want_rank), (rank.cpu(), want_rank)
    hit = ops.in_top_k(xg[:, :V], yg, 5).cpu()
    assert torch.equal(hit, (want_rank >= 0) & (want_rank < 5))
    return loss.cpu(), want_loss, want_rank


def _check_forced(loss, want_loss, rank, y, V):
    assert int(y[0]) == 0 and int(y[1]) == V - 1           # labels at the row's two ends
    assert rank[2].item() == int(y[2])                    # all-equal row: the label itself
    assert rank[3].item() == -1 and loss[3].item() == 0.0  # ignored
    assert rank[4].item() == V and torch.isnan(loss[4]) and torch.isnan(want_loss[4])


def _ulp32(v):
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _train_kernel_loss(x, y, V):
    """The existing training loss kernel's per-row loss on the same stored values (labels are
    all valid here): softmax_xent for fp32, mlm_xent (weight 1, denom 1) for bf16."""
    N, ld = x.shape
    xg = x.cuda().contiguous()
    lab = y.long().cuda()
    rows = torch.empty(N, device="cuda", dtype=torch.float32)
    grad = torch.empty_like(xg)
    st = torch.cuda.current_stream().cuda_stream
    if x.dtype == torch.float32:
        assert ld == V
        native._K.softmax_xent(xg.data_ptr(), lab.data_ptr(), 8, N, V, rows.data_ptr(),
                               grad.data_ptr(), 1.0, st)
    else:
        w = torch.ones(N, device="cuda")
        denom = torch.ones(1, device="cuda")
        native._K.mlm_xent(xg.data_ptr(), lab.data_ptr(), w.data_ptr(), denom.data_ptr(), N, V,
                           ld, rows.data_ptr(), grad.data_ptr(), st)
    torch.cuda.synchronize()
    return rows.cpu()


def _check_loss(tag, x, y, V, loss, want):
    """eval_rows' loss error <= max(2 x the training kernel's maximum error on the same inputs,
    one fp32 ulp of the loss): its online sum orders the additions differently."""
    train = _train_kernel_loss(x, y, V)
    err_new = (loss.double() - want).abs()
    err_old = (train.double() - want).abs().max().item()
    print(f"{tag}: max loss-row error eval_rows {err_new.max().item():.3e}  "
          f"training kernel {err_old:.3e}")
    bound = torch.maximum(torch.full_like(want, 2 * err_old), _ulp32(want))
    assert (err_new <= bound).all(), (err_new, bound)


@pytest.mark.parametrize("i,shape", list(enumerate(FP32_SHAPES)))
def test_eval_rows_fp32(i, shape):
    N, V, ld = shape
    ldt = (torch.int64, torch.int32)[i % 2]
    x, y = _draw(torch.float32, N, V, ld, seed=10 + i)
    loss, want, _ = _check_ranks(x, y, V, ldt)
    _check_loss(f"fp32 {shape}", x, y, V, loss, want)
    xf, yf = _forced(torch.float32, V, ld, 10 + i, ignored=(-1, V)[i % 2])
    lf, wf, rf = _check_ranks(xf, yf, V, ldt)
    _check_forced(lf, wf, rf, yf, V)
    _check_loss(f"fp32 {shape} forced", xf[:3], yf[:3], V, lf[:3], wf[:3])


@pytest.mark.parametrize("i,shape", list(enumerate(BF16_SHAPES)))
def test_eval_rows_bf16(i, shape):
    N, V, ld = shape
    ldt = (torch.int64, torch.int32)[i % 2]
    x, y = _draw(BF16, N, V, ld, seed=20 + i)
    loss, want, _ = _check_ranks(x, y, V, ldt)
    _check_loss(f"bf16 {shape}", x, y, V, loss, want)
    xf, yf = _forced(BF16, V, ld, 20 + i, ignored=(V, -1)[i % 2])
    lf, wf, rf = _check_ranks(xf, yf, V, ldt)
    _check_forced(lf, wf, rf, yf, V)
    _check_loss(f"bf16 {shape} forced", xf[:3], yf[:3], V, lf[:3], wf[:3])


def test_eval_rows_takes_the_padded_vocabulary_view_in_place(monkeypatch):
    """The [:, :V] view of a [3, 30528] bf16 tensor (what BertForPreTraining.forward returns)
    goes to the kernel as it is: same data_ptr, row stride 30528, no copy."""
    V, ld = 30522, 30528
    x, y = _draw(BF16, 3, V, ld, seed=31)
    seen = []
    real = native._K.eval_rows

    def spy(ptr, elem_bytes, *rest):
        seen.append((ptr, elem_bytes, rest[3], rest[4]))       # V, ld
        return real(ptr, elem_bytes, *rest)

    monkeypatch.setattr(native._K, "eval_rows", spy)
    want_loss, want_rank = reference.eval_rows(x, y, vocab=V, loss_dtype=torch.float64)
    xg = x.cuda()
    view = xg[:, :V]
    assert not view.is_contiguous()
    loss, rank = ops.eval_rows(view, y.cuda())
    torch.cuda.synchronize()
    assert seen == [(xg.data_ptr(), 2, V, ld)]
    assert torch.equal(rank.cpu(), want_rank)
    _check_loss("bf16 view (3, 30522, 30528)", x, y, V, loss.cpu(), want_loss)
    xf, yf = _forced(BF16, V, ld, 31, ignored=-1)
    lf, wf, rf = _check_ranks(xf, yf, V, torch.int64, view=True)
    _check_forced(lf, wf, rf, yf, V)


def test_eval_rows_unaligned_base_and_checks():
    """A view whose first element is not 16-byte aligned, and the launcher's refusals."""
    V = 77
    x, y = _draw(BF16, 6, V, V, seed=41)
    buf = torch.zeros(6 * V + 3, dtype=BF16, device="cuda")
    buf[3:] = x.cuda().reshape(-1)
    view = buf[3:].view(6, V)
    assert view.data_ptr() % 16 == 6
    _, want_rank = reference.eval_rows(x, y)
    _, rank = ops.eval_rows(view, y.cuda())
    assert torch.equal(rank.cpu(), want_rank)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="too large"):     # > 2 GiB of addressing: refused
        native._K.eval_rows(view.data_ptr(), 2, y.cuda().data_ptr(), 8, 40000, 30522, 30528, 0, 0,
                            st)
    with pytest.raises(RuntimeError, match="row stride"):
        native._K.eval_rows(view.data_ptr(), 2, y.cuda().data_ptr(), 8, 6, V, V - 1, 0, 0, st)


# ----------------------------------------------------------------------------- accumulate
def _accumulate_oracle(loss, rank, w, k):
    w = (rank >= 0).double() * (torch.ones_like(loss, dtype=torch.float64) if w is None
                                else w.double())
    loss = torch.where(w != 0, loss.double(), torch.zeros_like(w))
    return torch.stack([w.sum(), (w * loss).sum(), (w * (rank < 1)).sum(), (w * (rank < k)).sum()])


def test_metrics_accumulate_exact_counts_and_bit_identical_runs():
    """N = 1030 rows: every thread of the one block makes more than four trips."""
    N, V, k = 1030, 10, 3
    x, y = _draw(torch.float32, N, V, V, seed=51)
    y[::97] = -1                                             # some ignored rows
    g = torch.Generator().manual_seed(52)
    w01 = torch.randint(0, 2, (N,), generator=g).float()
    wf = torch.rand(N, generator=g)
    loss, rank = ops.eval_rows(x.cuda(), y.cuda())
    lc, rc = loss.cpu(), rank.cpu()
    for w in (None, w01, wf):
        states = []
        for _ in range(2):
            st = torch.zeros(4, dtype=torch.float64, device="cuda")
            native.metrics_accumulate(st, loss, rank, None if w is None else w.cuda(), k)
            native.metrics_accumulate(st, loss, rank, None if w is None else w.cuda(), k)
            states.append(st.cpu())
        assert torch.equal(states[0], states[1])             # bit-identical runs
        want = 2 * _accumulate_oracle(lc, rc, w, k)
        got = states[0]
        if w is not wf:                                       # 0/1 weights: exact integers
            assert torch.equal(got[[0, 2, 3]], want[[0, 2, 3]]), (got, want)
            assert got[0].item() == float(int(got[0].item())) and got[0].item() > 0
        assert ((got - want).abs() <= 1e-12 * want.abs()).all(), (got, want)


def test_classification_metrics_gpu_matches_cpu_class():
    N, V = 300, 40
    x, y = _draw(BF16, N, V, V, seed=61)
    w = (torch.arange(N) % 3 != 0).float()
    gpu = ClassificationMetrics(k=5)
    for i in range(3):
        s = slice(100 * i, 100 * (i + 1))
        gpu.update(x[s].cuda(), y[s].cuda(), w[s].cuda())
    assert gpu.state.is_cuda and gpu.state.dtype == torch.float64
    want = ClassificationMetrics(k=5).update(x, y, w).result()
    got = gpu.result()
    assert got["count"] == want["count"] == 200.0
    assert got["top_1"] == want["top_1"] and got["top_k"] == want["top_k"]
    assert abs(got["loss"] - want["loss"]) < 1e-6 * want["loss"]   # fp32 loss rows vs fp64


# ----------------------------------------------------------------------------- end to end
def test_evaluate_mnist_cnn_bf16_hits_equal_oracle_on_own_logits():
    from distributedtensorflow_amd.data import DeviceArrayDataset, mnist
    imgs, labels = mnist.synthetic_mnist(64, seed=5)
    torch.manual_seed(0)
    model = dtf.models.MnistCNN().cuda()
    data = DeviceArrayDataset(imgs.reshape(64, 784), labels, 24, "cuda", BF16)
    m = ClassificationMetrics(k=3)
    res = dtf.train.evaluate(model, data.single_pass(), m)
    assert model.training and res["count"] == 64.0
    hits1 = hitsk = 0
    model.eval()
    with torch.no_grad():
        for x, y in data.single_pass():
            assert x.dtype == BF16
            _, rank = reference.eval_rows(model(x).cpu(), y.cpu())
            hits1 += int((rank < 1).sum())
            hitsk += int((rank < 3).sum())
    assert m.state.cpu()[[0, 2, 3]].tolist() == [64.0, float(hits1), float(hitsk)]


def test_evaluate_bert_padded_vocab_view_with_weights():
    from distributedtensorflow_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=1000, hidden_size=256, num_hidden_layers=2,
                     num_attention_heads=4, intermediate_size=512, max_position_embeddings=128)
    model = BertForPreTraining(cfg).cuda()
    # sequence length 64: the shortest the native attention kernels take
    data = dtf.data.SyntheticMLM(4, 64, vocab_size=1000, max_predictions=8, device="cuda",
                                 seed=9, pool=1)
    batch = dict(data.batches[0])
    w = torch.ones(4, 8, device="cuda")
    w[:, ::2] = 0                                            # half the masked_lm_weights are 0
    batch["masked_lm_weights"] = w
    m = ClassificationMetrics(k=5)
    res = dtf.train.evaluate(model, [batch], m)
    assert model.training and res["count"] == 16.0
    model.eval()
    with torch.no_grad():
        logits = model(batch["input_ids"], batch["segment_ids"], batch["input_mask"],
                       batch["masked_lm_positions"])
    assert logits.shape == (32, 1000) and logits.stride(0) == 1024 and logits.dtype == BF16
    _, rank = reference.eval_rows(logits.cpu(), batch["masked_lm_ids"].cpu())
    keep = w.reshape(-1).cpu() > 0
    assert m.state.cpu()[[0, 2, 3]].tolist() == [16.0, float((rank[keep] < 1).sum()),
                                                  float((rank[keep] < 5).sum())]


def _resnet_steps(eval_after):
    from distributedtensorflow_amd.models import resnet50
    from distributedtensorflow_amd.optimizers import MomentumOptimizer
    from distributedtensorflow_amd.parallel import OneDeviceStrategy
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(4, 64, 64, 3, generator=g).cuda().to(BF16) for _ in range(4)]
    ys = [torch.randint(0, 1000, (4,), generator=g).cuda() for _ in range(4)]
    losses, res = [], None
    with OneDeviceStrategy("cuda").scope():
        model = resnet50().cuda()
        opt = MomentumOptimizer(0.05, 0.9, weight_decay=1e-4)
        opt.build(list(model.parameters()))
        for step in range(4):
            loss = ops.sparse_softmax_cross_entropy(model(xs[step]), ys[step])
            opt.minimize(loss)
            losses.append(loss.detach().clone())
            if eval_after is not None and step + 1 == eval_after:
                live = records.live_count()
                res = dtf.train.evaluate(model, [(xs[3], ys[3]), (xs[0], ys[0])],
                                         ClassificationMetrics(k=5), optimizer=opt)
                assert model.training and records.live_count() == live
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return losses, state, res


def test_resnet_training_is_unperturbed_by_an_evaluation_between_steps():
    """2 steps, an evaluation, 2 steps == 4 steps: losses, parameters and BatchNorm moving
    statistics bit-identical (4 x 64 x 64 x 3: the geometry tests/test_resnet_gpu.py trains at)."""
    plain_losses, plain_state, _ = _resnet_steps(None)
    losses, state, res = _resnet_steps(2)
    assert res["count"] == 8.0 and res["loss"] > 0
    assert any("moving_mean" in k for k in state) and any("moving_variance" in k for k in state)
    for a, b in zip(losses, plain_losses):
        assert torch.equal(a, b)
    for k in plain_state:
        assert torch.equal(state[k], plain_state[k]), k
