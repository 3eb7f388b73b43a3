"""Masked temporal loss kernels (``mask_count_inv`` / ``temporal_xent`` / ``temporal_reg`` in csrc/kernels/loss.hip)
against the float64 oracles of ``temporal_oracle.py``, and the two per-time-step zoo models on the GPU.

Kernel tolerances are the project's own for fp32 loss kernels (``test_prob_xent_matches_fp32``,
``test_mse_kernel_matches_reference``): loss within ``1e-5 * max(1, |ref|)``, gradient ``rtol=1e-5, atol=1e-6``.
The softmax kernel uses ``expf`` / ``logf`` (not the fast intrinsics), so this tight bound is the one that holds for
the softmax gradient too; the looser bound of ``test_softmax_xent`` is not used."""
import functools

import numpy as np
import pytest
import torch

from masking_oracle import patterns
from temporal_oracle import reg_oracle, xent_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (B, T, K): degenerate minimum; rows not a multiple of the 4 rows per workgroup; exactly one lane pass; crossing the
# wavefront width; several lane passes; 1,030 rows, past one 1,024-thread stride of the row reduce
SHAPES = [(1, 1, 1), (3, 5, 3), (5, 7, 64), (5, 7, 65), (2, 3, 130), (10, 103, 5)]


@functools.lru_cache(maxsize=None)
def _xent_case(shape, form, masked):
    B, T, K = shape
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + K)
    logits = torch.randn(B, T, K, generator=g) * 2.0
    labels = torch.randint(0, K, (B, T), generator=g)
    probs = torch.softmax(torch.randn(B, T, K, generator=g), -1)
    mask = patterns(B, T) if masked else None
    kw = {"labels": labels} if form == "sparse" else {"probs": probs}
    return logits, kw, mask, xent_oracle(logits, mask, **kw)


@functools.lru_cache(maxsize=None)
def _reg_case(B, T, F, mae, masked):
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + F)
    pred, target = torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
    pred[0, 0] = target[0, 0]  # sign(0) = 0
    mask = patterns(B, T) if masked else None
    return pred, target, mask, reg_oracle(pred, target, mask, mae)


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(fn, x, *a, scale=None, **kw):
    xl = x.to(DEV).requires_grad_(True)
    loss = fn(xl, *a, **kw)
    (loss if scale is None else loss * scale).backward()
    return loss.detach().cpu(), xl.grad.cpu()


def _check(loss, grad, ref_loss, ref_grad):
    err = float((grad.double() - ref_grad).abs().max())
    print(f"loss {float(loss):.8g} ref {float(ref_loss):.8g}; max |grad - ref| {err:.3g} of {float(ref_grad.abs().max()):.3g}")
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
    assert torch.allclose(grad.double(), ref_grad, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["sparse", "dense"])
@pytest.mark.parametrize("shape", SHAPES)
def test_temporal_xent_kernel_matches_float64_oracle(shape, form, masked):
    from distributeddeeplearningspark_amd.ops.loss import temporal_softmax_cross_entropy as txe

    logits, kw, mask, (rl, rg) = _xent_case(shape, form, masked)
    loss, grad = _run(txe, logits, mask=_dev(mask), **{k: v.to(DEV) for k, v in kw.items()})
    _check(loss, grad, rl, rg)
    if masked:
        assert (grad[mask == 0] == 0).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mae", [False, True])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("bt", sorted({s[:2] for s in SHAPES}))
def test_temporal_regression_kernel_matches_float64_oracle(bt, F, mae, masked):
    from distributeddeeplearningspark_amd.ops import loss as L

    pred, target, mask, (rl, rg) = _reg_case(*bt, F, mae, masked)
    fn = L.temporal_mean_absolute_error if mae else L.temporal_mean_squared_error
    loss, grad = _run(fn, pred, target.to(DEV), mask=_dev(mask))
    _check(loss, grad, rl, rg)
    assert (grad[0, 0] == 0).all()
    if masked:
        assert (grad[mask == 0] == 0).all()


def _all_ops(shape=(3, 5, 3)):
    """(name, fn(x, mask), x) of the three ops in both target forms at one small shape."""
    from distributeddeeplearningspark_amd.ops import loss as L

    logits, kw, _, _ = _xent_case(shape, "sparse", True)
    _, kwd, _, _ = _xent_case(shape, "dense", True)
    pred, target, _, _ = _reg_case(*shape[:2], 3, False, True)
    labels, probs, target = kw["labels"].to(DEV), kwd["probs"].to(DEV), target.to(DEV)
    return [
        ("xent_sparse", lambda x, m, lab=labels: L.temporal_softmax_cross_entropy(x, labels=lab, mask=m), logits),
        ("xent_dense", lambda x, m, p=probs: L.temporal_softmax_cross_entropy(x, probs=p, mask=m), logits),
        ("mse", lambda x, m, t=target: L.temporal_mean_squared_error(x, t, mask=m), pred),
        ("mae", lambda x, m, t=target: L.temporal_mean_absolute_error(x, t, mask=m), pred),
    ]


def test_all_zero_mask_gives_exact_zeros():
    for name, fn, x in _all_ops():
        loss, grad = _run(fn, x, torch.zeros(x.shape[:2], dtype=torch.uint8, device=DEV))
        assert loss.item() == 0.0 and torch.isfinite(grad).all() and (grad == 0).all(), name


def test_values_at_masked_rows_do_not_matter():
    from distributeddeeplearningspark_amd.ops import loss as L

    B, T, K = 7, 5, 3
    mask = patterns(B, T)
    off = mask == 0
    for name, fn, x in _all_ops((B, T, K)):
        dirty_fn = fn
        if name == "xent_sparse":
            bad = _xent_case((B, T, K), "sparse", True)[1]["labels"].clone()
            bad[off] = -1
            bad[4] = K + 5  # the fully masked row
            bad = bad.to(DEV)
            dirty_fn = lambda x, m: L.temporal_softmax_cross_entropy(x, labels=bad, mask=m)
        dirty = x.clone()
        dirty[off] = float("nan")
        l0, g0 = _run(fn, x, mask.to(DEV))
        l1, g1 = _run(dirty_fn, dirty, mask.to(DEV))
        assert l0.item() == l1.item() and torch.equal(g0, g1), name
        assert (g1[off] == 0).all() and torch.isfinite(g1).all(), name


@pytest.mark.parametrize("form", ["sparse", "dense"])
def test_all_ones_mask_matches_softmax_cross_entropy_on_the_reshape(form):
    from distributeddeeplearningspark_amd.ops import loss as L

    B, T, K = 5, 7, 65
    logits, kw, _, _ = _xent_case((B, T, K), form, False)
    ones = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    kwd = {k: v.to(DEV) for k, v in kw.items()}
    loss, grad = _run(L.temporal_softmax_cross_entropy, logits, mask=ones, **kwd)
    flat = {"labels": kwd["labels"].reshape(-1)} if form == "sparse" else {"probs": kwd["probs"].reshape(B * T, K)}
    rl, rg = _run(lambda x: L.softmax_cross_entropy(x.reshape(B * T, K), **flat), logits)
    _check(loss, grad, rl.double(), rg.double())


def test_backward_under_a_non_unit_seed_scales_the_gradient():
    for name, fn, x in _all_ops():
        mask = patterns(*x.shape[:2]).to(DEV)
        l1, g1 = _run(fn, x, mask)
        l3, g3 = _run(fn, x, mask, scale=3.0)
        assert l1.item() == l3.item(), name
        assert torch.allclose(g3, g1 * 3.0, rtol=1e-6, atol=0), name


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


_LOSS_KERNELS = ("mask_count_inv", "temporal_xent", "temporal_reg", "rows_sum_scaled")


def test_loss_and_gradient_take_at_most_three_launches_of_project_kernels():
    """The forward computes the loss AND stores the gradient: masked xent = count + sweep + row reduce, unmasked xent
    = sweep + row reduce, MSE / MAE = one launch; nothing else runs on the device."""
    want = {"xent_sparse": 3, "xent_dense": 3, "mse": 1, "mae": 1}
    for name, fn, x in _all_ops((10, 103, 3)):
        xd, mask = x.to(DEV), patterns(*x.shape[:2]).to(DEV)
        fn(xd, mask)  # warm-up: code object load
        for m, n in ((mask, want[name]), (None, min(want[name], 2))):
            names = _kernel_names(lambda: fn(xd, m))
            assert len(names) == n and all("ddl::" in k for k in names), (name, names)
            assert all(any(t in k for t in _LOSS_KERNELS) for k in names), (name, names)


# ------------------------------------------------------------------------------------------------ step level
# torch kernels that would mean a layer's COMPUTE fell back to ATen / MIOpen / hipBLASLt (tests/test_gpu_masking.py)
_DENY = ("tanh", "sigmoid", "elu", "gelu", "softplus", "softmax", "dropout", "bernoulli", "avg_pool", "AvgPool",
         "avgpool", "embedding", "index_add", "indexing_backward", "Cijk", "gemm", "Gemm", "addmm", "nll", "max_pool",
         "MaxPool", "miopen", "rnn", "lstm", "gru", "relu", "threshold", "erf", "exp_kernel", "sort", "rocprim",
         "radix", "layer_norm", "LayerNorm", "cross_entropy", "log_softmax")


def _zoo_case(which):
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.utils import pad_sequences

    rng = np.random.default_rng(0)
    if which == "tagger":
        m = zoo.sequence_tagger(50, 9, 5, embed_dim=8, units=64)
        x = pad_sequences([list(rng.integers(1, 50, n)) for n in (9, 3, 1, 6, 5, 0)], maxlen=9, dtype="int64")
        y = rng.integers(0, 5, x.shape)
        m.compile("adam", "sparse_categorical_crossentropy")
    else:
        m = zoo.masked_seq2seq_regressor(units=64, seq_len=7)
        x = rng.random((6, 7, 1), dtype=np.float32) + 0.1
        x[patterns(6, 7).numpy() == 0] = 0.0
        y = rng.random((6, 7, 1), dtype=np.float32)
        m.compile("adagrad", "mean_squared_error")
    return m, x, y


@pytest.mark.parametrize("which", ["tagger", "regressor"])
def test_zoo_training_step_runs_only_hip_compute(which):
    m, x, y = _zoo_case(which)
    m.place(DEV, seed=0)
    xd, yd = m.to_input(x), m.to_target(y)
    m.train_on_batch(xd, yd)  # warm-up (lazy workspaces)
    names = _kernel_names(lambda: m.train_on_batch(xd, yd))
    fallen = sorted({n for n in names if "ddl::" not in n and any(d in n for d in _DENY)})
    assert not fallen, f"layer compute ran on torch kernels: {fallen}"
    assert any("mask_from_" in n for n in names), names
    loss = [n for n in names if any(t in n for t in _LOSS_KERNELS)]
    assert any("temporal_xent" in n if which == "tagger" else "temporal_reg" in n for n in loss), names
    assert 1 <= len(loss) <= 3, loss


def test_masked_seq2seq_graph_step_matches_eager(monkeypatch):
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.models.step import CompiledTrainStep

    steps, bs = 8, 8
    g = torch.Generator().manual_seed(0)
    x = torch.rand(bs * steps, 7, 1, generator=g) + 0.1
    x[patterns(bs * steps, 7) == 0] = 0.0
    x, y = x.numpy(), torch.rand(bs * steps, 7, 1, generator=g).numpy()
    res = {}
    for graphs in (False, True):
        monkeypatch.setenv("DDL_GRAPHS", "1" if graphs else "0")
        m = zoo.masked_seq2seq_regressor(units=64, seq_len=7)
        m.compile("adagrad", "mean_squared_error")
        m.place(DEV, seed=3)
        st = CompiledTrainStep(m)
        xs, ys = m.to_input(x), m.to_target(y)
        losses = [float(st(xs[i * bs:(i + 1) * bs], ys[i * bs:(i + 1) * bs])) for i in range(steps)]
        torch.cuda.synchronize()
        assert st.captured == graphs, st.fallback_reason
        res[graphs] = (np.array(losses), m.arena.master.detach().cpu().clone())
    (le, we), (lg, wg) = res[False], res[True]
    assert np.allclose(le, lg, rtol=2e-3, atol=1e-5), (le, lg)
    rel = ((we - wg).norm() / we.norm()).item()
    assert rel < 2e-3, rel


def test_sequence_tagger_matches_cpu():
    """Three SGD steps of the tagger on the GPU against the same weights on the CPU (the bound of
    test_text_lstm_classifier_matches_cpu, per step)."""
    def build(dev):
        m, x, y = _zoo_case("tagger")
        m.compile("sgd", "sparse_categorical_crossentropy")
        m.place(dev, seed=0)
        return m, x, y

    (mc, x, y), (mg, _, _) = build("cpu"), build(DEV)
    mg.set_weights(mc.get_weights())
    assert mg.compute_dtype == torch.float32
    for step in range(3):
        lc = float(mc.backward_step(mc.to_input(x), mc.to_target(y)).detach())
        lg = float(mg.backward_step(mg.to_input(x), mg.to_target(y)).detach())
        gc_ = mc.arena.to_canonical(mc.arena.grad).detach()
        gg = mg.arena.to_canonical(mg.arena.grad).detach().cpu()
        rel = ((gg - gc_).norm() / gc_.norm()).item()
        print(f"step {step}: loss cpu {lc:.6g} gpu {lg:.6g}; arena gradient rel L2 {rel:.3g}")
        assert abs(lg - lc) <= 1e-4 * abs(lc), (lc, lg)
        assert rel < 1e-4, rel
        mc.optimizer.step(1.0)
        mg.optimizer.step(1.0)
