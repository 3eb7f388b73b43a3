"""Masked recurrent kernels (MASK instantiations in csrc/kernels/rnn.hip) and the mask-derivation kernels vs the
compaction oracle on the CPU (``masking_oracle.py``: the unmasked ``recurrent_ref`` over each row's unmasked steps).
Tolerance as ``test_gpu_rnn.py`` / ``test_gpu_birnn.py``: relative L2 < 1e-4."""
import functools

import numpy as np
import pytest
import torch

from masking_oracle import GATES, bidir_oracle, oracle, patterns, rel_l2, weights

pytestmark = pytest.mark.gpu

# (B, T, I, H), the directed tests' shapes: reg path + fused input + ragged 2-row workgroup; reg path + projection
# GEMM; T = 1 (every prefetch out of range, the single step masked in one row); generic kernels + ragged 4-row
# workgroup; GRU with 2H % 64 != 0 (unfused parameter gradients)
SHAPES = [(5, 7, 3, 64), (6, 4, 12, 128), (3, 1, 2, 64), (3, 5, 2, 32), (2, 3, 2, 16)]


@functools.lru_cache(maxsize=None)
def _case(cell, rs, shape, ract="hard_sigmoid"):
    """Inputs, mask and the CPU oracle outputs of the forward, the go_backwards and the Bidirectional (concat, sum)
    layer, autograd graphs kept; computed once per case."""
    B, T, I, H = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, I, generator=g)
    ws = weights(cell, I, H, g, 2)
    dy = torch.randn(B, T, 2 * H, generator=g) if rs else torch.randn(B, 2 * H, generator=g)
    mask = patterns(B, T)
    leaves = [t.clone().requires_grad_(True) for t in (x, *ws)]
    yf = oracle(cell, leaves[0], *leaves[1:4], rs, mask, False, "tanh", ract)
    yb = oracle(cell, leaves[0], *leaves[1:4], rs, mask, True, "tanh", ract)  # the same weights, processed backwards
    ybi = {m: bidir_oracle(cell, leaves[0], leaves[1:4], leaves[4:], rs, mask, m, "tanh", ract) for m in ("concat", "sum")}
    return x, ws, dy, mask, leaves, yf, yb, ybi


def _check(got, want):
    for what, a, r in zip(("y", "dx", "dW", "dU", "db", "dWb", "dUb", "dbb"), got, want):
        err = rel_l2(a, r)
        print(f"{what}: rel L2 {err:.3g}")
        assert err < 1e-4, (what, err)


def _run_one(cell, rs, shape, rev, ract="hard_sigmoid"):
    from distributeddeeplearningspark_amd.ops import rnn as R

    x, ws, dy, mask, leaves, yf, yb, _ = _case(cell, rs, shape, ract)
    B, T, I, H = shape
    yr = yb if rev else yf
    dyh = dy[..., :H].contiguous()
    ref = torch.autograd.grad(yr, leaves[:4], dyh, retain_graph=True)
    grads = [torch.zeros_like(t, device="cuda") for t in ws[:3]]
    xg = x.cuda().requires_grad_(True)
    y = R.recurrent(cell, xg, *(t.cuda() for t in ws[:3]), grads=tuple(grads), return_sequences=rs,
                    recurrent_activation=ract, go_backwards=rev, mask=mask.cuda())
    y.backward(dyh.cuda())
    _check([y, xg.grad, *grads], [yr, *ref])
    assert (xg.grad.cpu()[mask == 0] == 0).all(), "dx must be exactly zero at masked steps"
    if rs:  # a masked position repeats the preceding processed position bit for bit (zeros when there is none)
        yc = y.detach().cpu()
        mp = mask.flip(1) if rev else mask  # processing order, as the returned sequence
        for r in range(B):
            for s in range(T):
                if not mp[r, s]:
                    assert torch.equal(yc[r, s], yc[r, s - 1] if s else torch.zeros(H)), (r, s)


def _run_bidir(cell, rs, shape, merge, ract="hard_sigmoid"):
    from distributeddeeplearningspark_amd.ops import rnn as R

    x, ws, dy, mask, leaves, _, _, ybi = _case(cell, rs, shape, ract)
    H = shape[3]
    yr = ybi[merge]
    dyr = dy if merge == "concat" else dy[..., :H].contiguous()
    ref = torch.autograd.grad(yr, leaves, dyr, retain_graph=True)
    wd = [t.cuda() for t in ws]
    grads = [torch.zeros_like(t) for t in wd]
    xg = x.cuda().requires_grad_(True)
    y = R.bidirectional(cell, xg, wd[:3], wd[3:], grads=(grads[:3], grads[3:]), merge_mode=merge,
                        return_sequences=rs, recurrent_activation=ract, mask=mask.cuda())
    y.backward(dyr.cuda())
    _check([y, xg.grad, *grads], [yr, *ref])
    assert (xg.grad.cpu()[mask == 0] == 0).all()


def _cases():
    for shape in SHAPES:
        for cell in ("gru", "lstm"):
            if shape[3] == 16 and cell != "gru":
                continue
            for rs in (False, True):
                yield pytest.param(cell, rs, shape, id=f"{cell}-rs{int(rs)}-{'x'.join(map(str, shape))}")


@pytest.mark.parametrize("cell,rs,shape", list(_cases()))
def test_masked_layer_matches_compaction_oracle(cell, rs, shape):
    _run_one(cell, rs, shape, False)


@pytest.mark.parametrize("shape", [(5, 7, 3, 64), (3, 5, 2, 32)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_masked_go_backwards_matches_compaction_oracle(cell, rs, shape):
    _run_one(cell, rs, shape, True)


@pytest.mark.parametrize("shape", [(5, 7, 3, 64), (6, 4, 12, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("merge", ["concat", "sum"])
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_masked_bidirectional_matches_compaction_oracle(cell, rs, merge, shape):
    _run_bidir(cell, rs, shape, merge)


@pytest.mark.parametrize("rs", [False, True])
def test_masked_simple_rnn(rs):
    _run_one("rnn", rs, (3, 5, 2, 32), False)
    _run_one("rnn", rs, (3, 5, 2, 32), True)
    _run_bidir("rnn", rs, (3, 5, 2, 32), "concat")


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_masked_generic_kernels_at_reg_width(cell):
    """recurrent_activation='sigmoid' at H = 64: the masked generic kernels at a width the reg path would serve."""
    _run_one(cell, True, (5, 7, 3, 64), False, "sigmoid")
    _run_one(cell, True, (5, 7, 3, 64), True, "sigmoid")
    _run_bidir(cell, True, (5, 7, 3, 64), "concat", "sigmoid")


@pytest.mark.parametrize("shape", [(5, 7, 3, 64), (6, 4, 12, 128), (3, 5, 2, 32)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_all_ones_mask_is_bit_identical_to_unmasked(cell, shape):
    """The masked instantiations with every step valid: y bit-identical to the unmasked call, gradients within the
    bound (the parameter gradients are atomic sums)."""
    from distributeddeeplearningspark_amd.ops import rnn as R

    x, ws, dy, *_ = _case(cell, True, shape)
    B, T, I, H = shape
    ones = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    wd = [t.cuda() for t in ws]
    out = {}
    for name, mk in (("plain", None), ("ones", ones)):
        grads = [torch.zeros_like(t) for t in wd]
        xg = x.cuda().requires_grad_(True)
        y = R.recurrent(cell, xg, *wd[:3], grads=tuple(grads[:3]), return_sequences=True, mask=mk)
        y.backward(dy[..., :H].contiguous().cuda())
        gb = [torch.zeros_like(t) for t in wd]
        xb = x.cuda().requires_grad_(True)
        yb = R.bidirectional(cell, xb, wd[:3], wd[3:], grads=(gb[:3], gb[3:]), return_sequences=True, mask=mk)
        yb.backward(dy.cuda())
        out[name] = ([y.detach(), yb.detach()], [xg.grad, *grads[:3], xb.grad, *gb])
    for a, b in zip(out["plain"][0], out["ones"][0]):
        assert torch.equal(a, b)
    for a, b in zip(out["plain"][1], out["ones"][1]):
        assert rel_l2(b, a.cpu()) < 1e-4


@pytest.mark.parametrize("mask_value", [0.0, -1.0])
def test_mask_derivation_kernels(mask_value):
    from distributeddeeplearningspark_amd.ops import mask as M

    g = torch.Generator().manual_seed(1)
    for B, T, F in ((3, 5, 1), (7, 9, 3), (2, 3, 130)):  # F = 1, odd sizes over several blocks, F past one wave
        x = torch.randn(B, T, F, generator=g)
        x[patterns(B, T) == 0] = mask_value
        x[0, 0, F - 1] = mask_value  # one feature equal to the value: still data when F > 1
        yr, mr = M.feature_mask_ref(x, mask_value)
        xg = x.cuda().requires_grad_(True)
        y, m = M.masking(xg, mask_value)
        assert m.dtype == torch.uint8 and torch.equal(m.cpu(), mr)
        assert torch.equal(y.detach().cpu(), yr)
        dy = torch.randn(B, T, F, generator=g)
        y.backward(dy.cuda())
        assert torch.equal(xg.grad.cpu(), dy * mr.unsqueeze(-1))
    ids = torch.randint(0, 3, (7, 9), generator=g)
    for t in (ids, ids.int()):
        m = M.ids_mask(t.cuda())
        assert m.dtype == torch.uint8 and torch.equal(m.cpu(), (ids != 0).to(torch.uint8))


def test_binding_rejects_bad_masks():
    from distributeddeeplearningspark_amd.ops._native import C

    x, ws, *_ = _case("gru", True, (3, 5, 2, 32))
    xd, wd = x.cuda(), [t.cuda() for t in ws[:3]]
    for bad in (torch.ones(3, 5, device="cuda"), torch.ones(3, 4, dtype=torch.uint8, device="cuda"),
                torch.ones(3, 5, dtype=torch.uint8), torch.ones(5, 3, dtype=torch.uint8, device="cuda").t()):
        with pytest.raises(RuntimeError, match="mask"):
            C().rnn_fwd("gru", xd, *wd, True, mask=bad)
        with pytest.raises(RuntimeError, match="mask"):
            C().birnn_fwd("gru", xd, [wd[0]] * 2, [wd[1]] * 2, [wd[2]] * 2, True, mask=bad)


class _Sink(torch.autograd.Function):
    """Identity whose backward keeps the incoming gradient and passes nothing on (no accumulation kernel)."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.box.append(g)
        return None, None


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_masked_bidirectional_is_one_recurrence_launch_per_pass():
    from distributeddeeplearningspark_amd.ops import rnn as R

    x, ws, dy, mask, *_ = _case("gru", True, (5, 7, 3, 64))
    wd = [t.cuda() for t in ws]
    grads = [torch.zeros_like(t) for t in wd]  # fp32 contiguous buffers, as the arena's slices
    dyd, md = dy.cuda(), mask.cuda()
    xl = x.cuda().requires_grad_(True)
    box = []

    def step():
        y = R.bidirectional("gru", _Sink.apply(xl, box), wd[:3], wd[3:], grads=(grads[:3], grads[3:]),
                            return_sequences=True, mask=md)
        y.backward(dyd)

    step()  # warm-up: code object load
    names = _kernel_names(step)
    assert len(box) == 2 and box[-1].shape == x.shape
    assert sum("rnn_fwd" in n for n in names) == 1, names
    assert sum("rnn_bwd" in n for n in names) == 1, names
    assert not [n for n in names if "at::native" in n], names


# torch kernels that would mean a layer's COMPUTE fell back to ATen / MIOpen / hipBLASLt (tests/test_gpu_layers.py)
_DENY = ("tanh", "sigmoid", "elu", "gelu", "softplus", "softmax", "dropout", "bernoulli", "avg_pool", "AvgPool",
         "avgpool", "embedding", "index_add", "indexing_backward", "Cijk", "gemm", "Gemm", "addmm", "nll", "max_pool",
         "MaxPool", "miopen", "rnn", "lstm", "gru", "relu", "threshold", "erf", "exp_kernel", "sort", "rocprim",
         "radix", "layer_norm", "LayerNorm", "cross_entropy", "log_softmax")


def _zoo_case(which):
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.utils import pad_sequences

    rng = np.random.default_rng(0)
    if which == "text":
        m = zoo.text_lstm_classifier(50, 9, embed_dim=8, units=64)
        x = pad_sequences([list(rng.integers(1, 50, n)) for n in (9, 3, 1, 6, 5, 2)], maxlen=9, dtype="int64")
        y = rng.integers(0, 2, (6, 1)).astype(np.float32)
        m.compile("adam", "binary_crossentropy")
    else:
        m = zoo.masked_gru_regressor(units=64, seq_len=7)
        x = rng.random((6, 7, 1), dtype=np.float32) + 0.1
        x[patterns(6, 7).numpy() == 0] = 0.0
        y = rng.random((6, 1), dtype=np.float32)
        m.compile("adagrad", "mean_squared_error")
    return m, x, y


@pytest.mark.parametrize("which", ["text", "series"])
def test_zoo_training_step_runs_only_hip_compute(which):
    m, x, y = _zoo_case(which)
    m.place("cuda:0", seed=0)
    xd, yd = m.to_input(x), m.to_target(y)
    m.train_on_batch(xd, yd)  # warm-up (lazy workspaces)
    names = set(_kernel_names(lambda: m.train_on_batch(xd, yd)))
    fallen = sorted(n for n in names if "ddl::" not in n and any(d in n for d in _DENY))
    assert not fallen, f"layer compute ran on torch kernels: {fallen}"
    assert any("mask_from_" in n for n in names), names
    assert any("rnn_fwd_reg_kernel" in n for n in names) and any("rnn_bwd_reg_kernel" in n for n in names), names


def test_masked_gru_graph_step_matches_eager(monkeypatch):
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.models.step import CompiledTrainStep

    steps, bs = 8, 8
    g = torch.Generator().manual_seed(0)
    x = torch.rand(bs * steps, 7, 1, generator=g) + 0.1
    x[patterns(bs * steps, 7) == 0] = 0.0
    x, y = x.numpy(), torch.rand(bs * steps, 1, generator=g).numpy()
    res = {}
    for graphs in (False, True):
        monkeypatch.setenv("DDL_GRAPHS", "1" if graphs else "0")
        m = zoo.masked_gru_regressor(units=64, seq_len=7)
        m.compile("adagrad", "mean_squared_error")
        m.place("cuda:0", seed=3)
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


def test_text_lstm_classifier_matches_cpu():
    """A few training steps of the text model on the GPU against the same weights on the CPU (tolerance of
    test_stacked_directed_model_matches_cpu, per step)."""
    def build(dev):
        m, x, y = _zoo_case("text")
        m.compile("sgd", "binary_crossentropy")
        m.place(dev, seed=0)
        return m, x, y

    (mc, x, y), (mg, _, _) = build("cpu"), build("cuda:0")
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
