"""Directed recurrent kernels (``go_backwards`` / ``Bidirectional``, csrc/kernels/rnn.hip) vs the CPU oracle.

The oracle is the forward-direction reference on flipped tensors (``recurrent_ref(cell, x.flip(1), ...)``), flipped
back where the sequence is returned in input order; tolerance as ``test_gpu_rnn.py``: relative L2 < 1e-4."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, T, I, H): reg path + fused input + ragged 2-row workgroup; reg path + projection GEMM; T = 1 (every prefetch
# out of range); generic kernels + ragged 4-row workgroup; GRU with 2H % 64 != 0 (unfused parameter gradients)
SHAPES = [(5, 7, 3, 64), (6, 4, 12, 128), (3, 1, 2, 64), (3, 5, 2, 32), (2, 3, 2, 16)]
GATES = {"gru": 3, "lstm": 4, "rnn": 1}


@functools.lru_cache(maxsize=None)
def _case(cell, rs, shape, ract="hard_sigmoid"):
    """Inputs and the two directions' CPU reference outputs (autograd graphs kept), computed once per case."""
    from distributeddeeplearningspark_amd.ops.rnn import recurrent_ref

    B, T, I, H = shape
    G = GATES[cell]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, I, generator=g)
    ws = []
    for _ in range(2):
        ws += [torch.randn(I, G * H, generator=g) * 0.3, torch.randn(H, G * H, generator=g) * (1.0 / H ** 0.5),
               torch.randn(G * H, generator=g) * 0.1]
    dy = torch.randn(B, T, 2 * H, generator=g) if rs else torch.randn(B, 2 * H, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (x, *ws)]
    yf = recurrent_ref(cell, leaves[0], *leaves[1:4], rs, "tanh", ract)
    yb = recurrent_ref(cell, leaves[0].flip(1), *leaves[4:7], rs, "tanh", ract)  # processing order
    return x, ws, dy, leaves, yf, yb


def _check(got, want):
    for what, a, r in zip(("y", "dx", "dW", "dU", "db", "dWb", "dUb", "dbb"), got, want):
        err = ((a.detach().cpu().float() - r.detach()).norm() / (r.norm() + 1e-12)).item()
        print(f"{what}: rel L2 {err:.3g}")
        assert err < 1e-4, (what, err)


def _run_reverse(cell, rs, shape, ract="hard_sigmoid"):
    from distributeddeeplearningspark_amd.ops import rnn as R

    x, ws, dy, leaves, _, yb = _case(cell, rs, shape, ract)
    H = shape[3]
    dyh = dy[..., H:].contiguous()
    ref = torch.autograd.grad(yb, [leaves[0], *leaves[4:7]], dyh, retain_graph=True)
    grads = [torch.zeros_like(t, device="cuda") for t in ws[3:]]
    xg = x.cuda().requires_grad_(True)
    y = R.recurrent(cell, xg, *(t.cuda() for t in ws[3:]), grads=tuple(grads), return_sequences=rs,
                    recurrent_activation=ract, go_backwards=True)
    y.backward(dyh.cuda())
    _check([y, xg.grad, *grads], [yb, *ref])


def _run_bidir(cell, rs, shape, merge, ract="hard_sigmoid"):
    from distributeddeeplearningspark_amd.ops import rnn as R

    x, ws, dy, leaves, yf, yb = _case(cell, rs, shape, ract)
    H = shape[3]
    ybi = yb.flip(1) if rs else yb
    if merge == "concat":
        yr, dyr = torch.cat([yf, ybi], -1), dy
    else:
        yr, dyr = (yf + ybi if merge == "sum" else (yf + ybi) / 2), dy[..., :H].contiguous()
    ref = torch.autograd.grad(yr, leaves, dyr, retain_graph=True)
    wd = [t.cuda() for t in ws]
    grads = [torch.zeros_like(t) for t in wd]
    xg = x.cuda().requires_grad_(True)
    y = R.bidirectional(cell, xg, wd[:3], wd[3:], grads=(grads[:3], grads[3:]), merge_mode=merge,
                        return_sequences=rs, recurrent_activation=ract)
    y.backward(dyr.cuda())
    _check([y, xg.grad, *grads], [yr, *ref])


def _cases():
    for shape in SHAPES:
        for cell in ("gru", "lstm"):
            if shape[3] == 16 and cell != "gru":
                continue
            for rs in (False, True):
                yield pytest.param(cell, rs, shape, id=f"{cell}-rs{int(rs)}-{'x'.join(map(str, shape))}")


@pytest.mark.parametrize("cell,rs,shape", list(_cases()))
def test_reverse_matches_flip_oracle(cell, rs, shape):
    _run_reverse(cell, rs, shape)


@pytest.mark.parametrize("cell,rs,shape", list(_cases()))
def test_bidirectional_concat_matches_flip_oracle(cell, rs, shape):
    _run_bidir(cell, rs, shape, "concat")


@pytest.mark.parametrize("merge", ["sum", "ave"])
@pytest.mark.parametrize("rs", [False, True])
def test_bidirectional_sum_ave(merge, rs):
    _run_bidir("gru", rs, (5, 7, 3, 64), merge)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_generic_kernels_at_reg_width(cell):
    """recurrent_activation='sigmoid' at H = 64: the generic kernels at a width the reg path would serve."""
    _run_reverse(cell, True, (5, 7, 3, 64), "sigmoid")
    _run_bidir(cell, True, (5, 7, 3, 64), "concat", "sigmoid")


@pytest.mark.parametrize("rs", [False, True])
def test_simple_rnn_directed(rs):
    _run_reverse("rnn", rs, (3, 5, 2, 32))
    _run_bidir("rnn", rs, (3, 5, 2, 32), "concat")


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


@pytest.mark.parametrize("merge", ["concat", "sum"])
def test_one_recurrence_launch_per_pass_and_no_aten_kernels(merge):
    from torch.profiler import ProfilerActivity, profile

    from distributeddeeplearningspark_amd.ops import rnn as R

    x, ws, dy, *_ = _case("gru", True, (5, 7, 3, 64))
    wd = [t.cuda() for t in ws]
    grads = [torch.zeros_like(t) for t in wd]  # fp32 contiguous buffers, as the arena's slices
    dyd = (dy if merge == "concat" else dy[..., :64]).contiguous().cuda()
    xl = x.cuda().requires_grad_(True)
    box = []

    def step():
        y = R.bidirectional("gru", _Sink.apply(xl, box), wd[:3], wd[3:], grads=(grads[:3], grads[3:]),
                            merge_mode=merge, return_sequences=True)
        y.backward(dyd)

    step()  # warm-up: code object load
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(box) == 2 and box[-1].shape == x.shape
    assert sum("rnn_fwd" in n for n in names) == 1, names
    assert sum("rnn_bwd" in n for n in names) == 1, names
    assert not [n for n in names if "at::native" in n], names


def test_bigru_graph_step_matches_eager(monkeypatch):
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.models.step import CompiledTrainStep

    steps, bs = 8, 8
    g = torch.Generator().manual_seed(0)
    x = torch.rand(bs * steps, 7, 1, generator=g).numpy()
    y = torch.rand(bs * steps, 1, generator=g).numpy()
    res = {}
    for graphs in (False, True):
        monkeypatch.setenv("DDL_GRAPHS", "1" if graphs else "0")
        m = zoo.bigru_regressor(units=64, seq_len=7)
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


def test_stacked_directed_model_matches_cpu():
    from distributeddeeplearningspark_amd.models import GRU, Bidirectional, Dense, Sequential

    def build(dev):
        m = Sequential([Bidirectional(GRU(64, return_sequences=True), input_shape=(6, 3)), GRU(32, go_backwards=True),
                        Dense(1)])
        m.compile("sgd", "mean_squared_error")
        m.place(dev, seed=0)
        return m

    mc, mg = build("cpu"), build("cuda:0")
    mg.set_weights(mc.get_weights())
    assert mg.compute_dtype == torch.float32
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(5, 6, 3, generator=g), torch.randn(5, 1, generator=g)
    lc = float(mc.backward_step(mc.to_input(x), mc.to_target(y)).detach())
    lg = float(mg.backward_step(mg.to_input(x), mg.to_target(y)).detach())
    gc_ = mc.arena.to_canonical(mc.arena.grad).detach()
    gg = mg.arena.to_canonical(mg.arena.grad).detach().cpu()
    rel = ((gg - gc_).norm() / gc_.norm()).item()
    print(f"loss cpu {lc:.6g} gpu {lg:.6g}; arena gradient rel L2 {rel:.3g}")
    assert abs(lg - lc) <= 1e-4 * abs(lc), (lc, lg)
    assert rel < 1e-4, rel
