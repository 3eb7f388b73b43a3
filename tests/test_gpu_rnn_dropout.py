"""Recurrent kernels with dropout masks (DROP instantiations in csrc/kernels/rnn.hip, the masked input projection and
the per-gate parameter-gradient tiles) vs the fold oracle on the CPU in fp32 (``rnn_dropout_oracle.py``: per batch row
the unmasked layer with the row's masks folded into W and U).  Tolerance as ``test_gpu_rnn.py`` / ``test_gpu_birnn.py``
/ ``test_gpu_masking.py``: relative L2 < 1e-4.  The masks are dense random multipliers in [0.5, 1.5] with about a
quarter of the entries 0."""
import functools

import numpy as np
import pytest
import torch

from masking_oracle import patterns, rel_l2, weights
from rnn_dropout_oracle import bidir_oracle, oracle, random_masks

pytestmark = pytest.mark.gpu

# name -> (cell, (B, T, I, H), activation, recurrent_activation)
# generic kernels: B = 6 leaves a partial 4-row workgroup; H = 24 puts LSTM / SimpleRNN gates astride the 64-column
# parameter-gradient tiles and GRU's 2H off them.  Register-resident kernels: H = 64 / 128; I = 3 would fuse the
# projection without dropout, I = 12 would not.
CASES = {f"{c}-gen": (c, (6, 5, 5, 24), "tanh", "hard_sigmoid") for c in ("gru", "lstm", "rnn")}
CASES["gru-gen-relu-sigmoid"] = ("gru", (6, 5, 5, 24), "relu", "sigmoid")
for _c in ("gru", "lstm"):
    for _h in (64, 128):
        for _i in (3, 12):
            CASES[f"{_c}-reg-h{_h}-i{_i}"] = (_c, (5, 6, _i, _h), "tanh", "hard_sigmoid")

# which masks are given, and whether a step mask (patterns: it contains a fully masked row) is
KINDS = {"in": (True, False, False), "rec": (False, True, False), "both": (True, True, False),
         "both-stepmask": (True, True, True)}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cell, (B, T, I, H), _, _ = CASES[name]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, I, generator=g)
    ws = weights(cell, I, H, g, 2)
    dys = {rs: torch.randn(B, T, 2 * H, generator=g) if rs else torch.randn(B, 2 * H, generator=g) for rs in (False, True)}
    dps = [random_masks(cell, B, I, g) for _ in range(2)]
    rdps = [random_masks(cell, B, H, g) for _ in range(2)]
    return x, ws, dys, dps, rdps, patterns(B, T)


def _check(got, want):
    for what, a, r in zip(("y", "dx", "dW", "dU", "db", "dWb", "dUb", "dbb"), got, want):
        err = rel_l2(a, r)
        print(f"{what}: rel L2 {err:.3g}")
        assert err < 1e-4, (what, err)


def _pick(ms, use, n):
    return [m if use else None for m in ms[:n]]


def _cuda(t):
    return None if t is None else t.cuda()


def _run(name, kind, layer, rs):
    from distributeddeeplearningspark_amd.ops import rnn as R

    cell, (B, T, I, H), act, ract = CASES[name]
    x, ws, dys, dps, rdps, pat = _inputs(name)
    use_dp, use_rdp, use_mask = KINDS[kind]
    mask = pat if use_mask else None
    leaves = [t.clone().requires_grad_(True) for t in (x, *ws)]
    xg = x.cuda().requires_grad_(True)
    wd = [t.cuda() for t in ws]
    grads = [torch.zeros_like(t) for t in wd]
    if layer in ("fwd", "rev"):
        rev = layer == "rev"
        (dp,), (rdp,) = _pick(dps, use_dp, 1), _pick(rdps, use_rdp, 1)
        dy = dys[rs][..., :H].contiguous()
        yr = oracle(cell, leaves[0], *leaves[1:4], rs, dp, rdp, mask, rev, act, ract)
        ref = torch.autograd.grad(yr, leaves[:4], dy)
        y = R.recurrent(cell, xg, *wd[:3], grads=tuple(grads[:3]), return_sequences=rs, activation=act,
                        recurrent_activation=ract, go_backwards=rev, mask=_cuda(mask), dropout_mask=_cuda(dp),
                        recurrent_dropout_mask=_cuda(rdp))
        y.backward(dy.cuda())
        _check([y, xg.grad, *grads[:3]], [yr, *ref])
    else:
        dp2, rdp2 = _pick(dps, use_dp, 2), _pick(rdps, use_rdp, 2)
        dy = dys[rs] if layer == "concat" else dys[rs][..., :H].contiguous()
        yr = bidir_oracle(cell, leaves[0], leaves[1:4], leaves[4:], rs, dp2, rdp2, mask, layer, act, ract)
        ref = torch.autograd.grad(yr, leaves, dy)
        y = R.bidirectional(cell, xg, wd[:3], wd[3:], grads=(grads[:3], grads[3:]), merge_mode=layer,
                            return_sequences=rs, activation=act, recurrent_activation=ract, mask=_cuda(mask),
                            dropout_mask=[_cuda(m) for m in dp2], recurrent_dropout_mask=[_cuda(m) for m in rdp2])
        y.backward(dy.cuda())
        _check([y, xg.grad, *grads], [yr, *ref])
    if mask is not None:
        assert (xg.grad.cpu()[mask == 0] == 0).all(), "dx must be exactly zero at masked steps"


@pytest.mark.parametrize("layer", ["fwd", "rev", "concat", "sum"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(CASES))
def test_dropout_kernels_match_fold_oracle(name, kind, layer):
    for rs in (False, True):
        _run(name, kind, layer, rs)


def test_wide_generic_lstm_with_staged_masks_past_64k_lds():
    """LSTM at H = 416 with a sigmoid recurrent activation: the generic forward kernel's LDS (state, gates and the
    staged masks: 160 H bytes) passes the 64 KB a launch gets by default."""
    from distributeddeeplearningspark_amd.ops import rnn as R

    B, T, I, H = 2, 2, 3, 416
    g = torch.Generator().manual_seed(1)
    x, ws = torch.randn(B, T, I, generator=g), weights("lstm", I, H, g)
    dp, rdp = random_masks("lstm", B, I, g), random_masks("lstm", B, H, g)
    dy = torch.randn(B, T, H, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (x, *ws)]
    yr = oracle("lstm", leaves[0], *leaves[1:], True, dp, rdp, None, False, "tanh", "sigmoid")
    ref = torch.autograd.grad(yr, leaves, dy)
    xg = x.cuda().requires_grad_(True)
    grads = [torch.zeros_like(t, device="cuda") for t in ws]
    y = R.recurrent("lstm", xg, *(t.cuda() for t in ws), grads=tuple(grads), return_sequences=True,
                    recurrent_activation="sigmoid", dropout_mask=dp.cuda(), recurrent_dropout_mask=rdp.cuda())
    y.backward(dy.cuda())
    _check([y, xg.grad, *grads], [yr, *ref])


def test_binding_rejects_bad_dropout_masks():
    from distributeddeeplearningspark_amd.ops._native import C

    x, ws, *_ = _inputs("gru-gen")
    B, T, I, H = CASES["gru-gen"][1]
    xd, wd = x.cuda(), [t.cuda() for t in ws[:3]]
    ok = torch.ones(3, B, I, device="cuda")
    for bad in (ok.double(), torch.ones(4, B, I, device="cuda"), torch.ones(3, B, I),
                torch.ones(3, I, B, device="cuda").transpose(1, 2)):
        with pytest.raises(RuntimeError, match="dropout_mask"):
            C().rnn_fwd("gru", xd, *wd, True, dropout_mask=bad)
    with pytest.raises(RuntimeError, match="recurrent_dropout_mask"):
        C().rnn_fwd("gru", xd, *wd, True, recurrent_dropout_mask=ok)  # [G, B, I], not [G, B, H]
    with pytest.raises(RuntimeError, match="every direction"):
        C().birnn_fwd("gru", xd, [wd[0]] * 2, [wd[1]] * 2, [wd[2]] * 2, True, dropout_masks=[ok, None])


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_recurrent_dropout_stays_on_the_register_path_in_one_launch_per_pass():
    from distributeddeeplearningspark_amd.ops import rnn as R

    name = "lstm-reg-h128-i3"
    x, ws, dys, dps, rdps, _ = _inputs(name)
    wd = [t.cuda() for t in ws]
    grads = [torch.zeros_like(t) for t in wd]
    xd, dyd = x.cuda(), dys[True].cuda()
    dm, rm = [m.cuda() for m in dps], [m.cuda() for m in rdps]

    def step():
        y = R.bidirectional("lstm", xd.clone().requires_grad_(True), wd[:3], wd[3:], grads=(grads[:3], grads[3:]),
                            return_sequences=True, dropout_mask=dm, recurrent_dropout_mask=rm)
        y.backward(dyd)

    step()  # warm-up: code object load
    names = _kernel_names(step)
    assert sum("rnn_fwd_reg_kernel" in n for n in names) == 1, names
    assert sum("rnn_bwd_reg_kernel" in n for n in names) == 1, names
    assert any("rnn_drop_x" in n for n in names) and any("rnn_drop_dx" in n for n in names), names
    assert not [n for n in names if "Cijk" in n or "gemm" in n.lower() and "ddl::" not in n], names


# ------------------------------------------------------------------------------------ mask generation
def test_dropout_masks_are_inverted_dropout_draws():
    from distributeddeeplearningspark_amd.ops.act import tick_dropout_step
    from distributeddeeplearningspark_amd.ops.rnn import dropout_masks

    m = dropout_masks(4, 64, 128, 0.25, "cuda")
    assert m.shape == (4, 64, 128) and m.dtype == torch.float32 and m.is_cuda
    vals = m.unique().cpu()
    assert vals.numel() == 2 and vals[0] == 0 and vals[1] > 1, vals  # 0 and one positive scale
    s, n = vals[1].item(), m.numel()
    mean = m.double().mean().item()
    print(f"scale {s:.6g}, mean {mean:.6g}, bound {5 * ((s - 1) / n) ** 0.5:.3g}")
    # N independent draws with E = 1 and per-element variance s - 1: five standard deviations of their mean
    assert abs(mean - 1) <= 5 * ((s - 1) / n) ** 0.5
    assert not torch.equal(m, dropout_masks(4, 64, 128, 0.25, "cuda"))  # two calls differ
    assert torch.equal(dropout_masks(4, 64, 128, 0.25, "cuda", seed=7), dropout_masks(4, 64, 128, 0.25, "cuda", seed=7))
    # captured: the seed is fixed at capture time, the device step counter varies the draw per replay
    dropout_masks(1, 1, 64, 0.25, "cuda")  # nothing lazy left for the capture
    tick_dropout_step("cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        with torch.cuda.graph(g, stream=s_):
            out = dropout_masks(4, 64, 128, 0.25, "cuda")
    torch.cuda.current_stream().wait_stream(s_)
    g.replay()
    a = out.clone()
    tick_dropout_step("cuda")
    g.replay()
    b = out.clone()
    torch.cuda.synchronize()
    assert not torch.equal(a, b)
    assert a.unique().numel() == 2 and b.unique().numel() == 2


# ------------------------------------------------------------------------------------------- models
def _text_model(dev, dropout=0.2, recurrent_dropout=0.2, optimizer="adam"):
    from distributeddeeplearningspark_amd.models import LSTM, Dense, Embedding, Sequential

    m = Sequential([Embedding(50, 8, mask_zero=True, input_shape=(9,)),
                    LSTM(64, dropout=dropout, recurrent_dropout=recurrent_dropout), Dense(2, activation="softmax")])
    m.compile(optimizer, "categorical_crossentropy")
    m.place(dev, seed=0)
    return m


def _text_data(n=64):
    from distributeddeeplearningspark_amd.utils import pad_sequences

    rng = np.random.default_rng(0)
    ids = pad_sequences([list(rng.integers(1, 50, k)) for k in rng.integers(1, 10, n)], maxlen=9, dtype="int64")
    y = np.eye(2, dtype=np.float32)[(ids[:, -1] > 25).astype(int)]  # the last token decides
    return ids, y


def test_text_model_with_dropout_trains_and_predicts_as_the_cpu_model():
    from distributeddeeplearningspark_amd.models import optimizers

    ids, y = _text_data()
    m = _text_model("cuda:0", optimizer=optimizers.Adam(lr=0.01))
    xd, yd = m.to_input(ids), m.to_target(y)
    losses = [float(m.train_on_batch(xd, yd)) for _ in range(30)]
    print("losses", np.round(losses, 4))
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5])
    names = set(_kernel_names(lambda: m.train_on_batch(xd, yd)))
    assert any("rnn_fwd_reg_kernel" in n for n in names) and any("rnn_bwd_reg_kernel" in n for n in names), names
    mc = _text_model("cpu")
    mc.set_weights(m.get_weights())
    pg, pc = m.predict(ids), mc.predict(ids)
    rel = np.linalg.norm(pg - pc) / np.linalg.norm(pc)
    print(f"predict rel L2 {rel:.3g}")
    assert rel < 1e-4, rel  # the per-step bound of test_text_lstm_classifier_matches_cpu
    m0 = _text_model("cuda:0", 0.0, 0.0)
    m0.set_weights(m.get_weights())
    np.testing.assert_array_equal(m0.predict(ids), pg)  # inference: no masks, the rate-0 model bit for bit


def test_graph_replayed_step_draws_fresh_masks(monkeypatch):
    """The graph-replayed worker step with a zero learning rate: the weights never move, so two replays on the same
    batch differ only by their dropout masks."""
    from distributeddeeplearningspark_amd.models import optimizers
    from distributeddeeplearningspark_amd.models.step import CompiledTrainStep, _uses_dropout

    monkeypatch.setenv("DDL_GRAPHS", "1")
    monkeypatch.setenv("DDL_GRAPHS_STRICT", "1")
    ids, y = _text_data(16)
    m = _text_model("cuda:0", optimizer=optimizers.SGD(lr=0.0))
    assert _uses_dropout(m)
    st = CompiledTrainStep(m)
    xd, yd = m.to_input(ids), m.to_target(y)
    losses = [float(st(xd, yd)) for _ in range(5)]  # 2 eager warm-up steps, the capture, 2 replays
    torch.cuda.synchronize()
    assert st.captured, st.fallback_reason
    print("losses", losses)
    assert np.isfinite(losses).all()
    assert losses[3] != losses[4] and losses[2] != losses[3]
    m0 = _text_model("cuda:0", 0.0, 0.0, optimizers.SGD(lr=0.0))
    st0 = CompiledTrainStep(m0)
    l0 = [float(st0(xd, yd)) for _ in range(5)]
    assert l0[3] == l0[4]  # without dropout the replays agree: the difference above is the masks'


def test_replica_batching_declines_recurrent_dropout_on_the_gpu():
    from distributeddeeplearningspark_amd.models import GRU, Dense, Sequential
    from distributeddeeplearningspark_amd.parallel import replica_batch

    class Rep:
        bs = 8

        def __init__(self, model):
            self.model = model
            self.X, self.Y = torch.zeros(16, 5, 1, device="cuda"), torch.zeros(16, 1, device="cuda")

    class Group:
        gpu, rule = True, "downpour"

    def reason(**kw):
        grp = Group()
        grp.reps = []
        for _ in range(2):
            m = Sequential([GRU(64, input_shape=(5, 1), **kw), Dense(1)])
            m.compile("adagrad", "mean_squared_error")
            m.place("cuda:0", seed=0)
            grp.reps.append(Rep(m))
        return replica_batch.why_not(grp)

    assert reason(recurrent_dropout=0.2) == "recurrent dropout (the batched kernels take no dropout masks)"
    assert reason() is None
