"""``go_backwards`` and ``Bidirectional`` recurrent layers on the CPU path.

The oracle is the existing forward-direction math on flipped tensors: ``recurrent_ref(cell, x.flip(1), ...)`` is the
reverse direction (a returned sequence in processing order), flipped back where the sequence is returned in input
order; the two directions concatenated / summed / averaged are Bidirectional."""
import numpy as np
import pytest
import torch

CELLS = {"gru": ("GRU", 3), "lstm": ("LSTM", 4), "rnn": ("SimpleRNN", 1)}


def _weights(cell, I, H, seed):
    G = CELLS[cell][1]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(I, G * H, generator=g) * 0.3, torch.randn(H, G * H, generator=g) * (1.0 / H ** 0.5),
            torch.randn(G * H, generator=g) * 0.1)


def _oracle(cell, x, wf, wb, rs, merge):
    """Flip composition of the forward-only reference.  ``wf`` None: the bare reverse layer."""
    from distributeddeeplearningspark_amd.ops.rnn import recurrent_ref

    yb = recurrent_ref(cell, x.flip(1), *wb, rs)  # processing order
    if wf is None:
        return yb
    yf = recurrent_ref(cell, x, *wf, rs)
    if rs:
        yb = yb.flip(1)
    if merge == "concat":
        return torch.cat([yf, yb], -1)
    return yf + yb if merge == "sum" else (yf + yb) / 2


def _rel(a, r):
    return ((a.detach().float() - r.detach()).norm() / (r.norm() + 1e-12)).item()


@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
@pytest.mark.parametrize("rs", [False, True])
def test_go_backwards_op_matches_flip_composition(cell, rs):
    from distributeddeeplearningspark_amd.ops import rnn as R

    B, T, I, H = 3, 5, 2, 8
    x = torch.randn(B, T, I, generator=torch.Generator().manual_seed(1))
    w = _weights(cell, I, H, 2)
    dy = torch.randn((B, T, H) if rs else (B, H), generator=torch.Generator().manual_seed(3))
    g = [torch.zeros_like(t) for t in w]
    xg = x.clone().requires_grad_(True)
    y = R.recurrent(cell, xg, *w, grads=tuple(g), return_sequences=rs, go_backwards=True)
    y.backward(dy)
    leaves = [t.clone().requires_grad_(True) for t in (x, *w)]
    yr = _oracle(cell, leaves[0], None, leaves[1:], rs, None)
    yr.backward(dy)
    for a, r, what in [(y, yr, "y"), (xg.grad, leaves[0].grad, "dx"), (g[0], leaves[1].grad, "dW"),
                       (g[1], leaves[2].grad, "dU"), (g[2], leaves[3].grad, "db")]:
        assert _rel(a, r) < 1e-5, (what, _rel(a, r))


@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("merge", ["concat", "sum", "ave"])
def test_bidirectional_layer_matches_unidirectional_layers(cell, rs, merge):
    """Bidirectional(layer) == merge(layer(x), flip(go_backwards layer(x))) with shared weights: output and all
    gradients, through the existing unidirectional layers and through the flip oracle."""
    from distributeddeeplearningspark_amd.models import Bidirectional, Sequential
    from distributeddeeplearningspark_amd.models import layers as L

    cls = getattr(L, CELLS[cell][0])
    T, I, H, B = 5, 2, 6, 4
    bi = Sequential([Bidirectional(cls(H, return_sequences=rs), merge_mode=merge, input_shape=(T, I))])
    bi.place("cpu", seed=0)
    ws = bi.get_weights()
    assert len(ws) == 6
    uni_f = Sequential([cls(H, return_sequences=rs, input_shape=(T, I))])
    uni_b = Sequential([cls(H, return_sequences=rs, input_shape=(T, I))])  # forward layer fed the flipped input
    uni_f.place("cpu", seed=1)
    uni_b.place("cpu", seed=2)
    uni_f.set_weights(ws[:3])
    uni_b.set_weights(ws[3:])
    x = torch.randn(B, T, I, generator=torch.Generator().manual_seed(5))
    xs = [x.clone().requires_grad_(True) for _ in range(3)]
    y = bi.forward(xs[0], training=True)
    yf = uni_f.forward(xs[1], training=True)
    yb = uni_b.forward(xs[2].flip(1), training=True)
    if rs:
        yb = yb.flip(1)
    ref = torch.cat([yf, yb], -1) if merge == "concat" else (yf + yb if merge == "sum" else (yf + yb) / 2)
    assert y.shape == ref.shape == (B, *bi.output_shape)
    dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(6))
    for m in (bi, uni_f, uni_b):
        m.arena.zero_grad()
    y.backward(dy)
    ref.backward(dy)
    assert _rel(y, ref) < 1e-5
    assert _rel(xs[0].grad, xs[1].grad + xs[2].grad) < 1e-5
    got = [p.grad for p in bi.all_params()]
    want = [p.grad for p in uni_f.all_params()] + [p.grad for p in uni_b.all_params()]
    for a, r, p in zip(got, want, bi.all_params()):
        assert _rel(a, r) < 1e-5, p.name
    # and against the flip oracle on the raw reference math
    wt = [torch.from_numpy(w) for w in ws]
    assert _rel(y, _oracle(cell, x, wt[:3], wt[3:], rs, merge)) < 1e-5


@pytest.mark.parametrize("rs", [False, True])
def test_go_backwards_layer_output_is_in_processing_order(rs):
    from distributeddeeplearningspark_amd.models import GRU, Sequential

    T, I, H = 4, 3, 5
    m = Sequential([GRU(H, return_sequences=rs, go_backwards=True, input_shape=(T, I))])
    f = Sequential([GRU(H, return_sequences=rs, input_shape=(T, I))])
    m.place("cpu", seed=0)
    f.place("cpu", seed=1)
    f.set_weights(m.get_weights())
    x = np.random.default_rng(0).standard_normal((3, T, I)).astype(np.float32)
    np.testing.assert_allclose(m.predict(x), f.predict(x[:, ::-1].copy()), rtol=1e-5, atol=1e-6)
    assert m.layers[0].get_config()["go_backwards"] is True
    assert f.layers[0].get_config()["go_backwards"] is False


@pytest.mark.parametrize("merge", ["mul", None])
def test_unsupported_merge_modes_raise(merge):
    from distributeddeeplearningspark_amd.models import GRU, Bidirectional

    with pytest.raises(ValueError, match="not supported"):
        Bidirectional(GRU(4), merge_mode=merge)


def test_bidirectional_weights_config_and_serialisation():
    from distributeddeeplearningspark_amd.models import GRU, LSTM, Bidirectional, Dense, Sequential, model_from_json
    from distributeddeeplearningspark_amd.utils import deserialize_keras_model, serialize_keras_model

    T, I, H = 6, 3, 8
    m = Sequential([Bidirectional(GRU(H, return_sequences=True), input_shape=(T, I)),
                    Bidirectional(LSTM(5), merge_mode="ave"), Dense(1)])
    m.place("cpu", seed=0)
    bi = m.layers[0]
    single = Sequential([GRU(H, input_shape=(T, I))])
    single.build_model()
    assert bi.count_params() == 2 * single.count_params()
    assert bi.output_shape == (T, 2 * H) and m.layers[1].output_shape == (5,)
    ws = m.get_weights()
    assert [w.shape for w in ws[:6]] == [(I, 3 * H), (H, 3 * H), (3 * H,)] * 2
    assert [w.shape for w in ws[6:12]] == [(2 * H, 20), (5, 20), (20,)] * 2
    names = [p.name for p in bi.all_params()]
    inner = bi.layer.name
    assert names == [f"{bi.name}/{d}_{inner}/{w}" for d in ("forward", "backward")
                     for w in ("kernel", "recurrent_kernel", "bias")]
    assert bi.forward_layer.go_backwards is False and bi.backward_layer.go_backwards is True
    # the order is forward first: the forward copy's recurrent kernel is entry 1
    np.testing.assert_array_equal(ws[1], bi.forward_layer.recurrent_kernel.master.detach().numpy())
    np.testing.assert_array_equal(ws[4], bi.backward_layer.recurrent_kernel.master.detach().numpy())
    cfg = bi.get_config()
    assert cfg["merge_mode"] == "concat" and cfg["layer"]["class_name"] == "GRU"
    assert cfg["layer"]["config"]["units"] == H and cfg["layer"]["config"]["return_sequences"] is True

    x = np.random.default_rng(1).standard_normal((4, T, I)).astype(np.float32)
    ref = m.predict(x)
    # set_weights(get_weights()) round-trips
    rng = np.random.default_rng(2)
    new = [rng.standard_normal(w.shape).astype(np.float32) * 0.2 for w in ws]
    m.set_weights(new)
    for a, b in zip(m.get_weights(), new):
        np.testing.assert_array_equal(a, b)
    m.set_weights(ws)
    np.testing.assert_array_equal(m.predict(x), ref)
    # to_json -> model_from_json -> identical predictions
    m2 = model_from_json(m.to_json())
    m2.place("cpu")  # as m: "identical" means the same arithmetic, so the same device
    m2.set_weights(ws)
    assert isinstance(m2.layers[0], Bidirectional) and m2.layers[1].merge_mode == "ave"
    np.testing.assert_array_equal(m2.predict(x), ref)
    assert m2.count_params() == m.count_params()
    # the dist-keras wire format
    m3 = deserialize_keras_model(serialize_keras_model(m), device="cpu")
    np.testing.assert_array_equal(m3.predict(x), ref)
    lines = []
    m.summary(print_fn=lines.append)
    assert any("Bidirectional" in l for l in lines) and any(f"{m.count_params():,}" in l for l in lines)


class _Group:
    gpu, rule = True, "downpour"

    def __init__(self, reps):
        self.reps = reps


class _Rep:
    bs = 8

    def __init__(self, model):
        self.model = model
        self.X = torch.zeros(16, 5, 1)
        self.Y = torch.zeros(16, 1)


def test_replica_batching_declines_directed_models():
    from distributeddeeplearningspark_amd.models import GRU, Dense, Sequential, zoo
    from distributeddeeplearningspark_amd.parallel import replica_batch

    def reason(build):
        reps = []
        for _ in range(2):
            m = build()
            m.compile("adagrad", "mean_squared_error")
            m.place("cpu", seed=0)
            reps.append(_Rep(m))
        return replica_batch.why_not(_Group(reps))

    r = reason(lambda: Sequential([GRU(64, go_backwards=True, input_shape=(5, 1)), Dense(1)]))
    assert r is not None and "go_backwards" in r
    r = reason(lambda: zoo.bigru_regressor(units=64, seq_len=5))
    assert r == "not a GRU/LSTM -> Dense Sequential"


def test_bigru_regressor_trains():
    from distributeddeeplearningspark_amd.models import zoo

    m = zoo.bigru_regressor(units=16, seq_len=5)
    m.compile("adagrad", "mean_squared_error")
    m.place("cpu", seed=0)
    rng = np.random.default_rng(0)
    x = rng.random((16, 5, 1), dtype=np.float32)
    y = rng.random((16, 1), dtype=np.float32)
    l0 = m.train_on_batch(x, y)
    for _ in range(10):
        l1 = m.train_on_batch(x, y)
    assert l1 < l0
    assert zoo.bilstm_regressor(units=8, seq_len=5).layers[0].layer.cell == "lstm"


def test_wrapper_grad_hook_fires_once_after_both_directions():
    from distributeddeeplearningspark_amd.models import GRU, Bidirectional, Sequential

    m = Sequential([Bidirectional(GRU(4), input_shape=(3, 2))])
    m.place("cpu", seed=0)
    bi = m.layers[0]
    seen = []

    def hook():
        # both directions' gradients are already in the arena when the wrapper's hook runs
        seen.append([float(p.grad.abs().sum()) for p in bi.all_params()])

    bi.grad_hook = hook
    sub = []
    bi.forward_layer.grad_hook = lambda: sub.append("f")
    bi.backward_layer.grad_hook = lambda: sub.append("b")
    m.arena.zero_grad()
    x = torch.randn(2, 3, 2, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    m.forward(x, training=True).sum().backward()
    assert len(seen) == 1 and all(v > 0 for v in seen[0])
    assert sorted(sub) == ["b", "f"]
