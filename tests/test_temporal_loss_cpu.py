"""Masked per-time-step losses (``ops/loss.py`` temporal_*), ``TimeDistributed`` and the mask flow to the output, on
the CPU path.

Oracles are float64 and written in ``temporal_oracle.py`` from plain torch, ``sum(score * mask) / sum(mask)`` with
autograd; they use no project code.  Mask patterns come from ``masking_oracle.patterns``.  Op tolerance: 1e-6
relative (the torch fp32 formula against float64 at these sizes; the gradient relative to its largest element);
model tolerance: relative L2 < 1e-4, as ``test_masking_cpu.py``."""
import json

import numpy as np
import pytest
import torch

from masking_oracle import bidir_oracle, oracle, patterns, rel_l2
from temporal_oracle import reg_oracle, xent_oracle

B, T = 7, 5


def _rel(a, r):
    return float((a.double() - r).abs().max() / r.abs().max().clamp_min(1e-30))


def _xent_inputs(K, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, K, generator=g) * 2.0
    labels = torch.randint(0, K, (B, T), generator=g)
    probs = torch.softmax(torch.randn(B, T, K, generator=g), -1)
    return logits, labels, probs


def _run(fn, x, *a, **kw):
    xl = x.clone().requires_grad_(True)
    loss = fn(xl, *a, **kw)
    loss.backward()
    return loss.detach(), xl.grad


# ------------------------------------------------------------------------------------------------ the three ops
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["sparse", "dense"])
@pytest.mark.parametrize("K", [1, 3, 10])
def test_temporal_xent_matches_float64_oracle(K, form, masked):
    from distributeddeeplearningspark_amd.ops.loss import temporal_softmax_cross_entropy as txe

    logits, labels, probs = _xent_inputs(K)
    mask = patterns(B, T) if masked else None
    kw = {"labels": labels} if form == "sparse" else {"probs": probs}
    loss, grad = _run(txe, logits, mask=mask, **kw)
    rl, rg = xent_oracle(logits, mask, **kw)
    print(f"loss {float(loss):.8g} ref {float(rl):.8g}; grad rel err {_rel(grad, rg) if K > 1 else 0.0:.3g}")
    assert abs(float(loss) - float(rl)) <= 1e-6 * abs(float(rl))
    assert float((grad.double() - rg).abs().max()) <= 1e-6 * float(rg.abs().max())


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mae", [False, True])
@pytest.mark.parametrize("F", [1, 3])
def test_temporal_regression_losses_match_float64_oracle(F, mae, masked):
    from distributeddeeplearningspark_amd.ops import loss as L

    fn = L.temporal_mean_absolute_error if mae else L.temporal_mean_squared_error
    g = torch.Generator().manual_seed(1)
    pred, target = torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
    pred[0, 0] = target[0, 0]  # sign(0) = 0
    mask = patterns(B, T) if masked else None
    loss, grad = _run(fn, pred, target, mask=mask)
    rl, rg = reg_oracle(pred, target, mask, mae)
    print(f"loss {float(loss):.8g} ref {float(rl):.8g}; grad rel err {_rel(grad, rg):.3g}")
    assert abs(float(loss) - float(rl)) <= 1e-6 * abs(float(rl))
    assert float((grad.double() - rg).abs().max()) <= 1e-6 * float(rg.abs().max())
    assert (grad[0, 0] == 0).all()


def _all_ops():
    """(name, fn(x, mask), x) of the three ops in both target forms, over shared inputs."""
    from distributeddeeplearningspark_amd.ops import loss as L

    logits, labels, probs = _xent_inputs(3)
    g = torch.Generator().manual_seed(2)
    pred, target = torch.randn(B, T, 3, generator=g), torch.randn(B, T, 3, generator=g)
    return [
        ("xent_sparse", lambda x, m, lab=labels: L.temporal_softmax_cross_entropy(x, labels=lab, mask=m), logits),
        ("xent_dense", lambda x, m: L.temporal_softmax_cross_entropy(x, probs=probs, mask=m), logits),
        ("mse", lambda x, m: L.temporal_mean_squared_error(x, target, mask=m), pred),
        ("mae", lambda x, m: L.temporal_mean_absolute_error(x, target, mask=m), pred),
    ]


def test_all_ones_mask_equals_no_mask_exactly():
    for name, fn, x in _all_ops():
        l0, g0 = _run(fn, x, None)
        l1, g1 = _run(fn, x, torch.ones(B, T, dtype=torch.uint8))
        assert l0.item() == l1.item() and torch.equal(g0, g1), name


def test_all_zero_mask_gives_exact_zeros():
    for name, fn, x in _all_ops():
        loss, grad = _run(fn, x, torch.zeros(B, T, dtype=torch.uint8))
        assert loss.item() == 0.0 and torch.isfinite(grad).all() and (grad == 0).all(), name


def test_values_at_masked_rows_do_not_matter():
    from distributeddeeplearningspark_amd.ops import loss as L

    mask = patterns(B, T)
    off = mask == 0
    logits, labels, probs = _xent_inputs(3)
    bad_labels = labels.clone()
    bad_labels[off] = -1
    bad_labels[4] = 3 + 5  # the fully masked row
    for name, fn, x in _all_ops():
        if name == "xent_sparse":
            dirty_fn = lambda x, m: L.temporal_softmax_cross_entropy(x, labels=bad_labels, mask=m)
        else:
            dirty_fn = fn
        dirty = x.clone()
        dirty[off] = float("nan")
        l0, g0 = _run(fn, x, mask)
        l1, g1 = _run(dirty_fn, dirty, mask)
        assert l0.item() == l1.item() and torch.equal(g0, g1), name
        assert (g1[off] == 0).all() and torch.isfinite(g1).all(), name


def test_bf16_and_shape_errors():
    from distributeddeeplearningspark_amd.ops import loss as L

    logits, labels, _ = _xent_inputs(3)
    with pytest.raises(ValueError, match="fp32"):
        L.temporal_softmax_cross_entropy(logits.bfloat16(), labels=labels)
    with pytest.raises(ValueError, match="fp32"):
        L.temporal_mean_squared_error(logits.bfloat16(), logits.bfloat16())
    with pytest.raises(ValueError):
        L.temporal_softmax_cross_entropy(logits, labels=labels, mask=torch.ones(B, T + 1, dtype=torch.uint8))
    with pytest.raises(ValueError):
        L.temporal_softmax_cross_entropy(logits)


# ------------------------------------------------------------------------------------------------ TimeDistributed
def test_time_distributed_equals_dense_on_the_reshaped_input():
    from distributeddeeplearningspark_amd.models import Dense, Sequential, TimeDistributed

    m = Sequential([TimeDistributed(Dense(4, activation="tanh"), input_shape=(T, 3))])
    m.place("cpu", seed=0)
    k, b = [torch.from_numpy(a) for a in m.get_weights()]
    assert k.shape == (3, 4) and b.shape == (4,)  # Keras order: kernel, bias
    assert m.count_params() == 3 * 4 + 4 and m.layers[0].count_params() == 16
    x = torch.randn(B, T, 3, generator=torch.Generator().manual_seed(0))
    want = torch.tanh(x.reshape(B * T, 3) @ k + b).reshape(B, T, 4)
    got = torch.from_numpy(m.predict(x.numpy()))
    assert got.shape == (B, T, 4) and torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    names = [p.name for p in m.all_params()]
    td = m.layers[0]
    assert names == [f"{td.name}/{td.layer.name}/kernel", f"{td.name}/{td.layer.name}/bias"]
    assert td.activation_name == "tanh" and td.supports_skip and td.passes_mask
    logits = td.call(x, skip_activation=True)
    assert torch.allclose(logits, (x.reshape(-1, 3) @ k + b).reshape(B, T, 4), rtol=1e-5, atol=1e-6)


def test_time_distributed_config_round_trips():
    from distributeddeeplearningspark_amd.models import (GRU, Dense, Masking, Sequential, TimeDistributed,
                                                         model_from_json)
    from distributeddeeplearningspark_amd.utils import deserialize_keras_model, serialize_keras_model

    m = Sequential([Masking(input_shape=(T, 2)), GRU(3, return_sequences=True),
                    TimeDistributed(Dense(2, activation="softmax"))])
    m.place("cpu", seed=1)
    td = m.layers[-1]
    assert td.name.startswith("time_distributed_")
    rows = []
    m.summary(print_fn=rows.append)
    assert any("(TimeDistributed)" in r and "(None, 5, 2)" in r for r in rows), rows
    cfg = json.loads(m.to_json())["config"]["layers"][-1]
    assert cfg["class_name"] == "TimeDistributed" and cfg["config"]["layer"]["class_name"] == "Dense"
    x = np.random.default_rng(0).random((4, T, 2), dtype=np.float32)
    want = m.predict(x)
    m2 = model_from_json(m.to_json())
    m2.set_weights(m.get_weights())
    assert m2.layers[-1].name == td.name and m2._output_masked
    np.testing.assert_allclose(m2.predict(x), want, rtol=1e-6, atol=1e-7)
    m3 = deserialize_keras_model(serialize_keras_model(m))
    np.testing.assert_allclose(m3.predict(x), want, rtol=1e-6, atol=1e-7)
    # a Keras config dict in place of the layer instance, as Bidirectional takes
    td2 = TimeDistributed({"class_name": "Dense", "config": {"units": 2, "activation": "softmax"}})
    assert td2.units == 2 and td2.activation_name == "softmax"


def test_time_distributed_trainable_and_non_dense():
    from distributeddeeplearningspark_amd.models import GRU, Dense, Sequential, TimeDistributed

    with pytest.raises(ValueError, match="Dense"):
        TimeDistributed(GRU(3))
    with pytest.raises(ValueError, match="Dense"):
        TimeDistributed({"class_name": "Activation", "config": {"activation": "relu"}})
    m = Sequential([GRU(3, return_sequences=True, input_shape=(T, 2)), TimeDistributed(Dense(2), trainable=False)])
    m.compile("sgd", "mean_squared_error")
    m.place("cpu", seed=0)
    td = m.layers[-1]
    assert not td.trainable and not td.inner.trainable
    fired = []
    td.inner.grad_hook = lambda: fired.append(1)  # where the data-parallel engine installs it (the weights' owner)
    g = torch.Generator().manual_seed(0)
    m.backward_step(torch.randn(4, T, 2, generator=g), torch.randn(4, T, 2, generator=g))
    assert (td.inner.kernel.grad == 0).all() and (td.inner.bias.grad == 0).all()
    assert m.layers[0].kernel.grad.abs().sum() > 0
    td.trainable = True
    assert td.inner.trainable
    m.backward_step(torch.randn(4, T, 2, generator=g), torch.randn(4, T, 2, generator=g))
    assert td.inner.kernel.grad.abs().sum() > 0 and fired


# ------------------------------------------------------------------------------------------------ mask flow
def test_mask_flow_to_a_temporal_head():
    from distributeddeeplearningspark_amd.models import (GRU, Activation, Dense, Dropout, Masking, Sequential,
                                                         TimeDistributed)

    def stack(*tail):
        m = Sequential([Masking(input_shape=(T, 2)), GRU(3, return_sequences=True), *tail])
        m.build_model()
        return m

    m = stack(TimeDistributed(Dense(1)))
    assert m._masked and m._output_masked
    for tail in ([Activation("softmax")], [Dropout(0.5)], [Activation("relu"), Dropout(0.5)]):
        assert stack(TimeDistributed(Dense(2)), *tail)._output_masked
    with pytest.raises(ValueError, match="model output"):
        stack(Dense(1))
    with pytest.raises(ValueError, match="model output"):
        stack()
    with pytest.raises(ValueError, match="model output"):
        stack(TimeDistributed(Dense(2)), Dense(1))  # the last layer with weights is a plain Dense
    # no mask at the output: nothing recorded, the temporal losses run unmasked
    m = Sequential([GRU(3, return_sequences=True, input_shape=(T, 2)), TimeDistributed(Dense(1))])
    m.build_model()
    assert not m._masked and not m._output_masked and m._temporal_head is m.layers[-1]
    # forward / predict return the outputs alone, every step present
    m = stack(TimeDistributed(Dense(1)))
    m.place("cpu", seed=0)
    out = m.forward(torch.zeros(2, T, 2))
    assert isinstance(out, torch.Tensor) and out.shape == (2, T, 1)


def test_unsupported_losses_on_a_temporal_head_name_the_supported_ones():
    from distributeddeeplearningspark_amd.models import GRU, Dense, Masking, Sequential, TimeDistributed

    x, y = torch.zeros(2, T, 2), torch.zeros(2, T, 1)
    m = Sequential([Masking(input_shape=(T, 2)), GRU(3, return_sequences=True), TimeDistributed(Dense(1))])
    m.compile("sgd", "binary_crossentropy")
    m.place("cpu", seed=0)
    with pytest.raises(ValueError, match="mean_absolute_error") as e:
        m.compute_loss(x, y)
    for name in ("categorical_crossentropy", "sparse_categorical_crossentropy", "mean_squared_error"):
        assert name in str(e.value)
    m.compile("sgd", "sparse_categorical_crossentropy")  # cross-entropy on a head without softmax
    with pytest.raises(ValueError, match="softmax"):
        m.compute_loss(x, y)
    m.compile("sgd", lambda out, yy: ((out - yy) ** 2).mean())  # a callable loss receives forward's output
    assert m.compute_loss(x, y).shape == ()


# ------------------------------------------------------------------------------------------------ model level
def _arena_grad_oracle(m, grads):
    """The oracle's gradients (Keras layouts, ``get_weights`` order) as the model's canonical flat gradient."""
    a = m.arena
    assert len(a.params) == len(grads)
    out = torch.zeros(a.canon_numel)
    for p, off, g in zip(a.params, a.canon_offsets, grads):
        out[off:off + p.numel] = torch.from_numpy(np.ascontiguousarray(p.from_keras(g.numpy()))).reshape(-1)
    return out


def _tagger_case():
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.utils import pad_sequences

    rng = np.random.default_rng(0)
    m = zoo.sequence_tagger(20, 6, 4, embed_dim=4, units=5)
    ids = pad_sequences([list(rng.integers(1, 20, n)) for n in (6, 2, 1, 4, 3)], maxlen=6, dtype="int64")
    ids = np.concatenate([ids, pad_sequences([[3, 7, 5]], maxlen=6, dtype="int64", padding="post"),
                          np.zeros((1, 6), np.int64)])  # post-padded and fully padded rows too
    tags = rng.integers(0, 4, ids.shape)
    return m, ids, tags


def _tagger_oracle(w, ids, tags, dense_targets=False):
    w = [t.clone().requires_grad_(True) for t in w]
    mask = (ids != 0).to(torch.uint8)
    h = w[0][ids]
    h = bidir_oracle("lstm", h, w[1:4], w[4:7], True, mask)
    logits = h @ w[7] + w[8]
    keep = mask.bool()
    lp = torch.log_softmax(logits[keep], -1)
    loss = -lp.gather(1, tags[keep][:, None]).sum() / max(int(keep.sum()), 1)
    return loss.detach(), torch.autograd.grad(loss, w)


@pytest.mark.parametrize("form", ["sparse", "dense"])
def test_sequence_tagger_matches_hand_composed_oracle(form):
    m, ids, tags = _tagger_case()
    m.compile("sgd", "sparse_categorical_crossentropy" if form == "sparse" else "categorical_crossentropy")
    m.place("cpu", seed=0)
    w = [torch.from_numpy(a) for a in m.get_weights()]
    want, grads = _tagger_oracle(w, torch.from_numpy(ids), torch.from_numpy(tags))
    y = torch.from_numpy(tags) if form == "sparse" else torch.nn.functional.one_hot(torch.from_numpy(tags), 4).float()
    loss = m.backward_step(m.to_input(ids), m.to_target(y)).detach()
    got = m.arena.to_canonical(m.arena.grad).detach()
    ref = _arena_grad_oracle(m, grads)
    err = rel_l2(got, ref)
    print(f"loss {float(loss):.7g} oracle {float(want):.7g}; arena gradient rel L2 {err:.3g}")
    assert abs(float(loss) - float(want)) <= 1e-4 * abs(float(want))
    assert err < 1e-4
    # predict: softmax over the tags per step, every step present; evaluate: the masked loss
    p = m.predict(ids)
    assert p.shape == (7, 6, 4) and np.allclose(p.sum(-1), 1.0, atol=1e-5)
    assert abs(m.evaluate(ids, y.numpy()) - float(want)) <= 1e-4 * abs(float(want))


def _regressor_case():
    from distributeddeeplearningspark_amd.models import zoo

    g = torch.Generator().manual_seed(3)
    m = zoo.masked_seq2seq_regressor(units=5, seq_len=6, features=2, outputs=3)
    mask = patterns(7, 6)
    x = (torch.rand(7, 6, 2, generator=g) + 0.1) * mask.unsqueeze(-1)
    y = torch.randn(7, 6, 3, generator=g)
    return m, x, y, mask


@pytest.mark.parametrize("loss_name", ["mean_squared_error", "mean_absolute_error"])
def test_masked_seq2seq_regressor_matches_hand_composed_oracle(loss_name):
    m, x, y, mask = _regressor_case()
    m.compile("sgd", loss_name)
    m.place("cpu", seed=0)
    w = [torch.from_numpy(a).clone().requires_grad_(True) for a in m.get_weights()]
    out = oracle("gru", x, *w[0:3], True, mask) @ w[3] + w[4]
    d = out[mask.bool()] - y[mask.bool()]
    want = (d.abs() if loss_name == "mean_absolute_error" else d * d).mean(-1).sum() / int(mask.sum())
    grads, want = torch.autograd.grad(want, w), want.detach()
    loss = m.backward_step(m.to_input(x), m.to_target(y)).detach()
    err = rel_l2(m.arena.to_canonical(m.arena.grad).detach(), _arena_grad_oracle(m, grads))
    print(f"loss {float(loss):.7g} oracle {float(want):.7g}; arena gradient rel L2 {err:.3g}")
    assert abs(float(loss) - float(want)) <= 1e-4 * abs(float(want))
    assert err < 1e-4


def test_inputs_at_masked_steps_do_not_reach_loss_or_gradients():
    """A masked step's input is the padding value by definition (id 0, or features equal to ``mask_value``), so what
    can differ there is the target: labels of -1 and past the classes, NaN regression targets.  (The embedding row
    the padded ids read is perturbed in the next test.)"""
    m, ids, tags = _tagger_case()
    m.compile("sgd", "sparse_categorical_crossentropy")
    m.place("cpu", seed=0)
    l0 = float(m.backward_step(m.to_input(ids), m.to_target(tags)).detach())
    g0 = m.arena.grad.detach().clone()
    dirty = tags.copy()
    dirty[ids == 0] = -1
    dirty[-1] = 9  # the fully padded row: a label past the classes
    l1 = float(m.backward_step(m.to_input(ids), m.to_target(dirty)).detach())
    assert l0 == l1 and torch.equal(g0, m.arena.grad)

    m, x, y, mask = _regressor_case()
    m.compile("sgd", "mean_squared_error")
    m.place("cpu", seed=0)
    l0 = float(m.backward_step(m.to_input(x), m.to_target(y)).detach())
    g0 = m.arena.grad.detach().clone()
    dirty = y.clone()
    dirty[mask == 0] = float("nan")
    l1 = float(m.backward_step(m.to_input(x), m.to_target(dirty)).detach())
    assert l0 == l1 and torch.equal(g0, m.arena.grad)


def test_embedding_rows_of_padded_steps_do_not_reach_loss_or_gradients():
    """Perturbing the INPUT at masked steps: row 0 of the embedding table is what a padded step feeds the BiLSTM."""
    m, ids, tags = _tagger_case()
    m.compile("sgd", "sparse_categorical_crossentropy")
    m.place("cpu", seed=0)
    l0 = float(m.backward_step(m.to_input(ids), m.to_target(tags)).detach())
    g0 = m.arena.grad.detach().clone()
    w = m.get_weights()
    w[0][0] = 1e3
    m.set_weights(w)
    l1 = float(m.backward_step(m.to_input(ids), m.to_target(tags)).detach())
    assert l0 == l1 and torch.equal(g0, m.arena.grad)
    assert (m.layers[0].embeddings.grad[0] == 0).all()


# ------------------------------------------------------------------------------------------------ a trainer run
@pytest.fixture(scope="module")
def spark():
    from distributeddeeplearningspark_amd.context import SparkSession

    return SparkSession.builder.master("local[2]").getOrCreate()


def test_single_trainer_learns_a_tag_per_token(spark):
    """tag = token id mod 4 over zero-padded sequences, a ``[T]`` label vector column: 30 steps of batch 8."""
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.sql.dataframe import from_columns
    from distributeddeeplearningspark_amd.trainers import SingleTrainer
    from distributeddeeplearningspark_amd.utils import pad_sequences

    rng = np.random.default_rng(0)
    ids = pad_sequences([list(rng.integers(1, 12, rng.integers(1, 7))) for _ in range(48)], maxlen=6)
    tags = (ids % 4).astype(np.float32)  # the label column is a float vector, cast by the sparse loss
    df = from_columns({"ids": ids, "label": tags}, num_partitions=1)
    m = zoo.sequence_tagger(12, 6, 4, embed_dim=8, units=8)
    tr = SingleTrainer(keras_model=m, worker_optimizer="adam", loss="sparse_categorical_crossentropy",
                       features_col="ids", label_col="label", batch_size=8, num_epoch=5, device="cpu")
    tr.train(df)
    h = tr.get_history()[0]
    assert len(h) == 30 and np.isfinite(h).all()
    assert np.mean(h[-6:]) < np.mean(h[:6]), h
