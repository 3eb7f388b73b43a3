"""Masking / Embedding(mask_zero) and masked recurrent layers on the CPU path.

The oracle is the compaction oracle of ``masking_oracle.py``: the unmasked ``recurrent_ref`` (no ``mask``) over each
row's unmasked steps.  Tolerance as the other recurrent tests: relative L2 < 1e-4."""
import json

import numpy as np
import pytest
import torch

from masking_oracle import bidir_oracle, oracle, patterns, rel_l2, weights

B, T, I, H = 5, 7, 3, 8  # one row of every mask pattern


def _leaves(ts):
    return [t.clone().requires_grad_(True) for t in ts]


def _close(got, want, names):
    for what, a, r in zip(names, got, want):
        err = rel_l2(a, r)
        print(f"{what}: rel L2 {err:.3g}")
        assert err < 1e-4, (what, err)


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_recurrent_ref_matches_compaction_oracle(cell, rs, rev):
    from distributeddeeplearningspark_amd.ops.rnn import recurrent_ref

    g = torch.Generator().manual_seed(0)
    x, ws = torch.randn(B, T, I, generator=g), weights(cell, I, H, g)
    dy = torch.randn(B, T, H, generator=g) if rs else torch.randn(B, H, generator=g)
    mask = patterns(B, T)
    la, lb = _leaves([x, *ws]), _leaves([x, *ws])
    y = recurrent_ref(cell, la[0], *la[1:], rs, go_backwards=rev, mask=mask)
    yr = oracle(cell, lb[0], *lb[1:], rs, mask, rev)
    got, ref = torch.autograd.grad(y, la, dy), torch.autograd.grad(yr, lb, dy)
    _close([y, *got], [yr, *ref], ("y", "dx", "dW", "dU", "db"))
    assert (got[0][mask == 0] == 0).all()  # dx is exactly zero at masked steps
    assert (y[4] == 0).all()  # the fully masked row


@pytest.mark.parametrize("merge", ["concat", "sum"])
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_bidirectional_ref_matches_compaction_oracle(cell, rs, merge):
    from distributeddeeplearningspark_amd.ops.rnn import bidirectional_ref

    g = torch.Generator().manual_seed(1)
    x, ws = torch.randn(B, T, I, generator=g), weights(cell, I, H, g, 2)
    Hy = 2 * H if merge == "concat" else H
    dy = torch.randn(B, T, Hy, generator=g) if rs else torch.randn(B, Hy, generator=g)
    mask = patterns(B, T)
    la, lb = _leaves([x, *ws]), _leaves([x, *ws])
    y = bidirectional_ref(cell, la[0], la[1:4], la[4:], rs, merge, mask=mask)
    yr = bidir_oracle(cell, lb[0], lb[1:4], lb[4:], rs, mask, merge)
    got, ref = torch.autograd.grad(y, la, dy), torch.autograd.grad(yr, lb, dy)
    _close([y, *got], [yr, *ref], ("y", "dx", "dW", "dU", "db", "dWb", "dUb", "dbb"))


@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_masked_ops_match_oracle_and_accumulate_gradients(cell):
    """``recurrent(mask=)`` / ``bidirectional(mask=)`` (the autograd nodes, CPU path): gradients land in the given
    buffers and the mask saved in forward serves the backward."""
    from distributeddeeplearningspark_amd.ops import rnn as R

    g = torch.Generator().manual_seed(2)
    x, ws = torch.randn(B, T, I, generator=g), weights(cell, I, H, g, 2)
    mask = patterns(B, T)
    lb = _leaves([x, *ws])
    for rev in (False, True):
        dy = torch.randn(B, T, H, generator=g)
        yr = oracle(cell, lb[0], *lb[1:4], True, mask, rev)
        ref = torch.autograd.grad(yr, lb[:4], dy)
        grads = [torch.zeros_like(t) for t in ws[:3]]
        xl = x.clone().requires_grad_(True)
        y = R.recurrent(cell, xl, *ws[:3], grads=tuple(grads), return_sequences=True, go_backwards=rev, mask=mask)
        y.backward(dy)
        _close([y, xl.grad, *grads], [yr, *ref], ("y", "dx", "dW", "dU", "db"))
    dy = torch.randn(B, 2 * H, generator=g)
    yr = bidir_oracle(cell, lb[0], lb[1:4], lb[4:], False, mask)
    ref = torch.autograd.grad(yr, lb, dy)
    grads = [torch.zeros_like(t) for t in ws]
    xl = x.clone().requires_grad_(True)
    y = R.bidirectional(cell, xl, ws[:3], ws[3:], grads=(grads[:3], grads[3:]), mask=mask)
    y.backward(dy)
    _close([y, xl.grad, *grads], [yr, *ref], ("y", "dx", "dW", "dU", "db", "dWb", "dUb", "dbb"))
    with pytest.raises(ValueError):
        R.recurrent(cell, x, *ws[:3], mask=mask.bool())
    with pytest.raises(ValueError):
        R.recurrent(cell, x, *ws[:3], mask=mask[:, :-1])


@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_all_ones_mask_is_bit_identical_to_no_mask(cell):
    from distributeddeeplearningspark_amd.ops.rnn import bidirectional_ref, recurrent_ref

    g = torch.Generator().manual_seed(3)
    x, ws = torch.randn(B, T, I, generator=g), weights(cell, I, H, g, 2)
    ones = torch.ones(B, T, dtype=torch.uint8)
    for rs in (False, True):
        for rev in (False, True):
            assert torch.equal(recurrent_ref(cell, x, *ws[:3], rs, go_backwards=rev, mask=ones),
                               recurrent_ref(cell, x, *ws[:3], rs, go_backwards=rev))
        assert torch.equal(bidirectional_ref(cell, x, ws[:3], ws[3:], rs, mask=ones),
                           bidirectional_ref(cell, x, ws[:3], ws[3:], rs))


@pytest.mark.parametrize("mask_value", [0.0, -1.0])
def test_masking_layer(mask_value):
    from distributeddeeplearningspark_amd.models import Masking

    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 6, 3, generator=g)
    x[0, 2:] = mask_value
    x[1, :3] = mask_value
    x[2, 1, :2] = mask_value  # one feature differs: the step is data
    x[3] = mask_value
    want = torch.ones(4, 6, dtype=torch.uint8)
    want[0, 2:] = 0
    want[1, :3] = 0
    want[3] = 0
    l = Masking(mask_value=mask_value)
    xl = x.clone().requires_grad_(True)
    y, mask = l.call(xl, return_mask=True)
    assert mask.dtype == torch.uint8 and torch.equal(mask, want)
    assert (y[want == 0] == 0).all() and torch.equal(y[want == 1], x[want == 1])
    assert torch.equal(l.call(x), y.detach())
    dy = torch.randn(4, 6, 3, generator=g)
    y.backward(dy)
    assert torch.equal(xl.grad, dy * want.unsqueeze(-1))
    assert l.get_config()["mask_value"] == mask_value


def test_embedding_mask_zero():
    from distributeddeeplearningspark_amd.models import Embedding, Sequential

    ids = torch.tensor([[0, 0, 3, 1], [2, 0, 0, 4], [0, 0, 0, 0]])
    m = Sequential([Embedding(5, 3, mask_zero=True, input_shape=(4,))])
    with pytest.raises(ValueError):  # the mask would reach the output
        m.build_model()
    e = Embedding(5, 3, mask_zero=True, input_shape=(4,))
    e.ensure_built((4,))
    from distributeddeeplearningspark_amd.models.params import ParamArena

    ParamArena(e.all_params(), torch.device("cpu"), torch.float32, seed=0)
    y, mask = e.call(ids, return_mask=True)
    assert mask.dtype == torch.uint8 and torch.equal(mask, (ids != 0).to(torch.uint8))
    assert y.shape == (3, 4, 3) and e.embeddings.data.shape == (5, 3)  # the table keeps input_dim rows
    assert e.get_config()["mask_zero"] is True
    e0 = Embedding(5, 3)
    assert e0.get_config()["mask_zero"] is False and not e0.produces_mask


def _text_model(maxlen, mask_zero=True):
    from distributeddeeplearningspark_amd.models import LSTM, Dense, Embedding, Sequential

    m = Sequential([Embedding(20, 4, mask_zero=mask_zero, input_shape=(maxlen,)), LSTM(6), Dense(1, activation="sigmoid")])
    m.compile("adam", "binary_crossentropy")
    m.place("cpu", seed=0)
    return m


@pytest.mark.parametrize("padding", ["pre", "post"])
def test_predictions_do_not_depend_on_the_padded_length(padding):
    from distributeddeeplearningspark_amd.utils import pad_sequences

    seqs = [[3, 4, 5], [7], [1, 2, 3, 4, 5, 6], [9, 8]]
    T0 = 6
    a, b = pad_sequences(seqs, maxlen=T0, padding=padding), pad_sequences(seqs, maxlen=T0 + 3, padding=padding)
    for mask_zero in (True, False):
        m1, m2 = _text_model(T0, mask_zero), _text_model(T0 + 3, mask_zero)
        m2.set_weights(m1.get_weights())
        p1, p2 = m1.predict(a), m2.predict(b)
        if mask_zero:
            np.testing.assert_allclose(p1, p2, rtol=1e-6, atol=1e-7)
        else:
            assert np.abs(p1 - p2).max() > 1e-4  # the padding is run through the cell


def test_zoo_models_round_trip_through_json():
    from distributeddeeplearningspark_amd.models import Embedding, Masking, model_from_json, zoo
    from distributeddeeplearningspark_amd.utils import deserialize_keras_model, pad_sequences, serialize_keras_model

    rng = np.random.default_rng(0)
    ids = pad_sequences([list(rng.integers(1, 30, n)) for n in (2, 5, 8, 1)], maxlen=8)
    x = rng.random((4, 6, 2), dtype=np.float32)
    x[0, 4:] = 0
    x[1, :2] = 0
    for m, inp in ((zoo.text_lstm_classifier(30, 8, embed_dim=4, units=6), ids),
                   (zoo.masked_gru_regressor(units=6, seq_len=6, features=2), x)):
        m.place("cpu", seed=1)
        ref = m.predict(inp)
        m2 = model_from_json(m.to_json())
        m2.place("cpu")
        m2.set_weights(m.get_weights())
        np.testing.assert_array_equal(m2.predict(inp), ref)
        assert type(m2.layers[0]) is type(m.layers[0]) and m2._masked
        m3 = deserialize_keras_model(serialize_keras_model(m), device="cpu")
        np.testing.assert_array_equal(m3.predict(inp), ref)
    assert isinstance(zoo.text_lstm_classifier(30, 8).layers[0], Embedding)
    assert isinstance(zoo.masked_gru_regressor().layers[0], Masking)
    # an Embedding config written before mask_zero existed
    d = json.loads(zoo.text_lstm_classifier(30, 8).to_json())
    del d["config"]["layers"][0]["config"]["mask_zero"]
    old = model_from_json(json.dumps(d))
    old.build_model()
    assert old.layers[0].mask_zero is False and not old._masked


def test_static_mask_check():
    from distributeddeeplearningspark_amd.models import (GRU, Activation, Bidirectional, Dense, Dropout, Flatten, Masking,
                                                         Sequential)

    def build(*layers):
        Sequential(list(layers)).build_model()

    with pytest.raises(ValueError, match="Flatten"):
        build(Masking(input_shape=(4, 2)), Flatten(), Dense(1))
    with pytest.raises(ValueError, match="Masking"):
        build(Masking(input_shape=(4, 2)), Masking(), GRU(3), Dense(1))
    with pytest.raises(ValueError, match="model output"):
        build(Masking(input_shape=(4, 2)), GRU(3, return_sequences=True), Dense(1))
    with pytest.raises(ValueError, match="model output"):
        build(Masking(input_shape=(4, 2)), Dense(3))
    # every layer that passes a mask on, then a consumer
    build(Masking(input_shape=(4, 2)), Dense(3), Activation("tanh"), Dropout(0.1),
          Bidirectional(GRU(3, return_sequences=True)), GRU(3), Dense(1))
    m = Sequential([GRU(3, input_shape=(4, 2)), Dense(1)])
    m.build_model()
    assert m._masked is False


def test_masked_stack_matches_oracle_through_the_model():
    """Masking -> Dense -> Bidirectional(GRU, sequences) -> LSTM(go_backwards) -> Dense: the mask reaches every
    recurrent layer (checked against the oracle composed by hand from the same weights)."""
    from distributeddeeplearningspark_amd.models import GRU, LSTM, Bidirectional, Dense, Masking, Sequential

    m = Sequential([Masking(input_shape=(T, I)), Dense(4), Bidirectional(GRU(5, return_sequences=True)),
                    LSTM(6, go_backwards=True), Dense(2)])
    m.place("cpu", seed=0)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, I, generator=g)
    mask = patterns(B, T)
    x = x * mask.unsqueeze(-1)
    w = [torch.from_numpy(a) for a in m.get_weights()]
    h = x @ w[0] + w[1]
    h = bidir_oracle("gru", h, w[2:5], w[5:8], True, mask)
    h = oracle("lstm", h, *w[8:11], False, mask, True)
    want = h @ w[11] + w[12]
    got = torch.from_numpy(m.predict(x.numpy()))
    assert rel_l2(got, want) < 1e-4


def test_pad_sequences():
    from distributeddeeplearningspark_amd.utils import pad_sequences

    seqs = [[1, 2, 3], [4], [], [5, 6, 7, 8, 9]]
    out = pad_sequences(seqs)
    assert out.dtype == np.int32 and out.shape == (4, 5)
    np.testing.assert_array_equal(out, [[0, 0, 1, 2, 3], [0, 0, 0, 0, 4], [0, 0, 0, 0, 0], [5, 6, 7, 8, 9]])
    np.testing.assert_array_equal(pad_sequences(seqs, maxlen=3),
                                  [[1, 2, 3], [0, 0, 4], [0, 0, 0], [7, 8, 9]])
    np.testing.assert_array_equal(pad_sequences(seqs, maxlen=3, padding="post", truncating="post"),
                                  [[1, 2, 3], [4, 0, 0], [0, 0, 0], [5, 6, 7]])
    np.testing.assert_array_equal(pad_sequences(seqs, maxlen=3, padding="post"),
                                  [[1, 2, 3], [4, 0, 0], [0, 0, 0], [7, 8, 9]])
    out = pad_sequences([[1.5], [2.5, 3.5]], dtype="float32", value=-1.0)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, [[-1.0, 1.5], [2.5, 3.5]])
    steps = pad_sequences([np.ones((2, 3)), np.ones((1, 3))], dtype="float32", padding="post")
    assert steps.shape == (2, 2, 3) and (steps[1, 1] == 0).all()
    with pytest.raises(ValueError):
        pad_sequences(seqs, padding="left")
    with pytest.raises(ValueError):
        pad_sequences(seqs, truncating="left")


class _Group:
    gpu, rule = True, "downpour"

    def __init__(self, reps):
        self.reps, self.batched, self.batch_reason = reps, None, None


class _Rep:
    bs = 8

    def __init__(self, model):
        self.model = model
        self.X, self.Y = torch.zeros(16, 5, 1), torch.zeros(16, 1)


def test_replica_batching_declines_masked_models(capsys):
    """A co-located group of masked models falls back to the per-replica path with a recorded reason."""
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.parallel import replica_batch, replicas

    for build in (lambda: zoo.masked_gru_regressor(units=64, seq_len=5),
                  lambda: zoo.text_lstm_classifier(30, 5, embed_dim=4, units=64)):
        reps = []
        for _ in range(2):
            m = build()
            m.compile("adagrad", "mean_squared_error")
            m.place("cpu", seed=0)
            reps.append(_Rep(m))
        grp = _Group(reps)
        assert "step mask" in replica_batch.why_not(grp)
        assert replicas.ReplicaGroup._try_batched(grp) is False
        assert grp.batched is None and "step mask" in grp.batch_reason
    assert "step mask" in capsys.readouterr().out  # logged


@pytest.fixture(scope="module")
def spark():
    from distributeddeeplearningspark_amd.context import SparkSession

    return SparkSession.builder.master("local[2]").getOrCreate()


def _padded_frame(n=64, maxlen=8, parts=1):
    """Token sequences of ragged length in a zero-padded id column; the label is whether token 1 occurs."""
    from distributeddeeplearningspark_amd.sql.dataframe import from_columns
    from distributeddeeplearningspark_amd.utils import pad_sequences

    rng = np.random.default_rng(0)
    seqs = [list(rng.integers(1, 6, rng.integers(1, maxlen + 1))) for _ in range(n)]
    ids = pad_sequences(seqs, maxlen=maxlen)
    y = np.array([[float(1 in s)] for s in seqs], dtype=np.float32)
    return from_columns({"ids": ids, "label": y}, num_partitions=parts)


def test_single_trainer_on_a_padded_id_column(spark):
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.trainers import SingleTrainer

    m = zoo.text_lstm_classifier(6, 8, embed_dim=4, units=8)
    tr = SingleTrainer(keras_model=m, worker_optimizer="adam", loss="binary_crossentropy", features_col="ids",
                       label_col="label", batch_size=8, num_epoch=12, device="cpu")
    tr.train(_padded_frame())
    h = tr.get_history()[0]
    assert np.isfinite(h).all() and np.mean(h[-8:]) < np.mean(h[:8])


def test_adag_two_gloo_workers_on_a_padded_id_column(spark, monkeypatch):
    from distributeddeeplearningspark_amd.models import zoo
    from distributeddeeplearningspark_amd.trainers import ADAG

    monkeypatch.setenv("DDL_REPLICA_GROUPS", "0")  # one process per worker (gloo)
    m = zoo.text_lstm_classifier(6, 8, embed_dim=4, units=8)
    tr = ADAG(keras_model=m, worker_optimizer="adam", loss="binary_crossentropy", num_workers=2, batch_size=8,
              communication_window=2, num_epoch=12, features_col="ids", label_col="label", device="cpu")
    tr.train(_padded_frame(parts=2))
    hist = tr.get_history()
    assert len(hist) == 2
    for h in hist:
        assert np.isfinite(h).all() and np.mean(h[-8:]) < np.mean(h[:8])
