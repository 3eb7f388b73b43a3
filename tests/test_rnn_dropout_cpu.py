"""``dropout`` / ``recurrent_dropout`` of the recurrent layers on the CPU path.

The oracle is the fold oracle of ``rnn_dropout_oracle.py``: per batch row the unmasked layer with the row's masks
folded into W and U (no code that takes a dropout argument).  Tolerance as ``test_masking_cpu.py``: relative
L2 < 1e-4."""
import json

import numpy as np
import pytest
import torch

from masking_oracle import patterns, rel_l2, weights
from rnn_dropout_oracle import bidir_oracle, oracle, random_masks

B, T, I, H = 5, 7, 3, 8  # one row of every step-mask pattern
NAMES = ("y", "dx", "dW", "dU", "db", "dWb", "dUb", "dbb")


def _leaves(ts):
    return [t.clone().requires_grad_(True) for t in ts]


def _close(got, want):
    for what, a, r in zip(NAMES, got, want):
        err = rel_l2(a, r)
        print(f"{what}: rel L2 {err:.3g}")
        assert err < 1e-4, (what, err)


def _masks(cell, which, gen, n=1):
    """n directions' (dp, rdp); which = 'in' | 'rec' | 'both'."""
    out = []
    for _ in range(n):
        dp = random_masks(cell, B, I, gen) if which in ("in", "both") else None
        rdp = random_masks(cell, B, H, gen) if which in ("rec", "both") else None
        out.append((dp, rdp))
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "stepmask"])
@pytest.mark.parametrize("which", ["in", "rec", "both"])
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_recurrent_with_dropout_masks_matches_fold_oracle(cell, rs, rev, which, masked):
    """``recurrent`` (the autograd node; on the CPU it runs ``recurrent_ref``'s literal formulas): outputs and
    gradients, the gradients landing in the given buffers from the masks saved in forward."""
    from distributeddeeplearningspark_amd.ops import rnn as R

    g = torch.Generator().manual_seed(0)
    x, ws = torch.randn(B, T, I, generator=g), weights(cell, I, H, g)
    dy = torch.randn(B, T, H, generator=g) if rs else torch.randn(B, H, generator=g)
    (dp, rdp), = _masks(cell, which, g)
    mask = patterns(B, T) if masked else None
    lb = _leaves([x, *ws])
    yr = oracle(cell, lb[0], *lb[1:], rs, dp, rdp, mask, rev)
    ref = torch.autograd.grad(yr, lb, dy)
    grads = [torch.zeros_like(t) for t in ws]
    xl = x.clone().requires_grad_(True)
    y = R.recurrent(cell, xl, *ws, grads=tuple(grads), return_sequences=rs, go_backwards=rev, mask=mask,
                    dropout_mask=dp, recurrent_dropout_mask=rdp)
    y.backward(dy)
    _close([y, xl.grad, *grads], [yr, *ref])
    la = _leaves([x, *ws])  # and recurrent_ref itself, differentiated directly
    y2 = R.recurrent_ref(cell, la[0], *la[1:], rs, go_backwards=rev, mask=mask, dropout_mask=dp,
                         recurrent_dropout_mask=rdp)
    _close([y2, *torch.autograd.grad(y2, la, dy)], [yr, *ref])


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "stepmask"])
@pytest.mark.parametrize("which", ["in", "rec", "both"])
@pytest.mark.parametrize("merge", ["concat", "sum"])
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("cell", ["gru", "lstm", "rnn"])
def test_bidirectional_with_dropout_masks_matches_fold_oracle(cell, rs, merge, which, masked):
    from distributeddeeplearningspark_amd.ops import rnn as R

    g = torch.Generator().manual_seed(1)
    x, ws = torch.randn(B, T, I, generator=g), weights(cell, I, H, g, 2)
    Hy = 2 * H if merge == "concat" else H
    dy = torch.randn(B, T, Hy, generator=g) if rs else torch.randn(B, Hy, generator=g)
    (dpf, rdpf), (dpb, rdpb) = _masks(cell, which, g, 2)  # each direction its own masks
    mask = patterns(B, T) if masked else None
    lb = _leaves([x, *ws])
    yr = bidir_oracle(cell, lb[0], lb[1:4], lb[4:], rs, (dpf, dpb), (rdpf, rdpb), mask, merge)
    ref = torch.autograd.grad(yr, lb, dy)
    grads = [torch.zeros_like(t) for t in ws]
    xl = x.clone().requires_grad_(True)
    y = R.bidirectional(cell, xl, ws[:3], ws[3:], grads=(grads[:3], grads[3:]), merge_mode=merge, return_sequences=rs,
                        mask=mask, dropout_mask=(dpf, dpb), recurrent_dropout_mask=(rdpf, rdpb))
    y.backward(dy)
    _close([y, xl.grad, *grads], [yr, *ref])


def test_ones_masks_change_nothing_and_bad_masks_are_rejected():
    from distributeddeeplearningspark_amd.ops import rnn as R

    g = torch.Generator().manual_seed(2)
    x, ws = torch.randn(B, T, I, generator=g), weights("gru", I, H, g)
    plain = R.recurrent("gru", x, *ws, return_sequences=True)
    ones = R.recurrent("gru", x, *ws, return_sequences=True, dropout_mask=torch.ones(3, B, I),
                       recurrent_dropout_mask=torch.ones(3, B, H))
    assert rel_l2(ones, plain) < 1e-6
    for bad in (torch.ones(3, B, I).double(), torch.ones(4, B, I), torch.ones(3, B + 1, I), torch.ones(3, B, H)):
        with pytest.raises(ValueError, match="dropout_mask"):
            R.recurrent("gru", x, *ws, dropout_mask=bad)
    with pytest.raises(ValueError, match="recurrent_dropout_mask"):
        R.recurrent("gru", x, *ws, recurrent_dropout_mask=torch.ones(3, B, I))
    with pytest.raises(ValueError, match="dropout_mask"):
        R.bidirectional("gru", x, ws, ws, dropout_mask=(torch.ones(3, B, I), torch.ones(3, B, H)))


def test_dropout_masks_on_the_cpu():
    from distributeddeeplearningspark_amd.ops.rnn import dropout_masks

    torch.manual_seed(0)
    m = dropout_masks(4, 64, 128, 0.25, "cpu")
    assert m.shape == (4, 64, 128) and m.dtype == torch.float32
    vals = m.unique()
    assert vals.numel() == 2 and vals[0] == 0 and abs(vals[1].item() - 1 / 0.75) < 1e-6
    s, n = vals[1].item(), m.numel()
    assert abs(m.mean().item() - 1) <= 5 * ((s - 1) / n) ** 0.5  # five standard deviations of the mean
    assert not torch.equal(m, dropout_masks(4, 64, 128, 0.25, "cpu"))


# ------------------------------------------------------------------------------------------- layers
def test_layers_take_the_arguments_and_check_their_range():
    from distributeddeeplearningspark_amd.models import GRU, LSTM, SimpleRNN

    for cls in (GRU, LSTM, SimpleRNN):
        l = cls(4, dropout=0.2, recurrent_dropout=0.3)  # a TypeError before the arguments existed
        assert (l.dropout, l.recurrent_dropout) == (0.2, 0.3) and l.uses_dropout
        assert not cls(4).uses_dropout
        for bad in (1.0, -0.1):
            with pytest.raises(ValueError, match="dropout"):
                cls(4, dropout=bad)
            with pytest.raises(ValueError, match="recurrent_dropout"):
                cls(4, recurrent_dropout=bad)


def _model(dropout, recurrent_dropout, bidir=False):
    from distributeddeeplearningspark_amd.models import LSTM, Bidirectional, Dense, Embedding, Sequential

    rnn = LSTM(6, dropout=dropout, recurrent_dropout=recurrent_dropout)
    m = Sequential([Embedding(20, 4, mask_zero=True, input_shape=(8,)), Bidirectional(rnn) if bidir else rnn,
                    Dense(2, activation="softmax")])
    m.compile("adam", "categorical_crossentropy")
    m.place("cpu", seed=0)
    return m


def _ids(n=6):
    from distributeddeeplearningspark_amd.utils import pad_sequences

    rng = np.random.default_rng(0)
    return pad_sequences([list(rng.integers(1, 20, k)) for k in rng.integers(1, 9, n)], maxlen=8, dtype="int64")


@pytest.mark.parametrize("bidir", [False, True])
def test_config_and_json_round_trip(bidir):
    from distributeddeeplearningspark_amd.models import model_from_json
    from distributeddeeplearningspark_amd.utils import deserialize_keras_model, serialize_keras_model

    m = _model(0.3, 0.1, bidir)
    cfg = m.layers[1].get_config()
    cfg = cfg["layer"]["config"] if bidir else cfg
    assert (cfg["dropout"], cfg["recurrent_dropout"]) == (0.3, 0.1)
    for m2 in (model_from_json(m.to_json()), deserialize_keras_model(serialize_keras_model(m), device="cpu")):
        m2.build_model()
        subs = [m2.layers[1].forward_layer, m2.layers[1].backward_layer] if bidir else [m2.layers[1]]
        for l in subs:  # Bidirectional clones the rates into both directions
            assert (l.dropout, l.recurrent_dropout) == (0.3, 0.1)
    # a Keras export carries the keys among others this project ignores or already reads
    d = json.loads(m.to_json())
    lc = d["config"]["layers"][1]["config"]
    assert (lc["layer"]["config"] if bidir else lc)["recurrent_dropout"] == 0.1


@pytest.mark.parametrize("bidir", [False, True])
def test_inference_ignores_the_rates_and_training_draws_fresh_masks(bidir):
    from distributeddeeplearningspark_amd.models.step import _uses_dropout

    ids = _ids()
    m, m0 = _model(0.3, 0.3, bidir), _model(0.0, 0.0, bidir)
    m0.set_weights(m.get_weights())
    np.testing.assert_array_equal(m.predict(ids), m0.predict(ids))  # bit-identical: no mask exists in inference
    assert _uses_dropout(m) and not _uses_dropout(m0)
    x = m.to_input(ids)
    torch.manual_seed(0)
    a, b = m.forward(x, training=True).detach(), m.forward(x, training=True).detach()
    assert not torch.equal(a, b)  # two training forwards draw different masks
    assert torch.equal(m0.forward(x, training=True).detach(), m0.forward(x, training=True).detach())
    assert torch.equal(m.forward(x, training=False).detach(), m0.forward(x, training=False).detach())


def test_training_with_dropout_reduces_the_loss():
    ids = _ids(32)
    y = np.eye(2, dtype=np.float32)[(ids[:, -1] > 10).astype(int)]  # the last token decides
    m = _model(0.2, 0.2)
    torch.manual_seed(0)
    losses = [float(m.train_on_batch(ids, y)) for _ in range(40)]
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5])


def test_zoo_models_take_the_rates():
    from distributeddeeplearningspark_amd.models import zoo

    m = zoo.text_lstm_classifier(30, 8, embed_dim=4, units=6, dropout=0.2, recurrent_dropout=0.1)
    assert (m.layers[1].dropout, m.layers[1].recurrent_dropout) == (0.2, 0.1)
    m = zoo.masked_gru_regressor(units=6, seq_len=6, dropout=0.1, recurrent_dropout=0.2)
    assert (m.layers[1].dropout, m.layers[1].recurrent_dropout) == (0.1, 0.2)
    for m in (zoo.text_lstm_classifier(30, 8), zoo.masked_gru_regressor()):
        assert not m.layers[1].uses_dropout  # the defaults leave the models as they were


class _Group:
    gpu, rule = True, "downpour"

    def __init__(self, reps):
        self.reps, self.batched, self.batch_reason = reps, None, None


class _Rep:
    bs = 8

    def __init__(self, model):
        self.model = model
        self.X, self.Y = torch.zeros(16, 5, 1), torch.zeros(16, 1)


def test_replica_batching_declines_recurrent_dropout():
    from distributeddeeplearningspark_amd.models import GRU, Dense, Sequential
    from distributeddeeplearningspark_amd.parallel import replica_batch

    def reason(**kw):
        reps = []
        for _ in range(2):
            m = Sequential([GRU(64, input_shape=(5, 1), **kw), Dense(1)])
            m.compile("adagrad", "mean_squared_error")
            m.place("cpu", seed=0)
            reps.append(_Rep(m))
        return replica_batch.why_not(_Group(reps))

    assert reason(recurrent_dropout=0.2) == "recurrent dropout (the batched kernels take no dropout masks)"
    assert reason(dropout=0.2) == "recurrent dropout (the batched kernels take no dropout masks)"
    r0 = reason()
    assert r0 is None or "dropout" not in r0
