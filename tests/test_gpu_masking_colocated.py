"""A real co-located replica group of masked models: the replica-batched kernels take no step mask, so
the group runs per replica and says why in the log and the result dicts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _padded_series(n=512, T=25, seed=2):
    """Random walks of ragged length, post-padded with zeros; the label follows the last real step."""
    from distributeddeeplearningspark_amd.sql.dataframe import from_columns

    rng = np.random.default_rng(seed)
    x = (np.cumsum(rng.normal(size=(n, T, 1)) * 0.1, axis=1) + 1.0).astype(np.float32)
    lens = rng.integers(1, T + 1, n)
    y = (x[np.arange(n), lens - 1, 0:1] * 0.8 + 0.1).astype(np.float32)
    x[np.arange(T)[None, :] >= lens[:, None]] = 0.0
    return from_columns({"features": x, "label": y}, num_partitions=4)


def test_masked_replica_group_falls_back_with_reason(monkeypatch, capsys):
    from distributeddeeplearningspark_amd import trainers as T
    from distributeddeeplearningspark_amd.models import zoo

    monkeypatch.setenv("DDL_WORKERS_PER_GPU", "4")
    monkeypatch.setenv("DDL_REPLICA_GROUPS", "1")
    m = zoo.masked_gru_regressor(units=128, seq_len=25)
    tr = T.ADAG(keras_model=m, worker_optimizer="adagrad", loss="mean_squared_error", num_workers=4, batch_size=32,
                num_epoch=2, features_col="features", label_col="label", communication_window=5)
    tr.train(_padded_series())
    res = tr._results
    assert all(r["replica_group"]["replicas"] == 4 for r in res), "replica group not used"
    assert not any(r["replica_group"]["batched"] for r in res)
    assert "step mask" in res[0]["replica_group"]["batch_reason"]
    assert "runs per replica (not batched)" in capsys.readouterr().out
    for r in res:
        assert len(r["history"]) == 8 and np.isfinite(r["history"]).all()  # 128 rows, 2 epochs of 4 batches
