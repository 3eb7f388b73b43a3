"""Training-step time of GRU / LSTM regressors at the NYISO shape (batch 32, 25x1) with and without the recurrent
layers' ``dropout`` / ``recurrent_dropout``.

Configurations per (cell, units): ``rate0`` (no dropout: the undirected kernels, fused input projection), ``rec``
(``recurrent_dropout=0.2``: the DROP register-resident kernels, one batch row per workgroup, projection GEMM up
front), ``in`` (``dropout=0.2``: masked copies of x and one projection GEMM per gate) and ``both``.  Every model is
built, warmed and captured once; then all configurations are timed alternately ``--rounds`` times, eager
(``train_on_batch``, ``--eager-steps`` steps) and graph-replayed (``CompiledTrainStep``, ``--steps`` steps), so drift
hits all of them alike.  ``--only-rate0`` times the rate-0 models alone; ``--root DIR`` imports the package from another
checkout (the parent commit's build), which knows no dropout arguments and so needs ``--only-rate0``.
``--trace CELL UNITS CFG`` runs 25 eager steps of one configuration and nothing else, for a kernel trace:

    python scripts/bench_rnn_dropout.py [--rounds 5] [--units 128,64] [--cells lstm,gru] [--only-rate0] [--root DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/bench_rnn_dropout.py --trace lstm 128 rec
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--eager-steps", type=int, default=100)
ap.add_argument("--units", default="128,64")
ap.add_argument("--cells", default="lstm,gru")
ap.add_argument("--only-rate0", action="store_true")
ap.add_argument("--root", default=None)
ap.add_argument("--trace", nargs=3, metavar=("CELL", "UNITS", "CFG"), default=None)
ap.add_argument("--tag", default="")
A = ap.parse_args()
sys.path.insert(0, os.path.abspath(A.root) if A.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from distributeddeeplearningspark_amd.models import GRU, LSTM, Dense, Sequential  # noqa: E402
from distributeddeeplearningspark_amd.models.step import CompiledTrainStep  # noqa: E402

CFGS = {"rate0": {}, "rec": {"recurrent_dropout": 0.2}, "in": {"dropout": 0.2},
        "both": {"dropout": 0.2, "recurrent_dropout": 0.2}}
B, T = 32, 25


def build(cell, units, cfg):
    cls = GRU if cell == "gru" else LSTM
    m = Sequential([cls(units, input_shape=(T, 1), **CFGS[cfg]), Dense(1, activation="linear")])
    m.compile("adagrad" if cell == "gru" else "adam", "mean_squared_error")
    m.place("cuda:0", seed=0)
    rng = np.random.default_rng(0)
    return m, m.to_input(rng.random((B, T, 1), dtype=np.float32)), m.to_target(rng.random((B, 1), dtype=np.float32))


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6  # us per step


def main():
    cases = []
    for cell in A.cells.split(","):
        for units in map(int, A.units.split(",")):
            for cfg in (["rate0"] if A.only_rate0 else list(CFGS)):
                m, x, y = build(cell, units, cfg)
                st = CompiledTrainStep(m)
                for _ in range(6):  # eager warm-up, the capture, first replays
                    st(x, y)
                assert st.captured, st.fallback_reason
                eager = lambda m=m, x=x, y=y: m.train_on_batch(x, y)
                for _ in range(5):
                    eager()
                cases.append(((cell, units, cfg), eager, lambda st=st, x=x, y=y: st(x, y)))
    res = {k: {"eager": [], "graph": []} for k, _, _ in cases}
    for _ in range(A.rounds):  # interleaved: every configuration once per round
        for k, eager, graph in cases:
            res[k]["eager"].append(round(timed(eager, A.eager_steps), 1))
            res[k]["graph"].append(round(timed(graph, A.steps), 1))
    for (cell, units, cfg), r in res.items():
        line = {"bench": "rnn_dropout_step_us", "tag": A.tag, "cell": cell, "units": units, "cfg": cfg}
        for k, v in r.items():
            line[k] = v
            line[k + "_median"] = statistics.median(v)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    if A.trace:
        m, x, y = build(A.trace[0], int(A.trace[1]), A.trace[2])
        for _ in range(25):
            m.train_on_batch(x, y)
        torch.cuda.synchronize()
    else:
        main()
