"""Graph-replayed step time of GRU(128) / LSTM(128) regressors at the NYISO shape (batch 32, 25x1), masked and
unmasked.

``gru`` / ``lstm``                the regressors as shipped (``zoo.gru_regressor`` / ``zoo.lstm_regressor``);
``gru-masked`` / ``lstm-masked``  ``Masking -> GRU|LSTM -> Dense`` over post-padded series: row ``b`` keeps its first
                                  ``1 + (b * 24) // 31`` steps, so about half of the 32 x 25 steps are masked.
A masked step costs one more byte per row in the recurrence kernels plus the mask-derivation launch of the Masking
layer.  Every model is built and captured once, then the variants are timed alternately ``--pairs`` times,
``--steps`` replayed steps each, so drift hits all of them alike.

    python scripts/bench_masked_rnn.py [--steps 200] [--pairs 3] [--models gru,lstm]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributeddeeplearningspark_amd.models import GRU, LSTM, Dense, Masking, Sequential, zoo  # noqa: E402
from distributeddeeplearningspark_amd.models.step import CompiledTrainStep  # noqa: E402

B, T = 32, 25


def build(name, masked):
    if masked:
        cell = GRU if name == "gru" else LSTM
        m = Sequential([Masking(input_shape=(T, 1)), cell(128), Dense(1, activation="linear")])
    else:
        m = (zoo.gru_regressor if name == "gru" else zoo.lstm_regressor)()
    m.compile("adagrad" if name == "gru" else "adam", "mean_squared_error")
    m.place("cuda:0", seed=0)
    st = CompiledTrainStep(m)
    x = torch.rand(B, T, 1) + 0.1
    if masked:  # post-padded: lengths 1 .. 25 over the batch
        for b in range(B):
            x[b, 1 + (b * (T - 1)) // (B - 1):] = 0.0
    x, y = m.to_input(x), m.to_target(torch.rand(B, 1))
    for _ in range(5):
        st(x, y)
    torch.cuda.synchronize()
    assert st.captured, st.fallback_reason
    return st, x, y


def timed(st, x, y, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        st(x, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--models", default="gru,lstm")
    a = ap.parse_args()
    variants = []
    for name in a.models.split(","):
        variants.append((name, build(name, False)))
        variants.append((f"{name}-masked", build(name, True)))
    res = {k: [] for k, _ in variants}
    for _ in range(a.pairs):
        for k, (st, x, y) in variants:
            res[k].append(round(timed(st, x, y, a.steps), 1))
    for k, v in res.items():
        print(f"{k:>14}: " + "  ".join(f"{t:7.1f}" for t in v) + f"   us/step (min {min(v):.1f})", flush=True)
    print(json.dumps({"bench": "masked_rnn_step_us", "steps": a.steps, "results": res}), flush=True)


if __name__ == "__main__":
    main()
