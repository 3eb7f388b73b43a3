"""Graph-replayed step time of the GRU / LSTM / BiGRU / BiLSTM regressors (batch 32, 25x1 -> 128 units).

``--bidir fused``  the Bidirectional layer as shipped: one autograd node, ONE recurrence launch per pass
                   (both directions side by side, direction on blockIdx.y);
``--bidir split``  the same layer run as two single-direction ops (forward + go_backwards) and a concat:
                   TWO recurrence launches per pass (plus one small concat / split copy each way);
``--bidir both``   (default) both, alternately.
The unidirectional regressors are the floor.  Every model is built and captured once, then the variants are timed
alternately ``--pairs`` times, ``--steps`` replayed steps each, so drift hits all of them alike.

    python scripts/bench_birnn.py [--steps 200] [--pairs 3] [--bidir both|fused|split] [--models gru,lstm,bigru,bilstm]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributeddeeplearningspark_amd.models import Bidirectional, zoo  # noqa: E402
from distributeddeeplearningspark_amd.models.step import CompiledTrainStep  # noqa: E402


class SplitBidirectional(Bidirectional):
    """Bidirectional (concat, last state) as two single-direction ops: the two-launch baseline."""

    def call(self, x, training=False):
        yf = self.forward_layer.call(x, training)
        yb = self.backward_layer.call(x, training)
        if self.forward_layer.return_sequences:
            yb = yb.flip(1)
        return torch.cat([yf, yb], -1)


def build(name, split):
    base = {"gru": zoo.gru_regressor, "lstm": zoo.lstm_regressor, "bigru": zoo.bigru_regressor,
            "bilstm": zoo.bilstm_regressor}[name]
    m = base()
    if split:
        bi = m.layers[0]
        m.layers[0] = SplitBidirectional(bi.layer, merge_mode=bi.merge_mode, input_shape=bi._input_shape_arg)
    m.compile("adagrad" if "gru" in name else "adam", "mean_squared_error")
    m.place("cuda:0", seed=0)
    st = CompiledTrainStep(m)
    x = m.to_input(torch.rand(32, 25, 1))
    y = m.to_target(torch.rand(32, 1))
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
    ap.add_argument("--bidir", choices=("both", "fused", "split"), default="both")
    ap.add_argument("--models", default="gru,lstm,bigru,bilstm")
    a = ap.parse_args()
    variants = []
    for name in a.models.split(","):
        if name.startswith("bi"):
            if a.bidir in ("both", "fused"):
                variants.append((f"{name}-fused", build(name, False)))
            if a.bidir in ("both", "split"):
                variants.append((f"{name}-split", build(name, True)))
        else:
            variants.append((name, build(name, False)))
    res = {k: [] for k, _ in variants}
    for _ in range(a.pairs):
        for k, (st, x, y) in variants:
            res[k].append(round(timed(st, x, y, a.steps), 1))
    for k, v in res.items():
        print(f"{k:>14}: " + "  ".join(f"{t:7.1f}" for t in v) + f"   us/step (min {min(v):.1f})", flush=True)
    print(json.dumps({"bench": "birnn_step_us", "steps": a.steps, "results": res}), flush=True)


if __name__ == "__main__":
    main()
