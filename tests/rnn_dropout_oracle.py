"""Fold oracle of recurrent layers with dropout masks, shared by test_rnn_dropout_cpu.py and test_gpu_rnn_dropout.py.

It is built only from code that takes no dropout argument.  The masks fold into the weights per batch row,
``(x * dp[g][b]) W_g = x (diag(dp[g][b]) W_g)`` and ``(h * rdp[g][b]) U_g = h (diag(rdp[g][b]) U_g)`` (for the GRU
candidate too: r * h is what meets U_h), so row b of the dropout layer is the unmasked layer run on row b alone with
row-scaled W and U: the unmasked ``recurrent_ref`` without a step mask, ``masking_oracle.oracle`` with one.
Gradients come from autograd through this construction."""
import torch

from masking_oracle import GATES, oracle as masked_oracle


def random_masks(cell, B, n, gen):
    """fp32 [G, B, n] dense multipliers in [0.5, 1.5] with about a quarter of the entries 0: the kernels only
    multiply, so zeros and scales are both exercised."""
    G = GATES[cell]
    m = 0.5 + torch.rand(G, B, n, generator=gen)
    return m * (torch.rand(G, B, n, generator=gen) >= 0.25)


def _fold(M, m, H, r):
    """Column block g of M [n, G H] scaled by m[g][r][:, None]."""
    if m is None:
        return M
    return torch.cat([M[:, g * H:(g + 1) * H] * m[g, r][:, None] for g in range(m.shape[0])], 1)


def oracle(cell, x, W, U, b, rs, dp=None, rdp=None, mask=None, go_backwards=False, act="tanh", ract="hard_sigmoid"):
    from distributeddeeplearningspark_amd.ops.rnn import recurrent_ref

    H = U.shape[0]
    rows = []
    for r in range(x.shape[0]):
        Wr, Ur = _fold(W, dp, H, r), _fold(U, rdp, H, r)
        if mask is None:
            y = recurrent_ref(cell, x[r:r + 1], Wr, Ur, b, rs, act, ract, go_backwards)
        else:
            y = masked_oracle(cell, x[r:r + 1], Wr, Ur, b, rs, mask[r:r + 1], go_backwards, act, ract)
        rows.append(y[0])
    return torch.stack(rows)


def bidir_oracle(cell, x, fwd, bwd, rs, dps=(None, None), rdps=(None, None), mask=None, merge="concat", act="tanh",
                 ract="hard_sigmoid"):
    yf = oracle(cell, x, *fwd, rs, dps[0], rdps[0], mask, False, act, ract)
    yb = oracle(cell, x, *bwd, rs, dps[1], rdps[1], mask, True, act, ract)
    if rs:
        yb = yb.flip(1)  # back to input time order
    if merge == "concat":
        return torch.cat([yf, yb], -1)
    return yf + yb if merge == "sum" else (yf + yb) * 0.5
