"""Compaction oracle of masked recurrent layers, shared by test_masking_cpu.py and test_gpu_masking.py.

It is built only from the UNMASKED ``recurrent_ref`` (called without ``mask``): per batch row, the unmasked steps
are gathered in processing order and run as a shorter sequence.  The final state is the expected last output, the
outputs are the expected values at the unmasked positions, a masked position expects the preceding output in
processing order (zeros when there is none).  Gradients come from autograd through this construction, so a fully
masked row contributes none."""
import torch

GATES = {"gru": 3, "lstm": 4, "rnn": 1}


def patterns(B, T):
    """uint8 [B, T] mask; by row index: all valid, pre-padded, post-padded, interior holes, fully masked (then
    the same kinds again with other lengths)."""
    m = torch.ones(B, T, dtype=torch.uint8)
    for r in range(B):
        kind, turn = r % 5, r // 5
        if kind == 1:
            m[r, : min(T, max(1, T // 3) + turn)] = 0
        elif kind == 2:
            m[r, max(1, T - T // 2 - turn):] = 0
        elif kind == 3:
            m[r, 1 + turn % 2 : T - 1 : 2] = 0
        elif kind == 4:
            m[r] = 0
    return m


def oracle(cell, x, W, U, b, rs, mask, go_backwards=False, act="tanh", ract="hard_sigmoid"):
    from distributeddeeplearningspark_amd.ops.rnn import recurrent_ref

    B, T, _ = x.shape
    H = U.shape[0]
    zero = x.new_zeros(H)
    out = []
    for r in range(B):
        order = list(range(T - 1, -1, -1)) if go_backwards else list(range(T))
        valid = [t for t in order if mask[r, t]]
        ys = recurrent_ref(cell, x[r, valid].unsqueeze(0), W, U, b, True, act, ract)[0] if valid else None
        if not rs:
            out.append(ys[-1] if valid else zero)
            continue
        rows, last, j = [], zero, 0
        for t in order:
            if mask[r, t]:
                last, j = ys[j], j + 1
            rows.append(last)
        out.append(torch.stack(rows))
    return torch.stack(out)


def bidir_oracle(cell, x, fwd, bwd, rs, mask, merge="concat", act="tanh", ract="hard_sigmoid"):
    yf = oracle(cell, x, *fwd, rs, mask, False, act, ract)
    yb = oracle(cell, x, *bwd, rs, mask, True, act, ract)
    if rs:
        yb = yb.flip(1)  # back to input time order
    if merge == "concat":
        return torch.cat([yf, yb], -1)
    return yf + yb if merge == "sum" else (yf + yb) * 0.5


def weights(cell, I, H, gen, n=1):
    """n directions' (W, U, b) at the scale the recurrent tests use."""
    G = GATES[cell]
    ws = []
    for _ in range(n):
        ws += [torch.randn(I, G * H, generator=gen) * 0.3, torch.randn(H, G * H, generator=gen) * (1.0 / H ** 0.5),
               torch.randn(G * H, generator=gen) * 0.1]
    return ws


def rel_l2(a, r):
    return ((a.detach().cpu().float() - r.detach()).norm() / (r.detach().norm() + 1e-12)).item()
