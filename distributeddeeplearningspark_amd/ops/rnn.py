"""Keras-2 recurrent cells (GRU ``reset_after=False``, LSTM, SimpleRNN).

Math (Keras 2, the reference's GRU/LSTM, ``ddl_nyiso_aztk.py:201-203,249-251``):
  GRU : z = hs(x Wz + h Uz + bz); r = hs(x Wr + h Ur + br);
        hh = tanh(x Wh + (r*h) Uh + bh); h = z*h + (1-z)*hh
  LSTM: i,f,o = hs(x W + h U + b) (gate order i,f,c,o); c = f*c + i*tanh(...); h = o*tanh(c)
with hs = hard_sigmoid = clip(0.2x+0.5, 0, 1).

The whole input projection x@W for all T steps is ONE fp32 MFMA GEMM (or fused into the
register-resident kernel for narrow inputs); the recurrence runs in the persistent HIP kernels
(``csrc/kernels/rnn.hip``): the register-resident fast path for the Keras defaults (tanh +
hard_sigmoid, H = 64/128), the generic kernels for every other activation pair, SimpleRNN and
other widths.  CPU tensors use the reference path below.  Parameter gradients accumulate
into the arena in one launch.

``go_backwards`` (Keras: the sequence is processed last-to-first, a returned sequence is in
processing order) and ``bidirectional`` (both directions as ONE autograd node: one recurrence
launch per pass with the direction on ``blockIdx.y``, the concat output written in place) run
the directed instantiations of the same kernels; nothing is flipped or concatenated in memory.

``mask`` (``uint8 [B, T]`` in input time order, 1 = data; ``ops/mask.py``): a masked step carries the state over,
so its output is the previous output in processing order (zeros before the first data step) and the last
output is the state after the last data step; its gate gradients are zero and dh / dc pass through.  Masked
layers run the masked instantiations of the directed kernels; the mask is saved for the backward pass.

``dropout_mask`` / ``recurrent_dropout_mask`` (Keras ``dropout`` / ``recurrent_dropout``, ``implementation=1``;
fp32 ``[G, B, I]`` / ``[G, B, H]`` multipliers, one per gate, constant over the T steps; ``dropout_masks`` draws them):
gate g reads ``(x_t * dp[g]) W_g + b_g + (h * rdp[g]) U_g`` (the GRU candidate ``(r * h * rdp[2]) U_h``); the
element-wise state updates keep the unmasked h.  The recurrent masks act inside the DROP instantiations of the
directed kernels (the register-resident ones fold a row's mask into its U registers, one batch row per workgroup);
the input masks act in the projection, which is then computed up front and never fused.  The masks are saved for
the backward pass, not regenerated.
"""
from __future__ import annotations

import torch

from ._native import C, use_native
from ._ref import accumulate, ref_grads

GATES ={"gru": 3, "lstm": 4, "rnn": 1}


def _act(name):
    from .act import activation_ref

    if name == "softmax" or name == "gelu":
        raise ValueError(f"unsupported recurrent activation {name!r}")
    return lambda x: activation_ref(name, x)


def recurrent_ref(cell, x, W, U, b, return_sequences, activation="tanh", recurrent_activation="hard_sigmoid",
                  go_backwards=False, mask=None, dropout_mask=None, recurrent_dropout_mask=None):
    if dropout_mask is not None or recurrent_dropout_mask is not None:
        return _recurrent_dropout_ref(cell, x, W, U, b, return_sequences, activation, recurrent_activation,
                                      go_backwards, mask, dropout_mask, recurrent_dropout_mask)
    keep = None if mask is None else mask.to(torch.bool).unsqueeze(-1)  # [B, T, 1]
    if go_backwards:  # Keras: reversed input; a returned sequence stays in processing order
        x = x.flip(1)
        keep = None if keep is None else keep.flip(1)
    B, T, _ = x.shape
    H = U.shape[0]
    act, ract = _act(activation), _act(recurrent_activation)
    xw = x @ W
    if b is not None:
        xw = xw + b
    h = x.new_zeros((B, H))
    c = x.new_zeros((B, H))
    outs = []
    for t in range(T):
        xt = xw[:, t]
        hp, cp = h, c
        if cell == "gru":
            hu = h @ U[:, : 2 * H]
            z = ract(xt[:, :H] + hu[:, :H])
            r = ract(xt[:, H : 2 * H] + hu[:, H:])
            hh = act(xt[:, 2 * H :] + (r * h) @ U[:, 2 * H :])
            h = z * h + (1 - z) * hh
        elif cell == "lstm":
            g = xt + h @ U
            i = ract(g[:, :H])
            f = ract(g[:, H : 2 * H])
            cc = act(g[:, 2 * H : 3 * H])
            o = ract(g[:, 3 * H :])
            c = f * c + i * cc
            h = o * act(c)
        else:
            h = act(xt + h @ U)
        if keep is not None:  # a masked step carries the state (and so the output) over
            h = torch.where(keep[:, t], h, hp)
            c = torch.where(keep[:, t], c, cp)
        if return_sequences:
            outs.append(h)
    return torch.stack(outs, 1) if return_sequences else h


def _recurrent_dropout_ref(cell, x, W, U, b, return_sequences, activation, recurrent_activation, go_backwards, mask,
                           dp, rdp):
    """The Keras ``implementation=1`` formulas with per-gate dropout masks dp [G, B, I] / rdp [G, B, H] (either may
    be None): every gate contracts its own masked copy of x_t and of h (the GRU candidate of r * h); the state
    updates keep the unmasked h."""
    keep = None if mask is None else mask.to(torch.bool).unsqueeze(-1)  # [B, T, 1]
    if go_backwards:
        x = x.flip(1)
        keep = None if keep is None else keep.flip(1)
    B, T, _ = x.shape
    H = U.shape[0]
    G = GATES[cell]
    act, ract = _act(activation), _act(recurrent_activation)
    Wg, Ug = W.split(H, 1), U.split(H, 1)
    bg = [None] * G if b is None else b.split(H)
    xin = lambda xt, g: (xt if dp is None else xt * dp[g]) @ Wg[g] + (0 if bg[g] is None else bg[g])
    rec = lambda hh, g: (hh if rdp is None else hh * rdp[g]) @ Ug[g]
    h = x.new_zeros((B, H))
    c = x.new_zeros((B, H))
    outs = []
    for t in range(T):
        xt = x[:, t]
        hp, cp = h, c
        if cell == "gru":
            z = ract(xin(xt, 0) + rec(h, 0))
            r = ract(xin(xt, 1) + rec(h, 1))
            hh = act(xin(xt, 2) + rec(r * h, 2))
            h = z * h + (1 - z) * hh
        elif cell == "lstm":
            i = ract(xin(xt, 0) + rec(h, 0))
            f = ract(xin(xt, 1) + rec(h, 1))
            cc = act(xin(xt, 2) + rec(h, 2))
            o = ract(xin(xt, 3) + rec(h, 3))
            c = f * c + i * cc
            h = o * act(c)
        else:
            h = act(xin(xt, 0) + rec(h, 0))
        if keep is not None:  # a masked step carries the state over; the dropout masks are indifferent to it
            h = torch.where(keep[:, t], h, hp)
            c = torch.where(keep[:, t], c, cp)
        if return_sequences:
            outs.append(h)
    return torch.stack(outs, 1) if return_sequences else h


def bidirectional_ref(cell, x, fwd, bwd, return_sequences, merge_mode="concat", activation="tanh",
                      recurrent_activation="hard_sigmoid", mask=None, dropout_mask=(None, None),
                      recurrent_dropout_mask=(None, None)):
    """Both directions through ``recurrent_ref`` (the same mask to both, each its own dropout masks); the backward
    sequence is re-reversed before the merge."""
    yf = recurrent_ref(cell, x, *fwd, return_sequences, activation, recurrent_activation, mask=mask,
                       dropout_mask=dropout_mask[0], recurrent_dropout_mask=recurrent_dropout_mask[0])
    yb = recurrent_ref(cell, x, *bwd, return_sequences, activation, recurrent_activation, go_backwards=True,
                       mask=mask, dropout_mask=dropout_mask[1], recurrent_dropout_mask=recurrent_dropout_mask[1])
    if return_sequences:
        yb = yb.flip(1)
    if merge_mode == "concat":
        return torch.cat([yf, yb], -1)
    return yf + yb if merge_mode == "sum" else (yf + yb) * 0.5


def _act_codes(act, ract):
    codes = C().ACT_CODES
    for a in (act, ract):
        if a not in codes or a == "gelu":
            raise ValueError(f"recurrent activation {a!r} has no HIP kernel (supported: "
                             f"{sorted(k for k in codes if k != 'gelu')})")
    return codes[act], codes[ract]


class _RecurrentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, U, b, gW, gU, gb, cfg, mask=None, dp=None, rdp=None):
        cell, rs, act, ract, hook, rev = cfg
        ctx.cfg = cfg
        ctx.masked = mask is not None
        ctx.drop = (dp is not None, rdp is not None)
        keep = tuple(t for t in (mask, dp, rdp) if t is not None)  # saved for the backward, not recomputed
        drop = {} if dp is None and rdp is None else {"dropout_mask": dp, "recurrent_dropout_mask": rdp}
        dt = x.dtype
        xf, Wf, Uf = x.float(), W.float(), U.float()
        bf = None if b is None else b.float()
        if use_native(x):
            ctx.codes = _act_codes(act, ract)
            if mask is None and not drop:
                y, saved = C().rnn_fwd(cell, xf.contiguous(), Wf.contiguous(), Uf.contiguous(), bf, rs, *ctx.codes, rev)
            else:
                y, saved = C().rnn_fwd(cell, xf.contiguous(), Wf.contiguous(), Uf.contiguous(), bf, rs, *ctx.codes, rev,
                                       False, mask, **drop)
            ctx.native = True
            ctx.grads = (gW, gU, gb)
            ctx.needs_dx = ctx.needs_input_grad[0]
            ctx.save_for_backward(xf, Wf, Uf, bf, *keep, *saved)
            return y.to(dt)
        ctx.native = False
        with torch.no_grad():
            y = recurrent_ref(cell, xf, Wf, Uf, bf, rs, act, ract, rev, mask, dp, rdp)
        ctx.grads = (gW, gU, gb)
        ctx.save_for_backward(xf, Wf, Uf, bf, *keep)
        return y.to(dt)

    @staticmethod
    def backward(ctx, dy):
        cell, rs, act, ract, hook, rev = ctx.cfg
        saved = list(ctx.saved_tensors)
        xf, Wf, Uf, bf = saved[:4]
        mask = saved.pop(4) if ctx.masked else None
        dp = saved.pop(4) if ctx.drop[0] else None
        rdp = saved.pop(4) if ctx.drop[1] else None
        gW, gU, gb = ctx.grads
        if ctx.native:
            # fast path: dW/dU/db are accumulated into the fp32 arena slices in-kernel (None here)
            fp32 = lambda t: t if t is not None and t.dtype == torch.float32 and t.is_contiguous() else None
            drop = {} if dp is None and rdp is None else {"dropout_mask": dp, "recurrent_dropout_mask": rdp}
            extra = () if mask is None and not drop else (False, mask)
            dx, dW, dU, db = C().rnn_bwd(cell, dy.float().contiguous(), xf, Wf, Uf, bf, rs, saved[4:],
                                         fp32(gW), fp32(gU), fp32(gb), ctx.needs_dx, *ctx.codes, rev, *extra, **drop)
        else:
            fn = lambda xx, ww, uu, bb: recurrent_ref(cell, xx, ww, uu, bb, rs, act, ract, rev, mask, dp, rdp)
            dx, dW, dU, db = ref_grads(fn, [xf, Wf, Uf, bf], dy.float())
        accumulate(gW, dW)
        accumulate(gU, dU)
        accumulate(gb, db)
        if hook is not None:
            hook()
        return (None if dx is None else dx.to(dy.dtype)), None, None, None, None, None, None, None, None, None, None


def _check_mask(mask, x):
    if mask.dtype != torch.uint8 or mask.shape != x.shape[:2] or mask.device != x.device:
        raise ValueError(f"mask must be uint8 [B, T] = {tuple(x.shape[:2])} on the input's device, got "
                         f"{mask.dtype} {tuple(mask.shape)} on {mask.device}")
    return mask.contiguous()


def _check_drop(m, cell, x, n, what):
    """A dropout mask of the layer over x: fp32 [G, B, n] on the input's device (None passes)."""
    if m is None:
        return None
    want = (GATES[cell], x.shape[0], n)
    if m.dtype != torch.float32 or tuple(m.shape) != want or m.device != x.device:
        raise ValueError(f"{what} must be fp32 [G, B, n] = {want} on the input's device, got {m.dtype} "
                         f"{tuple(m.shape)} on {m.device}")
    return m.detach().contiguous()


def dropout_masks(G, B, n, rate, device, seed=None):
    """Inverted-dropout masks ``[G, B, n]`` fp32 (0 or 1 / (1 - rate)), one per gate, drawn once per forward call
    and held over all time steps.  On the GPU the counter-hash dropout kernel over a ones tensor (a capturing stream
    mixes the device step counter in, as ``ops.act.dropout`` does, so a replayed hipGraph draws fresh masks every
    step); seeds from ``act.next_seed`` (data-parallel ranks differ).  On the CPU ``F.dropout`` of ones."""
    from . import act as A

    ones = torch.ones((G, B, n), dtype=torch.float32, device=device)
    if not use_native(ones):
        return torch.nn.functional.dropout(ones, float(rate), training=True)
    out = torch.empty_like(ones)
    ds = A.dropout_step_counter(ones.device) if torch.cuda.is_current_stream_capturing() else None
    C().dropout(ones, out, float(rate), A.next_seed() if seed is None else int(seed), ds)
    return out


def recurrent(cell, x, W, U, b=None, *, grads=(None, None, None), return_sequences=False, activation="tanh",
              recurrent_activation="hard_sigmoid", on_grad=None, go_backwards=False, mask=None, dropout_mask=None,
              recurrent_dropout_mask=None):
    gW, gU, gb = grads
    cfg = (cell, bool(return_sequences), activation, recurrent_activation, on_grad, bool(go_backwards))
    mask = None if mask is None else _check_mask(mask, x)
    if dropout_mask is None and recurrent_dropout_mask is None:
        return _RecurrentFn.apply(x, W, U, b, gW, gU, gb, cfg, mask)
    return _RecurrentFn.apply(x, W, U, b, gW, gU, gb, cfg, mask,
                              _check_drop(dropout_mask, cell, x, x.shape[2], "dropout_mask"),
                              _check_drop(recurrent_dropout_mask, cell, x, U.shape[0], "recurrent_dropout_mask"))


MERGE_MODES = ("concat", "sum", "ave")


class _BidirectionalFn(torch.autograd.Function):
    """(x, Wf, Uf, bf, Wb, Ub, bb) -> merged output of the forward and the backward direction."""

    @staticmethod
    def forward(ctx, x, Wf, Uf, bf, Wb, Ub, bb, grads, cfg, mask=None, dpf=None, dpb=None, rdpf=None, rdpb=None):
        cell, rs, act, ract, hook, merge = cfg
        ctx.cfg, ctx.grads = cfg, grads
        ctx.masked = mask is not None
        keep = () if mask is None else (mask,)  # saved for the backward, not recomputed
        dms = (dpf, dpb, rdpf, rdpb)
        ctx.drop = tuple(t is not None for t in dms)
        keep += tuple(t for t in dms if t is not None)
        drop = {} if not any(ctx.drop) else {"dropout_masks": [dpf, dpb], "recurrent_dropout_masks": [rdpf, rdpb]}
        dt = x.dtype
        xf = x.float()
        ws = [None if t is None else t.float() for t in (Wf, Uf, bf, Wb, Ub, bb)]
        if use_native(x):
            ctx.codes = _act_codes(act, ract)
            y, saved = C().birnn_fwd(cell, xf.contiguous(), [ws[0], ws[3]], [ws[1], ws[4]], [ws[2], ws[5]], rs, merge,
                                     *ctx.codes, mask, **drop)
            ctx.native = True
            ctx.needs_dx = ctx.needs_input_grad[0]
            ctx.has_b = (bf is not None, bb is not None)
            ctx.save_for_backward(xf, *keep, *(t for t in ws if t is not None), *saved)
            return y.to(dt)
        ctx.native = False
        with torch.no_grad():
            y = bidirectional_ref(cell, xf, ws[:3], ws[3:], rs, merge, act, ract, mask, (dpf, dpb), (rdpf, rdpb))
        ctx.has_b = (bf is not None, bb is not None)
        ctx.save_for_backward(xf, *keep, *(t for t in ws if t is not None))
        return y.to(dt)

    @staticmethod
    def backward(ctx, dy):
        cell, rs, act, ract, hook, merge = ctx.cfg
        saved = list(ctx.saved_tensors)
        xf = saved.pop(0)
        mask = saved.pop(0) if ctx.masked else None
        dpf, dpb, rdpf, rdpb = (saved.pop(0) if has else None for has in ctx.drop)
        drop = {} if not any(ctx.drop) else {"dropout_masks": [dpf, dpb], "recurrent_dropout_masks": [rdpf, rdpb]}
        ws = []
        for has_b in ctx.has_b:
            ws += [saved.pop(0), saved.pop(0), saved.pop(0) if has_b else None]
        g = list(ctx.grads[0]) + list(ctx.grads[1])  # gWf, gUf, gbf, gWb, gUb, gbb
        if ctx.native:
            fp32 = lambda t: t if t is not None and t.dtype == torch.float32 and t.is_contiguous() else None
            gg = [fp32(t) for t in g]
            dx, pg = C().birnn_bwd(cell, dy.float().contiguous(), xf, [ws[0], ws[3]], [ws[1], ws[4]], [ws[2], ws[5]],
                                   rs, merge, saved, [gg[0], gg[3]], [gg[1], gg[4]], [gg[2], gg[5]], ctx.needs_dx,
                                   *ctx.codes, mask, **drop)
            d = list(pg[0]) + list(pg[1])
        else:
            live = [t for t in ws if t is not None]

            def fn(xx, *flat):
                it = iter(flat)
                full = [None if t is None else next(it) for t in ws]
                return bidirectional_ref(cell, xx, full[:3], full[3:], rs, merge, act, ract, mask, (dpf, dpb),
                                         (rdpf, rdpb))

            out = ref_grads(fn, [xf, *live], dy.float())
            dx, it = out[0], iter(out[1:])
            d = [None if t is None else next(it) for t in ws]
        for buf, val in zip(g, d):
            accumulate(buf, val)
        if hook is not None:
            hook()  # once: both directions' gradients are final here
        return (None if dx is None else dx.to(dy.dtype)), *([None] * 13)


def bidirectional(cell, x, fwd, bwd, *, grads=((None, None, None), (None, None, None)), merge_mode="concat",
                  return_sequences=False, activation="tanh", recurrent_activation="hard_sigmoid", on_grad=None,
                  mask=None, dropout_mask=(None, None), recurrent_dropout_mask=(None, None)):
    """Bidirectional recurrent layer as one autograd node.  ``fwd`` / ``bwd`` = (W, U, b | None) of the forward and the
    backward direction, ``grads`` their (gW, gU, gb) gradient buffers; the backward direction's sequence is
    returned in input time order, merged by ``merge_mode`` (``concat`` / ``sum`` / ``ave``).  Both directions
    read the same ``mask``; ``dropout_mask`` / ``recurrent_dropout_mask`` are (forward, backward) pairs, each
    direction its own masks."""
    if merge_mode not in MERGE_MODES:
        raise ValueError(f"merge_mode {merge_mode!r} is not supported (supported: {MERGE_MODES})")
    (Wf, Uf, bf), (Wb, Ub, bb) = (tuple(fwd) + (None,))[:3], (tuple(bwd) + (None,))[:3]
    cfg = (cell, bool(return_sequences), activation, recurrent_activation, on_grad, merge_mode)
    mask = None if mask is None else _check_mask(mask, x)
    dps = [_check_drop(m, cell, x, x.shape[2], "dropout_mask") for m in dropout_mask]
    rdps = [_check_drop(m, cell, x, Uf.shape[0], "recurrent_dropout_mask") for m in recurrent_dropout_mask]
    if len(dps) != 2 or len(rdps) != 2:
        raise ValueError("bidirectional: one (forward, backward) pair of each dropout mask")
    g = tuple(tuple(t) for t in grads)
    if all(m is None for m in dps + rdps):
        return _BidirectionalFn.apply(x, Wf, Uf, bf, Wb, Ub, bb, g, cfg, mask)
    return _BidirectionalFn.apply(x, Wf, Uf, bf, Wb, Ub, bb, g, cfg, mask, *dps, *rdps)
