"""Losses.  ``softmax_cross_entropy`` is ONE fused HIP kernel that returns the loss and
stores dlogits during the forward sweep (the backward only hands them out)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import zpad as ZP
from ._native import C, use_native


# The root node of a ``loss.backward()`` a training step runs from a unit seed (models/core.py
# backward_unit): that loss node hands out its stored gradient as is — no scaling launch.  Only the
# root qualifies: a loss node inside a user's composite loss receives a non-unit gradient.
_UNIT_SEED = [None]


def unit_seed(ctx) -> bool:
    return ctx is _UNIT_SEED[0]


# small heads (B x K up to 16K logits: MNIST's 16 x 10): one workgroup computes every row AND the batch loss;
# larger ones (ResNet-50's 256 x 1000) keep a workgroup per row + one reduce launch (a single workgroup
# walking 256K logits measured ~0.1 ms/step slower)
_SMALL_LOGITS = 16384


class _SoftmaxXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, probs, smoothing, ignore_index):
        B, K = logits.shape
        if use_native(logits):
            if logits.stride(1) != 1:
                logits = logits.contiguous()
            ld = logits.stride(0)
            # dlogits in the logits' layout; the kernel zeroes the columns past K, so a padded logits row
            # (ops/zpad.py: a Dense(10) head writes [B, 16]) gives zero-padded dlogits the Dense reads as is
            dfull = torch.empty((B, ld), dtype=logits.dtype, device=logits.device)
            dl = ZP.logical(dfull, K)
            loss = torch.empty(1, dtype=torch.float32, device=logits.device)
            small = B * K <= _SMALL_LOGITS
            rows = None if small else torch.empty(B, dtype=torch.float32, device=logits.device)
            if labels is not None:
                # 1 / #valid labels on the device (no host sync): the gradient scale and the loss normaliser
                inv = torch.empty(1, dtype=torch.float32, device=logits.device)
                lab = labels.to(torch.int64).contiguous()
                C().label_count_inv(lab, ignore_index, inv)
                C().softmax_xent(logits, lab, None, rows, dl, 1.0, smoothing, ignore_index, inv,
                                 loss if small else None, 1.0)
                if not small:
                    C().rows_sum_scaled(rows, 1.0, inv, loss)
            else:
                C().softmax_xent(logits, None, probs.to(torch.float32).contiguous(), rows, dl, 1.0 / B, 0.0, -100,
                                 None, loss if small else None, 1.0 / B)
                if not small:
                    C().rows_sum_scaled(rows, 1.0 / B, None, loss)
            ctx.save_for_backward(dl)
            return loss.view(())
        with torch.enable_grad():
            lg = logits.detach().requires_grad_(True)
            lp = F.log_softmax(lg.float(), dim=-1)
            if labels is not None:
                loss = F.nll_loss(lp, labels.long(), ignore_index=ignore_index, reduction="none")
                if smoothing > 0:
                    sm = -lp.mean(dim=-1)
                    loss = (1 - smoothing) * loss + smoothing * sm * (labels != ignore_index)
                valid = (labels != ignore_index).sum().clamp_min(1)
                out = loss.sum() / valid
            else:
                out = -(probs.float() * lp).sum(-1).mean()
            (dl,) = torch.autograd.grad(out, [lg])
        ctx.save_for_backward(dl)
        return out.detach()

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        if unit_seed(ctx):
            return dl, None, None, None, None
        return (dl * g.to(dl.dtype)).to(dl.dtype), None, None, None, None


def softmax_cross_entropy(logits, labels=None, probs=None, label_smoothing=0.0, ignore_index=-100):
    """Mean CE of softmax(logits) against class ``labels`` or target ``probs`` rows."""
    if (labels is None) == (probs is None):
        raise ValueError("pass exactly one of labels / probs")
    return _SoftmaxXentFn.apply(logits, labels, probs, float(label_smoothing), int(ignore_index))


class _MSEFn(torch.autograd.Function):
    """One HIP launch computes the loss and stores d loss / d pred (backward = one scale)."""

    @staticmethod
    def forward(ctx, pred, target):
        p = pred.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        C().mse_fwd_bwd(p, target.contiguous(), loss, grad)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad if unit_seed(ctx) else grad * g), None


def mean_squared_error(pred, target):
    if use_native(pred) and pred.dtype == torch.float32 and target.dtype == torch.float32 \
            and pred.shape == target.shape:
        return _MSEFn.apply(pred, target)
    return ((pred.float() - target.float()) ** 2).mean()


def mean_absolute_error(pred, target):
    return (pred.float() - target.float()).abs().mean()


# ------------------------------------------------------------------------------------------------
# Masked per-time-step losses of a [B, T, .] output (Keras 2 ``weighted_masked_objective``:
# ``mean(score * mask / mean(mask))`` = ``sum(score * mask) / sum(mask)``).  ``mask`` is the uint8 [B, T]
# step mask of ``ops/mask.py`` (None: every step counts).  The normaliser ``1 / max(sum(mask), 1)`` is counted on
# the device, so a batch whose every step is masked gives a loss of exactly 0 and zero gradients (Keras divides
# by zero there and returns NaN).  A masked step is selected out, not multiplied by 0: whatever stands at it
# (NaN, a label outside the classes) never reaches the loss or the gradient, and its gradient row is zeros.
def _temporal_fp32(what, *tensors):
    for t in tensors:
        if t is not None and t.is_floating_point() and t.dtype != torch.float32:
            raise ValueError(f"{what} runs in fp32 (masked and recurrent models keep fp32), got {t.dtype}")


def _flat_mask(mask, B, T):
    if mask is None:
        return None
    if tuple(mask.shape) != (B, T):
        raise ValueError(f"the step mask must be [{B}, {T}], got {tuple(mask.shape)}")
    return mask.reshape(B * T)


class _TemporalXentFn(torch.autograd.Function):
    """Temporal softmax cross-entropy over rows [R, K]: count (masked only), sweep, row reduce: at most three
    HIP launches; the sweep stores dlogits, the backward hands them out."""

    @staticmethod
    def forward(ctx, logits, labels, probs, mask):
        R, K = logits.shape
        if use_native(logits):
            lg = logits.contiguous()
            dev = lg.device
            dl = torch.empty_like(lg)
            rows = torch.empty(R, dtype=torch.float32, device=dev)
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            lab = None if labels is None else labels.to(torch.int64).contiguous()
            pr = None if probs is None else probs.contiguous()
            inv = None
            if mask is not None:
                mask = mask.to(torch.uint8).contiguous()
                inv = torch.empty(1, dtype=torch.float32, device=dev)
                C().mask_count_inv(mask, inv)
            C().temporal_xent(lg, lab, pr, mask, inv, 1.0 / max(R, 1), rows, dl)
            C().rows_sum_scaled(rows, 1.0 if inv is not None else 1.0 / max(R, 1), inv, loss)
            ctx.save_for_backward(dl)
            return loss.view(())
        with torch.enable_grad():
            lg = logits.detach().requires_grad_(True)
            keep = torch.ones(R, dtype=torch.bool, device=lg.device) if mask is None else mask.bool()
            cnt = keep.sum().clamp_min(1).to(torch.float32)
            if labels is not None:
                lab = labels.long()
                keep = keep & (lab >= 0) & (lab < K)  # a label outside the classes: no loss, no gradient
            rows_kept = lg[keep]  # selection: nothing at a dropped row enters the graph
            lp = F.log_softmax(rows_kept, dim=-1)
            if labels is not None:
                ce = -lp.gather(1, lab[keep][:, None])[:, 0]
            else:
                ce = -(probs[keep] * lp).sum(-1)
            out = ce.sum() / cnt
            (dl,) = torch.autograd.grad(out, [lg])
        ctx.save_for_backward(dl)
        return out.detach()

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl if unit_seed(ctx) else dl * g), None, None, None


def temporal_softmax_cross_entropy(logits, labels=None, probs=None, mask=None):
    """Per-step CE of ``softmax(logits [B, T, K])`` (softmax over K) against class ``labels [B, T]`` or target
    ``probs [B, T, K]``, averaged over the steps where ``mask [B, T]`` is set: ``sum_r mask_r CE_r / max(sum(mask), 1)``.
    A batch with every step masked gives exactly 0 (Keras gives NaN); see the section comment above."""
    if (labels is None) == (probs is None):
        raise ValueError("pass exactly one of labels / probs")
    if logits.dim() != 3:
        raise ValueError(f"temporal_softmax_cross_entropy expects [B, T, K] logits, got {tuple(logits.shape)}")
    _temporal_fp32("temporal_softmax_cross_entropy", logits, probs)
    B, T, K = logits.shape
    if labels is not None:
        if labels.numel() != B * T:
            raise ValueError(f"labels must be [{B}, {T}], got {tuple(labels.shape)}")
        labels = labels.reshape(B * T)
    else:
        if tuple(probs.shape) != (B, T, K):
            raise ValueError(f"probs must be [{B}, {T}, {K}], got {tuple(probs.shape)}")
        probs = probs.reshape(B * T, K)
    return _TemporalXentFn.apply(logits.reshape(B * T, K), labels, probs, _flat_mask(mask, B, T))


class _TemporalRegFn(torch.autograd.Function):
    """Temporal MSE / MAE over rows [R, F]: ONE HIP launch counts the mask, computes the loss and stores the
    gradient."""

    @staticmethod
    def forward(ctx, pred, target, mask, mae):
        R, Fd = pred.shape
        if use_native(pred):
            p = pred.contiguous()
            loss = torch.empty((), dtype=torch.float32, device=p.device)
            grad = torch.empty_like(p)
            C().temporal_reg(p, target.contiguous(), None if mask is None else mask.to(torch.uint8).contiguous(),
                             bool(mae), loss, grad)
            ctx.save_for_backward(grad)
            return loss
        with torch.enable_grad():
            pg = pred.detach().requires_grad_(True)
            keep = torch.ones(R, dtype=torch.bool, device=pg.device) if mask is None else mask.bool()
            cnt = keep.sum().clamp_min(1).to(torch.float32)
            d = pg[keep] - target[keep]
            score = (d.abs() if mae else d * d).mean(-1)
            out = score.sum() / cnt
            (grad,) = torch.autograd.grad(out, [pg])
        ctx.save_for_backward(grad)
        return out.detach()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad if unit_seed(ctx) else grad * g), None, None, None


def _temporal_reg(what, pred, target, mask, mae):
    if pred.dim() != 3:
        raise ValueError(f"{what} expects [B, T, F] predictions, got {tuple(pred.shape)}")
    if target.numel() != pred.numel():
        raise ValueError(f"{what}: target {tuple(target.shape)} does not match pred {tuple(pred.shape)}")
    _temporal_fp32(what, pred, target)
    B, T, Fd = pred.shape
    return _TemporalRegFn.apply(pred.reshape(B * T, Fd), target.reshape(B * T, Fd), _flat_mask(mask, B, T), mae)


def temporal_mean_squared_error(pred, target, mask=None):
    """``sum_r mask_r mean_F (pred - target)^2 / max(sum(mask), 1)`` of ``[B, T, F]`` inputs and a ``[B, T]`` step
    mask (exactly 0 when every step is masked, where Keras gives NaN)."""
    return _temporal_reg("temporal_mean_squared_error", pred, target, mask, False)


def temporal_mean_absolute_error(pred, target, mask=None):
    """``sum_r mask_r mean_F |pred - target| / max(sum(mask), 1)``; the gradient is ``sign(pred - target)`` with
    ``sign(0) = 0`` (exactly 0 when every step is masked, where Keras gives NaN)."""
    return _temporal_reg("temporal_mean_absolute_error", pred, target, mask, True)


def binary_crossentropy(pred, target, eps=1e-7):
    p = pred.float().clamp(eps, 1 - eps)
    t = target.float()
    return -(t * torch.log(p) + (1 - t) * torch.log(1 - p)).mean()


class _ProbXentFn(torch.autograd.Function):
    """Keras cross-entropy on probabilities (``-sum y log clip(p, eps, 1 - eps)``, batch mean): one HIP
    sweep writes the per-row losses and d loss / d p; a second reduces the rows (no ATen on the GPU)."""

    @staticmethod
    def forward(ctx, probs, labels, target, eps, ignore_index):
        p = probs.float().contiguous()
        B = p.shape[0]
        rows = torch.empty(B, dtype=torch.float32, device=p.device)
        dp = torch.empty_like(p)
        C().prob_xent(p, None if labels is None else labels.to(torch.int64).contiguous(),
                      None if target is None else target.float().contiguous(), rows, dp, float(eps), 1.0 / B,
                      int(ignore_index))
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        C().rows_sum_scaled(rows, 1.0 / B, None, loss.view(1))
        ctx.save_for_backward(dp)
        ctx.in_dtype = probs.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        if unit_seed(ctx) and dp.dtype == ctx.in_dtype:
            return dp, None, None, None, None
        return (dp * g).to(ctx.in_dtype), None, None, None, None


def prob_cross_entropy(probs, labels=None, target=None, eps=1e-7, ignore_index=-100):
    """Mean Keras CE of probability rows ``probs`` [B, K] against class ``labels`` [B] (sparse form) or
    target rows [B, K] (``categorical_crossentropy`` on a model whose softmax is an output layer)."""
    if (labels is None) == (target is None):
        raise ValueError("pass exactly one of labels / target")
    if use_native(probs):
        return _ProbXentFn.apply(probs, labels, target, eps, ignore_index)
    p = probs.float().clamp(eps, 1 - eps)
    if labels is not None:
        lab = labels.long().reshape(-1)
        keep = (lab != ignore_index) & (lab >= 0) & (lab < p.shape[1])
        picked = torch.log(p.gather(1, lab.clamp(0, p.shape[1] - 1)[:, None])[:, 0])
        return -(picked * keep).sum() / p.shape[0]
    return -(target.float() * torch.log(p)).sum(-1).mean()


def categorical_crossentropy_probs(probs, target, eps=1e-7):
    """Keras semantics on already-softmaxed outputs: -sum(y*log(clip(p)))."""
    return prob_cross_entropy(probs.reshape(probs.shape[0], -1), target=target.reshape(probs.shape[0], -1), eps=eps)
