"""Step masks of padded sequences (Keras ``Masking`` / ``Embedding(mask_zero=True)``).

A mask is a ``uint8 [B, T]`` tensor in input time order, 1 where the step is data.  It is derived once in the
forward pass (HIP kernels in ``csrc/kernels/rnn.hip`` on the GPU, torch on the CPU), handed to the recurrent
ops (``ops/rnn.py``) and saved by them for the backward pass.
"""
from __future__ import annotations

import torch

from ._native import C, use_native


def feature_mask_ref(x, mask_value=0.0):
    """``mask[b, t] = any_f(x[b, t, f] != mask_value)`` and ``x * mask`` in plain torch."""
    mask = (x != mask_value).any(-1)
    return x * mask.unsqueeze(-1).to(x.dtype), mask.to(torch.uint8)


class _MaskingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask_value):
        if use_native(x):
            if x.dtype != torch.float32:
                raise ValueError("Masking runs in fp32 on the GPU (models with a recurrent layer keep fp32)")
            # mask_value == 0: a masked step is all zeros already, so the output is x itself
            y, mask = C().mask_from_features(x.contiguous(), float(mask_value), mask_value != 0)
            ctx.native = True
            if y.data_ptr() == x.data_ptr():
                y = x.view_as(x)
        else:
            y, mask = feature_mask_ref(x, mask_value)
            ctx.native = False
        ctx.save_for_backward(mask)
        ctx.mark_non_differentiable(mask)
        return y, mask

    @staticmethod
    def backward(ctx, dy, _dmask):
        (mask,) = ctx.saved_tensors
        if ctx.native:
            return C().mask_apply(dy.float().contiguous(), mask).to(dy.dtype), None
        return dy * mask.unsqueeze(-1).to(dy.dtype), None


def masking(x, mask_value=0.0):
    """(``x * mask``, ``mask``) of features ``x [B, T, F]``; the gradient is ``dy * mask``."""
    if x.dim() != 3:
        raise ValueError(f"Masking expects [B, T, F] input, got {tuple(x.shape)}")
    return _MaskingFn.apply(x, float(mask_value))


def ids_mask(ids):
    """``mask[b, t] = ids[b, t] != 0`` of integer token ids ``[B, T]``."""
    if ids.dim() != 2:
        raise ValueError(f"a token-id mask expects [B, T] ids, got {tuple(ids.shape)}")
    if use_native(ids):
        return C().mask_from_ids(ids.contiguous().long())
    return (ids != 0).to(torch.uint8)
