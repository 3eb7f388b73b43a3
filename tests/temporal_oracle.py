"""Float64 oracles of the masked per-time-step losses, shared by test_temporal_loss_cpu.py and
test_gpu_temporal_loss.py.  Plain torch on the CPU, no project code: ``sum(score * mask) / sum(mask)`` (Keras 2's
``weighted_masked_objective``) with autograd, the masked rows dropped before anything at them is read.  The one
departure from Keras is the project's: a fully masked batch divides by ``max(sum(mask), 1)`` and gives 0."""
import torch


def _keep(x, mask):
    return torch.ones(x.shape[:2], dtype=torch.bool) if mask is None else mask.cpu().bool()


def xent_oracle(logits, mask, labels=None, probs=None):
    """(loss, dlogits) of logits [B, T, K] against labels [B, T] or probs [B, T, K], in float64."""
    lg = logits.detach().cpu().double().clone().requires_grad_(True)
    keep = _keep(lg, mask)
    lp = torch.log_softmax(lg[keep], dim=-1)
    if labels is not None:
        ce = -lp.gather(1, labels.cpu()[keep].long()[:, None])[:, 0]
    else:
        ce = -(probs.cpu().double()[keep] * lp).sum(-1)
    loss = ce.sum() / max(int(keep.sum()), 1)
    (g,) = torch.autograd.grad(loss, [lg])
    return loss.detach(), g


def reg_oracle(pred, target, mask, mae):
    """(loss, dpred) of the temporal MSE (``mae=False``) / MAE of [B, T, F] inputs, in float64."""
    p = pred.detach().cpu().double().clone().requires_grad_(True)
    keep = _keep(p, mask)
    d = p[keep] - target.cpu().double()[keep]
    loss = (d.abs() if mae else d * d).mean(-1).sum() / max(int(keep.sum()), 1)
    (g,) = torch.autograd.grad(loss, [p])
    return loss.detach(), g
