"""Edges of the LayerNorm kernels (csrc/kernels/layernorm.hip) against a float64 LayerNorm of the bf16 input: every
template branch of the forward and backward dispatch on nv = H / 8 (<= 64, <= 128, <= 256 — the VPL = 4
instantiations, 1032 <= H <= 2048 — and above), widths whose last vector holds a single live lane (nv = 1, 65, 97,
129, 257), the maximum H = 4096, M = 1, more rows than the forward's grid covers in one pass (M = 8197: the
grid-stride loop and its prefetch), gamma / beta absent, and the outputs mean and rstd.

mean must be within 4 H 2^-24 max|x| and rstd within a relative 4 H 2^-24 of the float64 values: worst-case fp32
summation bounds with a factor 4 (derived, not measured).

Measured on an MI355X, largest error as a fraction of its bound over all forward cases:

    input                 mean                      rstd
    random                2.1e-05 (M=5, H=776)      0.031 (M=5, H=8)
    64 + N(0, 1)          3.8e-04 (M=5, H=520)      0.031 (M=5, H=8)
    constant rows         0 (exact)                 0.022 (M=5, H=8)
"""
import pytest
import torch

from test_gpu_transformer import _ln_bwd_case, close, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
WIDTHS = [8, 64, 520, 776, 1032, 1536, 2048, 2056, 4096]
SHAPES = [(5, H) for H in WIDTHS] + [(1, 8), (1, 1032), (1, 4096), (8197, 64), (8197, 1032)]


def _C():
    from distributeddeeplearningspark_amd.ops._native import C

    return C()


def _params(H, affine):
    if not affine:
        return None, None
    g = torch.Generator().manual_seed(H)
    return (torch.rand(H, generator=g) + 0.5).to(DEV), (torch.randn(H, generator=g) * 0.1).to(DEV)


def _fwd_check(x, gamma, beta, eps, what):
    """layernorm_fwd through the binding (outputs NaN-filled first) against float64: y with close(), mean and rstd
    with the derived fp32 bounds."""
    M, H = x.shape
    y = torch.full_like(x, NAN)
    mean, rstd = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
    _C().layernorm_fwd(x, gamma, beta, y, mean, rstd, eps, 0.0, 0)
    torch.cuda.synchronize()
    xd = x.cpu().double()
    mu = xd.mean(1)
    rs = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + eps)
    yr = (xd - mu[:, None]) * rs[:, None]
    if gamma is not None:
        yr = yr * gamma.cpu().double() + beta.cpu().double()
    bound = 4 * H * 2.0 ** -24
    em = (mean.cpu().double() - mu).abs().max().item() / (bound * xd.abs().max().item())
    er = ((rstd.cpu().double() - rs).abs() / rs).max().item() / bound
    print(f"LN_STAT {what} M={M} H={H} mean_err/bound={em:.3e} rstd_err/bound={er:.3e}")
    assert torch.isfinite(y.float()).all(), what
    close(y, yr, what=f"{what} y M={M} H={H}")
    assert em <= 1.0 and er <= 1.0, f"{what} M={M} H={H}: mean {em:.3e}, rstd {er:.3e} of their bounds"
    return y


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("M,H", SHAPES)
def test_layernorm_fwd_widths_and_rows(M, H, affine):
    x = (rnd(M, H, seed=H + M).float() * 3 + 1).to(torch.bfloat16)
    _fwd_check(x, *_params(H, affine), 1e-12, "random")


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("H", WIDTHS)
def test_layernorm_fwd_common_offset(H, affine):
    """x = 64 + N(0, 1) rounded to bf16: the two-pass (centred) variance must not cancel."""
    x = (rnd(5, H, seed=H + 1).float() + 64).to(torch.bfloat16)
    _fwd_check(x, *_params(H, affine), 1e-12, "offset")


@pytest.mark.parametrize("H", WIDTHS)
def test_layernorm_fwd_constant_rows(H):
    """All-equal rows: the variance is exactly 0, so at eps = 1e-5 y is beta (finite) and rstd = eps^-1/2."""
    vals = torch.tensor([0.0, 1.0, -2.5, 64.0, 300.0])
    x = vals[:, None].expand(5, H).to(torch.bfloat16).to(DEV).contiguous()
    gamma, beta = _params(H, True)
    y = _fwd_check(x, gamma, beta, 1e-5, "constant")
    assert torch.equal(y, beta.to(torch.bfloat16)[None, :].expand(5, H))
    y0 = _fwd_check(x, None, None, 1e-5, "constant")
    assert torch.all(y0 == 0)


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("M,H", [(5, H) for H in WIDTHS] + [(8197, 64), (8197, 1032)])
def test_layernorm_bwd_widths_and_rows(M, H, parts):
    _ln_bwd_case(M, H, parts, seed=H)


@pytest.mark.parametrize("M,H,parts", [(5, H, 2) for H in WIDTHS] + [(5, 1032, 3), (8197, 64, 3)])
def test_layernorm_bwd_without_gamma(M, H, parts):
    """gamma = None (the kernels substitute 1): dx and the partial rows of dgamma / dbeta (/ dbias) against float64."""
    x = (rnd(M, H, seed=H + 2).float() * 2 + 0.5).to(torch.bfloat16)
    dy = rnd(M, H, seed=H + 3)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    _C().layernorm_fwd(x, None, None, y, mean, rstd, 1e-12, 0.0, 0)
    P = _C().ln_bwd_rows(M, H)
    ws = torch.full((P, parts, H), NAN, device=DEV)
    dx = torch.full_like(x, NAN)
    dxd = torch.full_like(x, NAN) if parts == 3 else None
    _C().layernorm_bwd(dy, x, mean, rstd, None, dx, dxd, 0.0, 0, ws, 0.0, 0, parts)
    red = ws.sum(0)
    xr = x.cpu().double().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (H,), None, None, 1e-12).backward(dy.cpu().double())
    xhat = torch.nn.functional.layer_norm(x.cpu().double(), (H,), None, None, 1e-12)
    close(dx, xr.grad, what=f"ln dx (no gamma) M={M} H={H}")
    close(red[parts - 2], (dy.cpu().double() * xhat).sum(0), rtol=1e-2, atol=2e-2, what=f"ln dgamma (no gamma) H={H}")
    close(red[parts - 1], dy.cpu().double().sum(0), rtol=1e-2, atol=2e-2, what=f"ln dbeta (no gamma) H={H}")
    if parts == 3:
        assert torch.equal(dxd, dx)
        close(red[0], dxd.float().sum(0), rtol=1e-3, atol=1e-3, what=f"ln dbias (no gamma) H={H}")


def test_layernorm_dropout_paths_vpl4():
    """H = 1032 (VPL = 4, a single live lane in the third vector): the forward's output dropout, the backward's
    input dropout and its masked dx_drop output all reproduce dropout_ref's hash mask."""
    from distributeddeeplearningspark_amd.ops import transformer as T

    M, H, p, seed = 37, 1032, 0.2, 12345
    x = rnd(M, H, seed=6)
    y = torch.full_like(x, NAN)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    _C().layernorm_fwd(x, None, None, y, mean, rstd, 1e-5, p, seed)
    ref = T.dropout_ref(torch.nn.functional.layer_norm(x.float(), (H,), eps=1e-5), p, seed)
    close(y, ref, what="ln output dropout H=1032")
    assert torch.equal(y == 0, ref == 0), "the dropped elements are exactly the hash mask's"
    dy = rnd(M, H, seed=7)
    dx, dxd = torch.full_like(x, NAN), torch.full_like(x, NAN)
    _C().layernorm_bwd(dy, x, mean, rstd, None, dx, dxd, p, seed + 1, None, p, seed)
    xr = x.float().requires_grad_(True)
    T.dropout_ref(torch.nn.functional.layer_norm(xr, (H,), eps=1e-5), p, seed).backward(dy.float())
    close(dx, xr.grad, what="ln bwd with input dropout H=1032")
    close(dxd, T.dropout_ref(xr.grad, p, seed + 1), what="ln bwd dx_drop H=1032")


@pytest.mark.parametrize("H", [4104, 12])
def test_layernorm_width_limits_raise(H):
    """H > 4096 and H % 8 != 0 are refused by the binding's own check, on the host, before any launch."""
    M = 2
    x = rnd(M, H, seed=1)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    with pytest.raises(RuntimeError, match="H % 8 == 0 and H <= 4096"):
        _C().layernorm_fwd(x, None, None, y, mean, rstd, 1e-5, 0.0, 0)
    with pytest.raises(RuntimeError, match="H % 8 == 0 and H <= 4096"):
        _C().layernorm_bwd(x, x, mean, rstd, None, y, None, 0.0, 0, None, 0.0, 0, 2)
