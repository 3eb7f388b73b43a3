"""bn3's backward folded through conv3 (``ops/fused_blocks.py: _FOLD_BN3``, ``csrc/kernels/bn_fold.hip``).

Identity bottlenecks: the next block's conv1 data-gradient stores the block-output gradient already under
bn3's ReLU mask with its column sums (BNR premask), and conv3 + bn3's backward is evaluated from the small
products P = g^T y2, S = y2^T y2, s = sum y2 — no dx sweep, no read of the 4x-wide conv3 output.

Measured on MI355X (relative-norm error against the fp64 evaluation, folded / existing sweeps):
  (64, 256, 4096)   dW 3.4e-7 / 2.7e-3   d2 2.36e-3 / 2.34e-3   sum g 2.8e-8 / 2.7e-8   sum g (yc - mean) 1.5e-7 / 2.5e-3
  (64, 256, 4000)   dW 3.3e-7 / 2.8e-3   d2 2.36e-3 / 2.36e-3   sum g 2.4e-8 / 2.2e-8   sum g (yc - mean) 1.9e-7 / 2.8e-3
  (128, 512, 4096)  dW 4.3e-7 / 2.6e-3   d2 2.34e-3 / 2.34e-3   sum g 2.7e-8 / 2.5e-8   sum g (yc - mean) 1.6e-7 / 2.5e-3
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _C():
    from distributeddeeplearningspark_amd.ops._native import C

    return C()


def _bits(keep):
    return (keep.reshape(-1, 8).to(torch.uint8) << torch.arange(8, dtype=torch.uint8)).sum(1, dtype=torch.uint8)


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------- producer epilogue
@pytest.mark.parametrize("M,N,K,res", [
    (16384, 256, 64, "mask"),    # streaming kernel, stage-1 conv1 data-gradient + identity shortcut (WN 32)
    (16448, 512, 128, "mask"),   # streaming, ragged last tile, 256 -> 128-wide panels
    (16384, 1024, 256, "mask"),  # streaming, K = 256 two-slot ring (WN 16)
    (16384, 256, 64, "rsub"),    # streaming, stride-2 subgrid residual
    (16384, 256, 64, None),      # streaming, no residual
    (4096, 256, 64, "mask"),     # 128x128 kernel (EPI_BF16_BNR)
    (4000, 512, 128, "mask"),    # 128x128 kernel, ragged
    (4096, 256, 64, "rsub"),     # 128x128 kernel, stride-2 subgrid residual
])
def test_producer_stores_masked_gradient_and_its_sum(M, N, K, res):
    """linear_dgrad with ``bnr["premask"]``: the stored tensor is the plain launch's output AND the mask, bit
    for bit, and the workspace's first row-set holds its column sums (the second stays zero)."""
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    gen = torch.Generator().manual_seed(M + N + K)
    dy = torch.randn(M, K, generator=gen).to(DEV, torch.bfloat16)
    w = (torch.randn(K, N, generator=gen) / K ** 0.5).to(DEV, torch.bfloat16)
    keep = torch.rand(M, N, generator=gen) > 0.4
    mask = _bits(keep).to(DEV)
    kw = {}
    if res == "mask":
        rk = torch.rand(M, N, generator=gen) > 0.5
        kw = dict(resid=torch.randn(M, N, generator=gen).to(DEV, torch.bfloat16), resid_mask=_bits(rk).to(DEV))
    elif res == "rsub":  # rows = [M / 64][8][8] grid, residual on its [4][4] even subgrid
        kw = dict(resid=torch.randn(M // 4, N, generator=gen).to(DEV, torch.bfloat16), rsub=(8, 8))
    stream = G.use_stream(M, N, K, G.KC, G.RC, G.EPI_BF16, K, N, resid=kw.get("resid"), ldr=N if kw else 0)
    assert stream == (M >= 16384)
    x = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)  # must not be read
    mean = torch.full((N,), float("nan"), device=DEV)
    ws = torch.zeros((SHARDS, 2, N), dtype=torch.float32, device=DEV)
    bnr = {"x": x, "mask": mask, "mean": mean, "ws": ws, "premask": True}
    out = G.linear_dgrad(dy, w, bnr=bnr, **kw)
    assert bnr.get("done")
    plain = G.linear_dgrad(dy, w, **kw)
    want = torch.where(keep.to(DEV), plain, torch.zeros_like(plain))
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    got = ws.double().cpu().sum(0)
    s1 = want.double().cpu().sum(0)
    err = (got[0] - s1).abs().max().item()
    assert err <= 1e-4 * want.double().abs().sum(0).max().item(), err  # fp32 accumulation of M bf16 values
    assert torch.count_nonzero(got[1]) == 0


# ------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("Ci,Co,M", [(64, 256, 4096), (64, 256, 4000), (128, 512, 4096)])
def test_folded_backward_matches_fp64_as_well_as_the_sweeps(Ci, Co, M):
    """conv3 + bn3 backward, folded, against an fp64 evaluation of dW = y2^T (A g + B (y2 W^T) + K),
    d2 = (...) W and the two reduce sums; yardstick: the existing path (bn_bwd_reduce + bn_bwd_finalize +
    bn_bwd_dx + dgrad + wgrad) on the same inputs against the same reference.  Each folded relative-norm
    error is at most 2x the existing path's (the two paths round different intermediates to bf16)."""
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    gen = torch.Generator().manual_seed(Ci + Co + M)
    y2 = torch.relu(torch.randn(M, Ci, generator=gen) + 1.0).to(DEV, torch.bfloat16)
    w = (torch.randn(Co, Ci, generator=gen) / Ci ** 0.5).to(DEV, torch.bfloat16)
    gamma = (torch.rand(Co, generator=gen) + 0.5).to(DEV)
    keep = torch.rand(M, Co, generator=gen) > 0.4
    mask = _bits(keep).to(DEV)
    # the output gradient comes from its real producer: a conv1 data-gradient of the next block
    dy1 = torch.randn(M, Ci, generator=gen).to(DEV, torch.bfloat16)
    w1 = (torch.randn(Ci, Co, generator=gen) / Ci ** 0.5).to(DEV, torch.bfloat16)
    yc = G.linear_fwd(y2, w)  # bf16 [M, Co], as the forward stores it
    mean = yc.float().mean(0)
    var = yc.float().var(0, unbiased=False)
    eps = 1e-3
    invstd = torch.rsqrt(var + eps)
    dout = G.linear_dgrad(dy1, w1)

    # fp64 reference
    g64 = dout.double().cpu() * keep.double()
    y64, w64 = y2.double().cpu(), w.double().cpu()
    x64 = y64 @ w64.t()
    mu, inv, gam = mean.double().cpu(), invstd.double().cpu(), gamma.double().cpu()
    r1 = g64.sum(0)
    r2 = (g64 * (x64 - mu)).sum(0)
    A = gam * inv
    m1, m2 = r1 / M, r2 * inv / M
    dx64 = A * g64 + (-A * m2 * inv) * x64 + (-A * m1 + A * m2 * inv * mu)
    ref = {"dW": dx64.t() @ y64, "d2": dx64 @ w64, "sum g": r1, "sum g (yc - mean)": r2, "dgamma": r2 * inv}

    # existing path
    C = _C()
    ws = torch.empty((C.bn_partial_rows(M, Co), 2, Co), dtype=torch.float32, device=DEV)
    C.bn_bwd_reduce(dout, yc, mask, None, None, mean, ws, Co, 3)
    coef = torch.empty(3 * Co, dtype=torch.float32, device=DEV)
    dg0, db0 = torch.zeros(Co, device=DEV), torch.zeros(Co, device=DEV)
    C.bn_bwd_finalize(ws, M, Co, gamma, mean, invstd, dg0, db0, coef)
    dxc = torch.empty_like(dout)
    C.bn_bwd_dx(dout, yc, mask, None, None, coef, dxc, None, Co, 3)
    gw0 = torch.zeros(Co, Ci, dtype=torch.float32, device=DEV)
    G.linear_wgrad(dxc, y2, gw0)
    # the sums as bn_bwd_finalize forms them from the partial rows (added in double, then fp32), which is the
    # point where the folded path hands over its own (fp32) sums
    ws_sum = ws.double().sum(0).float()
    old = {"dW": gw0, "d2": G.linear_dgrad(dxc, w), "sum g": ws_sum[0], "sum g (yc - mean)": ws_sum[1], "dgamma": dg0}

    # folded path
    wsg = torch.zeros((SHARDS, 2, Co), dtype=torch.float32, device=DEV)
    bnr = {"x": yc, "mask": mask, "mean": mean, "ws": wsg, "premask": True}
    g = G.linear_dgrad(dy1, w1, bnr=bnr)
    assert bnr.get("done")
    gw1 = torch.zeros(Co, Ci, dtype=torch.float32, device=DEV)
    dg1, db1 = torch.zeros(Co, device=DEV), torch.zeros(Co, device=DEV)
    d2, sums = FB.fold_conv_bn_backward(w, gw1, g, y2, wsg, mean, invstd, gamma, dg1, db1)
    new = {"dW": gw1, "d2": d2, "sum g": sums[0], "sum g (yc - mean)": sums[1], "dgamma": dg1}

    errs = {k: (_rel(new[k], ref[k]), _rel(old[k], ref[k])) for k in ref}
    print(f"({Ci}, {Co}, {M}) folded / existing: " + "   ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in errs.items()))
    for k, (a, b) in errs.items():
        assert a <= 2.0 * b, f"{k}: folded {a:.3e} vs existing {b:.3e}"
    assert torch.equal(db1, sums[0])  # dbeta is the sum of g


def test_stream_dgrad_mode2_reduce_with_residual():
    """The streaming kernel's RES + BNR = 2 instantiation ([M, 256] x [256, 64] + r, the folded conv3
    data-gradient of the 64-wide stage): output equal to the plain launch, sums of the stored output under the
    recomputed ReLU mask."""
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    M, N, K = 16448, 64, 256
    gen = torch.Generator().manual_seed(5)
    dy = torch.randn(M, K, generator=gen).to(DEV, torch.bfloat16)
    w = (torch.randn(K, N, generator=gen) / K ** 0.5).to(DEV, torch.bfloat16)
    r = torch.randn(M, N, generator=gen).to(DEV, torch.bfloat16)
    x = torch.randn(M, N, generator=gen).to(DEV, torch.bfloat16)
    mean = torch.randn(N, generator=gen).to(DEV)
    scale = (torch.rand(N, generator=gen) + 0.5).to(DEV)
    shift = (torch.randn(N, generator=gen) * 0.5).to(DEV)
    assert G.use_stream(M, N, K, G.KC, G.RC, G.EPI_BF16, K, N, resid=r, ldr=N)
    ws = torch.zeros((SHARDS, 2, N), dtype=torch.float32, device=DEV)
    bnr = {"x": x, "scale": scale, "shift": shift, "mean": mean, "ws": ws}
    out = G.linear_dgrad(dy, w, resid=r, bnr=bnr)
    assert bnr.get("done")
    assert torch.equal(out, G.linear_dgrad(dy, w, resid=r))
    keep = (x.float() * scale + shift > 0).double().cpu()
    d = out.double().cpu() * keep
    s1, s2 = d.sum(0), (d * (x.double().cpu() - mean.double().cpu())).sum(0)
    got = ws.double().cpu().sum(0)
    assert (got[0] - s1).abs().max() <= 1e-4 * d.abs().sum(0).max()
    assert (got[1] - s2).abs().max() <= 1e-4 * (d * (x.double().cpu() - mean.double().cpu())).abs().sum(0).max()


# ------------------------------------------------------------------------------------- model level
class _Side(torch.autograd.Function):
    """Zero in the forward; hands half of its output gradient to ``x`` in the backward: a second consumer of
    ``x``, so autograd sums two gradients for it into a new tensor."""

    @staticmethod
    def forward(ctx, x):
        return torch.zeros_like(x)

    @staticmethod
    def backward(ctx, g):
        return 0.5 * g


def _run(monkeypatch, blocks, fold, x, y, second_consumer=False):
    from torch.profiler import ProfilerActivity, profile

    from distributeddeeplearningspark_amd.models.resnet import ResNet
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    monkeypatch.setattr(FB, "_FOLD_BN3", fold)
    monkeypatch.setattr(FB, "_FOLD_MIN_ELEMS", 0)  # the size gate is a speed rule; these shapes are small
    if second_consumer:
        # the input of the LAST block (the output of the identity block before it) also feeds a side branch: the
        # gradient that reaches that identity block is autograd's sum of the last block's (pre-masked,
        # column-summed) dx and the side gradient
        real, calls, nblk = FB.bottleneck, [0], sum(blocks)

        def tapped(block, xin, anchor):
            calls[0] += 1
            out = real(block, xin, anchor)
            return out + _Side.apply(xin) if calls[0] % nblk == 0 else out

        monkeypatch.setattr(FB, "bottleneck", tapped)
    m = ResNet(blocks=blocks, input_shape=(64, 64, 3), num_classes=10)
    m.compile("sgd", "sparse_categorical_crossentropy")
    m.place(DEV, seed=3)
    with torch.no_grad():  # the zero-initialised last BN scale would make bn3's input gradient vanish
        for blk in m.stages:
            blk.c3.bn.gamma.master.fill_(0.5)
    m.arena.sync_compute()
    xd, yd = m.to_input(x), m.to_target(y)
    m.backward_step(xd, yd)  # warm-up (workspace pool sizing)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss = m.backward_step(xd, yd)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    count = {k: sum(1 for n in names if k in n) for k in ("bn_bwd_dx", "bn_bwd_reduce", "bn_fold_coef")}
    return float(loss.detach()), m.arena.to_canonical(m.arena.grad.detach()).float().cpu().clone(), count


@pytest.mark.parametrize("blocks,folds", [((3,), 1), ((1, 2), 0)])
def test_model_gradients_within_noise_and_launch_counts(monkeypatch, blocks, folds):
    """Flag off / on / off: loss and arena gradients of the folded run within the unfolded runs' own spread;
    one bn_bwd_dx launch fewer per folded block and no added bn_bwd_reduce.  A block folds when it is an
    identity block (every stage's first block has a projection shortcut) followed by another bottleneck: the
    middle block of (3,); none of (1, 2), which must run exactly as with the flag off."""
    from noise import assert_scalar_within_noise, assert_within_noise

    torch.manual_seed(2)
    x = torch.randn(64, 64, 64, 3)
    y = torch.randint(0, 10, (64,))
    (l0, g0, c0), (l1, g1, c1), (l0b, g0b, _) = [_run(monkeypatch, blocks, f, x, y) for f in (False, True, False)]
    assert c0["bn_fold_coef"] == 0 and c1["bn_fold_coef"] == folds, (c0, c1)
    assert c1["bn_bwd_dx"] == c0["bn_bwd_dx"] - folds, (c0, c1)
    assert c1["bn_bwd_reduce"] == c0["bn_bwd_reduce"], (c0, c1)
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    d, spread = assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")
    print(f"{blocks}: folded vs unfolded {d:.3e}, unfolded spread {spread:.3e}")


def test_second_consumer_takes_the_fallback(monkeypatch):
    """The middle (identity) block's output has a second consumer, so the gradient that reaches it is a sum
    autograd formed: the block does not fold, its sweeps run on the sum (whose one term is pre-masked), and the
    result still matches the unfolded run."""
    from noise import assert_scalar_within_noise, assert_within_noise

    torch.manual_seed(2)
    x = torch.randn(64, 64, 64, 3)
    y = torch.randint(0, 10, (64,))
    (l0, g0, c0), (l1, g1, c1), (l0b, g0b, _) = [_run(monkeypatch, (3,), f, x, y, second_consumer=True)
                                                 for f in (False, True, False)]
    assert c1["bn_fold_coef"] == 0 and c1["bn_bwd_dx"] == c0["bn_bwd_dx"], (c0, c1)
    assert c1["bn_bwd_reduce"] == c0["bn_bwd_reduce"], (c0, c1)
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")


def test_resnet50_folded_gradient_per_stage_against_fp32_cpu(monkeypatch):
    """The gradient oracle of tests/test_gpu_determinism.py at its well-conditioned point (gamma3 = 0.1, 64x64,
    batch 16), on the NON-deterministic path with every identity bottleneck that can fold folding: per-stage
    cosine against the fp32 CPU gradient at least the fp32-vs-2^-7-perturbed-input baseline in every stage."""
    from test_gpu_determinism import _resnet50_conditioned, _stage_cosines

    from distributeddeeplearningspark_amd.models import ResNet50
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    m, lc, gc = _resnet50_conditioned("cpu")
    _, _, gp = _resnet50_conditioned("cpu", noise=2.0**-7)
    monkeypatch.setattr(FB, "_FOLD_BN3", True)
    monkeypatch.setattr(FB, "_FOLD_MIN_ELEMS", 0)
    folds = [0]
    real = FB._fold_bn3_backward

    def counted(*a, **k):
        folds[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(FB, "_fold_bn3_backward", counted)
    torch.manual_seed(0)
    x = torch.randn(16, 64, 64, 3)
    y = torch.randint(0, 10, (16,))
    mg = ResNet50(input_shape=(64, 64, 3), num_classes=10)
    mg.compile("sgd", "sparse_categorical_crossentropy")
    mg.place(DEV, seed=3)
    with torch.no_grad():
        for blk in mg.stages:
            blk.c3.bn.gamma.master.fill_(0.1)
    mg.arena.sync_compute()
    lg = float(mg.backward_step(mg.to_input(x), mg.to_target(y)).detach())
    torch.cuda.synchronize()
    gg = mg.arena.to_canonical(mg.arena.grad.detach()).float().cpu().clone()
    assert folds[0] == 11, folds  # identity blocks followed by another bottleneck: 2 + 3 + 5 + 1
    base = _stage_cosines(m, gc, gp)
    cos = _stage_cosines(m, gc, gg)
    print("per-stage cosine, fp32 CPU vs 2^-7 perturbed:", {k: round(v, 4) for k, v in base.items()})
    print("per-stage cosine, folded GPU vs fp32 CPU:", {k: round(v, 4) for k, v in cos.items()})
    assert abs(lg - lc) < 0.02 * max(1.0, abs(lc)), (lg, lc)
    for k in cos:
        assert base[k] >= 0.95, ("the check point is not well conditioned", k, base[k])
        assert cos[k] >= base[k], (k, cos[k], base[k])
