"""The forward of a folding identity bottleneck (``ops/fused_blocks.py: _FOLD_BN3_FWD``): bn3 applied in conv3's
epilogue, conv3's output never written.

conv3 is 1x1, so with S = y2^T y2 and s = sum_p y2 (one read of the 4x narrower y2: ``gram_colsum``) bn3's batch
statistics are mean_co = w_co . s / M and var_co = w_co^T (S / M - s_bar s_bar^T) w_co (``bn_fold_fwd_stats``);
``bn_finalize`` runs unchanged and ONE streaming GEMM writes relu(scale * (y2 W^T) + shift + x) and the ReLU bit
mask.  The folded backward takes S and s from the forward.

Inputs are the cancellation case throughout: y2 post-ReLU with clearly positive column means, weights of mixed
sign.  Every error is a relative-norm error against an fp64 evaluation; the yardstick is the existing path on the
same input against the same reference.

Measured on MI355X (new / existing):
  (64, 256, 4096)    S 5.0e-8 / 6.6e-8   s 4.6e-8 / 5.2e-8   mean 5.7e-8 / 4.0e-5   inverse std 1.2e-7 / 5.9e-5   y 1.66e-3 / 2.10e-3
  (64, 256, 4000)    S 5.0e-8 / 6.6e-8   s 4.3e-8 / 4.1e-8   mean 5.3e-8 / 3.5e-5   inverse std 1.2e-7 / 5.4e-5   y 1.66e-3 / 2.11e-3
  (128, 512, 4096)   S 4.8e-8 / 6.6e-8   s 4.9e-8 / 4.7e-8   mean 5.4e-8 / 3.4e-5   inverse std 1.3e-7 / 5.4e-5   y 1.66e-3 / 2.10e-3
  (256, 1024, 2000)  S 9.2e-8 / 8.8e-8   s 3.3e-8 / 4.2e-8   mean 4.7e-8 / 4.4e-5   inverse std 1.4e-7 / 7.6e-5   y 1.66e-3 / 2.12e-3
  (256, 1024, 5000)  S 6.2e-8 / 6.6e-8   s 4.1e-8 / 5.7e-8   (three chunks of rows per panel of S)
Running mean / variance after one call: new path 4.0e-8 ... 4.8e-8 from fp64, existing path 6.5e-6 ... 9.1e-6; the
two paths differ by the existing error x (1 - 6e-4 ... 1 + 8e-4).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(64, 256, 4096), (64, 256, 4000), (128, 512, 4096), (256, 1024, 2000)]
EPS, MOM = 1e-3, 0.1


def _C():
    from distributeddeeplearningspark_amd.ops._native import C

    return C()


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-300))


_CASES = {}


def _case(Ci, Co, M):
    """Inputs and fp64 references of one shape, built once and shared (never modified)."""
    key = (Ci, Co, M)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(Ci + Co + M)
        y2 = torch.relu(torch.randn(M, Ci, generator=gen) + 1.0).to(DEV, torch.bfloat16)
        w = (torch.randn(Co, Ci, generator=gen) / Ci ** 0.5).to(DEV, torch.bfloat16)
        x = torch.randn(M, Co, generator=gen).to(DEV, torch.bfloat16)
        gamma = (torch.rand(Co, generator=gen) + 0.5).to(DEV)
        beta = (torch.randn(Co, generator=gen) * 0.5).to(DEV)
        y64, w64 = y2.double().cpu(), w.double().cpu()
        yc64 = y64 @ w64.t()
        _CASES[key] = dict(y2=y2, w=w, x=x, gamma=gamma, beta=beta, y64=y64, w64=w64, yc64=yc64,
                           S64=y64.t() @ y64, s64=y64.sum(0), mean64=yc64.mean(0), var64=yc64.var(0, unbiased=False))
    return _CASES[key]


def _gram(y2):
    Ci = y2.shape[1]
    S = torch.zeros(Ci, Ci, dtype=torch.float32, device=DEV)
    s = torch.zeros(Ci, dtype=torch.float32, device=DEV)
    _C().gram_colsum(y2, S, s)
    return S, s


# ------------------------------------------------------------------------------------- 1. S and s in one read
# one workgroup takes at least 2048 rows at Ci = 256, so M = 2000 is a single chunk per 64-column panel of S; 5000
# rows make three chunks (the last one ragged) on each of the four panels: the atomics across workgroups
@pytest.mark.parametrize("Ci,Co,M", SHAPES + [(256, 1024, 5000)])
def test_gram_colsum_against_fp64(Ci, Co, M):
    """S = y2^T y2 and s = sum y2 from ONE kernel against fp64; yardstick: the pair the folded backward ran so
    far on the same input (``linear_wgrad(y2, y2, S)``; a ``bn_stats`` sweep summed by ``bn_fold_sums``).  The new
    error may exceed the existing one by at most a quarter (the sums are fp32 atomics: arrival-order noise)."""
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    c = _case(Ci, Co, M)
    y2 = c["y2"]
    C = _C()
    S1, s1 = _gram(y2)
    S0 = torch.zeros(Ci, Ci, dtype=torch.float32, device=DEV)
    G.linear_wgrad(y2, y2, S0)
    wsy = torch.empty((C.bn_partial_rows(M, Ci), 2, Ci), dtype=torch.float32, device=DEV)
    C.bn_stats(y2, wsy, Ci)
    s0 = torch.zeros(Ci, dtype=torch.float32, device=DEV)
    C.bn_fold_sums(c["w"], torch.zeros(Co, Ci, device=DEV), torch.zeros(SHARDS, 2, Co, device=DEV),
                   torch.zeros(Co, device=DEV), wsy, torch.empty(2 * Co, device=DEV), s0)
    eS = (_rel(S1, c["S64"]), _rel(S0, c["S64"]))
    es = (_rel(s1, c["s64"]), _rel(s0, c["s64"]))
    print(f"({Ci}, {Co}, {M}) new / existing: S {eS[0]:.2e} / {eS[1]:.2e}   s {es[0]:.2e} / {es[1]:.2e}")
    assert eS[0] <= 1.25 * eS[1], eS
    assert es[0] <= 1.25 * es[1], es


# ------------------------------------------------------------------------------------- 2. analytic statistics
def _finalize(ws, M, c, Co):
    rm = torch.linspace(-1.0, 1.0, Co, device=DEV)
    rv = torch.linspace(0.5, 2.0, Co, device=DEV)
    scale, shift, mean, invstd = torch.empty(4, Co, dtype=torch.float32, device=DEV).unbind(0)
    _C().bn_finalize(ws, M, Co, c["gamma"], c["beta"], EPS, MOM, rm, rv, mean, invstd, scale, shift)
    return dict(mean=mean, invstd=invstd, scale=scale, shift=shift, rm=rm, rv=rv)


@pytest.mark.parametrize("Ci,Co,M", SHAPES)
def test_analytic_statistics_match_fp64_better_than_the_fused_ones(Ci, Co, M):
    """``bn_fold_fwd_stats`` + ``bn_finalize`` against the fp64 mean / inverse std of y2 W^T; yardstick: the conv
    with fused statistics + ``bn_finalize`` on the same input (it measures the bf16-rounded conv output).  The
    new error is no larger than the existing one, for the saved mean / inverse std and for the running mean /
    variance.  The two paths' running statistics after the call agree within the existing path's own error
    against fp64 plus the new path's (docs/PERFORMANCE.md, "Numerics": the new path sits ~1e-3 of that error from
    the fp64 value, so the distance between the two paths IS the existing error to within that fraction, on either
    side of it; the new path's own error is the only slack the bound has)."""
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    c = _case(Ci, Co, M)
    ws0 = torch.zeros(SHARDS, 2, Co, dtype=torch.float32, device=DEV)
    G.linear_fwd(c["y2"], c["w"], stats=ws0)
    old = _finalize(ws0, M, c, Co)
    S, s = _gram(c["y2"])
    ws1 = torch.zeros(SHARDS, 2, Co, dtype=torch.float32, device=DEV)
    _C().bn_fold_fwd_stats(c["w"], S, s, M, ws1)
    assert torch.count_nonzero(ws1[1:]) == 0  # shard row 0 only
    new = _finalize(ws1, M, c, Co)
    rm0 = torch.linspace(-1.0, 1.0, Co).double()
    rv0 = torch.linspace(0.5, 2.0, Co).double()
    ref = dict(mean=c["mean64"], invstd=1.0 / torch.sqrt(c["var64"] + EPS),
               rm=(1 - MOM) * rm0 + MOM * c["mean64"], rv=(1 - MOM) * rv0 + MOM * c["var64"] * M / (M - 1))
    errs = {k: (_rel(new[k], ref[k]), _rel(old[k], ref[k])) for k in ref}
    print(f"({Ci}, {Co}, {M}) new / existing: " + "   ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in errs.items()))
    for k, (a, b) in errs.items():
        assert a <= b, f"{k}: new {a:.3e} vs existing {b:.3e}"
    for k in ("rm", "rv"):
        d = _rel(new[k], old[k].double().cpu())
        print(f"  {k}: new vs existing {d:.6e}, existing vs fp64 {errs[k][1]:.6e}, new vs fp64 {errs[k][0]:.3e}")
        assert d <= errs[k][1] + errs[k][0], f"{k}: new vs existing {d:.3e}, existing vs fp64 {errs[k][1]:.3e}"


# ------------------------------------------------------------------------------------- 3. conv3 with bn3 in its epilogue
@pytest.mark.parametrize("Ci,Co,M", SHAPES)
def test_fused_gemm_output_and_mask(Ci, Co, M):
    """y = relu(scale * (y2 W^T) + shift + x) from ONE launch against fp64, no worse than the existing pair (conv,
    then ``bn_apply``); its mask bytes are packbits(stored y > 0), bit for bit, and nothing is written behind
    them; with a column scale of ones and no mask output the launch equals the plain RES + ReLU launch."""
    from distributeddeeplearningspark_amd.ops import gemm as G

    c = _case(Ci, Co, M)
    y2, w, x = c["y2"], c["w"], c["x"]
    assert G.stream_colscale_ok(Co, Ci)
    gen = torch.Generator().manual_seed(7)
    scale = (torch.rand(Co, generator=gen) + 0.5).to(DEV)
    shift = (torch.randn(Co, generator=gen) * 0.5).to(DEV)
    nmask, guard = M * Co // 8, 4096
    mbuf = torch.full((nmask + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    y1 = G.linear_fwd(y2, w, bias=shift, relu=True, resid=x, colscale=scale, relu_mask_out=mbuf)
    yc = G.linear_fwd(y2, w)
    y0 = torch.empty_like(yc)
    m0 = torch.empty(-(-M * Co // 32) * 4, dtype=torch.uint8, device=DEV)
    _C().bn_apply(yc, scale, shift, x, y0, Co, True, m0)
    ref = torch.relu(scale.double().cpu() * c["yc64"] + shift.double().cpu() + x.double().cpu())
    e1, e0 = _rel(y1, ref), _rel(y0, ref)
    print(f"({Ci}, {Co}, {M}) new / existing: y {e1:.3e} / {e0:.3e}")
    assert e1 <= e0, (e1, e0)
    want = np.packbits((y1.float() > 0).cpu().numpy().reshape(-1), bitorder="little")
    got = mbuf.cpu().numpy()
    assert want.size == nmask and np.array_equal(got[:nmask], want)
    assert (got[nmask:] == 0xA5).all(), "bytes written past the mask"
    # column scale of ones, no mask: the existing residual + ReLU launch of the streaming kernel, bit for bit
    ones = torch.ones(Co, device=DEV)
    ya = G.linear_fwd(y2, w, relu=True, resid=x, colscale=ones)
    yb = torch.empty_like(ya)
    G.gemm(y2, w, yb, M, Co, Ci, G.KC, G.KC, Ci, Ci, Co, G.EPI_BF16, relu=G.ACT_RELU, resid=x, ldr=Co, tile=G.TILE_STREAM)
    assert torch.equal(ya, yb)


def test_colscale_is_refused_off_the_streaming_shapes():
    from distributeddeeplearningspark_amd.ops import gemm as G

    y2 = torch.zeros(4096, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(128, 64, dtype=torch.bfloat16, device=DEV)  # K = 64 on a 128-wide panel: not instantiated
    x = torch.zeros(4096, 128, dtype=torch.bfloat16, device=DEV)
    assert not G.stream_colscale_ok(128, 64)
    with pytest.raises(ValueError):
        G.linear_fwd(y2, w, relu=True, resid=x, colscale=torch.ones(128, device=DEV))


def test_native_launcher_refuses_colscale_off_the_streaming_kernel():
    """The native entry point itself (not the Python wrapper in front of it) refuses a column scale on the 128x128
    tile, a shape the streaming kernel has no column-scale instantiation for, and a scaled accumulator
    (alpha != 1) next to a column scale; nothing is launched and the output stays as it was."""
    from distributeddeeplearningspark_amd.ops import gemm as G

    M, N, K = 4096, 256, 64
    y2 = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    x = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    out = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=DEV)
    ones = torch.ones(N, device=DEV)

    def launch(n, tile, alpha=1.0):
        _C().gemm(y2, w[:n], out[:, :n], M, n, K, G.KC, G.KC, K, K, N, G.EPI_BF16, tile, K, alpha, 0.0, None, x[:, :n], N,
                  G.ACT_RELU, colscale=ones[:n])

    with pytest.raises(RuntimeError):
        launch(N, 0)  # tile id 0: the 128x128 kernel
    with pytest.raises(RuntimeError):
        launch(128, G.TILE_STREAM)  # K = 64 on a 128-wide panel
    with pytest.raises(RuntimeError):
        launch(N, G.TILE_STREAM, alpha=0.5)
    with pytest.raises(ValueError):
        G.gemm(y2, w, out, M, N, K, G.KC, G.KC, K, K, N, G.EPI_BF16, alpha=0.5, relu=G.ACT_RELU, resid=x, ldr=N,
               colscale=ones)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    launch(N, G.TILE_STREAM)  # the same call on the streaming kernel runs: relu(0 * 1 + 0) = 0
    assert bool((out == 0.0).all())


# ------------------------------------------------------------------------------------- 4. model level
def _counted(monkeypatch, names):
    """Launch counters on the native module's entry points (the imported ``_run`` profiles other kernels)."""
    C = _C()
    n = {k: 0 for k in names}
    for k in names:
        real = getattr(C, k)

        def wrap(*a, _real=real, _k=k, **kw):
            n[_k] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(C, k, wrap)
    return n


def _xy():
    torch.manual_seed(2)
    return torch.randn(64, 64, 64, 3), torch.randint(0, 10, (64,))


def test_model_gradients_within_noise_and_launch_counts(monkeypatch):
    """ResNet (3,) at 64 x 64, batch 64, the backward fold on throughout; forward flag off / on / off: loss and
    arena gradients of the on run within the off runs' own spread.  Blocks 2 and 3 are identity blocks and take
    the new forward: per step two ``bn_apply`` launches fewer and two ``gram_colsum`` launches; block 2's backward
    folds with the forward's S and s (no ``bn_stats`` launch, one with the flag off); block 3 is the network's
    last block, its backward does not fold and recomputes conv3's output."""
    from noise import assert_scalar_within_noise, assert_within_noise
    from test_gpu_bn_fold import _run

    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    x, y = _xy()
    n = _counted(monkeypatch, ("bn_apply", "bn_stats", "gram_colsum", "bn_fold_fwd_stats"))
    rec = [0]
    real = FB._recompute_yc

    def counted(*a, **k):
        rec[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(FB, "_recompute_yc", counted)
    res, counts = [], []
    for flag in (False, True, False):
        monkeypatch.setattr(FB, "_FOLD_BN3_FWD", flag)
        for k in n:
            n[k] = 0
        rec[0] = 0
        res.append(_run(monkeypatch, (3,), True, x, y))
        counts.append(dict(n, recompute=rec[0]))  # two steps each (warm-up + measured)
    (l0, g0, c0), (l1, g1, c1), (l0b, g0b, _) = res
    off, on = counts[0], counts[1]
    assert c0["bn_fold_coef"] == 1 and c1["bn_fold_coef"] == 1, (c0, c1)
    assert on["gram_colsum"] == 2 * 2 and on["bn_fold_fwd_stats"] == 2 * 2 and off["gram_colsum"] == 0, (off, on)
    assert on["bn_apply"] == off["bn_apply"] - 2 * 2, (off, on)
    assert off["bn_stats"] == 2 * 1 and on["bn_stats"] == 0, (off, on)
    assert on["recompute"] == 2 * 1 and off["recompute"] == 0, (off, on)
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    d, spread = assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")
    print(f"forward fold on vs off {d:.3e}, off spread {spread:.3e}")


def test_backward_after_a_pool_reset_forms_its_own_gram(monkeypatch):
    """S and s of the forward live in the per-step statistics pool; a backward that finds the pool's epoch changed
    since its forward (a reset in between: the memory may have been handed out again) must not read them.  The
    epoch is advanced right before block 2's folded backward (the pool's memory itself is left alone: the column
    sums of the incoming gradient live there too): that backward then forms S and s itself, as with the forward
    flag off (its ``bn_stats`` launch is back), and loss and gradients stay within the flag-off runs' spread."""
    from noise import assert_scalar_within_noise, assert_within_noise
    from test_gpu_bn_fold import _run

    from distributeddeeplearningspark_amd.ops import fused_blocks as FB
    from distributeddeeplearningspark_amd.ops import norm as NM

    x, y = _xy()
    n = _counted(monkeypatch, ("bn_stats", "gram_colsum"))
    real = FB._fold_bn3_backward
    seen = []

    def stale(unit, s3, s2, g, ws_g, bnr2):
        key = NM._POOL._key(g.device)
        NM._POOL.epoch[key] = NM._POOL.epoch.get(key, 0) + 1  # a counter of resets: only ever grows
        seen.append(s3.gram is not None and s3.gram[2] != NM.pool_epoch(g.device))
        return real(unit, s3, s2, g, ws_g, bnr2)

    res, counts = [], []
    for flag in (False, True, False):
        monkeypatch.setattr(FB, "_FOLD_BN3_FWD", flag)
        monkeypatch.setattr(FB, "_fold_bn3_backward", stale if flag else real)
        for k in n:
            n[k] = 0
        res.append(_run(monkeypatch, (3,), True, x, y))
        counts.append(dict(n))
    (l0, g0, c0), (l1, g1, c1), (l0b, g0b, _) = res
    assert seen == [True, True], seen  # two steps, one folded backward each, both found a stale epoch
    assert c1["bn_fold_coef"] == 1, c1
    assert counts[1]["gram_colsum"] == 2 * 2 and counts[1]["bn_stats"] == counts[0]["bn_stats"] == 2 * 1, counts
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")


def test_second_consumer_recomputes_and_matches_the_unfolded_run(monkeypatch):
    """The middle block's output has a second consumer: its backward does not fold either, both identity blocks
    recompute conv3's output for the sweeps, and loss and gradients match the unfolded run (``_FOLD_BN3`` off,
    which switches the forward fold off too) within that run's spread."""
    from noise import assert_scalar_within_noise, assert_within_noise
    from test_gpu_bn_fold import _run

    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    x, y = _xy()
    monkeypatch.setattr(FB, "_FOLD_BN3_FWD", True)
    n = _counted(monkeypatch, ("gram_colsum",))
    rec = [0]
    real = FB._recompute_yc

    def counted(*a, **k):
        rec[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(FB, "_recompute_yc", counted)
    out = []
    for fold in (False, True, False):
        n["gram_colsum"], rec[0] = 0, 0
        out.append(_run(monkeypatch, (3,), fold, x, y, second_consumer=True) + (n["gram_colsum"], rec[0]))
    (l0, g0, c0, gr0, r0), (l1, g1, c1, gr1, r1), (l0b, g0b, _, _, _) = out
    assert gr0 == 0 and r0 == 0, "_FOLD_BN3 off must switch the forward fold off"
    assert gr1 == 2 * 2 and r1 == 2 * 2 and c1["bn_fold_coef"] == 0, (gr1, r1, c1)
    assert c1["bn_bwd_dx"] == c0["bn_bwd_dx"] and c1["bn_bwd_reduce"] == c0["bn_bwd_reduce"], (c0, c1)
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")


# ------------------------------------------------------------------------------------- 5. deterministic mode
def test_deterministic_mode_runs_the_old_step_bit_for_bit(monkeypatch):
    """Under the deterministic mode no new kernel is launched and the step is the step without this change, bit
    for bit: the same step with the forward fold flag on and off, loss and gradient arena equal."""
    from distributeddeeplearningspark_amd.models.resnet import ResNet
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB
    from distributeddeeplearningspark_amd.ops.determinism import deterministic

    monkeypatch.setattr(FB, "_FOLD_MIN_ELEMS", 0)
    n = _counted(monkeypatch, ("gram_colsum", "bn_fold_fwd_stats"))
    x, y = _xy()
    out = []
    for flag in (True, False):
        monkeypatch.setattr(FB, "_FOLD_BN3_FWD", flag)
        with deterministic(True):
            m = ResNet(blocks=(3,), input_shape=(64, 64, 3), num_classes=10)
            m.compile("sgd", "sparse_categorical_crossentropy")
            m.place(DEV, seed=3)
            with torch.no_grad():
                for blk in m.stages:
                    blk.c3.bn.gamma.master.fill_(0.5)
            m.arena.sync_compute()
            loss = m.backward_step(m.to_input(x), m.to_target(y))
            torch.cuda.synchronize()
            out.append((loss.detach().float().cpu().clone(), m.arena.to_canonical(m.arena.grad.detach()).float().cpu().clone()))
    assert n["gram_colsum"] == 0 and n["bn_fold_fwd_stats"] == 0, n
    (l1, g1), (l0, g0) = out
    assert torch.equal(l1, l0), (l1, l0)
    assert torch.equal(g1, g0), f"{(g1 != g0).sum().item()} of {g1.numel()} gradient elements differ"
