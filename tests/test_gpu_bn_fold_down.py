"""A folding projection bottleneck (``ops/fused_blocks.py: _FOLD_DOWN``): conv3 and the shortcut conv are both 1x1 /
stride 1 over the same pixels, so bn3 and the shortcut's BN are both linear in a 4x narrower input (y2 and the block
input x).  Forward: both BNs' statistics from ``gram_colsum`` + ``bn_fold_fwd_stats``, then ONE streaming GEMM with
two A operands and two fp32 accumulator sets,

    y = relu((y2 W3^T) * scale3 + (x Wd^T) * scale_d + shift3 + shift_d),

which writes y and its ReLU bit mask; neither pre-BN tensor is written.  Backward: ``fold_conv_bn_backward`` once per
unit on the same pre-masked gradient.

Every kernel error is a relative-norm error against an fp64 evaluation; the yardstick is the existing path on the
same input against the same reference.  The size gate (``_FOLD_DOWN_MIN_ELEMS``) is a speed rule and is set to 0
here only.

Measured on MI355X (new / existing), N = 256, K1 = K2 = 64:
  M = 4096   y 1.654e-03 / 2.279e-03
  M = 4000   y 1.650e-03 / 2.294e-03
  M = 100    y 1.683e-03 / 2.190e-03
Statistics (M = 4096 / 4000): the new path sits 3e-8 ... 1.2e-7 from fp64 in every quantity; the existing path
3.2e-5 ... 5.5e-5 (mean, inverse std of bn3), 1.4e-3 ... 1.8e-3 (mean of the shortcut's BN, whose mixed-sign input
leaves column means near zero) and 5e-6 ... 7e-6 (running statistics).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, K = 256, 64
EPS, MOM = 1e-3, 0.1


def _C():
    from distributeddeeplearningspark_amd.ops._native import C

    return C()


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-300))


_CASES = {}


def _case(M):
    """Inputs and fp64 references of one row count, built once and shared (never modified): post-ReLU A1 with
    clearly positive column means, mixed-sign A2 and weights, scales of both signs with one exact 0 column each."""
    if M not in _CASES:
        gen = torch.Generator().manual_seed(M)
        a1 = torch.relu(torch.randn(M, K, generator=gen) + 1.0).to(DEV, torch.bfloat16)
        a2 = torch.randn(M, K, generator=gen).to(DEV, torch.bfloat16)
        w1 = (torch.randn(N, K, generator=gen) / K ** 0.5).to(DEV, torch.bfloat16)
        w2 = (torch.randn(N, K, generator=gen) / K ** 0.5).to(DEV, torch.bfloat16)
        sc1 = torch.randn(N, generator=gen)
        sc2 = torch.randn(N, generator=gen)
        sc1[5], sc2[130] = 0.0, 0.0
        sh1 = torch.randn(N, generator=gen) * 0.5
        sh2 = torch.randn(N, generator=gen) * 0.5
        gamma = torch.rand(2, N, generator=gen) + 0.5
        beta = torch.randn(2, N, generator=gen) * 0.5
        c1 = a1.double().cpu() @ w1.double().cpu().t()
        c2 = a2.double().cpu() @ w2.double().cpu().t()
        f = lambda t: t.to(DEV)
        _CASES[M] = dict(a1=a1, a2=a2, w1=w1, w2=w2, sc1=f(sc1), sc2=f(sc2), sh1=f(sh1), sh2=f(sh2), gamma=f(gamma),
                         beta=f(beta), c1=c1, c2=c2,
                         y64=torch.relu(c1 * sc1.double() + c2 * sc2.double() + sh1.double() + sh2.double()))
    return _CASES[M]


# ------------------------------------------------------------------------------------- 1. the two-product GEMM
# 64-row tiles: 4096 rows are full tiles, 4000 leave a ragged last tile, 100 are fewer rows than two tiles
@pytest.mark.parametrize("M", [4096, 4000, 100])
def test_dual_gemm_output_and_mask(M):
    """y from ONE launch against fp64, no worse than the existing path on the same input (conv with fused statistics
    twice, then ``bn_apply`` with ``res_affine``: three bf16 roundings where the new path has one); its mask bytes
    are packbits(stored y > 0), bit for bit; the guard bytes behind y and behind the mask are untouched."""
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    c = _case(M)
    assert G.stream_dual_ok(N, K, K)
    guard = 4096
    ybuf = torch.full((M * N + guard,), 7.0, dtype=torch.bfloat16, device=DEV)
    nmask = M * N // 8
    mbuf = torch.full((nmask + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    y1 = G.linear_dual_fwd(c["a1"], c["w1"], c["sc1"], c["a2"], c["w2"], c["sc2"], shift1=c["sh1"], shift2=c["sh2"],
                           out=ybuf[: M * N].view(M, N), relu_mask_out=mbuf)
    yc3 = G.linear_fwd(c["a1"], c["w1"], stats=torch.zeros(SHARDS, 2, N, device=DEV))
    ysc = G.linear_fwd(c["a2"], c["w2"], stats=torch.zeros(SHARDS, 2, N, device=DEV))
    y0 = torch.empty_like(yc3)
    m0 = torch.empty(-(-M * N // 32) * 4, dtype=torch.uint8, device=DEV)
    _C().bn_apply(yc3, c["sc1"], c["sh1"], ysc, y0, N, True, m0, c["sc2"], c["sh2"])
    e1, e0 = _rel(y1, c["y64"]), _rel(y0, c["y64"])
    print(f"M = {M} new / existing: y {e1:.3e} / {e0:.3e}")
    assert e1 <= e0, (e1, e0)
    want = np.packbits((y1.float() > 0).cpu().numpy().reshape(-1), bitorder="little")
    got = mbuf.cpu().numpy()
    assert want.size == nmask and np.array_equal(got[:nmask], want)
    assert (got[nmask:] == 0xA5).all(), "bytes written past the mask"
    assert bool((ybuf[M * N :] == 7.0).all()), "elements written past y"
    # the exact-zero scale columns carry the other product alone
    only2 = torch.relu(c["c2"][:, 5] * c["sc2"][5].double().cpu() + (c["sh1"][5] + c["sh2"][5]).double().cpu())
    assert _rel(y1[:, 5], only2) <= 2.0 ** -8


def test_native_entry_refuses_everything_but_the_dual_form():
    """The native entry point itself refuses a residual, a statistics pointer, alpha != 1, a K half other than 64,
    a row-contiguous operand and the 128x128 tile next to a second product; nothing is launched and the output
    stays as it was."""
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    M = 4096
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    a1, a2, w1, w2, x = z(M, 128), z(M, 128), z(N, 128), z(N, 128), z(M, N)
    out = torch.full((M, N), 3.0, dtype=torch.bfloat16, device=DEV)
    ones = torch.ones(N, device=DEV)
    ws = torch.zeros(SHARDS, 2, N, device=DEV)

    def launch(k=64, b_mode=G.KC, tile=G.TILE_STREAM, alpha=1.0, resid=None, stats=None):
        ldb = 128 if b_mode == G.KC else N
        b1, b2 = (w1, w2) if b_mode == G.KC else (z(128, N), z(128, N))
        _C().gemm(a1, b1, out, M, N, k, G.KC, b_mode, 128, ldb, N, G.EPI_BF16, tile, k, alpha, 0.0, None, resid,
                  N if resid is not None else 0, G.ACT_RELU, stats=stats, colscale=ones, a2=a2, b2=b2, lda2=128,
                  ldb2=ldb, colscale2=ones)

    for kw in (dict(resid=x), dict(stats=ws), dict(alpha=0.5), dict(k=128), dict(b_mode=G.RC), dict(tile=0)):
        with pytest.raises(RuntimeError):
            launch(**kw)
    with pytest.raises(ValueError):
        G.linear_dual_fwd(a1, w1, ones, a2, w2, ones, out=out)  # K = 128 per product: the wrapper refuses as well
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    launch()  # the same call in the dual form runs: relu(0 * 1 + 0 * 1) = 0
    assert bool((out == 0.0).all())


# ------------------------------------------------------------------------------------- 2. statistics of both BNs
@pytest.mark.parametrize("M", [4096, 4000])
def test_statistics_of_both_bns_against_fp64(M):
    """``gram_colsum`` + ``bn_fold_fwd_stats`` + ``bn_finalize`` for bn3 (post-ReLU input) and the shortcut's BN
    (mixed-sign input) against fp64; yardstick: the conv with fused statistics + ``bn_finalize`` on the same input.
    Mean, inverse std and the running statistics: the new error is no larger than the existing one, and the two
    paths agree within the existing path's own error plus the new path's — all three distances on the scale of the
    fp64 value (with the distance between the paths divided by the existing path's own norm instead, the bound is
    off by that path's relative error: 1.8e-3 for the near-zero means of the shortcut's BN)."""
    from distributeddeeplearningspark_amd.ops import gemm as G
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    c = _case(M)
    rm0, rv0 = torch.linspace(-1.0, 1.0, N), torch.linspace(0.5, 2.0, N)

    def finalize(ws, i):
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        scale, shift, mean, invstd = torch.empty(4, N, dtype=torch.float32, device=DEV).unbind(0)
        _C().bn_finalize(ws, M, N, c["gamma"][i], c["beta"][i], EPS, MOM, rm, rv, mean, invstd, scale, shift)
        return dict(mean=mean, invstd=invstd, rm=rm, rv=rv)

    for i, (a, w, yc64) in enumerate(((c["a1"], c["w1"], c["c1"]), (c["a2"], c["w2"], c["c2"]))):
        ws0 = torch.zeros(SHARDS, 2, N, dtype=torch.float32, device=DEV)
        G.linear_fwd(a, w, stats=ws0)
        old = finalize(ws0, i)
        S = torch.zeros(K, K, dtype=torch.float32, device=DEV)
        s = torch.zeros(K, dtype=torch.float32, device=DEV)
        _C().gram_colsum(a, S, s)
        ws1 = torch.zeros(SHARDS, 2, N, dtype=torch.float32, device=DEV)
        _C().bn_fold_fwd_stats(w, S, s, M, ws1)
        new = finalize(ws1, i)
        mean64, var64 = yc64.mean(0), yc64.var(0, unbiased=False)
        ref = dict(mean=mean64, invstd=1.0 / torch.sqrt(var64 + EPS), rm=(1 - MOM) * rm0.double() + MOM * mean64,
                   rv=(1 - MOM) * rv0.double() + MOM * var64 * M / (M - 1))
        for k in ref:
            e_new, e_old = _rel(new[k], ref[k]), _rel(old[k], ref[k])
            d = float((new[k].double().cpu() - old[k].double().cpu()).norm() / ref[k].norm())
            print(f"M = {M} BN {i} {k}: new {e_new:.3e}  existing {e_old:.3e}  new vs existing {d:.3e}")
            assert e_new <= e_old, (i, k, e_new, e_old)
            assert d <= e_old + e_new, (i, k, d, e_old, e_new)


# ------------------------------------------------------------------------------------- 2b. the shortcut's input gradient
def test_shortcut_input_gradient_has_vanishing_column_sums():
    """A BN's dx has zero column sums, so d x = dx W has them too.  The folded d x = g WA + x Gm + kv reads bf16 WA
    and Gm; with kv from the unrounded coefficients their rounding leaves sum_p d x off by (sum g) dWA + s dGm, which
    grows with M where the sum of the M output roundings grows with sqrt(M).  Behind conv3 a BN takes the offset out;
    the shortcut's d x is the block-input gradient itself (it reached the stem BN's beta gradient), so there kv is
    formed from the rounded matrices (``exact_colsum``).  Bound from the number formats: the stored d x and the
    residual operand r = x Gm + kv are each one bf16 rounding, relative error at most 2^-9, independent and
    zero-mean with variance at most u^2 / 3 each; six standard deviations of their sum per column (64 columns).
    Measured on MI355X, largest |column sum| over that bound: 0.61 with ``exact_colsum``, 17.2 without."""
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB
    from distributeddeeplearningspark_amd.ops.norm import SHARDS

    M, Ci, Co = 16384, 64, 256
    gen = torch.Generator().manual_seed(11)
    x = torch.relu(torch.randn(M, Ci, generator=gen) + 1.0).to(DEV, torch.bfloat16)
    w = (torch.randn(Co, Ci, generator=gen) / Ci ** 0.5).to(DEV, torch.bfloat16)
    g = ((torch.randn(M, Co, generator=gen) + 0.3) * (torch.rand(M, Co, generator=gen) < 0.6)).to(DEV, torch.bfloat16)
    gamma = (torch.rand(Co, generator=gen) + 0.5).to(DEV)
    x64, w64, g64 = x.double().cpu(), w.double().cpu(), g.double().cpu()
    yc = x64 @ w64.t()
    mean, invstd = yc.mean(0), 1.0 / torch.sqrt(yc.var(0, unbiased=False) + EPS)
    xhat = (yc - mean) * invstd
    t = gamma.double().cpu() * invstd * (-g64.mean(0) - xhat * (g64 * xhat).mean(0))  # dx without its A g term
    r64 = t @ w64
    ws_g = torch.zeros(SHARDS, 2, Co, dtype=torch.float32, device=DEV)
    ws_g[0, 0] = g64.sum(0).float().to(DEV)
    worst = {}
    for exact in (True, False):
        gw, dgamma, dbeta = torch.zeros(Co, Ci, device=DEV), torch.zeros(Co, device=DEV), torch.zeros(Co, device=DEV)
        d, _ = FB.fold_conv_bn_backward(w, gw, g, x, ws_g, mean.float().to(DEV), invstd.float().to(DEV), gamma, dgamma,
                                        dbeta, exact_colsum=exact)
        d64 = d.double().cpu()
        bound = 6.0 * 2.0 ** -9 / 3.0 ** 0.5 * torch.sqrt((d64 ** 2 + r64 ** 2).sum(0))
        worst[exact] = float((d64.sum(0).abs() / bound).max())
    print(f"largest |column sum| / bound: exact_colsum {worst[True]:.3f}, without {worst[False]:.3f}")
    assert worst[True] <= 1.0, worst


# ------------------------------------------------------------------------------------- 3. block and model level
def _xy():
    torch.manual_seed(2)
    return torch.randn(64, 64, 64, 3), torch.randint(0, 10, (64,))


def _hooked(monkeypatch, record):
    """Every public entry point of the native module reports its name to ``record`` when called."""
    C = _C()
    for k in dir(C):
        real = getattr(C, k)
        if k.startswith("_") or not callable(real) or isinstance(real, type):
            continue

        def wrap(*a, _real=real, _k=k, **kw):
            record(_k)
            return _real(*a, **kw)

        monkeypatch.setattr(C, k, wrap)


def _count_recompute(monkeypatch):
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    rec, real = [0], FB._recompute_yc

    def counted(*a, **k):
        rec[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(FB, "_recompute_yc", counted)
    return rec


def test_model_gradients_within_noise_and_launch_counts(monkeypatch):
    """ResNet (2,) at 64 x 64, batch 64; ``_FOLD_DOWN`` off / on / off: loss and arena gradients of the on run within
    the off runs' own spread.  Block 1 is the projection block (64 -> 256, stride 1) and takes the new path; block 2
    (identity, the network's last block) runs as before: its forward folds, its backward recomputes.  Per step one
    ``bn_apply`` fewer, two ``gram_colsum`` and two ``bn_fold_coef`` more, both ``bn_bwd_dx*`` sweeps of the block gone
    and no added recompute."""
    from noise import assert_scalar_within_noise, assert_within_noise
    from test_gpu_bn_fold import _run

    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    x, y = _xy()
    monkeypatch.setattr(FB, "_FOLD_DOWN_MIN_ELEMS", 0)
    n = {}
    _hooked(monkeypatch, lambda k: n.__setitem__(k, n.get(k, 0) + 1))
    rec = _count_recompute(monkeypatch)
    res, counts = [], []
    for flag in (False, True, False):
        monkeypatch.setattr(FB, "_FOLD_DOWN", flag)
        n.clear()
        rec[0] = 0
        res.append(_run(monkeypatch, (2,), True, x, y))
        counts.append(dict(n, recompute=rec[0]))  # two steps each (warm-up + measured)
    (l0, g0, c0), (l1, g1, c1), (l0b, g0b, _) = res
    off, on = counts[0], counts[1]
    assert on["bn_apply"] == off["bn_apply"] - 2 * 1, (off, on)
    assert on["gram_colsum"] == off["gram_colsum"] + 2 * 2, (off, on)
    assert on["bn_fold_fwd_stats"] == off["bn_fold_fwd_stats"] + 2 * 2, (off, on)
    assert on.get("bn_bwd_dx_red", 0) == off["bn_bwd_dx_red"] - 2 * 1, (off, on)
    assert on["recompute"] == off["recompute"], (off, on)
    assert c1["bn_fold_coef"] == c0["bn_fold_coef"] + 2, (c0, c1)  # kernels of the measured step
    assert c1["bn_bwd_dx"] == c0["bn_bwd_dx"] - 2, (c0, c1)
    assert c1["bn_bwd_reduce"] == c0["bn_bwd_reduce"], (c0, c1)
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    d, spread = assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")
    print(f"projection fold on vs off {d:.3e}, off spread {spread:.3e}")


def test_second_consumer_recomputes_both_and_matches_the_unfolded_run(monkeypatch):
    """The projection block's output has a second consumer: its backward does not fold, recomputes conv3's AND the
    shortcut conv's output (two more recomputes per step than the run without a folding projection block), runs the
    existing sweeps, and loss and gradients match the unfolded run (``_FOLD_BN3`` off) within that run's spread."""
    from noise import assert_scalar_within_noise, assert_within_noise
    from test_gpu_bn_fold import _run

    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    x, y = _xy()
    monkeypatch.setattr(FB, "_FOLD_DOWN_MIN_ELEMS", 0)
    rec = _count_recompute(monkeypatch)
    out = []
    for fold in (False, True, False):
        rec[0] = 0
        out.append(_run(monkeypatch, (2,), fold, x, y, second_consumer=True) + (rec[0],))
    monkeypatch.setattr(FB, "_FOLD_DOWN", False)
    rec[0] = 0
    _run(monkeypatch, (2,), True, x, y, second_consumer=True)
    base = rec[0]
    (l0, g0, c0, r0), (l1, g1, c1, r1), (l0b, g0b, _, _) = out
    assert r0 == 0 and r1 == base + 2 * 2, (r0, r1, base)
    assert c1["bn_fold_coef"] == 0 and c1["bn_bwd_dx"] == c0["bn_bwd_dx"], (c0, c1)
    assert c1["bn_bwd_reduce"] == c0["bn_bwd_reduce"], (c0, c1)
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")


def test_backward_after_a_pool_reset_forms_its_own_gram(monkeypatch):
    """The pool's epoch is advanced right before the projection block's folded backward (its memory is left alone:
    the gradient's column sums live there too): both units then form S and s themselves (one ``bn_stats`` sweep over
    the narrow input each), and loss and gradients stay within the flag-off runs' spread."""
    from noise import assert_scalar_within_noise, assert_within_noise
    from test_gpu_bn_fold import _run

    from distributeddeeplearningspark_amd.ops import fused_blocks as FB
    from distributeddeeplearningspark_amd.ops import norm as NM

    x, y = _xy()
    monkeypatch.setattr(FB, "_FOLD_DOWN_MIN_ELEMS", 0)
    n = {}
    _hooked(monkeypatch, lambda k: n.__setitem__(k, n.get(k, 0) + 1))
    real = FB._fold_unit_backward
    seen = []

    def stale(unit, st, xin, g, ws_g, bnr2, **kw):
        key = NM._POOL._key(g.device)
        NM._POOL.epoch[key] = NM._POOL.epoch.get(key, 0) + 1  # a counter of resets: only ever grows
        seen.append(st.gram is not None and st.gram[2] != NM.pool_epoch(g.device))
        return real(unit, st, xin, g, ws_g, bnr2, **kw)

    res, counts = [], []
    for flag in (False, True, False):
        monkeypatch.setattr(FB, "_FOLD_DOWN", flag)
        monkeypatch.setattr(FB, "_fold_unit_backward", stale if flag else real)
        n.clear()
        res.append(_run(monkeypatch, (2,), True, x, y))
        counts.append(dict(n))
    (l0, g0, c0), (l1, g1, c1), (l0b, g0b, _) = res
    assert seen == [True] * 4, seen  # two steps, two units each, all found a stale epoch
    assert c1["bn_fold_coef"] == c0["bn_fold_coef"] + 2, (c0, c1)
    assert counts[1].get("bn_stats", 0) == counts[0].get("bn_stats", 0) + 2 * 2, counts
    assert_scalar_within_noise(l1, l0, l0b, floor=1e-3)
    assert_within_noise(g1, g0, g0b, floor=2e-3, what="arena gradients")


def _step(det=False):
    from distributeddeeplearningspark_amd.models.resnet import ResNet
    from distributeddeeplearningspark_amd.ops.determinism import deterministic

    x, y = _xy()
    with deterministic(det):
        m = ResNet(blocks=(2,), input_shape=(64, 64, 3), num_classes=10)
        m.compile("sgd", "sparse_categorical_crossentropy")
        m.place(DEV, seed=3)
        with torch.no_grad():
            for blk in m.stages:
                blk.c3.bn.gamma.master.fill_(0.5)
        m.arena.sync_compute()
        loss = m.backward_step(m.to_input(x), m.to_target(y))
        torch.cuda.synchronize()
        return loss.detach().float().cpu().clone(), m.arena.to_canonical(m.arena.grad.detach()).float().cpu().clone()


def test_deterministic_mode_runs_the_old_step_bit_for_bit(monkeypatch):
    """Under the deterministic mode no projection block folds: the step with the flag on equals the step with the
    flag off, loss and gradient arena bit for bit, and no Gram kernel is launched."""
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    monkeypatch.setattr(FB, "_FOLD_MIN_ELEMS", 0)
    monkeypatch.setattr(FB, "_FOLD_DOWN_MIN_ELEMS", 0)
    n = {}
    _hooked(monkeypatch, lambda k: n.__setitem__(k, n.get(k, 0) + 1))
    out = []
    for flag in (True, False):
        monkeypatch.setattr(FB, "_FOLD_DOWN", flag)
        out.append(_step(det=True))
    assert n.get("gram_colsum", 0) == 0 and n.get("bn_fold_fwd_stats", 0) == 0, n
    (l1, g1), (l0, g0) = out
    assert torch.equal(l1, l0), (l1, l0)
    assert torch.equal(g1, g0), f"{(g1 != g0).sum().item()} of {g1.numel()} gradient elements differ"


def test_flag_off_gives_the_old_launch_sequence(monkeypatch):
    """``_FOLD_DOWN = False`` with the size gate open runs exactly the native calls, in order, of the step in which
    the gate keeps the block out (the configuration every earlier test pins), and the block's existing sweeps are in
    it; with the flag on the sequence differs."""
    from distributeddeeplearningspark_amd.ops import fused_blocks as FB

    monkeypatch.setattr(FB, "_FOLD_MIN_ELEMS", 0)
    seq = []
    _hooked(monkeypatch, seq.append)
    runs = []
    for flag, gate in ((False, 0), (True, 1 << 62), (True, 0)):
        monkeypatch.setattr(FB, "_FOLD_DOWN", flag)
        monkeypatch.setattr(FB, "_FOLD_DOWN_MIN_ELEMS", gate)
        del seq[:]
        _step()
        runs.append(list(seq))
    assert runs[0] == runs[1]
    assert "bn_bwd_dx_red" in runs[0] and "bn_bwd_dx_red" not in runs[2] and runs[2].count("gram_colsum") == 3
