"""Edges of the fused attention kernels (csrc/kernels/attention.hip) against the float64 oracle of
tests/attention_oracle.py: key-padding boundaries on, below and above every 64-key tile and 128-key block edge
(spike fixture: one key too many or too few moves everything by order 1), wholly padded blocks and empty
sequences, padding invariance (bit-exact), grids whose size is no multiple of 8, scale / seed / dropout-rate
parameters, the non-packed layout with strided o / dout, and the saved tensors lse and dvec.

Every case is compared twice with ``attention_ref64``: with the suite's ``close()`` band, and per row,
``row_err(kernel) <= 4 * row_err(attention_rounded)`` — the factor 4 covers fp32 accumulation order and the hardware
exp2, which the rounding model leaves out (derived, not measured).

Measured on an MI355X (per-row error of the kernel / of the rounding model, both against ``attention_ref64``):

    case          o                    dQ                   dK                   dV
    sweep0        2.12e-03 / 2.12e-03  1.43e-01 / 1.43e-01  1.44e-02 / 1.44e-02  4.01e-03 / 4.01e-03
    sweep1        3.68e-03 / 2.12e-03  5.35e-02 / 5.35e-02  1.17e-02 / 1.20e-02  4.06e-03 / 4.06e-03
    sweep2        3.00e-03 / 2.33e-03  4.58e-02 / 4.58e-02  1.86e-02 / 1.03e-02  4.24e-03 / 4.24e-03
    sweep1_drop   3.72e-03 / 2.06e-03  5.73e-02 / 5.73e-02  1.62e-02 / 1.08e-02  4.08e-03 / 4.08e-03
    padded        3.41e-03 / 2.38e-03  8.87e-02 / 8.87e-02  1.23e-02 / 1.80e-02  4.22e-03 / 4.22e-03
    grid1         2.76e-03 / 2.76e-03  3.73e-03 / 3.73e-03  3.42e-03 / 3.41e-03  2.96e-03 / 2.96e-03
    grid3         3.26e-03 / 2.39e-03  4.79e-03 / 4.80e-03  3.90e-03 / 3.58e-03  3.18e-03 / 3.18e-03
    grid10        2.79e-03 / 2.49e-03  4.08e-03 / 4.08e-03  3.75e-03 / 3.52e-03  3.28e-03 / 3.28e-03
    grid9         3.94e-03 / 3.07e-03  3.50e-03 / 3.57e-03  3.42e-03 / 3.57e-03  3.35e-03 / 3.35e-03
    grid27        2.94e-03 / 2.66e-03  3.93e-03 / 3.99e-03  4.33e-03 / 4.51e-03  3.71e-03 / 3.71e-03
    scale0.3      3.93e-03 / 2.42e-03  1.68e-02 / 1.68e-02  1.01e-02 / 1.10e-02  4.22e-03 / 4.22e-03
    seed_hi       3.53e-03 / 2.84e-03  4.25e-03 / 4.20e-03  3.59e-03 / 3.33e-03  3.56e-03 / 3.56e-03
    drop_1_256    3.13e-03 / 2.65e-03  4.32e-03 / 4.32e-03  3.70e-03 / 3.63e-03  3.42e-03 / 3.42e-03
    drop_0.5      3.44e-03 / 2.89e-03  4.05e-03 / 4.05e-03  3.52e-03 / 3.89e-03  3.35e-03 / 3.35e-03
    drop_0.999    4.24e-03 / 4.31e-03  1.12e-02 / 1.59e-02  6.87e-03 / 6.12e-03  4.26e-03 / 4.26e-03
    drop_0.001    3.13e-03 / 2.65e-03  4.32e-03 / 4.32e-03  3.70e-03 / 3.63e-03  3.42e-03 / 3.42e-03
    layout        3.01e-03 / 2.61e-03  4.28e-03 / 3.98e-03  3.89e-03 / 3.92e-03  3.67e-03 / 3.67e-03

    largest kernel / model ratio: 1.80 (bound 4)

Saved tensors: the largest lse error / max(1, |lse|) is 2.28e-07 (padded) and 1.24e-07 (grid27) against the bound
2^-20 = 9.54e-07; the largest dvec error / rowsum|dO * O| is 3.51e-08 (padded) and 4.74e-08 (grid27) against the
bound 64 * 2^-24 = 3.81e-06.

No case failed on first contact with the kernels.  With one comparison of the dK/dV kernel's key-validity test
moved by one key (an experiment, never committed) the boundary sweep's dK is off by a relative l2 of 2.6e+02 to
4.6e+03 and the padding-invariance test sees different bits.
"""
import pytest
import torch

from attention_oracle import (CASES, TENSORS, attention_rounded, case_inputs, case_oracle, clamp_lens, rand_bf16,
                              rel_l2, row_err, shifted, spike_qkv)
from test_gpu_transformer import close

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _C():
    from distributeddeeplearningspark_amd.ops._native import C

    return C()


def _lens_t(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


def run_binding(c, qkv, dout, lens="case"):
    """Forward and backward straight through the bindings on a packed qkv; every output buffer is NaN-filled first,
    so an element that the kernels do not store shows up."""
    B, H, S, HD = c["B"], c["H"], c["S"], c["H"] * 64
    lt = _lens_t(c["lens"] if isinstance(lens, str) else lens)
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    o = torch.full((B * S, HD), NAN, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, S), NAN, device=DEV)
    dvec = torch.full((B, H, S), NAN, device=DEV)
    dqkv = torch.full_like(qkv, NAN)
    _C().attn_fwd(qkv, B, S, H, *c["offs"], o, lse, lt, c["scale"], c["drop_p"], c["seed"])
    _C().attn_bwd(qkv, B, S, H, *c["offs"], o, lse, lt, c["scale"], c["drop_p"], c["seed"], dout, dvec, dqkv)
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "dvec": dvec, "dqkv": dqkv, "dq": dqkv[:, :HD], "dk": dqkv[:, HD : 2 * HD],
            "dv": dqkv[:, 2 * HD :]}


def run_wrapper(c, qkv, dout):
    """Forward and backward through ops.transformer.attention (packed layout: dqkv is allocated without a fill, so
    a NaN-filled block of its size is left in the caching allocator first)."""
    from distributeddeeplearningspark_amd.ops import transformer as T

    B, H, S, HD = c["B"], c["H"], c["S"], c["H"] * 64
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    x = qkv.clone().requires_grad_(True)
    o = T.attention(x, B, S, H, lens=_lens_t(c["lens"]), scale=c["scale"], drop_p=c["drop_p"], seed=c["seed"])
    dirty = torch.full_like(qkv, NAN)
    del dirty
    o.backward(dout)
    torch.cuda.synchronize()
    g = x.grad
    return {"o": o.detach(), "dqkv": g, "dq": g[:, :HD], "dk": g[:, HD : 2 * HD], "dv": g[:, 2 * HD :]}


def check(name, got):
    """The two comparisons of a case with the oracle; the figures are printed before they are asserted."""
    ref, mod = case_oracle(name), case_oracle(name, attention_rounded)
    rows = {}
    for t in TENSORS:
        assert torch.isfinite(got[t].float()).all(), f"{name} {t}: not finite"
        rows[t] = (row_err(got[t], ref[t], t != "o"), row_err(mod[t], ref[t], t != "o"))
        print(f"ATTN_ROW {name:12s} {t:2s} kernel={rows[t][0]:.3e} model={rows[t][1]:.3e}")
    for t in TENSORS:
        close(got[t], ref[t], what=f"{name} {t}")
        assert rows[t][0] <= 4 * rows[t][1], f"{name} {t}: row_err kernel={rows[t][0]:.3e} model={rows[t][1]:.3e}"


def check_saved(name, got, dout):
    """lse against the float64 reference (2^-20 max(1, |lse|): fp32 exp2 / log2 and up to 384-term sums) and dvec
    against the float64 rowsum(dO * O) of the bf16 o the kernel wrote (64 * 2^-24 * rowsum(|dO * O|))."""
    c = CASES[name]
    B, H, S = c["B"], c["H"], c["S"]
    ref = case_oracle(name)
    lse, want = got["lse"].cpu().double(), ref["lse"]
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(lse) & (lse > 0), inf), f"{name}: lse = +inf exactly where no key is valid"
    err = ((lse - want).abs() / want.abs().clamp(min=1.0))[~inf]
    print(f"ATTN_SAVED {name} lse max err / max(1,|lse|) = {err.max().item():.3e} (bound {2.0 ** -20:.3e})")
    prod = (dout.double() * got["o"].cpu().double()).view(B, S, H, 64)
    dd, da = prod.sum(-1).permute(0, 2, 1), prod.abs().sum(-1).permute(0, 2, 1)
    derr = (got["dvec"].cpu().double() - dd).abs()
    ratio = (derr / da.clamp(min=1e-300))[da > 0]
    print(f"ATTN_SAVED {name} dvec max err / rowsum|dO*O| = {ratio.max().item():.3e} (bound {64 * 2.0 ** -24:.3e})")
    assert err.max().item() <= 2.0 ** -20
    assert torch.all(derr <= 64 * 2.0 ** -24 * da)


# ------------------------------------------------------------------------------------------ boundary sweep
@pytest.mark.parametrize("name", ["sweep0", "sweep1", "sweep2", "sweep1_drop"])
def test_boundary_sweep(name):
    """lens 1, 63, 64, 65 / 127, 128, 129, 191 / 192, 193, 255, 256 at S = 256 on the spike fixture: a sequence
    shorter than one tile, len on a tile or block edge (no masked tile), one key either side of it."""
    c, qkv, dout = case_inputs(name)
    got = run_binding(c, qkv, dout)
    check(name, got)
    # the teeth, shown on the kernel's own output: the reference at lens -+ 1 is nowhere near it
    g = torch.cat([got[t].cpu().double() for t in ("dq", "dk", "dv")], 1)
    for d in (-1, 1):
        mv = case_oracle(name, lens=shifted(c["lens"], d))
        assert rel_l2(got["o"], mv["o"]) > 0.45 and rel_l2(g, torch.cat([mv[t] for t in ("dq", "dk", "dv")], 1)) > 0.45


# ------------------------------------------------------------------------- padded blocks, empty sequences
def test_padded_blocks_and_empty_sequence():
    """S = 384, lens [0, 100, 128, 384]: 128-key blocks wholly in the padding (dK/dV: any_key false, nqt = 0) and a
    sequence without a valid key (forward: lse = +inf, inv = 0).  Zeros are asserted exactly."""
    name = "padded"
    c, qkv, dout = case_inputs(name)
    B, S, HD = c["B"], c["S"], c["H"] * 64
    got = run_binding(c, qkv, dout)
    check(name, got)
    check_saved(name, got, dout)
    for b, n in enumerate(clamp_lens(c["lens"], B, S)):
        for t in ("dk", "dv"):
            assert torch.all(got[t].view(B, S, HD)[b, n:] == 0), f"{t} rows at or past len of sequence {b}"
    for t in ("o", "dq", "dk", "dv"):
        assert torch.all(got[t].view(B, S, HD)[0] == 0), f"{t} of the empty sequence"
    assert torch.all(got["lse"][0] == float("inf"))
    assert torch.all(got["dvec"][0] == 0)


def test_lens_clamped_bit_identical():
    """lens [-5, 500] is clamped in the kernels to [0, S]."""
    c = dict(CASES["padded"], B=2, lens=[0, 384])
    qkv = spike_qkv(2, c["S"], c["H"], c["lens"], 15)
    dout = rand_bf16(2 * c["S"], c["H"] * 64, 16)
    a = run_binding(c, qkv, dout)
    b = run_binding(c, qkv, dout, lens=[-5, 500])
    for t in ("o", "lse", "dvec", "dqkv"):
        assert torch.equal(a[t], b[t]), t
    assert torch.isfinite(a["dqkv"].float()).all() and torch.all(a["dqkv"].view(2, c["S"], -1)[0] == 0)


# ---------------------------------------------------------------------------------- padding invariance
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_padding_invariance_bit_exact(drop_p):
    """K / V of the padded rows never reach a result: the forward and dQ kernels read the zero page for them and
    the dK/dV kernel masks P to 0, so other finite values there (up to 50) leave every output bit-identical."""
    B, H, S, lens = 2, 2, 256, [131, 64]
    HD = H * 64
    c = dict(CASES["seed_hi"], B=B, H=H, S=S, lens=lens, drop_p=drop_p, seed=77)
    qkv = rand_bf16(B * S, 3 * HD, 51)
    dout = rand_bf16(B * S, HD, 52)
    other = qkv.clone().view(B, S, 3 * HD)
    g = torch.Generator().manual_seed(53)
    for b, n in enumerate(lens):
        other[b, n:, HD:] = ((torch.rand(S - n, 2 * HD, generator=g) * 2 - 1) * 50).to(torch.bfloat16)
    other = other.view(B * S, 3 * HD)
    assert torch.equal(other[:, :HD], qkv[:, :HD]) and not torch.equal(other, qkv)
    a, b2 = run_binding(c, qkv, dout), run_binding(c, other, dout)
    for t in ("o", "lse", "dvec", "dqkv"):
        assert torch.isfinite(a[t].float()).all(), t
        assert torch.equal(a[t], b2[t]), t


# ------------------------------------------------------------------------------------------- grid sizes
@pytest.mark.parametrize("name", ["grid1", "grid3", "grid10", "grid9", "grid27"])
def test_grid_sizes(name):
    """1, 3, 10, 9 and 27 workgroups per launch through xcd_remap (nwg % 8 != 0), forward and backward, with key
    padding and dropout."""
    c, qkv, dout = case_inputs(name)
    if name == "grid27":
        got = run_binding(c, qkv, dout)
        check_saved(name, got, dout)
    else:
        got = run_wrapper(c, qkv, dout)
    check(name, got)


# ------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("name", ["scale0.3", "seed_hi", "drop_1_256", "drop_0.5", "drop_0.999"])
def test_parameters(name):
    """scale != 0.125 (p.scale multiplies dQ and dK), a dropout seed with bits above 2^32 (row_key mixes in
    seed >> 32), and dropout thresholds 1, 128 and 255."""
    c, qkv, dout = case_inputs(name)
    check(name, run_wrapper(c, qkv, dout))


def test_drop_rate_quantised_to_threshold_one():
    """drop_p = 0.001 quantises to threshold 1 like 1 / 256 (drop_thresh never switches dropout off for p > 0)."""
    from distributeddeeplearningspark_amd.ops import transformer as T

    assert T.drop_thresh(0.001) == 1 == T.drop_thresh(1.0 / 256) and T.drop_thresh(0.999) == 255
    c, qkv, dout = case_inputs("drop_0.001")
    a = run_wrapper(c, qkv, dout)
    check("drop_0.001", a)
    c2, qkv2, dout2 = case_inputs("drop_1_256")
    assert torch.equal(qkv, qkv2) and torch.equal(dout, dout2)
    b = run_wrapper(c2, qkv2, dout2)
    assert torch.equal(a["o"], b["o"]) and torch.equal(a["dqkv"], b["dqkv"])
    # and dropout is on: the result differs from drop_p = 0
    off = run_wrapper(dict(c, drop_p=0.0), qkv, dout)
    assert not torch.equal(a["o"], off["o"])


# ----------------------------------------------------------------------------------------------- layout
def test_layout_offsets_strided_buffers():
    """q / k / v at offsets (512, 0, 256) of a [B*S, 1024] buffer, o as the first 128 columns of a wider buffer, dout
    a column slice of a wider buffer, dqkv zero-filled with NaN in the head columns: the gradients match, every
    column that no head owns stays exactly 0, o's neighbours stay untouched."""
    from distributeddeeplearningspark_amd.ops import transformer as T

    name = "layout"
    c, qkv, dout = case_inputs(name)
    B, H, S, HD = c["B"], c["H"], c["S"], c["H"] * 64
    qo, ko, vo = c["offs"]
    lt = _lens_t(c["lens"])
    qkv = qkv.to(DEV)
    obuf = torch.full((B * S, HD + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    o = obuf[:, :HD]
    dbuf = torch.full((B * S, HD + 128), 5.0, dtype=torch.bfloat16, device=DEV)
    dbuf[:, 64 : 64 + HD] = dout.to(DEV)
    dsl = dbuf[:, 64 : 64 + HD]
    owned = torch.zeros(qkv.shape[1], dtype=torch.bool, device=DEV)
    for off in c["offs"]:
        owned[off : off + HD] = True
    dqkv = torch.zeros_like(qkv)
    dqkv[:, owned] = NAN
    lse = torch.full((B, H, S), NAN, device=DEV)
    dvec = torch.full((B, H, S), NAN, device=DEV)
    _C().attn_fwd(qkv, B, S, H, qo, ko, vo, o, lse, lt, c["scale"], c["drop_p"], c["seed"])
    _C().attn_bwd(qkv, B, S, H, qo, ko, vo, o, lse, lt, c["scale"], c["drop_p"], c["seed"], dsl, dvec, dqkv)
    torch.cuda.synchronize()
    got = {"o": o, "dq": dqkv[:, qo : qo + HD], "dk": dqkv[:, ko : ko + HD], "dv": dqkv[:, vo : vo + HD]}
    check(name, got)
    assert torch.all(dqkv[:, ~owned] == 0), "columns that no head owns"
    assert torch.all(obuf[:, HD:] == 7.0), "o's neighbouring columns"
    assert torch.all(dbuf[:, :64] == 5.0) and torch.all(dbuf[:, 64 + HD :] == 5.0)
    # the wrapper's backward on this layout: zero-filled dqkv, gaps stay zero
    x = qkv.clone().requires_grad_(True)
    ow = T.attention(x, B, S, H, q_off=qo, k_off=ko, v_off=vo, lens=lt, scale=c["scale"], drop_p=c["drop_p"],
                     seed=c["seed"])
    ow.backward(dout.to(DEV))
    assert torch.equal(ow.detach(), o)
    assert torch.equal(x.grad, dqkv)


def test_wrapper_moves_host_lens_to_the_device():
    """ops.transformer.attention takes lens from the host (int64 here) and hands the kernels a device int32 copy:
    the results are bit-identical to those with a device lens.  (The binding refuses a host lens before any launch.)"""
    from distributeddeeplearningspark_amd.ops import transformer as T

    c, qkv, dout = case_inputs("grid10")
    B, H, S = c["B"], c["H"], c["S"]
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    outs = []
    for lens in (torch.tensor(c["lens"]), _lens_t(c["lens"])):
        x = qkv.clone().requires_grad_(True)
        o = T.attention(x, B, S, H, lens=lens, drop_p=c["drop_p"], seed=c["seed"])
        o.backward(dout)
        outs.append((o.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
