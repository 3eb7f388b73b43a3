"""Float64 oracle of the fused attention kernels, shared by test_attention_oracle_cpu.py and
test_gpu_attention_edges.py.

``attention_ref64`` is independent of ``ops.transformer.attention_ref``: per sequence it slices the valid keys
``k[:len]`` / ``v[:len]`` (no ``masked_fill`` / ``nan_to_num``), runs a plain softmax over them and returns the
output, the base-2 log-sum-exp, dQ / dK / dV and ``D = rowsum(dO * O)`` in closed form (no autograd).  Only the
dropout mask is shared (``ops.transformer.attn_keep_ref``: it IS the specification of the hash).

``attention_rounded`` is the same mathematics with the roundings that csrc/kernels/attention.hip declares: bf16
inputs, P rounded to bf16 before P V, the dropped P rounded to bf16 before dV, dS rounded to bf16 before dQ / dK, O
rounded to bf16 with D taken from the rounded O, bf16 outputs.  It only sizes tolerances: a kernel whose per-row
error stays within a small factor of this model's error has no error source beyond its declared roundings.

``spike_qkv`` is the boundary fixture: in every head the last valid key and the first padded key carry about e^8
of each row's softmax mass, with V rows of +3 and -3, so one key too many or too few moves the output and the
gradient by order 1 (asserted in test_attention_oracle_cpu.py)."""
import functools
import math

import torch

LN2 = math.log(2.0)


def clamp_lens(lens, B, S):
    if lens is None:
        return [S] * B
    return [min(max(int(n), 0), S) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]


def rand_bf16(rows, cols, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(torch.bfloat16)


def _bf(x):
    """Round a float64 tensor to bf16 (through fp32: the double rounding is far below a bf16 ulp)."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _attention(qkv, B, S, H, offs, lens, scale, drop_p, seed, dout, rounded):
    from distributeddeeplearningspark_amd.ops.transformer import attn_drop_scale, attn_keep_ref

    x = qkv.detach().cpu().double().view(B, S, -1)
    g = dout.detach().cpu().double().view(B, S, H, 64).permute(0, 2, 1, 3)  # [B, H, S, 64]

    def heads(off):
        return x[..., off : off + H * 64].reshape(B, S, H, 64).permute(0, 2, 1, 3)

    q, k, v = heads(offs[0]), heads(offs[1]), heads(offs[2])
    rnd = _bf if rounded else (lambda t: t)
    dsc = attn_drop_scale(drop_p) if drop_p > 0 else 1.0
    o = torch.zeros(B, H, S, 64, dtype=torch.float64)
    dq, dk, dv = torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(o)
    lse = torch.full((B, H, S), float("inf"), dtype=torch.float64)
    dvec = torch.zeros(B, H, S, dtype=torch.float64)
    for b, n in enumerate(clamp_lens(lens, B, S)):
        if n == 0:
            continue  # no valid key: o = 0, lse = +inf, no gradient
        qb, kb, vb, gb = q[b], k[b, :, :n], v[b, :, :n], g[b]
        s = torch.einsum("hid,hjd->hij", qb, kb) * scale
        m = s.max(dim=-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(dim=-1, keepdim=True)
        p = e / l
        lse[b] = ((m + torch.log(l)) / LN2).squeeze(-1)
        if drop_p > 0:
            row = (torch.arange(b * H, (b + 1) * H).view(H, 1, 1) * S + torch.arange(S).view(1, S, 1))
            keep = attn_keep_ref(seed, row, torch.arange(n).view(1, 1, n), drop_p).double()
        else:
            keep = torch.ones(H, S, n, dtype=torch.float64)
        # forward: the kernel rounds the unnormalised, dropped exponentials and folds 1 / l and the dropout
        # scale into the normalisation of O
        ob = torch.einsum("hij,hjd->hid", rnd(e * keep), vb) * (dsc / l)
        ob = rnd(ob)
        o[b] = ob
        # backward: P from the saved log-sum-exp; D from the (rounded) O
        pd = rnd(p * keep * dsc)
        dv[b, :, :n] = torch.einsum("hij,hid->hjd", pd, gb)
        dp = torch.einsum("hid,hjd->hij", gb, vb) * keep * dsc
        dd = (gb * ob).sum(-1)
        dvec[b] = dd
        ds = rnd(p * (dp - dd[..., None]))
        dq[b] = torch.einsum("hij,hjd->hid", ds, kb) * scale
        dk[b, :, :n] = torch.einsum("hij,hid->hjd", ds, qb) * scale

    def flat(t):
        return rnd(t).permute(0, 2, 1, 3).reshape(B * S, H * 64)

    return {"o": flat(o), "lse": lse, "dq": flat(dq), "dk": flat(dk), "dv": flat(dv), "dvec": dvec}


def attention_ref64(qkv, B, S, H, offs, lens, scale, drop_p, seed, dout):
    """Float64 attention forward and backward.  Returns a dict: ``o``, ``dq``, ``dk``, ``dv`` as [B*S, H*64] (head
    h at columns 64h), ``lse`` (base 2) and ``dvec`` = rowsum(dO * O) as [B, H, S]."""
    return _attention(qkv, B, S, H, offs, lens, scale, drop_p, seed, dout, False)


def attention_rounded(qkv, B, S, H, offs, lens, scale, drop_p, seed, dout):
    """``attention_ref64`` with the kernel's declared bf16 roundings (see the module docstring)."""
    return _attention(qkv, B, S, H, offs, lens, scale, drop_p, seed, dout, True)


# Conditioning of the spike fixture.  dS at the spike key is p (dP - D) with p close to 1 and dP - D = O(1 - p): it
# cancels, and D carries the rounding of the bf16 O (|O| ~ 3: ulp 2^-6), which the kernel declares.  With N(0, 1)
# values the other keys hold 3..7 % of a row's mass and the ROUNDING MODEL ITSELF leaves the close() band on dQ
# (bad fraction 4e-3..7e-3, relative l2 up to 2.4e-2: it all sits in dQ's coordinate 0, which is 2 dS_spike).  The
# fixture therefore draws its random values from N(0, 1.5^2): the other scores get a standard deviation of about
# 2.2, the other keys 10..20 % of the mass (the spike still about e^8), and the model stays at a relative l2 of
# 7e-3 while one key more or less still moves everything by about 1 (test_attention_oracle_cpu.py asserts both).
# The spike cases' dO is N(0, 0.25^2): D's error is absolute, sum |dO| 2^-7, and close() has an absolute term.
SPIKE_SIGMA = 1.5
SPIKE_DOUT_SIGMA = 0.25


def spike_qkv(B, S, H, lens, seed):
    """Packed [B*S, 3*H*64] bf16 boundary fixture (see the module docstring)."""
    HD = H * 64
    x = rand_bf16(B * S, 3 * HD, seed, SPIKE_SIGMA).view(B, S, 3, H, 64).clone()
    x[:, :, 0, :, 0] = 4.0  # Q
    x[:, :, 1, :, 0] = 0.0  # K
    for b, n in enumerate(clamp_lens(lens, B, S)):
        if n >= 1:
            x[b, n - 1, 1, :, 0] = 16.0
            x[b, n - 1, 2] = 3.0
        if n < S:
            x[b, n, 1, :, 0] = 16.0
            x[b, n, 2] = -3.0
    return x.view(B * S, 3 * HD)


def rel_l2(a, r):
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    return ((a - r).norm() / (r.norm() + 1e-300)).item()


def row_err(got, ref, per_head=False):
    """max over rows of ||got_r - ref_r|| / max(||ref_r||, median_r ||ref_r||); with ``per_head`` a row is one
    head's 64 columns of a token.  A row where both are exactly equal counts 0 (also where the reference is 0)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if per_head:
        got, ref = got.reshape(-1, 64), ref.reshape(-1, 64)
    d = (got - ref).norm(dim=1)
    n = ref.norm(dim=1)
    den = torch.maximum(n, n.median())
    e = torch.where(d == 0, torch.zeros_like(d), d / den)
    return e.max().item()


def close_stats(a, b, rtol=2e-2, atol=2e-2):
    """The two figures of the suite's ``close()`` band (tests/test_gpu_transformer.py): the fraction of elements
    outside atol + rtol |b| and the relative l2 error; the band is bad < 2e-3 and rel < 2e-2."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = (a - b).abs()
    return (err > atol + rtol * b.abs()).float().mean().item(), (err.norm() / (b.norm() + 1e-12)).item()


# ---------------------------------------------------------------------------------------------- cases
# Every case the GPU module runs against the oracle: name -> parameters.  ``fix`` is the fixture ("spike" or
# "rand"), ``offs`` / ``ld`` the column layout (None: packed).  test_attention_oracle_cpu.py checks the rounding
# model on all of them and the +-1 separation on every spike case.
def _case(B, H, S, lens, fix="rand", drop_p=0.0, seed=77, scale=0.125, offs=None, ld=None, data_seed=1):
    return dict(B=B, H=H, S=S, lens=lens, fix=fix, drop_p=drop_p, seed=seed, scale=scale,
                offs=offs or (0, H * 64, 2 * H * 64), ld=ld or 3 * H * 64, data_seed=data_seed)


SWEEP_LENS = ([1, 63, 64, 65], [127, 128, 129, 191], [192, 193, 255, 256])
PAD_LENS = [0, 100, 128, 384]

CASES = {
    # boundary sweep: lens on, one below and one above every 64-key tile / 128-key block edge
    "sweep0": _case(4, 2, 256, SWEEP_LENS[0], "spike", data_seed=11),
    "sweep1": _case(4, 2, 256, SWEEP_LENS[1], "spike", data_seed=12),
    "sweep2": _case(4, 2, 256, SWEEP_LENS[2], "spike", data_seed=13),
    "sweep1_drop": _case(4, 2, 256, SWEEP_LENS[1], "spike", drop_p=0.1, data_seed=12),
    # wholly padded 128-key blocks and an empty sequence
    "padded": _case(4, 2, 384, PAD_LENS, "spike", data_seed=14),
    # grid sizes 1, 3, 10, 9 and 27 blocks (xcd_remap with nwg % 8 != 0)
    "grid1": _case(1, 1, 128, [77], drop_p=0.1, data_seed=21),
    "grid3": _case(1, 3, 128, [128], drop_p=0.1, data_seed=22),
    "grid10": _case(1, 5, 256, [200], drop_p=0.1, data_seed=23),
    "grid9": _case(1, 1, 1152, [1000], drop_p=0.1, data_seed=24),
    "grid27": _case(3, 3, 384, [384, 129, 300], drop_p=0.1, data_seed=25),
    # launch parameters
    "scale0.3": _case(2, 2, 256, [256, 131], scale=0.3, data_seed=31),
    "seed_hi": _case(2, 2, 256, [256, 131], drop_p=0.1, seed=(3 << 32) | 9, data_seed=32),
    "drop_1_256": _case(2, 2, 256, [256, 131], drop_p=1.0 / 256, data_seed=33),
    "drop_0.5": _case(2, 2, 256, [256, 131], drop_p=0.5, data_seed=34),
    "drop_0.999": _case(2, 2, 256, [256, 131], drop_p=0.999, data_seed=35),
    "drop_0.001": _case(2, 2, 256, [256, 131], drop_p=0.001, data_seed=33),  # same data as drop_1_256
    # q / k / v at arbitrary offsets of a wider buffer
    "layout": _case(2, 2, 128, [128, 77], drop_p=0.1, offs=(512, 0, 256), ld=1024, data_seed=41),
}
SPIKE_CASES = [n for n, c in CASES.items() if c["fix"] == "spike"]
TENSORS = ("o", "dq", "dk", "dv")


def case_inputs(name):
    """(case, qkv [B*S, ld] bf16, dout [B*S, H*64] bf16) on the CPU."""
    c = CASES[name]
    B, H, S = c["B"], c["H"], c["S"]
    if c["fix"] == "spike":
        qkv = spike_qkv(B, S, H, c["lens"], c["data_seed"])
    else:
        qkv = rand_bf16(B * S, c["ld"], c["data_seed"])
    dout = rand_bf16(B * S, H * 64, c["data_seed"] + 1000, SPIKE_DOUT_SIGMA if c["fix"] == "spike" else 1.0)
    return c, qkv, dout


@functools.lru_cache(maxsize=None)
def _case_oracle(name, rounded, lens):
    c, qkv, dout = case_inputs(name)
    fn = attention_rounded if rounded else attention_ref64
    return fn(qkv, c["B"], c["S"], c["H"], c["offs"], list(lens), c["scale"], c["drop_p"], c["seed"], dout)


def case_oracle(name, fn=None, lens=None):
    """The oracle of a case, computed once and shared (callers must not modify it)."""
    return _case_oracle(name, fn is attention_rounded, tuple(CASES[name]["lens"] if lens is None else lens))


def shifted(lens, d):
    return [n + d for n in lens]
