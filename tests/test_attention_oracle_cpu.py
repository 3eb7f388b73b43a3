"""The attention oracle checked against itself on the CPU (tests/attention_oracle.py):

* ``attention_ref64`` (closed form, valid keys sliced) agrees with ``ops.transformer.attention_ref`` plus autograd
  (``masked_fill`` / ``nan_to_num``) to 1e-6 relative l2: two independent formulations of the same operation;
* on the spike fixture, moving every ``len`` by one key changes the output and the gradient by more than 0.5
  relative l2 — the condition under which the GPU boundary sweep (test_gpu_attention_edges.py) cannot pass with an
  off-by-one in a ``>= len`` / ``< len`` test;
* ``attention_rounded``, the model of the kernel's declared bf16 roundings, stays inside the suite's ``close()``
  band of ``attention_ref64`` on every GPU case: were it outside, the GPU test could not pass either;
* the ``attention`` wrapper takes ``lens`` from any device (CPU fallback path)."""
import pytest
import torch

from attention_oracle import (CASES, SPIKE_CASES, TENSORS, attention_ref64, case_inputs, case_oracle, clamp_lens,
                              close_stats, rand_bf16, rel_l2, row_err, shifted, spike_qkv)


def _ref_autograd(qkv, B, S, H, offs, lens, scale, drop_p, seed, dout):
    from distributeddeeplearningspark_amd.ops import transformer as T

    x = qkv.float().requires_grad_(True)
    lt = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    o = T.attention_ref(x, B, S, H, *offs, lt, scale, drop_p, seed)  # fp32
    o.backward(dout.float())
    return o.detach(), x.grad


@pytest.mark.parametrize("lens,drop_p,seed,offs,ld", [
    (None, 0.0, 0, None, None),
    ([256, 131], 0.0, 0, None, None),
    (None, 0.1, 77, None, None),
    ([200, 256], 0.1, (5 << 32) | 3, None, None),
    ([0, 77], 0.0, 0, None, None),
    ([0, 256], 0.25, 1 << 32, None, None),
    ([256, 65], 0.1, 9, (512, 0, 256), 1024),
])
def test_ref64_matches_attention_ref_autograd(lens, drop_p, seed, offs, ld):
    B, S, H = 2, 256, 2
    HD = H * 64
    offs = offs or (0, HD, 2 * HD)
    qkv = rand_bf16(B * S, ld or 3 * HD, 3)
    dout = rand_bf16(B * S, HD, 4)
    r = attention_ref64(qkv, B, S, H, offs, lens, 0.125, drop_p, seed, dout)
    o, g = _ref_autograd(qkv, B, S, H, offs, lens, 0.125, drop_p, seed, dout)
    assert rel_l2(r["o"], o) < 1e-6
    for name, off in zip(("dq", "dk", "dv"), offs):
        assert rel_l2(r[name], g[:, off : off + HD]) < 1e-6, name
    owned = torch.zeros(qkv.shape[1], dtype=torch.bool)
    for off in offs:
        owned[off : off + HD] = True
    assert torch.all(g[:, ~owned] == 0)
    # lse against a direct logsumexp of the valid scores; D against the definition
    x = qkv.double().view(B, S, -1)
    for b, n in enumerate(clamp_lens(lens, B, S)):
        for h in range(H):
            if n == 0:
                assert torch.all(torch.isinf(r["lse"][b, h])) and torch.all(r["lse"][b, h] > 0)
                assert torch.all(r["o"].view(B, S, HD)[b] == 0)
                continue
            q = x[b, :, offs[0] + 64 * h : offs[0] + 64 * h + 64]
            k = x[b, :n, offs[1] + 64 * h : offs[1] + 64 * h + 64]
            want = torch.logsumexp(q @ k.t() * 0.125, dim=-1) / torch.log(torch.tensor(2.0, dtype=torch.float64))
            assert (r["lse"][b, h] - want).abs().max().item() < 1e-9
    dd = (dout.double() * r["o"]).view(B, S, H, 64).sum(-1).permute(0, 2, 1)
    assert (r["dvec"] - dd).abs().max().item() < 1e-9


@pytest.mark.parametrize("name", SPIKE_CASES)
@pytest.mark.parametrize("d", [-1, 1])
def test_spike_fixture_separates_lens_by_one(name, d):
    """The boundary fixture has teeth: with every len moved by one key (in the reference only) the output and the
    gradient are more than 0.5 relative l2 away — 25 times the close() band of the GPU test."""
    c = CASES[name]
    base = case_oracle(name)
    moved = case_oracle(name, lens=shifted(c["lens"], d))
    assert rel_l2(moved["o"], base["o"]) > 0.5
    gb = torch.cat([base[t] for t in ("dq", "dk", "dv")], 1)
    gm = torch.cat([moved[t] for t in ("dq", "dk", "dv")], 1)
    assert rel_l2(gm, gb) > 0.5
    # and per sequence whose clamped len really moved
    B, S, HD = c["B"], c["S"], c["H"] * 64
    for b, (n0, n1) in enumerate(zip(clamp_lens(c["lens"], B, S), clamp_lens(shifted(c["lens"], d), B, S))):
        if n0 != n1:
            assert rel_l2(moved["o"].view(B, S, HD)[b], base["o"].view(B, S, HD)[b]) > 0.5, (b, n0, n1)
            assert rel_l2(gm.view(B, S, -1)[b], gb.view(B, S, -1)[b]) > 0.5, (b, n0, n1)


def test_spike_fixture_layout():
    B, S, H = 3, 128, 2
    x = spike_qkv(B, S, H, [0, 5, 128], 1).view(B, S, 3, H, 64).float()
    assert torch.all(x[:, :, 0, :, 0] == 4.0)
    k0 = x[:, :, 1, :, 0]
    assert torch.all(k0[0, 0] == 16.0) and torch.all(k0[0, 1:] == 0)
    assert torch.all(k0[1, 4:6] == 16.0) and torch.all(k0[1, :4] == 0) and torch.all(k0[1, 6:] == 0)
    assert torch.all(k0[2, 127] == 16.0) and torch.all(k0[2, :127] == 0)
    assert torch.all(x[0, 0, 2] == -3.0) and torch.all(x[1, 4, 2] == 3.0) and torch.all(x[1, 5, 2] == -3.0)
    assert torch.all(x[2, 127, 2] == 3.0)


@pytest.mark.parametrize("name", list(CASES))
def test_rounding_model_inside_close_band(name):
    from attention_oracle import attention_rounded

    ref = case_oracle(name)
    mod = case_oracle(name, attention_rounded)
    for t in TENSORS:
        bad, rel = close_stats(mod[t], ref[t])
        assert bad < 2e-3 and rel < 2e-2, f"{name} {t}: frac_bad={bad:.2e} rel_l2={rel:.2e}"
        assert row_err(mod[t], ref[t], t != "o") < float("inf"), (name, t)  # the GPU bound is 4 x this figure
    assert torch.equal(mod["lse"], ref["lse"])


def test_row_err():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, 0.0]]).repeat(1, 32)
    got = ref.clone()
    assert row_err(got, ref) == 0.0
    got[0, 0] += 1.0
    assert abs(row_err(got, ref) - 1.0 / ref[0].double().norm().item()) < 1e-12
    got[1, 0] = 1e-3  # a zero reference row with a zero median: any error there is unbounded
    assert row_err(got, ref) == float("inf")


def test_attention_wrapper_accepts_lens_on_any_device():
    """ops.transformer.attention moves lens to qkv's device as int32 (CPU fallback path: an int64 list-built lens and
    a clamped out-of-range lens give what attention_ref64 gives)."""
    from distributeddeeplearningspark_amd.ops import transformer as T

    B, S, H = 2, 128, 1
    qkv = rand_bf16(B * S, 3 * H * 64, 8)
    dout = rand_bf16(B * S, H * 64, 9)
    lens = torch.tensor([100, 500])  # int64, on the CPU
    x = qkv.clone().requires_grad_(True)
    o = T.attention(x, B, S, H, lens=lens)
    o.backward(dout)
    r = attention_ref64(qkv, B, S, H, (0, 64, 128), [100, 500], 0.125, 0.0, 0, dout)
    assert rel_l2(o, r["o"]) < 1e-2
    assert rel_l2(x.grad, torch.cat([r["dq"], r["dk"], r["dv"]], 1)) < 1e-2
    assert lens.dtype == torch.int64  # the caller's tensor is left alone
