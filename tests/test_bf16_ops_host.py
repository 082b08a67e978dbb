"""The gates of tests/test_gpu_bf16_ops.py proven on the CPU, both ways (no GPU): the contract's emulation evaluated in fp32 passes
against the float64 one, and every wrong variant the kernels invite FAILS — operands not rounded, truncated instead of rounded to
nearest even, one (channel, tap) dropped, a tap reading the neighbouring utterance's row instead of zero; for the attention one
key dropped, the mask off by one, and the normalised P rounded instead of the un-normalised one (it separates on every case:
5.8 to 11.8 flips against 3 allowed, 99.9 % of pairs against 5 %, so it is asserted like the others).  Run with -s for the figures (profiles/bf16_ops_r09.md records them)."""
import pytest
import torch

from tests import bf16_emu as E

GEMM_SHAPES = [(512, 512, 5), (256, 1024, 9), (1024, 256, 1), (80, 512, 5), (256, 80, 1)]  # (Cin, N, KW): the mel path's own
B, S = 3, 33


def _gemm_case(Cin, N, KW, seed=0):
    g = torch.Generator().manual_seed(seed + Cin + N + KW)
    x = torch.randn(B, S, Cin, generator=g)
    w = torch.randn(N, Cin, KW, generator=g)
    b = torch.randn(N, generator=g)
    return x, w, b


def _variants(x, w, b, KW):
    """name -> the output of a WRONG implementation of the contraction, evaluated in float64 (its only error is the mutation)"""
    wd = E.bf(w).clone()
    wd[:, x.shape[2] // 3, KW // 2] = 0  # one (channel, tap) of every output column
    out = {
        "unrounded": E.conv_rows(x, w, b),
        "truncated": E.conv_rows(E.bf_trunc(x), E.bf_trunc(w), b),
        "one (c, tap) dropped": E.conv_rows(E.bf(x), wd, b),
    }
    if KW > 1:
        out["neighbour's row for zero"] = E.conv_rows(E.bf(x), E.bf(w), b, cross_utterance=True)
    return out


@pytest.mark.parametrize("Cin,N,KW", GEMM_SHAPES)
def test_gemm_gate_passes_fp32_and_rejects_wrong_variants(Cin, N, KW):
    x, w, b = _gemm_case(Cin, N, KW)
    ref, unit = E.gemm_emu(x, w, b), E.gemm_unit(x, w, b)
    good = E.gemm_check(E.gemm_emu(x, w, b, dtype=torch.float32), x, w, b, ref=ref, unit=unit)
    print(f"\ngemm Cin={Cin} N={N} KW={KW}: fp32 CPU {good.worst * E.GEMM_REL:.2e} of unit ({good.worst:.2e} x bound)")
    assert good.ok and good.worst < 0.1, str(good)  # an fp32 sum of K <= 2560 products sits two orders below the bound
    for name, y in _variants(x, w, b, KW).items():
        bad = E.gemm_check(y, x, w, b, ref=ref, unit=unit)
        print(f"  {name}: {bad.worst * E.GEMM_REL:.2e} of unit = {bad.worst:.3g} x bound")
        assert not bad.ok and bad.worst > 10, (name, str(bad))
    for act in ("relu", "tanh"):  # the bound is on the pre-activation sum and holds behind a 1-Lipschitz activation
        got = E.gemm_emu(x, w, b, act=act, dtype=torch.float32)
        assert E.gemm_check(got, x, w, b, act=act, unit=unit).ok


def test_gemm_gate_rejects_single_wrong_rows_and_columns():
    """what a statistical gate lets through: one row of a partial last tile, one column of an N tail, off by a rounding-sized
    amount of bf16 (2^-9 of the value)"""
    x, w, b = _gemm_case(256, 80, 1)
    ref, unit = E.gemm_emu(x, w, b), E.gemm_unit(x, w, b)
    for idx in ((2, S - 1, slice(None)), (slice(None), slice(None), 79), (0, 0, 0)):
        y = ref.clone()
        y[idx] *= 1 + 2.0 ** -9
        assert not E.gemm_check(y, x, w, b, ref=ref, unit=unit).ok, idx


def test_bf_is_ties_to_even_and_trunc_is_not():
    import numpy as np

    def f32(bits):
        return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())

    # 1.0 + half a bf16 ulp (tie, even lower neighbour -> down), 1.0078125 + half (odd lower neighbour -> up), one fp32 ulp either side
    t = f32([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000])
    want = f32([0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000, 0xBF800000, 0xBF820000])
    assert torch.equal(E.bf(t), want)
    assert torch.equal(E.bf(t.double()), want.double())
    assert not torch.equal(E.bf_trunc(t), want)


@pytest.mark.parametrize("Cin,N,KW,d", [(1024, 256, 1, 256), (256, 256, 1, 256), (1024, 512, 1, 512), (512, 512, 1, 512)])
def test_layernorm_gate_passes_fp32_and_rejects_wrong_variants(Cin, N, KW, d):
    """LayerNorm(gemm + x): the fp32 evaluation of the reference stays inside the first-order bound; a dropped channel, unrounded
    operands and a row normalised with its neighbour's statistics do not"""
    g = torch.Generator().manual_seed(Cin + N)
    x = torch.randn(B, S, Cin, generator=g).relu() if Cin != d else torch.randn(B, S, Cin, generator=g)
    w = torch.randn(N, Cin, KW, generator=g) / Cin ** 0.5
    b, resid = torch.randn(N, generator=g) * 0.1, torch.randn(B, S, N, generator=g)
    ln_g, ln_b = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    z32 = E.gemm_emu(x, w, b, dtype=torch.float32) + resid
    good = E.gemm_ln_check(E.layernorm_emu(z32, ln_g, ln_b, dtype=torch.float32), x, w, b, resid, ln_g, ln_b)
    print(f"\nlayernorm Cin={Cin} N={N}: fp32 CPU {good.worst:.3g} x bound")
    assert good.ok and good.worst < 0.5, str(good)
    wd = E.bf(w).clone()
    wd[:, 7, 0] = 0
    z64 = E.gemm_emu(x, w, b) + resid.double()
    shifted = E.layernorm_emu(z64, ln_g, ln_b)
    mean, mean_n = z64.mean(-1, keepdim=True), z64.roll(1, 1).mean(-1, keepdim=True)
    shifted[:, 5] = (shifted - (mean_n - mean) / torch.sqrt(z64.var(-1, unbiased=False, keepdim=True) + E.LN_EPS) * ln_g.double())[:, 5]
    for name, y in (("unrounded", E.layernorm_emu(E.conv_rows(x, w, b) + resid.double(), ln_g, ln_b)),
                    ("one channel dropped", E.layernorm_emu(E.conv_rows(E.bf(x), wd, b) + resid.double(), ln_g, ln_b)),
                    ("neighbour's mean", shifted)):
        bad = E.gemm_ln_check(y, x, w, b, resid, ln_g, ln_b)
        print(f"  {name}: {bad.worst:.3g} x bound")
        assert not bad.ok, (name, str(bad))


ATT_CASES = [(8, 64, 300, [300, 257, 129]), (2, 128, 1010, [1010, 700, 33]), (4, 32, 130, [130, 1])]


def _rescale_case():
    """tests/test_gpu_attention.py's forced late rescale: one key far above the rest at a late tile, and a descending pattern"""
    torch.manual_seed(3)
    Bq, Sq, H, dk = 2, 257, 2, 128
    d = H * dk
    qkv = torch.randn(Bq, Sq, 3 * d) * 0.5
    q, k = qkv[..., :d], qkv[..., d:2 * d]
    k[0, 200, :dk] = 6.0
    q[0, :, :dk] += 1.0
    k[1, 3, dk:] = 8.0
    q[1, :, dk:] = q[1, :, dk:].abs() + 0.5
    return qkv, torch.tensor([257, 230]), H


@pytest.mark.parametrize("H,dk,S_,lens", ATT_CASES)
def test_attention_gate_passes_fp32_and_rejects_wrong_variants(H, dk, S_, lens):
    torch.manual_seed(S_ + dk)
    qkv = torch.randn(len(lens), S_, 3 * H * dk)
    lens_t = torch.tensor(lens)
    ref, unit, flip = E.attention_emu(qkv, lens_t, H)
    good = E.attention_check(E.attention_emu(qkv, lens_t, H, dtype=torch.float32)[0], ref, unit, flip, H)
    print(f"\nattention H={H} dk={dk} S={S_}: fp32 CPU: {good}")
    assert good.ok, str(good)
    wrong = {
        "one key dropped": dict(drop_key=0),
        "mask one key long": dict(mask_shift=1),
        "mask one key short": dict(mask_shift=-1),
        "operands unrounded": dict(round_fn=lambda t: t),
        "operands truncated": dict(round_fn=E.bf_trunc),
    }
    for name, kw in wrong.items():
        bad = E.attention_check(E.attention_emu(qkv, lens_t, H, **kw)[0], ref, unit, flip, H)
        print(f"  {name}: {bad}")
        assert not bad.ok, (name, str(bad))
    # rounding the normalised P instead: a different bf16 contraction, and the gate separates it on every case
    alt = E.attention_check(E.attention_emu(qkv, lens_t, H, normalised_p=True)[0], ref, unit, flip, H)
    print(f"  normalised P rounded: {alt}")
    assert not alt.ok, str(alt)


def test_attention_gate_on_the_forced_rescale_input():
    qkv, lens_t, H = _rescale_case()
    ref, unit, flip = E.attention_emu(qkv, lens_t, H)
    good = E.attention_check(E.attention_emu(qkv, lens_t, H, dtype=torch.float32)[0], ref, unit, flip, H)
    print(f"\nattention forced rescale: fp32 CPU: {good}")
    assert good.ok, str(good)
    bad = E.attention_check(E.attention_emu(qkv, lens_t, H, drop_key=200)[0], ref, unit, flip, H)
    print(f"  the dominant key dropped: {bad}")
    assert not bad.ok


def test_attention_emulation_matches_the_end_to_end_contract_and_zero_length_is_nan():
    """attention_emu in fp32 is the contract tests/test_gpu_bf16.py states (_attention_bf16), to fp32 rounding; a zero-length
    utterance gives NaN, a full one none"""
    import numpy as np

    torch.manual_seed(1)
    H, dk, S_ = 2, 128, 40
    qkv = torch.randn(2, S_, 3 * H * dk)
    lens_t = torch.tensor([0, 40])
    out = E.attention_emu(qkv, lens_t, H, dtype=torch.float32)[0]
    assert torch.isnan(out[0]).all() and torch.isfinite(out[1]).all()
    d = H * dk
    q, k, v = (qkv[1:, :, i * d:(i + 1) * d].reshape(1, S_, H, dk).permute(2, 0, 1, 3).reshape(-1, S_, dk) for i in range(3))
    s = torch.bmm(E.bf(q), E.bf(k).transpose(1, 2)) * np.float32(E.LOG2E / np.sqrt(dk))
    p = torch.exp2(s - torch.ceil(s.max(dim=2, keepdim=True).values))
    want = (torch.bmm(E.bf(p), E.bf(v)) / p.sum(dim=2, keepdim=True)).view(H, 1, S_, dk).permute(1, 2, 0, 3).reshape(1, S_, d)
    assert (out[1:] - want).abs().max() < 1e-6
