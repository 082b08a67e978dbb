"""The gate of tests/test_gpu_bf16x3_ops.py proven on the CPU, both ways, and its case tables checked against the dispatch itself
through ns_plan_gemm_b3 (no GPU).  The yardstick is tests/bf16x3_emu.py.

Measured here (run with -s), reduced shapes (3 x 13 rows, 48 columns) at the real contraction lengths K = 256 ... 2560, same-sign
operands: the six-term sum 0.006 ... 0.02 of the gate; a lost lo*hi, hi*lo or mid*mid 1.2 ... 2.6 x the gate at EVERY element, a lost
mid*hi / hi*mid / hi*hi 500 x or more; the weight's mid and lo planes exchanged is a lost mid*mid (it trades that term for mid*lo),
1.5 ... 2.6 x.  Random-sign operands: the same three small-term losses and the exchanged planes stay below 0.5 of the gate — a test on
random data alone cannot see them, which is why the same-sign variants exist.  The fp32 running sum in the kernel's own order
(kernel_order_fp32) stays below the gate at every K (worst 0.77 at K = 2560, 0.5 at K = 2304)."""
import numpy as np
import pytest
import torch

from tests import bf16x3_emu as X
from tests import bf16_emu as E

REL = E.FP32_REL


# ---------------------------------------------------------------------------------------------------- the split
def _f32(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_split3_is_exact_and_every_piece_is_a_bf16():
    """hi + mid + lo == x bit for bit and every piece has zero low 16 bits: random fp32, +-0, powers of two and their nextafter
    neighbours, the largest finite value, the smallest normal (Inf / NaN are out of scope: Inf - Inf)"""
    rs = np.random.RandomState(0)
    rnd = torch.from_numpy(np.concatenate([rs.standard_normal(4096).astype(np.float32) * s for s in (1.0, 1e-3, 1e4, 2.0 ** -60, 2.0 ** 60)]))
    p2 = torch.tensor([2.0 ** e for e in range(-100, 101, 4)], dtype=torch.float32)
    edge = torch.cat([p2, -p2, torch.nextafter(p2, torch.tensor(float("inf"))), torch.nextafter(p2, torch.tensor(0.0)),
                      _f32([0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000, 0x3F7FFFFF, 0x3F80FFFF, 0x3F800001, 0x3FFFFFFF])])
    for x in (rnd, edge):
        hi, mid, lo = X.split3(x)
        for p in (hi, mid, lo):
            assert bool(((_bits(p) & 0xFFFF) == 0).all())
        assert torch.equal(_bits((hi + mid) + lo), _bits(x)) and torch.equal(_bits(hi + (mid + lo)), _bits(x))
        assert torch.equal((hi.double() + mid.double() + lo.double()).float(), x)
        assert bool((hi.abs() <= x.abs()).all()) and bool(((hi == 0) | (torch.sign(hi) == torch.sign(x))).all())
        for p in (mid, lo):  # truncation: every piece carries its operand's sign
            assert bool(((p == 0) | (torch.sign(p) == torch.sign(x))).all())
    # zeros: hi is the operand itself (sign bit included), the rest +0 (the float sum of -0 and +0 is +0: the one value whose
    # BITS the identity does not return, and the contraction cannot tell)
    z = torch.tensor([0.0, -0.0])
    hi, mid, lo = X.split3(z)
    assert torch.equal(_bits(hi), _bits(z)) and bool((_bits(mid) == 0).all()) and bool((_bits(lo) == 0).all())
    # the split is the three-bf16 reading of the mantissa where the residues do not renormalise: 1 + 2^-8 + 2^-16
    hi, mid, lo = X.split3(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -16]))
    assert (float(hi), float(mid), float(lo)) == (1.0, 2.0 ** -8, 2.0 ** -16)


def test_six_term_is_the_product_less_the_three_dropped_terms():
    x, w, b = X.host_case(256, 9, False)
    xp, wp = X._pieces(x), X._pieces(w)
    dropped = sum(E.conv_rows(xp[a], wp[c], None) for a, c in X.DROPPED)
    assert float((X.six_term(x, w, b) + dropped - E.conv_rows(x, w, b)).abs().max()) <= 1e-13 * float(E.gemm_unit(x, w, b, round_fn=E.exact).max())
    assert set(X.TERMS) | set(X.DROPPED) == {(a, c) for a in X.PIECES for c in X.PIECES} and len(X.TERMS) == 6


# ---------------------------------------------------------------------------------------------------- the gate, both ways
def _shares(y, ref, unit):
    """|y - f64| / (REL * unit) per element"""
    return (y.double() - ref).abs() / (REL * unit)


@pytest.mark.parametrize("Cin,KW", X.HOST_SHAPES)
def test_gate_passes_six_terms_and_rejects_every_mutant_on_same_sign_operands(Cin, KW):
    x, w, b = X.host_case(Cin, KW, True)
    ref, unit = E.conv_rows(x, w, b), E.gemm_unit(x, w, b, round_fn=E.exact)
    good = E.gemm_check(X.six_term(x, w, b), x, w, b, rel=REL, ref=ref, unit=unit)
    k32 = E.gemm_check(X.kernel_order_fp32(x, w, b), x, w, b, rel=REL, ref=ref, unit=unit)
    print(f"\nsame sign Cin={Cin} KW={KW}: six terms {good.worst:.3g} x gate, fp32 running sum in the kernel's order {k32.worst:.3g} x")
    assert good.ok and good.worst < 0.05, str(good)
    assert k32.ok, str(k32)  # "fp32-sized error" holds for a running fp32 sum at this K
    for name, f in X.mutants(KW).items():
        s = _shares(f(x, w, b), ref, unit)
        print(f"  {name}: {float(s.min()):.3g} ... {float(s.max()):.3g} x gate")
        assert float(s.max()) > 1.0, name
        if "dropped" in name:
            assert float(s.min()) > 1.0, (name, float(s.min()))  # a lost term shifts EVERY element past the gate


@pytest.mark.parametrize("Cin,KW", X.HOST_SHAPES)
def test_random_sign_operands_cannot_see_the_small_terms(Cin, KW):
    """the fact the same-sign variants exist for: on random-sign data a lost lo*hi, hi*lo or mid*mid is a random walk over K — at the
    long contractions (K >= 1024) inside the gate at every element, at K = 256 / 512 at all but a stray one (under 1 % of them;
    measured: one of 1872 at 1.3 x the gate, K = 256, mid*mid), the typical element at a fifth of the gate or less.  The large terms
    fail everywhere.  The exchanged planes are a lost mid*mid (they trade it for mid*lo), as invisible."""
    x, w, b = X.host_case(Cin, KW, False)
    ref, unit = E.conv_rows(x, w, b), E.gemm_unit(x, w, b, round_fn=E.exact)
    assert E.gemm_check(X.six_term(x, w, b), x, w, b, rel=REL, ref=ref, unit=unit).ok
    blind = {f"x_{a} * w_{c} dropped": X.six_term(x, w, b, drop=(a, c)) for a, c in X.SMALL_TERMS}
    blind["w mid and lo planes exchanged"] = X.six_term(x, w, b, swap_w_mid_lo=True)
    for name, y in blind.items():
        s = _shares(y, ref, unit)
        print(f"random sign Cin={Cin} KW={KW}: {name}: median {float(s.median()):.3g}, worst {float(s.max()):.3g} x gate, {int((s > 1).sum())} of {s.numel()} outside")
        assert float(s.median()) < 0.25 and float((s > 1).double().mean()) < 0.01, name
        assert KW * Cin < 1024 or float(s.max()) < 1.0, name
    for a, c in X.TERMS[3:]:
        assert float(_shares(X.six_term(x, w, b, drop=(a, c)), ref, unit).median()) > 10, (a, c)


def test_signed_mean_yardstick():
    """mean((y - f64) / unit) on the same-sign shapes: the six-term sum's is the three dropped products' (about -2^-24), every lost
    term's at least MIN_MUTANT_BIAS = min_mutant_bias() — computed here, and what a same-sign GPU case is held to a half of"""
    floor = X.min_mutant_bias()
    for Cin, KW in X.SAME_SIGN_SHAPES:
        good, bad = X.mutant_biases(Cin, KW)
        print(f"\nsame sign Cin={Cin} KW={KW}: six terms {good:.3g}, lost terms " + ", ".join(f"{v:.3g}" for v in bad.values()))
        assert -2.0 ** -22 < good <= 0.0          # only ever short, by the dropped products
        assert all(v < 0 for v in bad.values())   # a lost term of same-sign data is a shortfall
        assert abs(good) < floor / 20             # ... and the contract itself uses a twentieth of the GPU's allowance at most
    assert len({len(X.mutant_biases(*s)[1]) for s in X.SAME_SIGN_SHAPES}) == 1 and len(X.mutant_biases(256, 9)[1]) == 6
    assert REL < floor < 4 * REL, floor  # a lost small term is one to a few gates, as the elementwise test found
    assert {X.shape_of(n, c)[::2] for _, n, c, *_, same in X.PLAIN_CASES if same} == set(X.SAME_SIGN_SHAPES)


def test_fp32_torch_evaluation_is_inside_the_gate_on_same_sign_operands():
    """the reported (not gated) CPU figure of the GPU cases: torch's fp32 evaluation of the unsplit operands"""
    for Cin, KW in X.HOST_SHAPES:
        x, w, b = X.host_case(Cin, KW, True)
        assert E.gemm_check(E.gemm_emu(x, w, b, dtype=torch.float32, round_fn=E.exact), x, w, b, rel=REL, round_fn=E.exact).ok


# ---------------------------------------------------------------------------------------------------- the case tables
def _plan(M, shape, epi=0):
    from smart_nar_fast_tts_amd import ops

    Cin, N, KW = shape
    return ops.plan_gemm_b3(M, N, Cin, KW, epi)


@pytest.mark.parametrize("case,name,config,B,S,BM,tiles,same", X.PLAIN_CASES, ids=lambda v: v if isinstance(v, str) and len(v) == 2 else None)
def test_plain_cases_take_their_forms(case, name, config, B, S, BM, tiles, same):
    shape = X.shape_of(name, config)
    M, N = B * S, shape[1]
    assert _plan(M, shape) == (BM, 256, 0, tiles[0] * tiles[1]), "a threshold of the dispatch moved: pick a size that takes this form again"
    assert tiles == ((M + BM - 1) // BM, (N + 255) // 256) and M % BM != 0, "the last row tile must be partial"
    below = (tiles[0] - 1) * BM  # one row tile fewer
    if BM == 128:
        assert _plan(below, shape) is None, "not the fewest row tiles conv_gemm_b3_ok admits"
    else:
        assert _plan(below, shape)[0] == 128, "not the fewest row tiles the 256-row launch admits"
    assert (N % 256 != 0) == (case == "P4")
    utts = X.judged_utterances(B, S, BM)
    assert {0, B - 1, B // 2, BM // S, (tiles[0] - 1) * BM // S} == set(utts) and len(utts) >= 3 and B >= 3 and S >= 12
    assert same == (case != "P3")


def test_the_column_edge_is_reached():
    """ns_create takes conv_filter_size 1056 (any multiple of 32), so P4's fifth column tile is 32 wide: the weight-row guard and the
    store guard of the plain kernel run"""
    (p4,) = [c for c in X.PLAIN_CASES if c[0] == "P4"]
    Cin, N, KW = X.shape_of(p4[1], p4[2])
    assert (N, N % 32, N % 256, (N + 255) // 256) == (1056, 0, 32, 5)


@pytest.mark.parametrize("case,op,config,B,S,form", X.LN_CASES, ids=lambda v: v if isinstance(v, str) and len(v) == 2 else None)
def test_layernorm_cases_take_their_forms(case, op, config, B, S, form):
    d = X.D_MODEL[config]
    shape = (d if op == "mha" else X.D_INNER[config], d, 1)
    M = B * S
    assert _plan(M, shape, 1) == form, "a threshold of the dispatch moved: pick a size that takes this form again"
    assert M % form[0] != 0 and form[3] == (M + form[0] - 1) // form[0] * (1 if form[2] else (d + 255) // 256)
    assert _plan((form[3] // (1 if form[2] else 2) - 1) * form[0], shape, 1) is None  # one row tile fewer: the fp32 ladder
    lens = X.ragged_lens(B, S)
    assert len(lens) == B and max(lens) == S and min(lens) == 1 and {S, S - 1, 1} <= set(lens) and all(1 <= n <= S for n in lens)


def test_handover_case_sits_on_the_threshold():
    name, config, B, S0, S1 = X.HANDOVER
    shape = X.shape_of(name, config)
    assert _plan(B * S0, shape) is None and _plan(B * S1, shape) == (128, 256, 0, 200)
    assert (B * S0 + 127) // 128 * 4 == 196 and S1 == S0 + 1


# ---------------------------------------------------------------------------------------------------- the dispatch, swept
def _ceil(a, b):
    return (a + b - 1) // b


def _want(M, N, Cin, KW, epi):
    """the two gates restated from include/nar_fs2.h ns_plan_gemm_b3's words"""
    covered = Cin % 32 == 0 and N % 16 == 0 and 3 * N * KW * Cin * 2 < 2 ** 31
    plain = covered and _ceil(M, 128) * _ceil(N, 256) >= 200
    if epi == 1 and covered and N == 256 and _ceil(M, 64) >= 200:
        return (64, 256, 1, _ceil(M, 64))
    if plain and (epi == 0 or (epi == 1 and N != 256)):
        bm = 256 if _ceil(M, 256) * _ceil(N, 256) >= 240 else 128
        return (bm, 256, 0, _ceil(M, bm) * _ceil(N, 256))
    return None


SWEEP_SHAPES = {  # (N, Cin, KW) of every contraction that has planes
    "tiny": [(768, 256, 1), (256, 256, 1), (1024, 256, 9), (256, 1024, 1), (512, 512, 5)],
    "tiny512": [(1536, 512, 1), (512, 512, 1), (1024, 512, 9), (512, 1024, 1), (512, 512, 5)],
    "ljspeech": [(768, 256, 1), (256, 256, 1), (1024, 256, 9), (256, 1024, 1), (512, 512, 5)],
}


def test_hook_agrees_with_the_gates_at_every_threshold():
    """M across every multiple of 64 up to past the last threshold (240 tiles of 256 rows at N = 256: 61 185 rows), one row either
    side of each; epi = 1 takes each of its three answers somewhere"""
    from smart_nar_fast_tts_amd import _lib, ops

    answers = set()
    for config, shapes in SWEEP_SHAPES.items():
        for N, Cin, KW in shapes:
            seen = set()
            for k in range(0, 62000 // 64):
                for M in (64 * k - 1, 64 * k, 64 * k + 1):
                    if M <= 0:
                        continue
                    for epi in (0, 1):
                        got = ops.plan_gemm_b3(M, N, Cin, KW, epi)
                        assert got == _want(M, N, Cin, KW, epi), (config, M, N, Cin, KW, epi, got)
                        seen.add((epi, None if got is None else got[:3]))
                        if epi == 1 and N in (256, 512) and KW == 1:
                            answers.add("fp32 ladder" if got is None else "full-row tile" if got[2] else "plain + k_layernorm")
            assert {(0, None), (0, (128, 256, 0)), (0, (256, 256, 0))} <= seen, (config, N, Cin, KW, seen)
    assert answers == {"fp32 ladder", "full-row tile", "plain + k_layernorm"}
    # refusals and the null out
    lib = _lib.load()
    assert ops.plan_gemm_b3(20000, 1024, 72, 1) is None and ops.plan_gemm_b3(20000, 1000, 256, 1) is None  # Cin % 32, N % 16
    assert ops.plan_gemm_b3(0, 1024, 256, 9) is None and ops.plan_gemm_b3(20000, 1024, 256, 9, 2) is None
    assert ops.plan_gemm_b3(20000, 768, 256, 1, 1) == ops.plan_gemm_b3(20000, 768, 256, 1, 0)  # (a width that is no row: still two launches)
    assert lib.ns_plan_gemm_b3(6289, 1024, 256, 9, 0, None) == 1 and lib.ns_plan_gemm_b3(6270, 1024, 256, 9, 0, None) == 0
    assert ops.plan_gemm_b3(4995, 1056, 256, 9) == (128, 256, 0, 200)  # N % 16 == 0 and no multiple of 256: the column edge
