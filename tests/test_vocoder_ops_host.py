"""The gate of tests/test_gpu_vocoder_ops.py proven on the CPU, both ways, the geometry of its case table, and the host-side
validation of ns_voc_op_conv_form (no GPU).  The launch, the gate and its E term are derived in tests/vocoder_ops.py.

INSIDE: torch's fp32 evaluation of the same launch on the CPU (bf16 mode: the fp32 evaluation of the emulation) stays inside the
gate with room for a second summation order (< 0.5 of it), at EVERY case of the table.  Measured (run with -s): fp32 mode 0.0029
... 0.094 of the bound (the largest on the upsamplers, the smallest on mrf 2, whose bound is not divided by n_rb), bf16 mode
0.0005 ... 0.024.  E is at most 2.5 % of the bound (mrf 1, three epilogue sums on C = 32).

OUTSIDE: every mutant below — a float64 evaluation of a wrong implementation, so the mutation is its only error — fails the gate
by at least MUTANT_FLOOR = 3, on every form it applies to, at the smallest cases of the form's table (stage 3 / upsampler 3: the
long and the short size, both modes).  Measured factors over the bound, smallest ... largest over those cases:
    neighbour's row for zero at an utterance edge in a later tile      5 470 ... 1 330 000
    first row of the second row tile holds its neighbour's value      10 300 ... 274 000
    one 32-wide K chunk dropped                                        2 450 ... 230 000
    output lrelu skipped                                              25 900 ... 189 000
    output lrelu with slope 0.01                                       2 590 ... 18 900
    input lrelu applied on a c2 launch                                 5 980 ... 107 000
    residual omitted                                                   9 180 ... 376 000
    residual taken from row t + 1                                     15 200 ... 490 000
    residual added before the output lrelu                            65 600 ... 268 000
    mrf 1 stores where it must accumulate                             33 300 ... 152 000
    mrf 2 omits the division                                          30 300 ... 116 000
    mrf 2 divides by 2                                                 7 570 ... 29 100
    upsampler: the two taps' weight halves exchanged                  58 500 ... 287 000
    upsampler: output shifted by one row                              82 200 ... 336 000
    upsampler: the last u/2 output rows left unwritten                inf (the poison is NaN: a value that is not finite fails)
    upsampler: bias indexed by n                                          94 ... 513
No mutant needed other inputs to separate: the weakest is the upsampler's bias indexed by n (a bias of at most 0.05 / sqrt(K)
against a bound of 4e-6 ... 1.5e-5 of a unit near 1), still 94x.  "Residual added before the output lrelu" cannot differ on any
form stage() launches (none has both); it is checked on act_res, a form the entry point admits (tests/vocoder_ops.py)."""
import ctypes as C

import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from tests import vocoder_ops as V

pytestmark = pytest.mark.filterwarnings("ignore::FutureWarning")

MUTANT_FLOOR = 3.0
INSIDE_SHARE = 0.5
SMALLEST = [c for c in V.CASES if c.stage == 3]  # the fewest products per form: C = 32 resblocks, the 64 -> 32 upsampler


@pytest.fixture(scope="module")
def h():
    return V.model()[0]


# ---------------------------------------------------------------------------------------------------- geometry of the table
def test_tile_rule_is_the_dispatch():
    """tile() against the two dispatch functions, read from their sources: a changed tile height or width rule fails here"""
    import os
    import re

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smart-nar_fast_tts_amd", "csrc")
    for mode, src, fn in (("fp32", "vocoder.hip", "voc_launch"), ("bf16", "vocoder_bf16.hip", "voc_launch_bf16")):
        text = open(os.path.join(csrc, src)).read()
        rules = re.findall(r"(?:if \(p\.N % (\d+) == 0\) )?return " + fn + r"<(\d+), (\d+), \d+, \d+>\(p, st\);", text)
        assert len(rules) == (3 if mode == "fp32" else 4) and rules[-1][0] == "", rules
        for N in range(32, 2049, 32):
            want = next((int(bm), int(bn)) for div, bm, bn in rules if div == "" or N % int(div) == 0)
            assert V.tile(mode, N) == want, (mode, N)
        assert {int(bm) for _, bm, _ in rules} == {V.TILE_M[mode]}


@pytest.mark.parametrize("c", V.CASES, ids=lambda c: c.id)
def test_case_geometry(h, c):
    Sg, N, K = V.grid(h, c)
    g = V.geometry(c.mode, N, c.B, Sg)
    print(f"\n{c.id}: N={N} K={K} tile {g['BM']}x{g['BN']}, {g['M']} rows = {g['tiles']} row tiles (last {g['last']} rows), tile boundary "
          f"{g['tile_boundary']} inside utterance {g['tile_boundary'] // Sg}, utterance boundary {g['utt_boundary']} inside tile "
          f"{g['utt_boundary'] // g['BM']}")
    assert g["tiles"] >= 3, "at least three row tiles"
    assert g["last"] != 0, "a partial last tile"
    assert g["tile_boundary"] is not None and g["tile_boundary"] % Sg != 0, "a tile boundary strictly inside an utterance"
    e = g["utt_boundary"]
    assert e is not None and e // g["BM"] >= 1 and e % g["BM"] != 0 and e % 32 != 0 and e % Sg == 0, "an utterance boundary in a later tile"
    f = V.FORMS.get(c.form)
    if f is not None and (c.B, c.S) == V.CONV_LONG[c.mode]:
        L = V.launch_of(c)
        assert c.S > 2 * (L.d * (L.k - 1) // 2), "an utterance longer than twice the reach"
    if (c.B, c.S) in (V.CONV_SHORT[c.mode], V.UP_SHORT[c.mode]):
        assert Sg < 28, "several utterances inside one 32-row block"
    assert c.B >= 3


def test_table_covers_what_it_says(h):
    widths = {m: {V.tile(m, V.grid(h, c)[1])[1] for c in V.PLAIN_CASES if c.mode == m} for m in V.MODES}
    assert widths == {"fp32": {128, 64, 32}, "bf16": {256, 128, 64, 32}}  # every tile width the resblocks take
    for m in V.MODES:
        kd = {(V.launch_of(c).k, V.launch_of(c).d) for c in V.PLAIN_CASES if c.mode == m}
        assert kd == {(3, 1), (11, 5)}
        for st in (0, 3):
            for f in V.EPILOGUES:
                sizes = {(c.B, c.S) for c in V.EPILOGUE_CASES if (c.mode, c.stage, c.form) == (m, st, f.key)}
                assert sizes == {V.CONV_LONG[m], V.CONV_SHORT[m]}, (m, st, f.key)
        for i in range(4):
            N = V.grid(h, V.Case("up", "up", i, m, 3, 1))[1]
            assert V.UP_LONG[m][1] == V.smallest_up_S(m, N), (m, i)
            assert {(c.B, c.S) for c in V.UP_CASES if (c.mode, c.stage) == (m, i)} == {V.UP_LONG[m], V.UP_SHORT[m]}
    # what stage() launches, as forms: c1, a middle c2, and the last c2 of resblock j with mrf = j
    assert [(f.in_act, f.out_act, f.resid, f.mrf, f.which) for f in V.EPILOGUES[:5]] == [
        (True, True, False, 0, 1), (False, False, True, 0, 2), (False, False, True, 0, 2), (False, False, True, 1, 2), (False, False, True, 2, 2)]
    assert [f.j for f in V.EPILOGUES[2:5]] == [0, 1, 2] and all(f.n == 2 for f in V.EPILOGUES[2:5]) and V.EPILOGUES[1].n < 2
    assert len({c.id for c in V.CASES}) == len(V.CASES)


# ---------------------------------------------------------------------------------------------------- the gate, inside
@pytest.mark.parametrize("c", V.CASES, ids=lambda c: c.id)
def test_gate_passes_the_cpu_fp32_evaluation(c):
    L = V.launch_of(c)
    x, resid, acc = V.inputs(c)
    ref = V.evaluate(L, x, resid, acc)
    std, neg = float(ref.v.std()), float((ref.v < 0).double().mean())
    assert 0.5 <= std <= 2.0 and 0.3 <= neg <= 0.7 and 0.3 <= float((x < 0).double().mean()) <= 0.7, (std, neg)  # both lrelu branches live
    assert torch.equal(x[c.B - 1], x[0]) and torch.equal(ref.out[c.B - 1], ref.out[0])
    good = V.check(V.evaluate(L, x, resid, acc, dtype=torch.float32).out, ref)
    e_share = float(((ref.bound - V.REL[c.mode] * ref.unit) / ref.bound).max())
    print(f"\n{c.id}: torch fp32 on the CPU at {good.worst:.3g} of the gate; pre-activation std {std:.2f}, {100 * neg:.0f} % negative; "
          f"E is at most {100 * e_share:.2g} % of the bound")
    assert good.ok and good.worst < INSIDE_SHARE, str(good)
    assert e_share < 0.25  # E is the smaller part of the gate everywhere: the contraction's bound is what is under test


# ---------------------------------------------------------------------------------------------------- the gate, outside
def _later_edge_rows(c, L, g, Sg):
    """flat output rows within the launch's reach of the utterance boundary geometry() found in a later tile"""
    b = g["utt_boundary"] // Sg
    if c.kind == "up":
        o, reach = b * c.S * L.u, L.u // 2
    else:
        o, reach = b * c.S, L.d * (L.k - 1) // 2
    return slice(o - reach, o + reach)


def mutants(c, h):
    """name -> output of a WRONG implementation in float64 (the mutation is its only error)"""
    L = V.launch_of(c)
    x, resid, acc = V.inputs(c)
    ref = V.evaluate(L, x, resid, acc)
    Sg, N, _ = V.grid(h, c)
    g = V.geometry(c.mode, N, c.B, Sg)
    ev = lambda **kw: V.evaluate(L, x, resid, acc, with_bound=False, **kw).out  # noqa: E731
    flat = lambda t: t.reshape(-1, t.shape[-1])  # noqa: E731
    out = {}
    rows = _later_edge_rows(c, L, g, Sg)
    m = ref.out.clone()
    flat(m)[rows] = flat(ev(cross_utterance=True))[rows]
    assert not torch.equal(flat(m)[rows], flat(ref.out)[rows])
    out["neighbour's row for zero at an edge in a later tile"] = m
    m = ref.out.clone()
    if c.kind == "up":  # grid row BM = (utterance b, q) stores output rows [q u - u / 2, (q + 1) u - u / 2) of b, clipped
        b, q = divmod(g["BM"], Sg)
        lo, hi = max(q * L.u - L.u // 2, 0), min((q + 1) * L.u - L.u // 2, c.S * L.u)
        src = lo + L.u if hi + L.u <= c.S * L.u else lo - L.u
        m[b, lo:hi] = ref.out[b, src:src + hi - lo]
    else:
        flat(m)[g["BM"]] = flat(ref.out)[g["BM"] + 1]
    out["first row of the second row tile holds its neighbour's value"] = m
    out["one 32-wide K chunk dropped"] = ev(drop_chunk=True)
    if L.out_act:
        out["output lrelu skipped"] = ev(out_act=False)
        out["output lrelu with slope 0.01"] = ev(out_slope=0.01)
    if c.kind == "conv" and not L.in_act:
        out["input lrelu applied on a c2 launch"] = ev(in_act=True)
    if resid is not None:
        out["residual omitted"] = ev(resid_mode="omit")
        out["residual taken from row t + 1"] = ev(resid_mode="next_row")
    if resid is not None and L.out_act:
        out["residual added before the output lrelu"] = ev(resid_mode="before_act")
    if L.mrf == 1:
        out["mrf 1 stores where it must accumulate"] = ev(mrf_mode="store")
    if L.mrf == 2:
        out["mrf 2 omits the division"] = ev(mrf_mode="no_div")
        out["mrf 2 divides by 2"] = ev(mrf_mode="div2")
    if c.kind == "up":
        u, cout = L.u, L.w.shape[1]
        out["upsampler: the two taps' weight halves exchanged"] = ev(swap_halves=True)
        out["upsampler: output shifted by one row"] = ref.out.roll(1, dims=1)
        m = ref.out.clone()  # the output poisoned first, the last u / 2 rows of every utterance never written
        m[:, c.S * u - u // 2:] = float("nan")
        out["upsampler: the last u/2 output rows left unwritten"] = m
        # bias[n] for bias[n % Cout], n = r Cout + co: right for phase r = 0 only; past the bias the arena holds no bias at all
        # (modelled as zero).  Output row o has phase (o + u / 2) % u.
        phase = (torch.arange(c.S * u) + u // 2) % u
        m = ref.out - L.b.double() * (phase != 0)[None, :, None]
        out["upsampler: bias indexed by n"] = m
        assert cout == ref.out.shape[-1]
    return ref, out


EXPECTED = {
    "conv": {"neighbour's row for zero at an edge in a later tile", "first row of the second row tile holds its neighbour's value", "one 32-wide K chunk dropped"},
    "c1": {"output lrelu skipped", "output lrelu with slope 0.01"},
    "c2": {"input lrelu applied on a c2 launch", "residual omitted", "residual taken from row t + 1"},
    "act_res": {"output lrelu skipped", "output lrelu with slope 0.01", "residual omitted", "residual taken from row t + 1", "residual added before the output lrelu"},
    "c2_last_mrf1": {"mrf 1 stores where it must accumulate"},
    "c2_last_mrf2": {"mrf 2 omits the division", "mrf 2 divides by 2"},
    "up": {"upsampler: the two taps' weight halves exchanged", "upsampler: output shifted by one row",
           "upsampler: the last u/2 output rows left unwritten", "upsampler: bias indexed by n"},
}


@pytest.mark.parametrize("c", SMALLEST, ids=lambda c: c.id)
def test_gate_rejects_every_mutant(h, c):
    ref, muts = mutants(c, h)
    want = set(EXPECTED["conv"])
    for key in ("c1", "act_res", "c2_last_mrf1", "c2_last_mrf2", "up"):
        if c.form == key:
            want |= EXPECTED[key]
    if c.form.startswith("c2"):
        want |= EXPECTED["c2"]
    assert set(muts) == want, sorted(set(muts) ^ want)  # no mutant of the form's list is left out
    print(f"\n{c.id}")
    for name, y in muts.items():
        bad = V.check(y, ref)
        print(f"  {name}: {bad.worst:.3g} x the bound")
        assert not bad.ok and bad.worst >= MUTANT_FLOOR, (name, str(bad))


def test_every_listed_mutant_is_exercised():
    forms = {c.form for c in SMALLEST}
    assert forms == set(V.FORMS) | {"up"}
    assert {c.mode for c in SMALLEST} == set(V.MODES)
    for f in forms:  # the long and the short size of every form that has both
        sizes = {(c.B, c.S) for c in SMALLEST if c.form == f and c.mode == "fp32"}
        assert len(sizes) == (1 if f == "plain_k3_d1" else 2), (f, sizes)


# ---------------------------------------------------------------------------------------------------- ns_voc_op_conv_form, host side
def test_op_conv_form_refuses_bad_arguments_before_any_device_work(h):
    """every refusal comes before the handle's state is looked at: an unfinalized vocoder with no arena answers them all"""
    from smart_nar_fast_tts_amd import _lib
    from smart_nar_fast_tts_amd.vocoder import Generator

    g = Generator(h)
    lib, hd = g._lib, g._h
    buf = torch.zeros(3 * 7 * 32 + 4)
    x, y = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr())
    assert buf.data_ptr() % 16 == 0
    call = lambda name, xx, yy, mrf, hh=hd, B=3, S=7: lib.ns_voc_op_conv_form(hh, name, xx, None, yy, B, S, 0, 0, mrf, None)  # noqa: E731
    err = lambda: lib.ns_last_error().decode()  # noqa: E731
    ok_name = b"resblocks.9.convs2.2"
    assert call(ok_name, x, y, 0, hh=None) != 0 and "null vocoder" in err()
    for bad in (b"conv_pre", b"conv_post", b"ups.0", b"resblocks.12.convs1.0", b"resblocks.0.convs3.0", b"resblocks.0.convs1.3", b"resblocks.0.convs1.0x"):
        assert call(bad, x, y, 0) != 0 and "unknown module" in err(), bad
    assert call(None, x, y, 0) != 0 and call(ok_name, None, y, 0) != 0 and call(ok_name, x, None, 0) != 0 and "bad argument" in err()
    assert call(ok_name, x, y, 0, B=0) != 0 and call(ok_name, x, y, 0, S=-1) != 0
    for mrf in (-1, 3):
        assert call(ok_name, x, y, mrf) != 0 and "mrf must be" in err()
    assert call(ok_name, C.c_void_p(buf.data_ptr() + 4), y, 0) != 0 and "16-byte aligned" in err()
    assert call(ok_name, x, y, 2) != 0 and "not finalized" in err()  # valid arguments: only now the handle's state
    assert lib.ns_voc_abi_version() == 1  # an added entry point: the ABI version stays
    assert "ns_voc_op_conv_form" in _lib.SIGNATURES


def test_op_conv_form_wrapper_arguments(h):
    from smart_nar_fast_tts_amd.vocoder import Generator

    g = Generator(h)
    g._sd = {"resblocks.9.convs2.2.weight": torch.zeros(32, 32, 3).numpy()}  # the argument checks under test come before any launch
    x = torch.zeros(3, 7, 32)
    g._ready = lambda t: None  # (_ready wants a cuda tensor; none exists here)
    with pytest.raises(ValueError, match="mrf must be"):
        g.op_conv_form("resblocks.9.convs2.2", x, mrf=3)
    with pytest.raises(ValueError, match="required when mrf != 0"):
        g.op_conv_form("resblocks.9.convs2.2", x, mrf=1)
    with pytest.raises(ValueError, match="refused when mrf == 0"):
        g.op_conv_form("resblocks.9.convs2.2", x, mrf=0, acc=x)
    with pytest.raises(ValueError, match="residual must be"):
        g.op_conv_form("resblocks.9.convs2.2", x, residual=torch.zeros(3, 7, 16))
    with pytest.raises(ValueError, match="takes .B, S, 32. activations"):
        g.op_conv_form("resblocks.9.convs2.2", torch.zeros(3, 7, 64))
    with pytest.raises(ValueError, match="out must be"):
        g.op_upsample(3, torch.zeros(3, 7, 64), out=torch.zeros(3, 14, 16))


def test_synthetic_weights_are_the_suite_s(h):
    sd = wl.synth_vocoder_state_dict(h, seed=0)
    assert all((sd[k] == v).all() for k, v in V.model()[1].items())
