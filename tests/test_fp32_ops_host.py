"""The gate of tests/test_gpu_fp32_ops.py proven on the CPU, both ways, and the table of its cases checked against the dispatch
itself (no GPU).

Contract of one exact-fp32 contraction (csrc/gemm_conv.hip k_conv_gemm): the operands are taken as they are, products are summed in
fp32 in some order, each utterance of S rows is zero padded, bias and activation are applied in fp32.  An evaluation differs from
the float64 one only by its summation, so the bound is elementwise:  |y - f64| <= FP32_REL * (conv(|x|, |w|) + |bias|), applied
before a 1-Lipschitz activation.  FP32_REL = 4e-6 is the project's fp32 figure (tests/bf16_emu.py; tests/test_gpu_vocoder.py holds
an fp32 MFMA GEMM with K up to 5632 to it).  Measured here (run with -s): torch's fp32 CPU evaluation sits at 0.0098 ... 0.059 of
the bound; a dropped (channel, tap) is 896 ... 12 196 x the bound, a dropped K chunk of 32 3871 ... 39 018 x, the neighbouring
utterance's row for zero 26 409 ... 71 639 x; ONE row off by 2^-12 of its value 6.8 ... 25 x and one column 3.6 ... 13.8 x (the
smallest at K = 4608, where the unit is largest against a value).

The second half is the coverage table: every template instantiation launch_conv_gemm_impl can dispatch with NS_PLAN unset
(FORMS), the GPU cases that take each of them (CASES ...), the forms no accepted contraction reaches (UNREACHED, with reasons), all
asserted through ns_plan_gemm_launches — the dispatch describing its own launches — so that a moved planner threshold fails here, on
every CPU run, and not silently on the GPU."""
import os

import pytest
import torch

from tests import bf16_emu as E

REL = E.FP32_REL
GEMM_SHAPES = [(256, 1024, 9), (1024, 256, 1), (512, 512, 5), (512, 2048, 9), (80, 512, 5), (512, 80, 5), (256, 768, 1)]  # (Cin, N, KW)
B, S = 3, 33


def _gemm_case(Cin, N, KW):
    g = torch.Generator().manual_seed(Cin + N + KW)
    return torch.randn(B, S, Cin, generator=g), torch.randn(N, Cin, KW, generator=g), torch.randn(N, generator=g)


def _variants(x, w, b, ref):
    """name -> (output of a WRONG implementation evaluated in float64: its only error is the mutation, the factor it must fail by)"""
    N, Cin, KW = w.shape
    wd = w.clone()
    wd[:, Cin // 3, KW // 2] = 0
    wc = w.clone()
    c0 = (Cin // 3) // 16 * 16
    wc[:, c0:c0 + 32, KW // 2] = 0
    out = {"one (c, tap) dropped": (E.conv_rows(x, wd, b), 100), "one K chunk of 32 dropped": (E.conv_rows(x, wc, b), 100)}
    if KW > 1:
        out["neighbour's row for zero"] = (E.conv_rows(x, w, b, cross_utterance=True), 100)
    row = ref.clone()
    row[B - 1, S - 1, :] *= 1 + 2.0 ** -12  # the last row of the partial last tile (M = 99)
    col = ref.clone()
    col[:, :, N - 1] *= 1 + 2.0 ** -12      # the last column (of the N = 80 tail, for the narrow shapes)
    out["one row off by 2^-12"] = (row, 3)
    out["one column off by 2^-12"] = (col, 3)
    return out


@pytest.mark.parametrize("Cin,N,KW", GEMM_SHAPES)
def test_fp32_gemm_gate_passes_fp32_and_rejects_wrong_variants(Cin, N, KW):
    x, w, b = _gemm_case(Cin, N, KW)
    ref, unit = E.gemm_emu(x, w, b, round_fn=E.exact), E.gemm_unit(x, w, b, round_fn=E.exact)
    assert torch.equal(ref, E.conv_rows(x, w, b))  # round_fn = exact: the operands as they are
    good = E.gemm_check(E.gemm_emu(x, w, b, dtype=torch.float32, round_fn=E.exact), x, w, b, rel=REL, ref=ref, unit=unit)
    print(f"\nfp32 gemm Cin={Cin} N={N} KW={KW}: fp32 CPU {good.worst * REL:.2e} of unit ({good.worst:.2e} x bound)")
    assert good.ok and good.worst < 0.1, str(good)
    for name, (y, factor) in _variants(x, w, b, ref).items():
        bad = E.gemm_check(y, x, w, b, rel=REL, ref=ref, unit=unit)
        print(f"  {name}: {bad.worst * REL:.2e} of unit = {bad.worst:.3g} x bound")
        assert not bad.ok and bad.worst > factor, (name, str(bad))
    for act in ("relu", "tanh"):  # the bound is on the pre-activation sum and holds behind a 1-Lipschitz activation
        got = E.gemm_emu(x, w, b, act=act, dtype=torch.float32, round_fn=E.exact)
        assert E.gemm_check(got, x, w, b, act=act, rel=REL, unit=unit, round_fn=E.exact).ok


def test_round_fn_default_is_the_bf16_contract():
    """the emulation's bf16 behaviour is what it was: the default rounds both operands, `exact` takes them as they are"""
    x, w, b = _gemm_case(256, 80, 1)
    assert torch.equal(E.gemm_emu(x, w, b), E.conv_rows(E.bf(x), E.bf(w), b))
    assert torch.equal(E.gemm_unit(x, w, b), E.conv_rows(E.bf(x).abs(), E.bf(w).abs(), b.abs()))
    assert not torch.equal(E.gemm_emu(x, w, b), E.gemm_emu(x, w, b, round_fn=E.exact))
    # an exact evaluation fails the bf16 gate and passes the fp32 one; the bf16 one fails the fp32 gate
    assert not E.gemm_check(E.conv_rows(x, w, b), x, w, b).ok
    assert E.gemm_check(E.conv_rows(x, w, b), x, w, b, rel=REL, round_fn=E.exact).ok
    assert not E.gemm_check(E.gemm_emu(x, w, b), x, w, b, rel=REL, round_fn=E.exact).ok


@pytest.mark.parametrize("Cin,N,d", [(1024, 256, 256), (256, 256, 256), (1024, 512, 512), (512, 512, 512)])
def test_fp32_layernorm_gate_passes_fp32_and_rejects_wrong_variants(Cin, N, d):
    """LayerNorm(gemm + x) at FP32_REL: the fp32 evaluation stays inside the first-order bound (0.008 ... 0.02 of it); a dropped
    channel (2174 ... 4768 x) and a row that added its neighbour's residual (26 387 ... 37 302 x) do not"""
    g = torch.Generator().manual_seed(Cin + N)
    x = torch.randn(B, S, Cin, generator=g).relu() if Cin != d else torch.randn(B, S, Cin, generator=g)
    w = torch.randn(N, Cin, 1, generator=g) / Cin ** 0.5
    b, resid = torch.randn(N, generator=g) * 0.1, torch.randn(B, S, N, generator=g)
    ln_g, ln_b = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    kw = dict(rel=REL, round_fn=E.exact)
    z32 = E.gemm_emu(x, w, b, dtype=torch.float32, round_fn=E.exact) + resid
    good = E.gemm_ln_check(E.layernorm_emu(z32, ln_g, ln_b, dtype=torch.float32), x, w, b, resid, ln_g, ln_b, **kw)
    print(f"\nfp32 layernorm Cin={Cin} N={N}: fp32 CPU {good.worst:.3g} x bound")
    assert good.ok and good.worst < 0.1, str(good)
    wd = w.clone()
    wd[:, 7, 0] = 0
    r2 = resid.clone()
    r2[1, 5] = resid[1, 6]
    for name, y in (("one channel dropped", E.layernorm_emu(E.conv_rows(x, wd, b) + resid.double(), ln_g, ln_b)),
                    ("neighbour's residual row", E.layernorm_emu(E.conv_rows(x, w, b) + r2.double(), ln_g, ln_b))):
        bad = E.gemm_ln_check(y, x, w, b, resid, ln_g, ln_b, **kw)
        print(f"  {name}: {bad.worst:.3g} x bound")
        assert not bad.ok and bad.worst > 100, (name, str(bad))


# ==================================================================================================== the coverage table
# A form is what launch_t records of itself: (BM, BN, BK, KS, MF, ROWEPI, TICKET).  FORMS is every instantiation
# launch_conv_gemm_impl dispatches with NS_PLAN unset (the 64 x 96 form and launch_tall are NS_PLAN=0 only).
def _f(bm, bn, bk=32, ks=1, mf=32, rowepi=0, ticket=0):
    return (bm, bn, bk, ks, mf, rowepi, ticket)


PLANNER32 = [_f(256, 256), _f(128, 256), _f(64, 256), _f(64, 128), _f(64, 64), _f(32, 128)]
F16W = [_f(16 * s, 256, mf=16) for s in range(3, 17)]
F16N = [_f(16 * s, 128, mf=16) for s in range(3, 11)]
LADDER = [_f(32, 32, ks=8), _f(32, 32, ks=4), _f(32, 64, ks=4), _f(48, 64, ks=4, mf=16), _f(32, 128, ks=2), _f(48, 128, ks=2, mf=16), _f(64, 64)]
NARROW = [_f(32, 96, ks=4), _f(48, 96, ks=4, mf=16), _f(80, 96, mf=16)]
BK16 = [_f(32, 32, bk=16, ks=4), _f(64, 256, bk=16), _f(64, 128, bk=16), _f(64, 64, bk=16)]
FULL_ROW = [_f(32, 256, rowepi=1), _f(48, 256, mf=16, rowepi=1), _f(80, 256, mf=16, rowepi=1), _f(112, 256, mf=16, rowepi=1),
            _f(32, 512, rowepi=1), _f(48, 512, mf=16, rowepi=1)]
TICKETED = [f[:6] + (t,) for t in (1, 2) for f in (_f(32, 32, ks=8), _f(32, 32, ks=4), _f(32, 64, ks=4), _f(48, 64, ks=4, mf=16), _f(32, 128, ks=2))]
FORMS = set(PLANNER32 + F16W + F16N + LADDER + NARROW + BK16 + FULL_ROW + TICKETED)
assert len(FORMS) == 57  # (64 x 64 is a planner tile and the ladder's last rung)

D_MODEL = {"tiny": 256, "ljspeech": 256, "tiny512": 512, "d512": 512}
LAST_LAYER = {"tiny": 0, "ljspeech": 3, "tiny512": 0, "d512": 5}
D_INNER, N_MEL, POSTNET_DIM = 1024, 80, 512


def shape_of(name, config):
    """(Cin, N, KW) of a contraction ops.gemm accepts (ops.gemm_shape without a model)"""
    d = D_MODEL[config]
    if name == "mel_linear":
        return d, N_MEL, 1
    if name.startswith("postnet.convolutions."):
        i = int(name.rsplit(".", 1)[1])
        return (N_MEL if i == 0 else POSTNET_DIM), (N_MEL if i == 4 else POSTNET_DIM), 5
    return {"qkv": (d, 3 * d, 1), "fc": (d, d, 1), "w_1": (d, D_INNER, 9), "w_2": (D_INNER, d, 1)}[name.rsplit(".", 1)[1]]


def all_shapes():
    """every (Cin, N, KW) the four configs offer to ops.gemm"""
    names = ["x.slf_attn.qkv", "x.slf_attn.fc", "x.pos_ffn.w_1", "x.pos_ffn.w_2", "mel_linear"] + [f"postnet.convolutions.{i}" for i in range(5)]
    return sorted({shape_of(n, c) for n in names for c in D_MODEL})


# (contraction, config, B, S, the forms of its launches).  Found by a scan over M = 3 S through ns_plan_gemm_launches: per form the
# contraction with the shortest K that reaches it, then the smallest M with B = 3 (taps cross both edges of the interior utterance),
# S >= 12, and a partial last row tile (rows of the last launch no multiple of its BM).  test_cases_are_the_smallest repeats the scan.
CASES = [
    ("postnet.convolutions.0", "tiny", 3, 12, [_f(32, 32, bk=16, ks=4)]),                                   # K = 400
    ("postnet.convolutions.0", "ljspeech", 3, 342, [_f(64, 64, bk=16)]),
    ("postnet.convolutions.0", "tiny512", 3, 2710, [_f(64, 128, bk=16)]),
    ("postnet.convolutions.0", "d512", 3, 10902, [_f(64, 256, bk=16)]),
    ("mel_linear", "tiny", 3, 5462, [_f(64, 64)]),                                                          # K = 256
    ("mel_decoder.layer_stack.0.slf_attn.fc", "tiny", 3, 683, [_f(48, 64, ks=4, mf=16)]),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 12, [_f(32, 32, ks=4)]),
    ("txt_encoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 107, [_f(32, 64, ks=4)]),
    ("mel_decoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 225, [_f(32, 128, ks=2)]),
    ("txt_encoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 449, [_f(48, 128, ks=2, mf=16)]),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 897, [_f(32, 128)]),
    ("txt_encoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 907, [_f(80, 128, mf=16)]),
    ("mel_decoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 1366, [_f(64, 128)]),
    ("txt_encoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 1814, [_f(144, 128, mf=16)]),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 2017, [_f(80, 256, mf=16)]),
    ("txt_encoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 2731, [_f(112, 256, mf=16)]),
    ("mel_decoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 3627, [_f(144, 256, mf=16)]),
    ("txt_encoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 4081, [_f(160, 256, mf=16)]),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 4545, [_f(176, 256, mf=16)]),
    ("txt_encoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 4987, [_f(192, 256, mf=16)]),
    ("mel_decoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 5462, [_f(208, 256, mf=16)]),
    ("txt_encoder.layer_stack.3.slf_attn.qkv", "ljspeech", 3, 5894, [_f(224, 256, mf=16)]),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 6358, [_f(240, 256, mf=16)]),
    ("txt_encoder.layer_stack.0.slf_attn.qkv", "tiny", 3, 6801, [_f(256, 256, mf=16)]),
    ("mel_decoder.layer_stack.0.pos_ffn.w_1", "tiny", 3, 1195, [_f(64, 256, mf=16)]),                       # K = 2304
    ("txt_encoder.layer_stack.0.pos_ffn.w_1", "tiny", 3, 1366, [_f(48, 128, mf=16)]),
    ("postnet.convolutions.4", "tiny", 3, 1366, [_f(32, 96, ks=4)]),                                        # K = 2560
    ("postnet.convolutions.4", "ljspeech", 3, 2731, [_f(48, 96, ks=4, mf=16)]),
    ("postnet.convolutions.4", "tiny512", 3, 5462, [_f(80, 96, mf=16)]),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", "tiny512", 3, 12, [_f(32, 32, ks=8)]),                       # K = 512
    ("txt_encoder.layer_stack.0.slf_attn.qkv", "tiny512", 3, 561, [_f(48, 256, mf=16)]),
    ("mel_decoder.layer_stack.5.slf_attn.qkv", "d512", 3, 683, [_f(112, 128, mf=16)]),
    ("txt_encoder.layer_stack.5.slf_attn.qkv", "d512", 3, 1569, [_f(128, 256, mf=16)]),
    ("mel_decoder.layer_stack.0.slf_attn.qkv", "tiny512", 3, 4534, [_f(64, 256)]),
    ("mel_decoder.layer_stack.0.pos_ffn.w_2", "tiny512", 3, 3414, [_f(96, 256, mf=16)]),                    # K = 1024
    ("txt_encoder.layer_stack.0.pos_ffn.w_2", "tiny512", 3, 4779, [_f(128, 256)]),
]
# Long contractions (K > 512: the second accumulator set, chunks of 64 products) on the 32-row planner tiles that admit them
# (128 x 256 is the w_2 case above; 256 x 256 has no room and never gets one), a cut plan, and — the other side of
# long_k_threshold — K = 512 summed sequentially on a tile without room (144 x 256).  Of the 16-row family, 96 x 256 (w_2, K = 1024)
# and 48 x 128 / 64 x 256 (w_1, K = 2304) above are long-K cases with s <= 8 already.
# The last entry is the only long-K launch of the 32 x 128 tile any contraction reaches: the remainder of a cut at 61 500 rows.  Its
# float64 reference (290 GFLOP for all rows) is evaluated on utterance 0 (the 128 x 256 main launch) and on the utterances the
# remainder launch covers, 55 ... 59 — every row of the form under test; the replica and the finiteness checks cover all rows.
LONG_K_CASES = [
    ("mel_decoder.layer_stack.0.pos_ffn.w_1", "tiny", 3, 1217, [_f(64, 128)], None),                         # K = 2304
    ("mel_decoder.layer_stack.5.pos_ffn.w_2", "d512", 3, 7510, [_f(64, 256)], None),                         # K = 1024
    ("mel_decoder.layer_stack.3.pos_ffn.w_1", "ljspeech", 3, 3585, [_f(64, 128), _f(64, 64)], None),         # K = 2304, cut at row 10 240
    ("postnet.convolutions.1", "ljspeech", 3, 7169, [_f(64, 128), _f(64, 64)], None),                        # K = 2560, cut at row 20 480
    ("txt_encoder.layer_stack.5.slf_attn.qkv", "d512", 3, 1814, [_f(144, 256, mf=16)], None),                # K = 512, sequential
    ("txt_encoder.layer_stack.3.pos_ffn.w_1", "ljspeech", 60, 1025, [_f(128, 256), _f(32, 128)], [0, 55, 56, 57, 58, 59]),
]
# S below the kernel's reach (every tap but the centre ones reads padding or the only other rows), on the bottom ladder rung
SHORT_S_CASES = [
    ("mel_decoder.layer_stack.0.pos_ffn.w_1", "tiny", 5, 1, [_f(32, 32, ks=8)], None),
    ("mel_decoder.layer_stack.0.pos_ffn.w_1", "tiny", 5, 3, [_f(32, 32, ks=8)], None),
    ("postnet.convolutions.0", "tiny", 5, 1, [_f(32, 32, bk=16, ks=4)], None),
    ("postnet.convolutions.0", "tiny", 5, 2, [_f(32, 32, bk=16, ks=4)], None),
    ("postnet.convolutions.1", "tiny", 5, 1, [_f(32, 32, ks=8)], None),
    ("postnet.convolutions.4", "tiny", 5, 2, [_f(32, 32, ks=8)], None),
]
GEMM_CASES = [c + (None,) for c in CASES] + LONG_K_CASES + SHORT_S_CASES


def _lens(Bn, Sn):
    """ragged valid lengths: full, one short, the halves, tile edges, a single frame"""
    return ([Sn, Sn - 1, Sn // 2 + 1, Sn // 2, 129, 33, 1] if Bn == 7 else [Sn, 2 * Sn // 3 + 1, 1])[:Bn]


# LayerNorm forms: (op, config, B, S, form).  op "mha" = ops.multi_head_attention (fc + LayerNorm, K = d), "ffn" =
# ops.positionwise_ffn (w_2 + LayerNorm, K = 1024).  Which form a model takes is host_core.h's rule (fuse_row_epilogue /
# conv_gemm_ticket_ok): the full-row tile from ceil(M / 32) >= 200 row tiles, the ticketed ladder below; ln_epi restates it and
# test_layernorm_cases_take_their_forms asks ns_plan_gemm_launches for the form under that epilogue.  Every M leaves a partial last
# tile; lens are ragged (_lens).
LN_CASES = [(op, cfg, Bn, Sn, form) for cfg_pair, rows in (
    (("tiny", "ljspeech"), [(7, 911, _f(32, 256, rowepi=1)), (7, 1171, _f(48, 256, mf=16, rowepi=1)), (7, 2341, _f(80, 256, mf=16, rowepi=1)),
                            (7, 3511, _f(112, 256, mf=16, rowepi=1)), (3, 33, None), (3, 343, _f(32, 64, ks=4, ticket=1)),
                            (3, 701, _f(48, 64, ks=4, mf=16, ticket=1)), (3, 1031, _f(32, 128, ks=2, ticket=1))]),
    (("tiny512", "d512"), [(7, 911, _f(32, 512, rowepi=1)), (7, 1171, _f(48, 512, mf=16, rowepi=1)), (3, 33, _f(32, 32, ks=8, ticket=2)),
                           (3, 173, _f(32, 64, ks=4, ticket=2)), (3, 343, _f(48, 64, ks=4, mf=16, ticket=2)), (3, 517, _f(32, 128, ks=2, ticket=2))]))
    for i, (Bn, Sn, form) in enumerate(rows) for op, cfg in (("mha", cfg_pair[i % 2]), ("ffn", cfg_pair[(i + 1) % 2]))]
# (the first rung at 256 columns has two forms: K = 256 (fc) is 8 chunks -> four K groups, K = 1024 (w_2) 32 chunks -> eight)
LN_CASES = [(op, cfg, Bn, Sn, form or _f(32, 32, ks=4 if op == "mha" else 8, ticket=1)) for op, cfg, Bn, Sn, form in LN_CASES]
MASKED_ROW_CASES = [("ljspeech", 7, 911), ("tiny512", 3, 343)]  # fft_block: one full-row and one ticketed (16-row family) case

# Forms that no contraction ops.gemm accepts reaches at M <= 70 000 rows with NS_PLAN (and every other switch) unset, and why.
UNREACHED = {
    _f(256, 256): "the planner starts at 256 x 256 only for more than 16 K chunks that are not long (plan_rows `first`), and more than 16 chunks IS "
                  "K > 512 = long_k_threshold: since the long contractions moved to 128 x 256 the tile is taken under NS_LONG_K / NS_ACC_CHUNK=0 / NS_PLAN=0 only",
    _f(64, 128, mf=16): "16 s x 128 with even s ties 16 (s / 2) x 256 in workgroups and loses to it by the 2 % panel re-read (tile16_time) whenever "
                        "N % 256 == 0, and every N >= 128 of the four configs (256, 512, 768, 1024, 1536) is a multiple of 256",
    _f(96, 128, mf=16): "as 64 x 128 (MF 16): even s, every N a multiple of 256",
    _f(128, 128, mf=16): "as 64 x 128 (MF 16): even s, every N a multiple of 256",
    _f(160, 128, mf=16): "as 64 x 128 (MF 16): even s, every N a multiple of 256",
    _f(32, 32, ks=4, ticket=2): "the 512-wide ticketed first rung with four K groups needs fewer than 16 K chunks; both 512-wide LayerNorm GEMMs "
                                "(fc K = 512, w_2 K = 1024) have 16 or more and take eight",
}
# The planner families and the full-row heights are reachable by row count alone for a suitable width, so none of them should be
# unreached — and none is, except the five above, whose reasons are the widths of the configs (and, for 256 x 256, long_k_threshold),
# not the row count.  Named here so that a sixth cannot join them unnoticed.
PLANNER_FAMILY_UNREACHED = {_f(256, 256), _f(64, 128, mf=16), _f(96, 128, mf=16), _f(128, 128, mf=16), _f(160, 128, mf=16)}
SCAN_ROWS = 70000


def ln_epi(M):
    """host_core.h fuse_row_epilogue: 1 (full-row tile) from ceil(M / 32) >= 200, else 2 (ticketed ladder)"""
    return 1 if (M + 31) // 32 >= 200 else 2


def launches(M, shape, epi=0):
    from smart_nar_fast_tts_amd import ops

    Cin, N, KW = shape
    return ops.plan_gemm_launches(M, N, Cin, KW, epi)


_SCAN = {}


# The variance predictors' two contractions (csrc/api.hip predictor_conv1 / predictor_tail; conv1d_1 of a 512-wide model reads 512
# channels): ops.gemm cannot name them, they run under a row epilogue only — LayerNorm for conv1d_1, the predictor tail for conv1d_2,
# both dispatched like a LayerNorm launch.  Their cases are tests/test_predictor_ops_host.py PRED_CASES.
PRED_SHAPES = [(256, 256, 3), (512, 256, 3)]


def scan():
    """{form: {shape: smallest M}} over every accepted contraction and M = 1 ... SCAN_ROWS, plain and (row widths) LayerNorm, and
    the predictors' contractions under their row epilogue"""
    if not _SCAN:
        for shape in all_shapes() + PRED_SHAPES:
            plain = () if shape in PRED_SHAPES else ((lambda M: 0),)
            for epi_of in plain + ((ln_epi,) if shape[1] in (256, 512) and (shape[2] == 1 or shape in PRED_SHAPES) else ()):
                for M in range(1, SCAN_ROWS + 1):
                    for l in launches(M, shape, epi_of(M)):
                        _SCAN.setdefault(l[:7], {}).setdefault(shape, M)
    return _SCAN


@pytest.fixture(scope="module", autouse=True)
def _switches_unset():
    for k in ("NS_PLAN", "NS_TILE16", "NS_TILE16N", "NS_LONG_K", "NS_ACC_CHUNK"):
        if k in os.environ:
            pytest.fail(f"{k} is set: the coverage table describes the default dispatch")


def test_plan_gemm_launches_describes_the_dispatch():
    """the entry point against what ns_plan_gemm already answers inside the planner's range, and its answers outside it"""
    import ctypes

    from smart_nar_fast_tts_amd import _lib, ops

    lib = _lib.load()
    for shape in all_shapes():
        Cin, N, KW = shape
        for M in (1, 99, 788, 2158, 4771, 9090, 10755, 17170, 20200, 36900, 64640):
            L = launches(M, shape)
            assert 1 <= len(L) <= 2 and sum(l[7] for l in L) == M and all(l[:7] in FORMS for l in L), (shape, M, L)
            o = (ctypes.c_int32 * 8)()
            if lib.ns_plan_gemm(M, N, Cin, KW, o):
                want = [(o[0], o[1], o[6], o[2])] + ([(o[3], o[4], o[6], o[5])] if o[5] else [])
                assert [(l[0], l[1], l[4], l[7]) for l in L] == want, (shape, M, L, list(o))
    assert ops.plan_gemm_launches(0, 256, 256) == () and ops.plan_gemm_launches(100, 256, 256, 1, 3) == ()
    assert ops.plan_gemm_launches(100, 256, 72) == ()          # Cin % 16 != 0: the dispatch refuses the shape
    assert ops.plan_gemm_launches(100, 768, 256, 1, 1) == ()   # no full-row tile at 768 columns
    assert ops.plan_gemm_launches(6400, 512, 512, 1, 2) == ()  # beyond the ticketed ladder (conv_gemm_ticket_ok)
    assert lib.ns_plan_gemm_launches(100, 256, 256, 1, 0, None) == 1  # out may be null
    # full-row heights are ns_plan_row_tile's
    for M in (6369, 9090, 17170, 25000, 64640):
        for N in (256, 512):
            (l,) = ops.plan_gemm_launches(M, N, 1024, 1, 1)
            assert l[0] == lib.ns_plan_row_tile_k(M, N, 1024) and l[1] == N and l[5] == 1 and l[7] == M


@pytest.mark.parametrize("name,config,Bn,Sn,forms,utts", GEMM_CASES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_gemm_cases_take_their_forms(name, config, Bn, Sn, forms, utts):
    shape = shape_of(name, config)
    L = launches(Bn * Sn, shape)
    assert [l[:7] for l in L] == forms, "a threshold of the dispatch moved: pick a size that takes this form again"
    assert Bn >= 3 and (shape[2] != 9 or Sn >= 12 or forms == [_f(32, 32, ks=8)])
    assert L[-1][7] % L[-1][0] != 0, "the last row tile must be partial"
    if utts is not None:  # the reference's utterances: the first, and every one the last launch's rows touch
        first_row = Bn * Sn - L[-1][7]
        assert utts[0] == 0 and utts[1:] == list(range(first_row // Sn, Bn))


@pytest.mark.parametrize("op,config,Bn,Sn,form", LN_CASES, ids=str)
def test_layernorm_cases_take_their_forms(op, config, Bn, Sn, form):
    d = D_MODEL[config]
    M = Bn * Sn
    (l,) = launches(M, (d if op == "mha" else D_INNER, d, 1), ln_epi(M))
    assert l[:7] == form, "a threshold of the dispatch moved: pick a size that takes this form again"
    assert M % form[0] != 0 and len(set(_lens(Bn, Sn))) == Bn and max(_lens(Bn, Sn)) == Sn and Bn >= 3


def test_every_form_is_a_case_or_unreached():
    seen = {f for c in GEMM_CASES for f in c[4]} | {c[4] for c in LN_CASES}
    assert seen | set(UNREACHED) == FORMS, (sorted(FORMS - seen - set(UNREACHED)), sorted((seen | set(UNREACHED)) - FORMS))
    assert not seen & set(UNREACHED)
    reached = set(scan())
    assert reached <= FORMS, sorted(reached - FORMS)  # the enumeration above misses nothing the dispatch can name
    assert not reached & set(UNREACHED), sorted(reached & set(UNREACHED))
    assert reached == seen, (sorted(reached - seen), sorted(seen - reached))
    family = set(PLANNER32 + F16W + F16N + FULL_ROW)
    assert set(UNREACHED) & family == PLANNER_FAMILY_UNREACHED
    assert not set(UNREACHED) & set(FULL_ROW)
    # every unreached planner-family form but 256 x 256 IS a matter of width: a 384-column output takes one of them
    assert any(l[:7] == _f(96, 128, mf=16) for M in range(6000, 9000) for l in launches(M, (256, 384, 9)))
    # long contractions on every 32-row planner tile with room, both 16-row lists at s <= 8, a cut, and the sequential K = 512
    long_k = {f for c in GEMM_CASES for f in c[4] if shape_of(c[0], c[1])[0] * shape_of(c[0], c[1])[2] > 512}
    assert {_f(128, 256), _f(64, 256), _f(64, 128), _f(64, 64), _f(32, 128)} <= long_k
    assert any(f in long_k for f in F16W[:6]) and any(f in long_k for f in F16N[:6])
    assert any(len(c[4]) == 2 for c in LONG_K_CASES)
    assert any(shape_of(c[0], c[1])[0] == 512 and shape_of(c[0], c[1])[2] == 1 and c[4][0][0] * c[4][0][1] // (64 * 16) > 32 for c in LONG_K_CASES)


def test_cases_are_the_smallest():
    """CASES is what the scan gives: per form the shortest K that reaches it, then the smallest M = 3 S with S >= 12 and a partial
    last row tile"""
    best = {}
    for shape in all_shapes():
        Cin, N, KW = shape
        for M in range(36, SCAN_ROWS + 1, 3):
            L = launches(M, shape)
            if L[-1][7] % L[-1][0] == 0:
                continue
            for l in L:
                key = (KW * Cin, M)
                if l[:7] not in best or key < best[l[:7]][0]:
                    best[l[:7]] = (key, [x[:7] for x in L])
    got = {}
    for name, config, Bn, Sn, forms in CASES:
        assert Bn == 3
        shape = shape_of(name, config)
        for f in forms:
            got.setdefault(f, ((shape[0] * shape[2], Bn * Sn), forms))  # (which of two shapes with one K: either)
    assert got == best
    for c in ("tiny", "ljspeech", "tiny512", "d512"):
        assert any(case[1] == c for case in GEMM_CASES) and any(case[1] == c for case in LN_CASES)
