"""The case tables of tests/test_gpu_packed_ops.py proven on the CPU (no GPU): which launch form every case takes — asked of the
dispatch itself through ns_plan_attention_packed and ns_plan_gemm_launches — and the float64 / numpy restatements of
tests/packed_cpu.py held against the wrong versions a packed kernel could plausibly be.

Packed rows (csrc/kernels.h RowMap) are the default layout of the synchronous forwards.  What is specific to them, per stage:
the GEMM's tap window comes from row_t / row_w (row m - 1 may be another utterance's last frame), the LayerNorm mask from row_b /
row_t, attention has three launch forms of its own (strips on packed rows; the flat work list; the work list with key ranges and
a merge launch), and the plan / gather / unpack kernels exist only here.

Length sets (SETS): the last utterance is a copy of the first in content and length and starts at a row that is no multiple of 16,
32 or 48, so its tiles are cut differently and its bits must still be the first's.  dec256 / dec64 are the decoder's guard 20
(windows 128, 129, 32, 20, 256 == T, 128 and 64 == T, 21, 20, 64), pho33 the phoneme guard 2, dec1300 one long utterance pair beside
short ones (the work list), dec1300x7 6532 rows (the full-row LayerNorm tile starts at 6369), dec1300x12 13 057 rows (the bf16 mode's
64 x 256 LayerNorm tile starts at 12 737).

Mutants, each evaluated in float64 so that its only error is the mutation (measured here, run with -s): a tap leaking one row
across a window edge is 1.7e7 ... 5.3e7 x the fp32 bound with the four rows beyond the edge at 1e3, in either direction (2.2e4 ... 1.3e5 x on plain
N(0, 1) rows; torch's fp32 on the CPU 0.015 ... 0.04 x); keys masked at the window instead of the length move a valid row by 1e-2 or more against the gate of 2e-5 and turn
the zero-length utterance's NaN rows finite; the unclamped window, the reversed tie order and the moved unpack boundaries
(len + 9, T - 9) each change at least one int / frame exactly."""
import ctypes

import numpy as np
import pytest
import torch

import tests.test_fp32_ops_host as T
from tests import bf16_emu as E
from tests import packed_cpu as PC

_f = T._f
REL = E.FP32_REL
PACK_GUARD, PHONEME_GUARD = 20, 2

# name -> (S, lens, guard)
SETS = {
    "dec256": (256, [108, 109, 12, 0, 236, 108], PACK_GUARD),
    "dec64": (64, [44, 1, 0, 44], PACK_GUARD),
    "pho33": (33, [30, 31, 1, 0, 30], PHONEME_GUARD),
    "dec1300": (1300, [1270, 37, 0, 1270], PACK_GUARD),
    "dec1300x7": (1300, [1270, 37, 0, 1275, 1260, 1300, 1270], PACK_GUARD),
    "dec1300x12": (1300, [1270, 37, 0] + [1280] * 8 + [1270], PACK_GUARD),
}
# plans alone: B = 1, equal windows (ties), a negative length, lengths above S (and within the guard of it), B past one wave
PLAN_CASES = [(s, l, g, 2) for s, l, g in SETS.values()] + [
    (50, [7], 20, 2), (50, [50], 20, 2), (300, [100, 100, 100, 228, 100], 20, 2), (40, [-3, 5, 41, 1000, 21, 20, 19], 20, 8),
    (33, [31, 32, 33, 34, 0, -1], 2, 2), (700, list(range(0, 660, 10)) + [5], 20, 2), (16, [3, 3], 20, 4)]


def plan_of(name, H=2):
    S, lens, guard = SETS[name]
    return PC.plan_ref(lens, S, H, guard)


def layer(name):
    return ("txt_encoder" if name == "pho33" else "mel_decoder") + ".layer_stack.0"


# ---------------------------------------------------------------------------------------------------- the sets and the plan
def test_length_sets_are_what_the_cases_need():
    assert list(plan_of("dec256").win) == [128, 129, 32, 20, 256, 128] and list(plan_of("dec64").win) == [64, 21, 20, 64]
    assert list(plan_of("pho33").win) == [32, 33, 3, 2, 32]
    for name, (S, lens, guard) in SETS.items():
        p = plan_of(name)
        assert lens[-1] == lens[0] and all(int(p.off[-2]) % k for k in (16, 32, 48)), name
        assert 0 in lens and any(w % 32 for w in p.win), name                       # a zero length, a ragged window
        assert S in p.win or name == "dec1300", name                                # a window that is the whole axis
        assert p.Mp * 10 <= p.B * S * 9 or name == "dec1300x7"                      # (a saving the forwards would pack for)
    assert plan_of("dec1300x7").Mp == 6532 >= 6369


def test_plan_reference_by_hand():
    p = PC.plan_ref([5, 0, 5, 30], 40, 2, 20)
    assert list(p.win) == [25, 20, 25, 40] and list(p.off) == [0, 25, 45, 70, 110]
    assert list(p.att_order) == [3, 0, 2, 1] and list(p.att_off) == [0, 2, 4, 6, 8]
    assert list(p.row_b[23:27]) == [0, 0, 1, 1] and list(p.row_t[23:27]) == [23, 24, 0, 1] and list(p.row_w[23:27]) == [25, 25, 20, 20]
    assert list(p.ints(-7)[:5]) == [0, 25, 45, 70, 110] and p.ints(-7)[9] == -7 and p.ints(-7)[19] == -7 and len(p.ints()) == 4 * 4 + 4 + 3 * 110
    q = PC.plan_ref([200, 100], 300, 3, 20)
    assert list(q.att_off) == [0, 6, 9] and q.att_wgs == 9


@pytest.mark.parametrize("S,lens,guard,H", PLAN_CASES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_host_row_counts_equal_the_reference(S, lens, guard, H):
    """Mp and att_wgs as ns_op_pack_plan computes them on the host (the forwards' own helpers) against the restatement"""
    from smart_nar_fast_tts_amd import ops

    p, got = PC.plan_ref(lens, S, H, guard), ops.pack_plan(lens, S, H, guard)
    assert (got.Mp, got.att_wgs, got.plan) == (p.Mp, p.att_wgs, None)
    assert ops.pack_plan_ints(p.B, p.Mp) == len(p.ints())


def test_plan_cases_cover_the_edges():
    flat = [(S, l, g) for S, l, g, _ in PLAN_CASES]
    assert any(len(l) == 1 for _, l, _ in flat) and any(min(l) < 0 for _, l, _ in flat) and any(max(l) > S for S, l, _ in flat)
    assert any(len(l) > 64 for _, l, _ in flat)
    ties = [c for c in PLAN_CASES if len(set(PC.plan_ref(c[1], c[0], c[3], c[2]).win)) < len(c[1])]
    assert ties
    # the wrong versions differ on these very cases
    assert any(not np.array_equal(PC.plan_ref(l, S, H, g).ints(), PC.plan_ref(l, S, H, g, ties_by_index=False).ints()) for S, l, g, H in ties)
    for S, l, g, H in PLAN_CASES:
        if max(l) + g > S:
            bad = PC.plan_ref(l, S, H, g, clamp=False)
            assert bad.Mp != PC.plan_ref(l, S, H, g).Mp and max(bad.win) > S
    # ties the other way: same windows and offsets, another work list — only att_order tells
    a, b = PC.plan_ref([5, 5, 9], 40, 2, 20), PC.plan_ref([5, 5, 9], 40, 2, 20, ties_by_index=False)
    assert list(a.att_order) == [2, 0, 1] and list(b.att_order) == [2, 1, 0] and np.array_equal(a.off, b.off) and np.array_equal(a.att_off, b.att_off)


# ---------------------------------------------------------------------------------------------------- attention forms
STRIPS, LIST, LIST_SPLIT = "strips", "work list", "work list + merge"
# (set, split scratch, tickets, form, key ranges > 1, merge launch)
ATT_CASES = [
    ("pho33", True, True, STRIPS, False, 0),
    ("dec64", True, True, STRIPS, False, 0),
    ("dec256", True, True, STRIPS, True, 0),     # two key-range workgroups per strip, merged by the last arriver
    ("dec256", True, False, STRIPS, True, 1),    # ... by k_attention_merge
    ("dec256", False, False, STRIPS, False, 0),
    ("dec1300", False, False, LIST, False, 0),
    ("dec1300", True, True, LIST_SPLIT, True, 1),
]
ATT_DK = [128, 64, 32]
ATT_H = 2


def att_plan(name, dk, split, tickets):
    from smart_nar_fast_tts_amd import ops

    S, lens, guard = SETS[name]
    p = ops.pack_plan(lens, S, ATT_H, guard)
    _, part, tk = ops.attention_packed_scratch(p, dk, split, tickets)
    return ops.plan_attention_packed(p.B, S, ATT_H, dk, p.att_wgs, p.Mp, part, tk)


@pytest.mark.parametrize("dk", ATT_DK)
@pytest.mark.parametrize("name,split,tickets,form,ranges,merge", ATT_CASES)
def test_attention_cases_take_their_forms(name, split, tickets, form, ranges, merge, dk):
    f, nsplit, mg, tiles = att_plan(name, dk, split, tickets)
    got = STRIPS if f == 0 else (LIST_SPLIT if nsplit > 1 else LIST)
    assert (got, nsplit > 1, mg) == (form, ranges, merge), "a threshold of launch_attention moved: pick a size that takes this form again"
    assert tiles >= 1 and (f == 1 or tiles <= 4)


def test_every_packed_attention_form_is_reached():
    """a form counts only with a case in which some key range owns no valid tile and a case with a window that is no multiple of 32"""
    for form in (STRIPS, LIST, LIST_SPLIT):
        empty = ragged = False
        for name, split, tickets, f, _, _ in ATT_CASES:
            if f != form:
                continue
            p = plan_of(name, ATT_H)
            for dk in ATT_DK:
                fm, nsplit, _, _ = att_plan(name, dk, split, tickets)
                empty |= any(e > 0 for _, _, e in PC.key_ranges(p, fm, nsplit))
            ragged |= any(w % 32 for w in p.win)
        assert empty and ragged, form
    # the split work list leaves short utterances with ranges that own nothing (one key tile, eleven ranges), not only the empty one
    fm, nsplit, _, _ = att_plan("dec1300", 128, True, True)
    kr = PC.key_ranges(plan_of("dec1300"), fm, nsplit)
    assert kr[1][0] == 2 and kr[1][2] == nsplit - 2 and kr[2][2] == nsplit
    assert kr[0][:2] == (40, 4) and kr[0][2] == nsplit - 10  # (1270 keys: 40 tiles in ranges of ceil(40 / 11) = 4 — the last range owns none)


def test_plan_attention_packed_refuses_bad_arguments():
    from smart_nar_fast_tts_amd import _lib

    lib = _lib.load()
    o = (ctypes.c_int32 * 4)()
    for args in ((0, 64, 2, 128, 8, 100), (4, 0, 2, 128, 8, 100), (4, 64, 2, 48, 8, 100), (4, 64, 2, 128, 0, 100), (4, 64, 2, 128, 8, 0)):
        assert lib.ns_plan_attention_packed(*args, 0, 0, o) != 0 and lib.ns_last_error()
    assert lib.ns_plan_attention_packed(4, 64, 2, 128, 8, 100, 0, 0, None) != 0


def test_packed_entries_refuse_bad_arguments_before_any_device_work():
    """null pointers and inconsistent shapes are refused on a machine without a GPU: nothing was launched"""
    from smart_nar_fast_tts_amd import _lib

    lib = _lib.load()
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: every call below is refused first)
    mp, wg = ctypes.c_int32(0), ctypes.c_int32(0)
    host = torch.tensor([5, 7])
    assert lib.ns_op_pack_plan(nul, nul, 2, 40, 2, 20, nul, 0, ctypes.byref(mp), ctypes.byref(wg), nul) != 0
    assert lib.ns_op_pack_plan(nul, _lib.ptr(host), 2, 40, 2, 0, nul, 0, ctypes.byref(mp), ctypes.byref(wg), nul) != 0
    assert lib.ns_op_pack_plan(one, _lib.ptr(host), 2, 40, 2, 20, nul, 0, ctypes.byref(mp), ctypes.byref(wg), nul) != 0   # lens_dev without a plan
    assert lib.ns_op_pack_plan(one, _lib.ptr(host), 2, 40, 2, 20, one, 10, ctypes.byref(mp), ctypes.byref(wg), nul) != 0  # plan too small
    assert (mp.value, wg.value) == (52, 4)
    assert lib.ns_op_gemm_packed(nul, b"mel_linear", one, one, 2, 40, 52, 4, one, nul) != 0
    assert lib.ns_op_attention_core_packed(nul, one, one, 2, 40, 52, 4, 2, 128, one, nul, 0, nul, 0) != 0
    assert lib.ns_op_attention_core_packed(one, one, nul, 2, 40, 52, 4, 2, 128, one, nul, 0, nul, 0) != 0
    assert lib.ns_op_attention_core_packed(one, one, one, 2, 40, 81, 4, 2, 128, one, nul, 0, nul, 0) != 0   # Mp > B * S
    assert lib.ns_op_attention_core_packed(one, one, one, 2, 40, 52, 4, 2, 96, one, nul, 0, nul, 0) != 0
    assert lib.ns_op_attention_core_packed(one, one, one, 2, 40, 52, 4, 2, 128, one, nul, 0, nul, 4) != 0
    assert lib.ns_op_block_packed(nul, 0, b"mel_decoder.layer_stack.0", one, one, one, 2, 40, 52, 4, 0, one, one, 0, nul) != 0
    assert lib.ns_op_length_regulate_packed(one, one, one, 2, 9, 6, 40, 52, 2, one, nul, one, 1000, nul) != 0   # D % 4
    assert lib.ns_op_length_regulate_packed(one, one, one, 2, 9, 8, 40, 52, 2, one, nul, one, 10, nul) != 0     # plan too small
    assert lib.ns_op_embed_pos_packed(one, one, one, one, 2, 40, 52, 4, 6, 10, one, nul) != 0
    assert lib.ns_op_add_pos_packed(one, one, one, 2, 40, 52, 4, 6, one, nul) != 0
    assert lib.ns_op_pack_vector(nul, one, 2, 40, 52, 4, one, nul) != 0
    assert lib.ns_op_unpack_rows(one, nul, one, 2, 40, 52, 4, 0, one, nul) != 0
    assert lib.ns_op_unpack_phase1(one, one, nul, one, 2, 40, 52, 4, 8, one, one, nul) != 0
    assert lib.ns_op_unpack_outputs(one, 2, 40, 52, 4, 80, one, one, one, nul, nul, one, one, one, one, one, nul, nul, nul) != 0  # p_pred without p_p
    assert lib.ns_op_unpack_outputs(one, 2, 40, 52, 0, 80, one, one, one, nul, nul, one, one, one, one, nul, nul, nul, nul) != 0
    assert lib.ns_last_error()


# ---------------------------------------------------------------------------------------------------- GEMM / LayerNorm forms
_Q, _FC, _W1, _W2 = ".slf_attn.qkv", ".slf_attn.fc", ".pos_ffn.w_1", ".pos_ffn.w_2"
# (contraction (a layer suffix, mel_linear or a PostNet layer), config, set, the forms of its launches at the set's Mp rows)
GEMM_CASES = [
    (_Q, "tiny", "dec256", [_f(32, 128, ks=2)]), (_FC, "tiny", "dec256", [_f(32, 32, ks=4)]), (_W1, "tiny", "dec256", [_f(32, 128, ks=2)]),
    (_W2, "tiny", "dec256", [_f(32, 32, ks=8)]), ("mel_linear", "tiny", "dec256", [_f(32, 32, ks=4)]),
    ("postnet.convolutions.1", "tiny", "dec256", [_f(32, 64, ks=4)]),
    (_Q, "tiny512", "dec256", [_f(48, 128, ks=2, mf=16)]), (_FC, "tiny512", "dec256", [_f(32, 64, ks=4)]), (_W1, "tiny512", "dec256", [_f(32, 128, ks=2)]),
    (_W2, "tiny512", "dec256", [_f(32, 64, ks=4)]), ("mel_linear", "tiny512", "dec256", [_f(32, 32, ks=8)]),
    ("postnet.convolutions.1", "tiny512", "dec256", [_f(32, 64, ks=4)]),
    (_Q, "tiny", "dec64", [_f(32, 32, ks=4)]), (_FC, "tiny", "dec64", [_f(32, 32, ks=4)]), (_W1, "tiny", "dec64", [_f(32, 32, ks=8)]),
    (_W2, "tiny", "dec64", [_f(32, 32, ks=8)]), ("mel_linear", "tiny", "dec64", [_f(32, 32, ks=4)]),
    ("postnet.convolutions.1", "tiny", "dec64", [_f(32, 32, ks=8)]), ("postnet.convolutions.0", "tiny", "dec64", [_f(32, 32, bk=16, ks=4)]),
    (_Q, "tiny", "pho33", [_f(32, 32, ks=4)]), (_FC, "tiny", "pho33", [_f(32, 32, ks=4)]), (_W1, "tiny", "pho33", [_f(32, 32, ks=8)]),
    (_W2, "tiny", "pho33", [_f(32, 32, ks=8)]),
    (_FC, "tiny", "dec1300", [_f(48, 64, ks=4, mf=16)]), (_W1, "tiny", "dec1300", [_f(48, 256, mf=16)]),
    ("postnet.convolutions.0", "tiny", "dec1300", [_f(64, 64, bk=16)]), (_Q, "tiny512", "dec1300", [_f(64, 128)]),
    (_Q, "tiny", "dec1300x7", [_f(80, 256, mf=16)]), ("postnet.convolutions.4", "tiny", "dec1300x7", [_f(32, 96, ks=4)]),
    # the two-launch cut plan (gemm_conv.hip row_range: X / Y shifted, the row maps read at m + m_base): 12 288 rows + 769; the cut
    # falls INSIDE the last window, the copy of utterance 0, whose rows on both sides of it must carry utterance 0's bits
    (_W1, "tiny", "dec1300x12", [_f(64, 256), _f(64, 64)]), (_W1, "tiny512", "dec1300x12", [_f(64, 256), _f(64, 64)]),
]
# (op, config, set, row_epilogue, form of the LayerNorm launch): "mha" = fc + LayerNorm, "ffn" = w_2 + LayerNorm, each through the
# packed block entry; "two_launch" = the plain GEMM followed by k_layernorm with the row maps
_T1, _T2 = dict(ticket=1), dict(ticket=2)
LN_CASES = [
    ("mha", "tiny", "dec256", "fused", _f(32, 32, ks=4, **_T1)), ("ffn", "tiny", "dec256", "fused", _f(32, 32, ks=8, **_T1)),
    ("mha", "tiny", "dec64", "fused", _f(32, 32, ks=4, **_T1)), ("ffn", "tiny", "dec64", "fused", _f(32, 32, ks=8, **_T1)),
    ("mha", "tiny", "pho33", "fused", _f(32, 32, ks=4, **_T1)), ("ffn", "tiny", "pho33", "fused", _f(32, 32, ks=8, **_T1)),
    ("mha", "tiny", "dec1300", "fused", _f(48, 64, ks=4, mf=16, **_T1)), ("ffn", "tiny", "dec1300", "fused", _f(48, 64, ks=4, mf=16, **_T1)),
    ("mha", "tiny", "dec1300x7", "fused", _f(32, 256, rowepi=1)), ("ffn", "tiny", "dec1300x7", "fused", _f(32, 256, rowepi=1)),
    ("mha", "tiny512", "dec256", "fused", _f(32, 64, ks=4, **_T2)), ("ffn", "tiny512", "dec256", "fused", _f(32, 64, ks=4, **_T2)),
    ("mha", "tiny512", "dec1300", "fused", _f(32, 128, ks=2, **_T2)), ("ffn", "tiny512", "dec1300", "fused", _f(32, 128, ks=2, **_T2)),
    ("ffn", "tiny512", "dec1300x7", "fused", _f(32, 512, rowepi=1)),
    ("mha", "tiny", "dec256", "two_launch", _f(32, 32, ks=4)), ("ffn", "tiny", "dec256", "two_launch", _f(32, 32, ks=8)),
]
# fft block (both LayerNorms masked): one case per mask implementation — ticketed ladder, full-row tile, k_layernorm
MASKED_CASES = [("tiny", "dec256", "fused"), ("tiny", "pho33", "fused"), ("tiny512", "dec256", "fused"), ("tiny", "dec1300x7", "fused"),
                ("tiny", "dec256", "two_launch")]
# the listed forms that no case reaches at these row counts, and why: none.  (The k = 5 PostNet layers cut only from 21 505 rows; their
# cut goes through the same row_range() as w_1's, which the dec1300x12 cases run.)
UNREACHED = {}


def gemm_name(suffix, set_name):
    return suffix if suffix.startswith(("mel_linear", "postnet.")) else layer(set_name) + suffix


@pytest.mark.parametrize("suffix,config,set_name,forms", GEMM_CASES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_gemm_cases_take_their_forms(suffix, config, set_name, forms):
    Mp = plan_of(set_name).Mp
    L = T.launches(Mp, T.shape_of(gemm_name(suffix, set_name), config))
    assert [l[:7] for l in L] == forms, "a threshold of the dispatch moved: pick a set that takes this form again"
    assert L[-1][7] % L[-1][0] != 0, "the last row tile must be partial"


@pytest.mark.parametrize("op,config,set_name,mode,form", LN_CASES, ids=str)
def test_layernorm_cases_take_their_forms(op, config, set_name, mode, form):
    d, Mp = T.D_MODEL[config], plan_of(set_name).Mp
    (l,) = T.launches(Mp, (d if op == "mha" else T.D_INNER, d, 1), 0 if mode == "two_launch" else T.ln_epi(Mp))
    assert l[:7] == form and Mp % form[0] != 0


BF16_LN_CASES = [("ffn", "dec256", False), ("mha", "dec256", False), ("ffn", "dec1300x12", True), ("mha", "dec1300x12", True)]  # (op, set, full-row tile)


def test_bf16_layernorm_cases_take_their_forms():
    """bf16 mode: the plain bf16 GEMM + k_layernorm on the row maps below 12 737 rows, the 64 x 256 LayerNorm tile from there"""
    from smart_nar_fast_tts_amd import ops

    for op, set_name, full in BF16_LN_CASES:
        assert ops.plan_gemm_bf16_ln(plan_of(set_name).Mp, 256, 1024 if op == "ffn" else 256) == full
    assert not ops.plan_gemm_bf16_ln(12736, 256, 1024) and ops.plan_gemm_bf16_ln(12737, 256, 1024) and plan_of("dec1300x12").Mp % 64


def test_listed_forms_are_reached_or_unreached_with_a_reason():
    plain = {f for c in GEMM_CASES for f in c[3]}
    assert any(f[0] == 32 and f[4] == 32 and f[5] == 0 for f in plain)                         # a plain 32-row rung
    assert any(f[0] == 48 and f[4] == 16 and f[3] > 1 for f in plain)                          # the 48-row MF16 rung
    assert any(f[3] > 1 for f in plain) and any(f[3] == 1 for f in plain)                      # KS > 1, and a planner tile
    assert any(f[2] == 16 for f in plain) and any(f[1] == 96 for f in plain)                   # BK 16 (K = 400), the 80-column tail
    ln = {(c[3], c[4]) for c in LN_CASES}
    assert any(f[5] == 1 and f[1] == 256 for _, f in ln) and any(f[5] == 1 and f[1] == 512 for _, f in ln)   # the full-row LN tile
    assert any(f[6] == 1 for _, f in ln) and any(f[6] == 2 for _, f in ln)                     # the ticketed ladder, both widths
    assert any(m == "two_launch" and f[5] == 0 and f[6] == 0 for m, f in ln)                   # the two-launch LN form
    assert not UNREACHED
    cuts = [(n, c, s) for n, c, s, f in GEMM_CASES if len(f) == 2]                             # a two-launch cut plan
    assert cuts and min(M for M in range(1, 12000) if len(T.launches(M, (256, 1024, 9))) == 2) == 10753  # (the smallest cut of any shape)
    for n, c, s in cuts:  # the cut falls strictly inside the last window (the copy of utterance 0), and k = 9 taps cross it
        p, cut = plan_of(s), T.launches(plan_of(s).Mp, T.shape_of(gemm_name(n, s), c))[0][7]
        assert int(p.off[-2]) + 4 < cut < p.Mp - 4 and T.shape_of(gemm_name(n, s), c)[2] == 9
    for k in (9, 5):  # taps of both kernel widths cross window edges in some case
        assert any(T.shape_of(gemm_name(n, s), c)[2] == k for n, c, s, _ in GEMM_CASES)
    masked = {(c, m) for c, _, m in MASKED_CASES}
    assert ("tiny", "two_launch") in masked and any(T.ln_epi(plan_of(s).Mp) == 1 for _, s, _ in MASKED_CASES)


# ---------------------------------------------------------------------------------------------------- inputs shared with the GPU tests
def x_packed(p, C, seed, spike=None, side="tail"):
    """N(0, 1) packed rows [Mp, C], the last window a copy of the first; spike: four rows (the reach of a k = 9 tap) on ONE side of
    every window edge are set to that value — side "tail": the last rows of every window, read by a tap that leaks backwards out
    of the next window; "head": the first rows of every window, read by a tap that leaks forwards out of the previous one.  The
    rows on the other side of the edge stay N(0, 1), so the leaked value stands 1e3 above everything they may read."""
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal((p.Mp, C)).astype(np.float32))
    if spike is not None:
        for b in range(p.B):
            lo, hi = int(p.off[b]), int(p.off[b + 1])
            if side == "tail":
                x[max(hi - 4, lo):hi] = spike
            else:
                x[lo:min(lo + 4, hi)] = spike
    x[int(p.off[-2]):] = x[:int(p.win[0])]
    return x


# ---------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("Cin,N,KW", [(256, 1024, 9), (512, 512, 5), (80, 512, 5)])
@pytest.mark.parametrize("set_name", ["dec256", "pho33"])
def test_packed_contraction_rejects_a_leaked_tap(Cin, N, KW, set_name):
    p = plan_of(set_name)
    g = torch.Generator().manual_seed(Cin + N + KW)
    w, b = torch.randn(N, Cin, KW, generator=g), torch.randn(N, generator=g)
    for spike, side in ((None, "tail"), (1e3, "tail"), (1e3, "head")):
        x = x_packed(p, Cin, 5, spike, side)
        ref, unit = PC.gemm_packed_ref(x, w, b, p), PC.gemm_packed_unit(x, w, b, p)
        good = PC.gemm_packed_check(PC.gemm_packed_ref(x, w, b, p, dtype=torch.float32), x, w, b, p, ref=ref, unit=unit)
        bad = PC.gemm_packed_check(PC.conv_packed(x, w, b, p, leak=1), x, w, b, p, ref=ref, unit=unit)
        print(f"\n{set_name} Cin={Cin} N={N} KW={KW} spike={spike} {side}: fp32 CPU {good.worst:.3g} x bound, one leaked row {bad.worst:.3g} x")
        assert good.ok and good.worst < 0.1 and not bad.ok and bad.worst > (1e5 if spike else 1e3)
        # the copy of utterance 0 carries utterance 0's values exactly in the reference, and not with a leak
        assert torch.equal(ref[int(p.off[-2]):], ref[:int(p.win[0])])
        leaked = PC.conv_packed(x, w, b, p, leak=1)
        assert not torch.equal(leaked[int(p.off[-2]):], leaked[:int(p.win[0])])
    # the reference IS the per-utterance convolution of the padded grid where the grid has the rows
    xg = torch.zeros(p.B, p.S, Cin)
    for u, xw in enumerate(PC.windows(x, p)):
        xg[u, :xw.shape[0]] = xw
    full = [u for u in range(p.B) if p.win[u] == p.S]
    assert full and all(torch.equal(E.conv_rows(xg, w, b)[u], PC.windows(ref, p)[u]) for u in full)


@pytest.mark.parametrize("dk", ATT_DK)
@pytest.mark.parametrize("set_name", ["dec256", "pho33"])
def test_packed_attention_rejects_keys_masked_at_the_window(set_name, dk):
    p = plan_of(set_name, ATT_H)
    torch.manual_seed(dk)
    qkv = torch.randn(p.Mp, 3 * ATT_H * dk)
    ref, bad = PC.attention_packed_ref(qkv, p, ATT_H), PC.attention_packed_ref(qkv, p, ATT_H, keys_at_win=True)
    nan_rows = torch.isnan(ref).any(dim=1)
    zero_len = torch.from_numpy(np.asarray(p.lens)[p.row_b] <= 0)
    assert torch.equal(nan_rows, zero_len) and bool(nan_rows.any()) and bool(torch.isnan(ref[nan_rows]).all())
    assert bool(torch.isfinite(bad).all())                                     # the mutant fills the NaN rows
    short = torch.from_numpy((p.keys() < p.win)[p.row_b]) & ~nan_rows
    assert float((bad - ref).abs()[short].max()) > 1e-2 > 2e-5                 # ... and moves every utterance with guard rows
    fp32 = PC.attention_packed_ref(qkv, p, ATT_H, dtype=torch.float32)
    assert float((fp32.double() - ref).abs()[~nan_rows].max()) < 2e-6


def outputs_case(T_len=64, n_mel=80, lens=(30, 44, 33, 0, 64, 45, -2, 30), seed=3):
    """mel lengths with w == T (44 .. 64, also through the guard: 45), w < T with frames in all three PostNet regions (30: packed
    rows up to t = 39, deep padding 40 .. 53, the end of the axis from 54; 33: window 53, T - 11 = 53 is the last deep-padding
    frame), a zero and a negative length; every packed value distinct"""
    p = PC.plan_ref(list(lens), T_len, 2, PACK_GUARD)
    rs = np.random.RandomState(seed)
    v = rs.permutation(2 * p.Mp * n_mel + 2 * p.Mp + 12 * n_mel).astype(np.float32) + 1.0
    cut = np.cumsum([p.Mp * n_mel, p.Mp * n_mel, p.Mp, p.Mp, n_mel])
    mel_p, post_p, p_p, e_p, bias, const = np.split(v, cut)
    f = torch.from_numpy
    return p, torch.tensor(list(lens)), f(mel_p.reshape(p.Mp, n_mel)), f(post_p.reshape(p.Mp, n_mel)), f(p_p), f(e_p), f(bias), f(const.reshape(11, n_mel))


def test_unpack_outputs_reference_and_its_boundaries():
    p, lens, mel_p, post_p, p_p, e_p, bias, const = outputs_case()
    mel, post, pp, ep, mask = PC.unpack_outputs_ref(p, lens, mel_p, post_p, p_p, e_p, bias, const)
    T_len = p.S
    assert T_len in p.win and any(w < T_len for w in p.win)
    b = 0  # len 30, window 50
    o = int(p.off[b])
    assert torch.equal(post[b, 39], post_p[o + 39]) and torch.equal(post[b, 40], const[0])          # t = len + 9 | len + 10
    assert torch.equal(post[b, T_len - 11], const[0]) and torch.equal(post[b, T_len - 10], const[1])  # t = T - 11 | T - 10
    assert torch.equal(post[b, T_len - 1], const[10])
    assert torch.equal(mel[b, 49], mel_p[o + 49]) and torch.equal(mel[b, 50], bias) and pp[b, 49] == p_p[o + 49] and pp[b, 50] == 0
    assert list(mask[b, 29:31]) == [0, 1] and bool(mask[3].all()) and bool(mask[6].all()) and not bool(mask[4].any())
    for u in range(p.B):
        if p.win[u] == T_len:  # the whole axis: every frame is the packed row
            assert torch.equal(post[u], post_p[int(p.off[u]):int(p.off[u + 1])]) and torch.equal(mel[u], mel_p[int(p.off[u]):int(p.off[u + 1])])
    assert torch.equal(post[3, :10], post_p[int(p.off[3]):int(p.off[3]) + 10]) and torch.equal(post[3, 10], const[0])   # zero length
    assert torch.equal(post[6, :10], post_p[int(p.off[6]):int(p.off[6]) + 10]) and torch.equal(post[6, 10], const[0])   # negative length
    # the boundaries moved by one are other outputs, at exactly the frames next to them
    for kw, frames in ((dict(d_len=-1), {39}), (dict(d_end=1), set(range(T_len - 10, T_len)))):
        bad = PC.unpack_outputs_ref(p, lens, mel_p, post_p, p_p, e_p, bias, const, **kw)[1]
        diff = {int(t) for t in torch.nonzero((bad[b] != post[b]).any(dim=1)).flatten()}
        assert diff == frames, (kw, diff)
    assert PC.unpack_outputs_ref(p, lens, mel_p, post_p, None, None, bias, const)[2:4] == (None, None)


def test_data_movement_references_by_hand():
    p = PC.plan_ref([2, 0, 5], 6, 1, 2)  # windows 4, 2, 6
    assert list(p.win) == [4, 2, 6] and p.Mp == 12
    src = torch.arange(18, dtype=torch.float32).reshape(3, 6)
    v = PC.pack_vector_ref(src, p)
    assert v.tolist() == [0, 1, 2, 3, 6, 7, 12, 13, 14, 15, 16, 17]
    rows_p = torch.arange(24, dtype=torch.float32).reshape(12, 2) + 1
    lens = torch.tensor([2, 0, 5])
    u = PC.unpack_rows_ref(rows_p, lens, p)
    assert torch.equal(u[0, :2], rows_p[:2]) and not bool(u[0, 2:].any()) and not bool(u[1].any()) and torch.equal(u[2, :5], rows_p[6:11]) and not bool(u[2, 5].any())
    r, vec = PC.unpack_phase1_ref(rows_p, v + 1, lens, p)
    assert torch.equal(r[0, :4], rows_p[:4]) and not bool(r[0, 4:].any()) and torch.equal(r[1, :2], rows_p[4:6]) and torch.equal(r[2], rows_p[6:])
    assert vec[0].tolist() == [1, 2, 0, 0, 0, 0] and not bool(vec[1].any()) and vec[2].tolist() == [13, 14, 15, 16, 17, 0]
    assert torch.equal(PC.pack_rows(src[:, :, None], p)[:, 0], v)
    # length regulator: durations 2, 0, 3 -> rows 0 0 2 2 2, a window of 4 + zeros
    x = torch.arange(9, dtype=torch.float32).reshape(1, 3, 3) + 1
    q = PC.plan_ref([5], 8, 1, 2)
    out, status = PC.length_regulate_packed_ref(x, torch.tensor([[2, 2, 5]], dtype=torch.int32), [5], 8, q)
    assert out[:, 0].tolist() == [1, 1, 7, 7, 7, 0, 0] and status.tolist() == [0]
    assert PC.length_regulate_packed_ref(x, torch.tensor([[2, 2, 9]], dtype=torch.int32), [-1], 8, PC.plan_ref([-1], 8, 1, 2))[1].tolist() == [3]
    emb, pos = torch.arange(8, dtype=torch.float32).reshape(4, 2), torch.arange(16, dtype=torch.float32).reshape(8, 2) * 100
    e = PC.embed_pos_packed_ref(torch.tensor([[3, 9, -1, 1, 0, 0, 0, 0]]), emb, pos, q)
    assert e[:4].tolist() == [[6, 107], [200, 301], [400, 501], [602, 703]]
    assert torch.equal(PC.add_pos_ref(e, pos, q), e + pos[:7])
