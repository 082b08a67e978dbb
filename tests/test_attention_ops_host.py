"""The case table of tests/test_gpu_attention_ops.py proven on the CPU (no GPU): which of the seven dense launch forms every case
takes — asked of the dispatch itself through ns_plan_attention_dense, with exactly the scratch and the ticket flag the op hands to
launch_attention — that the table reaches every form with every edge, that the dispatch lifted into attention_plan_dense still
decides what launch_attention decided inline (tests/attention_cpu.py plan_dense_ref, a sweep over both sides of every threshold),
that k_attention's XCD remap is a bijection, and that the float64 yardstick at the project's gates rejects the wrong versions that
matter.

Forms (csrc/attention.hip, rm == nullptr):
  A  k_attention_strip, one workgroup per 32-query strip      fewer than 128 (query tile, head) blocks, a wave sweeps <= 4 key tiles
  B  strips, 2..8 key-range workgroups, last-arriver merge    as A with scratch and a ticket block
  C  strips, 2..8 key-range workgroups, k_attention_merge     as B without tickets
  D  k_attention, one sweep, fewer than 128 blocks            strips refused (more than 4 tiles per wave), no scratch
  E  k_attention + the small grid's own key split + merge     as D with scratch
  F  k_attention, one sweep, 128 blocks or more               no worthwhile split, or no scratch, or NS_PLAN=0
  G  k_attention + the planner's key split + merge            128 blocks or more whose last round of 256 fills badly

Mutants, each evaluated in float64 on the table's own inputs so that its only error is the mutation; the factor is the worst
error over the cases of a form (rows of utterances that have keys) divided by the gate of 2e-5, the smallest over the forms a mutant
applies to (measured here, run with -s): keys masked at S 7.5e4, mask one key late 3.4e4, scale 1 / d_k 8.6e4, head h + 1's K 1.1e5,
equal merge weights 5.8e4, last partial dropped 1.8e4, first range's l alone 1.2e5, an empty range's l = 1 2.5e3 (torch's fp32 on the
CPU: below 0.25).  Each is required to stay above MUTANT_FACTOR = 1000; a tile never written is the sentinel rule's to catch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attention_cpu as AC

TOL, TOL_SPIKED, TOL_SPLIT_VS_SINGLE = 2e-5, 5e-5, 1e-5  # the gates of tests/test_gpu_attention.py, unchanged
MUTANT_FACTOR = 1000.0
NO, R8, R16 = False, True, 16  # split_scratch of ops.attention_core: none, 8 ranges' worth in all, room for ATT_SPLIT_MAX ranges

_L33 = [129, 128, 127, 97, 96, 95, 65, 64, 63, 33, 32, 31, 1, 0, 200, 130] * 2
# (H, dk, B, S, lens, split_scratch, tickets) -> form.  The last utterance is a copy of the first in content and length.
CASES = [
    (2, 128, 4, 97, [97, 33, 0, 97], R16, True, "A"),
    (4, 32, 5, 290, [290, 300, 64, 63, 290], NO, True, "A"),
    (8, 64, 3, 300, [300, 257, 300], NO, True, "A"),
    (2, 128, 4, 545, [545, 33, 0, 545], R16, True, "B"),
    (4, 32, 5, 290, [290, 300, 64, 63, 290], R16, True, "B"),
    (4, 64, 3, 545, [544, 1000, 544], R16, True, "B"),
    (2, 128, 1, 788, [788], R8, True, "B"),
    (2, 128, 4, 545, [545, 33, 0, 545], R16, False, "C"),
    (4, 32, 5, 290, [290, 300, 64, 63, 290], R16, False, "C"),
    (4, 64, 3, 545, [544, 1000, 544], R16, False, "C"),
    (2, 128, 1, 788, [788], NO, True, "D"),
    (2, 128, 8, 545, [545, 33, 32, 31, 0, 1000, 64, 545], NO, True, "D"),
    (4, 32, 4, 545, [545, 600, 0, 545], NO, True, "D"),
    (2, 32, 1, 1640, [1640], NO, True, "D"),
    (2, 128, 8, 545, [545, 33, 32, 31, 0, 1000, 64, 545], R16, True, "E"),
    (4, 32, 4, 545, [545, 600, 0, 545], R16, True, "E"),
    (2, 32, 1, 1640, [1640], R16, True, "E"),
    (8, 32, 3, 544, [544, 100, 544], R16, False, "E"),
    (4, 32, 11, 300, [300, 33, 32, 31, 0, 400, 257, 129, 96, 1, 300], R16, True, "F"),
    (2, 128, 33, 129, [129] + _L33[1:32] + [129], R16, True, "F"),
    (4, 32, 18, 520, [520, 33, 0, 600] + [500, 385, 384, 383, 96, 7] * 2 + [64, 520], NO, True, "F"),
    (2, 128, 13, 600, [600, 33, 0, 700, 575, 576, 577, 600, 300, 600, 64, 600, 600], NO, True, "F"),
    (2, 128, 13, 600, [600, 33, 0, 700, 575, 576, 577, 600, 300, 600, 64, 600, 600], R16, True, "G"),
    (2, 128, 18, 512, [512, 40, 0, 513] + [480, 200] * 6 + [33, 512], R16, True, "G"),
    (4, 64, 8, 385, [385, 33, 0, 400, 352, 351, 353, 385], R16, True, "G"),
]
FORMS = "ABCDEFG"
SPLIT_FORMS, GRID_FORMS = "BCEG", "DEFG"
# BF = true runs every form once per d_k: one base shape per form (H, B, S, lens, split_scratch, tickets), run at d_k = 128, 64, 32.
# The strip decision does not read d_k (the scratch is sized in ranges), the planner's cost model does: G has a shape of its own
# that splits at all three.
BF16_CASES = {
    "A": (2, 4, 97, [97, 33, 0, 97], R16, True),
    "B": (2, 4, 300, [300, 33, 0, 300], R16, True),
    "C": (2, 4, 300, [300, 33, 0, 300], R16, False),
    "D": (8, 2, 545, [545, 545], NO, True),
    "E": (8, 2, 545, [545, 545], R16, True),
    "F": (2, 33, 129, [129] + _L33[1:32] + [129], R16, True),
    "G": (4, 8, 385, [385, 33, 0, 400, 352, 351, 353, 385], R16, True),
}
DKS = (128, 64, 32)


def case_id(c):
    H, dk, B, S, _, scratch, tickets, form = c
    return f"{form}-H{H}-dk{dk}-B{B}-S{S}-scratch{int(scratch)}-tickets{int(tickets)}"


def plan_case(H, dk, B, S, scratch, tickets):
    """the plan of a case, asked with exactly the partial floats and the ticket flag ops.attention_core hands to launch_attention"""
    from smart_nar_fast_tts_amd import ops

    _, part, has_tk = ops.attention_dense_scratch(B, S, H, dk, scratch, tickets)
    return ops.plan_attention_dense(B, S, H, dk, part, has_tk)


def case_input(c, spiked=False):
    """(qkv, lens) of a case: N(0, 1), the last utterance a copy of the first; spiked: N(0, 0.25) with a dominant key of head 0 in a
    late tile of utterance 0 (its last valid tile but one) and a dominant key of head 1 in the first tile"""
    H, dk, B, S, lens, _, _, _ = c
    seed = 1000 * S + 10 * B + dk + H
    if not spiked:
        return AC.make_qkv(B, S, H, dk, seed), torch.tensor(lens)
    qkv = AC.make_qkv(B, S, H, dk, seed + 1, scale=0.5)
    return AC.spike(qkv, lens, H, late_key=min(lens[0], S) - 40), torch.tensor(lens)


def spiked_case(form):
    """the first case of a form with two heads or more whose first utterance spans three key tiles or more — one with unspiked
    utterances beside the spiked pair (where softmax is all but one-hot and rounds to the dominant key's V row) before a single one"""
    ok = [c for c in CASES if c[7] == form and c[0] >= 2 and min(c[4][0], c[3]) >= 96]
    return next((c for c in ok if c[2] > 2), ok[0])


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_cases_take_their_forms(c):
    H, dk, B, S, lens, scratch, tickets, form = c
    assert len(lens) == B and lens[-1] == lens[0]
    pl = plan_case(H, dk, B, S, scratch, tickets)
    assert AC.form_of(pl, B, S, H) == form, f"a threshold of launch_attention moved ({pl}): pick a shape that takes form {form} again"
    assert pl[3] >= 1 and (pl[0] == AC.GRID or pl[3] <= 4)
    assert tuple(AC.plan_dense_ref(B, S, H, dk, *_handed(c))) == pl


def _handed(c):
    from smart_nar_fast_tts_amd import ops

    H, dk, B, S, _, scratch, tickets, _ = c
    return ops.attention_dense_scratch(B, S, H, dk, scratch, tickets)[1:]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dk", DKS)
def test_bf16_cases_take_their_forms(form, dk):
    H, B, S, lens, scratch, tickets = BF16_CASES[form]
    pl = plan_case(H, dk, B, S, scratch, tickets)
    assert AC.form_of(pl, B, S, H) == form and lens[-1] == lens[0] and len(lens) == B, f"a threshold of launch_attention moved ({pl})"


def test_every_form_is_reached_with_every_edge():
    assert {c[1] for c in CASES} == set(DKS)
    for form in FORMS:
        mine = [c for c in CASES if c[7] == form]
        assert len(mine) >= 2, form
        if form in "CEFG":
            assert 128 in {c[1] for c in mine} and {c[1] for c in mine} - {128}, form
        empty = ragged = zero = above = False
        edges, wg8 = set(), set()
        for H, dk, B, S, lens, scratch, tickets, _ in mine:
            pl = plan_case(H, dk, B, S, scratch, tickets)
            kr = AC.key_ranges_dense(lens, S, pl[0], pl[1])
            # a key range (a wave of a strip) that owns no valid tile in an utterance that has keys: a short utterance beside a long one.
            # (The single sweeps D and F have one range: it owns nothing only in a zero-length utterance.)
            empty |= any(e > 0 and (t > 0 or form in "DF") for t, _, e in kr) and min(l for l in lens if l > 0) * 4 < max(lens)
            ragged |= S % 32 != 0 and S % 128 != 0
            zero |= 0 in lens
            above |= max(lens) > S
            edges |= {(l + 1) % 32 for l in lens if 31 <= l <= S}
            wg8.add(AC.workgroups(pl, B, S, H) % 8 != 0)
        assert empty and ragged and zero and above, (form, empty, ragged, zero, above)
        assert {0, 1, 2} <= edges, (form, "lengths at 32 k - 1, 32 k and 32 k + 1")
        if form in GRID_FORMS:
            assert wg8 == {True, False}, (form, "k_attention's remap needs a launch with nblk % 8 != 0 and one with nblk % 8 == 0")
        s = spiked_case(form)
        pl = plan_case(*s[:4], s[5], s[6])
        tiles, per, _ = AC.key_ranges_dense(s[4], s[3], pl[0], pl[1])[0]
        late_tile = (min(s[4][0], s[3]) - 40) // 32
        assert late_tile >= 1 and (pl[1] == 1 and pl[0] == AC.GRID or late_tile // per >= 1), (form, "the spiked key lies in a later range")
    assert any(AC.workgroups(plan_case(*c[:4], c[5], c[6]), c[2], c[3], c[0]) > 256 and not c[5] for c in CASES if c[7] == "F")


def test_plan_attention_dense_refuses_bad_arguments():
    from smart_nar_fast_tts_amd import _lib

    lib = _lib.load()
    o = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    for args in ((0, 64, 2, 128), (4, 0, 2, 128), (4, 64, 0, 128), (4, 64, 2, 48), (-1, 64, 2, 32), (1, 700000, 8, 128)):
        assert lib.ns_plan_attention_dense(*args, 0, 0, o) != 0 and lib.ns_last_error()
    assert lib.ns_plan_attention_dense(4, 64, 2, 128, 0, 0, None) != 0
    assert tuple(o) == (7, 7, 7, 7)
    part, has = ctypes.c_size_t(0), ctypes.c_int32(0)
    assert lib.ns_op_attention_carve(0, 64, 2, 1024, 0, ctypes.byref(part), ctypes.byref(has)) != 0
    assert lib.ns_op_attention_carve(4, 64, 2, 1024, 0, None, ctypes.byref(has)) != 0
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the call is refused first)
    assert lib.ns_op_attention_core_mode(one, one, 2, 40, 2, 128, one, nul, 0, nul, 4) != 0 and b"flag" in lib.ns_last_error()


def test_the_op_hands_over_what_the_helper_says():
    """the carve rule of ns_op_attention_core_mode, by hand: the ticket block (B H ceil(S / 32) ints rounded up to 64) comes off the
    end unless bit 1 withholds it or the scratch is no larger than it"""
    from smart_nar_fast_tts_amd import ops

    B, S, H, dk = 4, 545, 2, 128
    one, tk = B * S * H * dk + 2 * B * S * H, (B * H * 18 + 63) // 64 * 64
    assert ops.attention_dense_scratch(B, S, H, dk, True, True) == (8 * one, 8 * one - tk, True)
    assert ops.attention_dense_scratch(B, S, H, dk, True, False) == (8 * one, 8 * one, False)
    assert ops.attention_dense_scratch(B, S, H, dk, 16, True) == (16 * one + tk, 16 * one, True)
    assert ops.attention_dense_scratch(B, S, H, dk, 16, False) == (16 * one, 16 * one, False)
    assert ops.attention_dense_scratch(B, S, H, dk, False, True) == (0, 0, False)
    ws = ops.attention_dense_scratch(B, S, H, dk, "workspace", True)
    assert ws == (16 * one + tk, 16 * one, True)  # (fewer than 128 blocks: the workspace reserves ATT_SPLIT_MAX ranges)
    # 8 ranges' worth in all leave room for 7 once the tickets are out: the single 788-frame utterance still takes 4 (13 waves' worth)
    assert plan_case(2, 128, 1, 788, True, True)[:3] == (AC.STRIP, 4, AC.LAST_ARRIVER)


# ---------------------------------------------------------------------------------------------------- old and new decisions agree
def _sweep():
    """(B, S, H, dk): both sides of 127 / 128 blocks, of 4 / 5 tiles per wave (16 n / 16 n + 1 tiles at n = 1 .. 8 strip ranges),
    of S = 512 / 513, the planner's B = 9, 17, 20 at T ~ 1000 and its neighbours"""
    shapes = set()
    for H, dk in ((2, 128), (8, 64), (4, 32), (2, 32), (4, 64), (1, 128)):
        for S in (1, 33, 128, 300, 512, 513, 545, 600, 788, 1010, 1025, 1640, 2049, 3900):
            for B in (1, 2, 3, 5, 9, 13, 17, 18, 20, 33):
                shapes.add((B, S, H, dk))
            q = (S + 127) // 128 * H
            for blocks in (127, 128, 129, 255, 256, 257):  # B on both sides of the block thresholds
                for B in {blocks // q, blocks // q + 1} - {0}:
                    shapes.add((B, S, H, dk))
    return sorted(shapes)


def test_new_entry_equals_the_restated_inline_decision():
    from smart_nar_fast_tts_amd import _lib, ops

    lib, n, forms = _lib.load(), 0, set()
    for B, S, H, dk in _sweep():
        if S * 3 * H * dk * 4 >= 1 << 31:
            continue
        one = B * S * H * dk + 2 * B * S * H
        floats = {0, 1, 2 * one - 1, 2 * one, 3 * one - 1, 3 * one, 5 * one - 1, 5 * one, 8 * one - 1, 8 * one, 16 * one - 1, 16 * one, 64 * one}
        for f in sorted(floats):
            for tk in (False, True):
                got = ops.plan_attention_dense(B, S, H, dk, f, tk)
                assert got == tuple(AC.plan_dense_ref(B, S, H, dk, f, tk)), (B, S, H, dk, f, tk, got)
                forms.add(AC.form_of(got, B, S, H))
                n += 1
        # ns_plan_attention_split: the ranges a workspace reserves; a launch handed the scratch for them splits into no more, and
        # where the planner decides (128 blocks or more) into exactly that many after the no-empty-range rounding
        nsp = lib.ns_plan_attention_split(B, S, H, dk)
        assert nsp == AC.attention_split_ref(B, S, H, dk)
        pl = ops.plan_attention_dense(B, S, H, dk, nsp * one if nsp > 1 else 0, False)
        assert pl[1] <= nsp
        if AC.blocks_of(B, S, H) >= AC.ATT_SPLIT_MAX_BLOCKS:
            assert pl == ops.plan_attention_dense(B, S, H, dk, 64 * one, False) and pl[1] == nsp
    assert n >= 3000 and forms == set(FORMS), (n, forms)


def test_sweep_holds_both_sides_of_every_threshold():
    sw = _sweep()
    blocks = {AC.blocks_of(B, S, H) for B, S, H, _ in sw}
    assert {127, 128} <= blocks and {512, 513} <= {S for _, S, _, _ in sw}
    tpr = {AC.strip_plan_ref(B, S, H, dk, B * S, 1 << 40)[2] for B, S, H, dk in sw if AC.blocks_of(B, S, H) < 128}
    assert {4, 5} <= tpr


_CHILD = """
import sys
sys.path.insert(0, {root!r})
from smart_nar_fast_tts_amd import ops
from tests import attention_cpu as AC
import tests.test_attention_ops_host as T
for c in T.CASES:
    if c[7] != "G":
        continue
    H, dk, B, S, lens, scratch, tickets, _ = c
    pl = T.plan_case(H, dk, B, S, scratch, tickets)
    assert AC.form_of(pl, B, S, H) == "F" and pl == tuple(AC.plan_dense_ref(B, S, H, dk, *T._handed(c), planner=False)), pl
    assert ops._lib.load().ns_plan_attention_split(B, S, H, dk) == 1
print("ok")
"""


def test_planner_off_turns_the_G_shapes_into_F():
    """NS_PLAN is read once per process: a child of its own (host only, no GPU)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=root)], env=dict(os.environ, NS_PLAN="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------- the remap
def test_xcd_remap_is_a_bijection_and_needs_its_remainder_branch():
    for nblk in range(1, 2049):
        assert AC.is_bijection(nblk), nblk
        # (without the remainder branch a launch of ONE workgroup still maps 0 -> 0: the only nblk % 8 != 0 that survives)
        assert AC.is_bijection(nblk, drop_remainder=True) == (nblk % 8 == 0 or nblk == 1), nblk
    assert [AC.xcd_remap(L, 14) for L in range(14)] == [0, 2, 4, 6, 8, 10, 12, 13, 1, 3, 5, 7, 9, 11]  # by hand: slices 2 2 2 2 2 2 1 1


# ---------------------------------------------------------------------------------------------------- the yardstick and its mutants
_REFS = {}


def reference(c, spiked=False):
    """(qkv, lens, float64 output) of a case, computed once and shared (tests/test_gpu_attention_ops.py reads the same)"""
    key = (c[:4], tuple(c[4]), spiked)
    if key not in _REFS:
        qkv, lens = case_input(c, spiked)
        ref = AC.ref_attention(qkv, lens, c[0])
        ref.requires_grad_(False)
        _REFS[key] = (qkv, lens, ref)
    return _REFS[key]


def _err(out, ref, lens):
    return AC.check_output(out, ref, lens.tolist())[0]


def _unique_inputs():
    seen = {}
    for c in CASES:
        seen.setdefault((c[:4], tuple(c[4])), []).append(c)
    return seen


def test_range_by_range_evaluation_is_the_same_function():
    """split_merge_ref with the right merge equals the one-pass softmax to float64 rounding under every split plan of the table, and
    the fp32 CPU evaluation sits far inside the gates (the 'how far is plain fp32' column)"""
    for c in CASES:
        H, dk, B, S, lens, scratch, tickets, form = c
        pl = plan_case(H, dk, B, S, scratch, tickets)
        for spiked in (False, True) if c is spiked_case(form) else (False,):
            qkv, lt, ref = reference(c, spiked)
            assert _err(AC.split_merge_ref(qkv, lt, H, pl[0], pl[1]), ref, lt) < 1e-12, case_id(c)
            assert _err(AC.ref_attention_fp32(qkv, lt, H), ref, lt) < 0.25 * (TOL_SPIKED if spiked else TOL), case_id(c)
            live = torch.tensor([n > 0 for n in lens])
            assert bool(torch.isnan(ref[~live]).all()) and bool(torch.isfinite(ref[live]).all())


MUTANTS = {
    # name: (forms it applies to, function of (qkv, lens, H, kernel, nsplit))
    "keys masked at S": (FORMS, lambda q, l, H, k, n: AC.mutant_attention(q, l, H, mask_at_S=True)),
    "mask one key late": (FORMS, lambda q, l, H, k, n: AC.mutant_attention(q, l, H, mask_shift=1)),
    "scale 1 / dk": (FORMS, lambda q, l, H, k, n: AC.mutant_attention(q, l, H, scale_dk=True)),
    "head h reads head h + 1's K": (FORMS, lambda q, l, H, k, n: AC.mutant_attention(q, l, H, head_shift=1)),
    # the merges: every form with more than one key range — a strip's four waves are ranges too (form A)
    "equal merge weights": ("ABCEG", lambda q, l, H, k, n: AC.split_merge_ref(q, l, H, k, n, same_reference=True)),
    "last range dropped": ("ABCEG", lambda q, l, H, k, n: AC.split_merge_ref(q, l, H, k, n, drop_last=True)),
    "first range's l alone": ("ABCEG", lambda q, l, H, k, n: AC.split_merge_ref(q, l, H, k, n, first_l_only=True)),
    "an empty range's l = 1": ("ABCEG", lambda q, l, H, k, n: AC.split_merge_ref(q, l, H, k, n, empty_l_one=True)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_gate_rejects_the_mutant(name):
    forms, fn = MUTANTS[name]
    worst, nan_broken = {}, False
    for c in CASES:
        H, dk, B, S, lens, scratch, tickets, form = c
        if form not in forms:
            continue
        pl = plan_case(H, dk, B, S, scratch, tickets)
        qkv, lt, ref = reference(c)
        out = fn(qkv, lt, H, pl[0], pl[1])
        err, nan_ok, _ = AC.check_output(out, ref, lens)  # (err: the utterances with keys only — a broken NaN rule is not counted)
        worst[form] = max(worst.get(form, 0.0), err / TOL)
        nan_broken |= not nan_ok
    print(name, {f: f"{v:.3g}" for f, v in worst.items()}, "NaN rule broken too" if nan_broken else "")
    assert set(worst) == set(forms) and min(worst.values()) >= MUTANT_FACTOR, (name, worst)


def test_sentinel_rule_catches_a_tile_never_written():
    """a (batch, head, 128-query tile) the kernel never wrote keeps the sentinel the test pre-filled: the count is not zero whatever
    the tile — also in a zero-length utterance, whose rows are NaN otherwise and tell the gate nothing"""
    c = CASES[3]
    H, dk, B, S, lens, _, _, _ = c
    qkv, lt, ref = reference(c)
    for b, h, qt in ((0, 0, 0), (1, 1, 4), (2, 0, 2), (B - 1, H - 1, (S - 1) // 128)):
        out = ref.float().clone()
        out[b, qt * 128:(qt + 1) * 128, h * dk:(h + 1) * dk] = AC.SENTINEL
        err, nan_ok, left = AC.check_output(out, ref, lens)
        assert left == (min(S, (qt + 1) * 128) - qt * 128) * dk and (lens[b] == 0 or err > 1e3)
        assert nan_ok == (lens[b] != 0)
    assert AC.check_output(ref.float(), ref, lens)[1:] == (True, 0)
    assert not bool((ref.float() == AC.SENTINEL).any()) and np.isfinite(AC.SENTINEL)
