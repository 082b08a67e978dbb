"""Every launch form of the dense (grid) self-attention ALONE on the MI355X, against the float64 yardstick of tests/attention_cpu.py.
tests/test_attention_ops_host.py holds the case table and proves on the CPU which of the seven forms (A .. G, listed there) every
case takes — asked of the dispatch itself, ns_plan_attention_dense, with exactly the scratch and ticket flag the op hands over — and
that the gates below reject the wrong versions that matter.  Here, for every row of the table through ops.attention_core:

  output        all S query rows of every utterance within 2e-5 of float64 on N(0, 1) inputs (5e-5 with a spiked key: per form one case
                with a dominant key in a late range / tile and another in the first tile); rows of a zero-length utterance NaN exactly,
                all others finite
  sentinel      `out` is a slice of a larger tensor pre-filled with a finite sentinel: none is left, and the values around the
                slice keep their bits
  replica       the last utterance is a copy of the first in content and length: its output carries the first's bits
  merge bits    forms B and C (last-arriver merge, k_attention_merge launch) give equal bits on the same input, fp32 and bf16
  split/single  every split form within 1e-5 of the single sweep of the same input
  BF = true     every form once per d_k at the attention_check gate of tests/bf16_emu.py
  NS_PLAN=0     a G shape in a fresh child process with the planner off: form F, same gate

Every test reports the form, the key ranges, the worst error on the GPU and torch's fp32 CPU evaluation of the same input (reported,
not gated); NS_ATTENTION_OPS_REPORT=<path> appends the rows to a JSON-lines file (profiles/attention_ops.md was written from one)."""
import os
import subprocess
import sys

import pytest
import torch

import tests.test_attention_ops_host as H
from tests import attention_cpu as AC
from tests import bf16_emu as E
from tests.util import reporter

pytestmark = pytest.mark.gpu

PAD = 1024  # floats on either side of `out` inside the larger tensor (a multiple of 4: the kernels store 16 bytes at a time)
_FP32 = {}


_report = reporter("NS_ATTENTION_OPS_REPORT")


def _cpu_fp32_err(c, spiked=False):
    key = (c[:4], tuple(c[4]), spiked)
    if key not in _FP32:
        qkv, lens, ref = H.reference(c, spiked)
        _FP32[key] = AC.check_output(AC.ref_attention_fp32(qkv, lens, c[0]), ref, c[4])[0]
    return _FP32[key]


def launch(qkv, lens, heads, scratch, tickets, bf16=False):
    """ops.attention_core into a slice of a larger tensor: the slice pre-filled with the sentinel, PAD distinct values on either
    side.  Returns the output on the CPU after requiring that no sentinel is left and that the surroundings kept their bits."""
    from smart_nar_fast_tts_amd import ops

    B, S, d3 = qkv.shape
    n = B * S * (d3 // 3)
    big = torch.arange(n + 2 * PAD, dtype=torch.float32, device="cuda") * 0.5 + 7.0
    before = big.clone()
    out = big[PAD:PAD + n].view(B, S, d3 // 3)
    out.fill_(AC.SENTINEL)
    ret = ops.attention_core(qkv.cuda(), torch.tensor(lens).cuda(), heads, split_scratch=scratch, tickets=tickets, bf16=bf16, out=out)
    assert ret.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(big[:PAD].view(torch.int32), before[:PAD].view(torch.int32)), "values BEFORE the output slice changed"
    assert torch.equal(big[PAD + n:].view(torch.int32), before[PAD + n:].view(torch.int32)), "values AFTER the output slice changed"
    got = out.cpu()
    left = int((got == AC.SENTINEL).sum())
    assert left == 0, f"{left} output values were never written (the sentinel is still there)"
    return got


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_case(c, spiked=False, scratch=None, tickets=None, form=None, what="output"):
    """one launch of a table row (or of its input under another scratch / ticket choice) held to every rule; returns the output"""
    heads, dk, B, S, lens, sc, tk, fm = c
    scratch, tickets, form = (sc if scratch is None else scratch), (tk if tickets is None else tickets), (form or fm)
    pl = H.plan_case(heads, dk, B, S, scratch, tickets)
    assert AC.form_of(pl, B, S, heads) in form, f"a threshold of launch_attention moved ({pl}): pick a shape that takes form {form} again"
    qkv, lens_t, ref = H.reference(c, spiked)
    got = launch(qkv, lens, heads, scratch, tickets)
    err, nan_ok, _ = AC.check_output(got, ref, lens)
    tol = H.TOL_SPIKED if spiked else H.TOL
    replica = _bits_equal(got[-1], got[0])
    _report(test=what, case=H.case_id(c), form=AC.form_of(pl, B, S, heads), kernel=pl[0], ranges=pl[1], merge=pl[2], tiles=pl[3],
            workgroups=AC.workgroups(pl, B, S, heads), spiked=spiked, gpu_max_abs_err=err, cpu_fp32_max_abs_err=_cpu_fp32_err(c, spiked), tol=tol,
            replica_bits=replica)
    assert nan_ok, "rows of a zero-length utterance must be NaN exactly, all others finite"
    assert err < tol, (H.case_id(c), err, _cpu_fp32_err(c, spiked))
    assert replica, "the copy of utterance 0 must carry its bits (same keys, same ranges, merged in key order)"
    return got


@pytest.mark.parametrize("c", H.CASES, ids=H.case_id)
def test_attention_form_vs_float64(c):
    check_case(c)


@pytest.mark.parametrize("form", H.FORMS)
def test_attention_form_spiked_keys(form):
    """head 0: one key far above the rest in the last valid tile but one of utterance 0 (a late key range of every split form): the
    reference point must move there; head 1: a dominant key in the first tile, so it must not move again"""
    check_case(H.spiked_case(form), spiked=True, what="spiked")


@pytest.mark.parametrize("c", [c for c in H.CASES if c[7] == "B"], ids=H.case_id)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_last_arriver_and_merge_launch_give_equal_bits(c, bf16):
    """forms B and C of the same input: the same partials, merged in the same order by merge_fma — equal bits, in both modes"""
    heads, dk, B, S, lens, scratch, _, _ = c
    pb, pc = H.plan_case(heads, dk, B, S, scratch, True), H.plan_case(heads, dk, B, S, scratch, False)
    assert (AC.form_of(pb, B, S, heads), AC.form_of(pc, B, S, heads)) == ("B", "C") and pb[1] == pc[1] and pb[3] == pc[3]
    qkv, _, _ = H.reference(c)
    b, cc = launch(qkv, lens, heads, scratch, True, bf16), launch(qkv, lens, heads, scratch, False, bf16)
    same = _bits_equal(b, cc)
    _report(test="merge_bits", case=H.case_id(c), bf16=bf16, ranges=pb[1], equal_bits=same)
    assert same, f"{int((b.view(torch.int32) != cc.view(torch.int32)).sum())} values differ between the last arriver's merge and k_attention_merge"


@pytest.mark.parametrize("c", [c for c in H.CASES if c[7] in H.SPLIT_FORMS], ids=H.case_id)
def test_split_forms_against_the_single_sweep(c):
    heads, dk, B, S, lens, scratch, tickets, form = c
    split = check_case(c, what="split")
    single = check_case(c, scratch=H.NO, form="ADF", what="single sweep")
    diff = float((torch.nan_to_num(split) - torch.nan_to_num(single)).abs().max())
    _report(test="split_vs_single", case=H.case_id(c), form=form, max_abs_diff=diff, tol=H.TOL_SPLIT_VS_SINGLE)
    assert torch.equal(torch.isnan(split), torch.isnan(single)) and diff < H.TOL_SPLIT_VS_SINGLE, diff


@pytest.mark.parametrize("dk", H.DKS)
@pytest.mark.parametrize("form", H.FORMS)
def test_attention_form_bf16_mode(form, dk):
    """the BF = true kernels of every form at the gate of tests/test_gpu_bf16_ops.py (attention_check: the fp32 tier plus budgeted
    flips of the rounded P)"""
    heads, B, S, lens, scratch, tickets = H.BF16_CASES[form]
    pl = H.plan_case(heads, dk, B, S, scratch, tickets)
    assert AC.form_of(pl, B, S, heads) == form, f"a threshold of launch_attention moved ({pl})"
    qkv = AC.make_qkv(B, S, heads, dk, seed=S + dk + B)
    got = launch(qkv, lens, heads, scratch, tickets, bf16=True)
    for b, n in enumerate(lens):
        assert bool(torch.isnan(got[b]).all()) if n == 0 else bool(torch.isfinite(got[b]).all()), (b, n)
    ref, unit, flip = E.attention_emu(qkv, torch.tensor(lens), heads)
    res = E.attention_check(got, ref, unit, flip, heads)
    replica = _bits_equal(got[-1], got[0])
    _report(test="bf16", form=form, dk=dk, H=heads, B=B, S=S, ranges=pl[1], worst_flips=res.worst_flips, worst_over_fp32_tier=res.worst_fp32,
            pair_share=res.pair_share, replica_bits=replica)
    assert res.ok, f"form {form} d_k {dk}: {res}"
    assert replica


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import tests.test_attention_ops_host as H
import tests.test_gpu_attention_ops as G
c = next(c for c in H.CASES if c[7] == "G")
G.check_case(c, form="F", what="NS_PLAN=0")
print("child ok")
"""


def test_planner_off_runs_a_G_shape_as_F():
    """NS_PLAN is read once per process: ONE fresh child with the variable set runs the first G row; there it must plan form F (one
    sweep) and pass the same rules"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=root)], env=dict(os.environ, NS_PLAN="0"), capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("child ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert '"form": "F"' in r.stdout
