"""The training loss's backward, everything that needs no GPU: the closed-form float64 gradients (tests/lossgrad_cpu.py) against the
gradients captured from the imported reference's own ``total.backward()`` and against torch's autograd of the masked_select statement,
the gate proven both ways (the fp32 reference uses at most half of it, every mutant leaves it), the ns_lossg_* C ABI's host side
(struct layout, versions, every refusal), the Python surface, and the kernel's register hygiene."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from smart_nar_fast_tts_amd import _lib
from smart_nar_fast_tts_amd.loss import GRAD_NAMES, FastSpeech2TrainingLoss
from tests import loss_cpu as lc
from tests import lossgrad_cpu as lg
from tests.util import assert_no_spill, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = (("lossgrad_tiny", "teacher_tiny"), ("lossgrad_tiny_phoneme_level", "teacher_tiny_phoneme_level"))
EPS64 = float(np.finfo(np.float64).eps)


def _close64(got, want, what, ulps=8):
    """A few float64 ulps of the tensor's largest magnitude, and zero exactly where the reference is zero."""
    for n, a, w in zip(lg.NAMES, got, want):
        tol = ulps * EPS64 * float(np.max(np.abs(w), initial=0.0))
        err = float(np.max(np.abs(a - w), initial=0.0))
        print(what, n, f"max |closed form - reference| = {err:.3e} (tolerance {tol:.3e})")
        assert a.shape == w.shape and a.dtype == np.float64 and err <= tol, (what, n, err, tol)
        assert not a[w == 0].any(), (what, n, "nonzero where the reference's gradient is zero")


@pytest.mark.parametrize("name,source", FIXTURES)
def test_closed_form_reproduces_the_reference_backward(name, source):
    """The reference's own float64 ``total.backward()`` (tests/golden/make_golden_lossgrad.py), W and the duration target in fp32 as
    the reference has them: the closed form agrees to a few float64 ulps on all nine tensors, the maps included.  The reference's own
    fp32 backward uses at most half of every gate (by the gate's construction), and the stored values are the loss fixture's."""
    meta, z = load_golden(name)
    ms, zs = load_golden(source)
    assert meta["names"] == list(lg.NAMES) and meta["grad_output"] == lg.G_TOTAL.tolist()
    inputs, predictions = lc.fixture_case(zs, ms, "")
    got = lg.closed_form(inputs, predictions, ms["pitch"], ms["energy"], lg.G_TOTAL)
    ref64, ref32 = [z[n + "_f64"] for n in lg.NAMES], [z[n] for n in lg.NAMES]
    _close64(got, ref64, name)
    gates = lg.gate(ref32, ref64, lg.G_TOTAL, lg.n_attn_of(inputs, predictions))
    share, _ = lg.shares(ref32, got, gates)
    print(name, "the reference's fp32 backward, share of the gate:", dict(zip(lg.NAMES, share.round(4))))
    assert (share <= 0.5).all(), share
    _, zl = load_golden(name.replace("lossgrad", "loss"))
    assert np.array_equal(z["values"], zl["values"]), "the fp32 forward values are those of the loss fixture"


@pytest.mark.parametrize("level", lc.LEVELS)
@pytest.mark.parametrize("name", list(lc.CASES))
def test_closed_form_against_autograd_of_the_masked_select_statement(name, level):
    inputs, predictions, g, want, gates, n_attn, r32, r64 = lg.case(name, level)
    _close64(want, r64, f"{name} {level}")
    share, _ = lg.shares(r32, want, gates)
    print(name, level, "torch fp32 autograd, share of the gate:", dict(zip(lg.NAMES, share.round(4))))
    assert (share <= 0.5).all(), share
    for w, hide in zip(want, lg.hidden(inputs, predictions, level, level)):
        assert not w[hide].any()


def test_statement_values_are_the_loss_values():
    """The differentiated statement computes what tests/loss_cpu.py computes (whose float64 values are pinned to the reference's)."""
    for level in lc.LEVELS:
        inputs, predictions, want, _ = lc.case("unaligned_prime_T_empty_utterances", level)
        f = lambda t: t.double() if torch.is_tensor(t) and t.dtype.is_floating_point else t  # noqa: E731
        i64 = tuple(f(t) for t in inputs)
        p64 = tuple([f(a) for a in t] if isinstance(t, list) else f(t) for t in predictions)
        got = lg.statement(i64, p64, level, level).numpy()
        assert np.allclose(got, want, rtol=1e-12, atol=0), (got, want)


MUTANT_LEAVES_GATE_ON = {
    "mean_over_all_elements": ("mel", "postnet", "pitch", "energy", "log_d", "attn0"),
    "factor_2_dropped": ("pitch", "energy", "log_d"),
    "g0_only": lg.NAMES,
    "W_on_every_head": ("attn0", "attn1", "attn2", "attn3"),
    "alpha_dropped": ("attn0", "attn3"),
    "log_without_plus_one": ("log_d",),
    "mask_off_by_one": ("mel", "postnet", "pitch", "energy", "log_d", "attn0"),
}


def test_gate_rejects_every_mutant():
    """Each deliberately wrong closed form leaves the gate on the tensors it changes, on a case with ragged lengths and two empty
    utterances; multiply-by-mask is NaN as soon as a padded position holds one."""
    name, level = "unaligned_prime_T_empty_utterances", "frame_level"
    inputs, predictions, g, want, gates, _, _, _ = lg.case(name, level)
    for m, tensors in MUTANT_LEAVES_GATE_ON.items():
        share, _ = lg.shares(lg.closed_form(inputs, predictions, level, level, g, mutate=m), want, gates)
        print(f"{m:24s}", dict(zip(lg.NAMES, share.round(1))))
        for t in tensors:
            assert share[lg.NAMES.index(t)] > 1.0, (m, t, share)
    pi, pp = lc.poison(inputs, predictions, level, level)
    clean = lg.closed_form(pi, pp, level, level, g)
    for a, w in zip(clean, want):
        assert a.tobytes() == w.tobytes(), "the selection does not see the poison"
    share, _ = lg.shares(lg.closed_form(inputs, predictions, level, level, g, mutate="multiply_by_mask"), want, gates)
    # clean data: the five predictions equal the selection; the maps are NaN already, W = 1 - exp(-(l / 0 - ..)^2 / ..) of the utterance
    # with src_lens == 0 being NaN itself
    assert (share[:5] <= 1.0).all() and np.isinf(share[5:]).all(), share
    share, _ = lg.shares(lg.closed_form(pi, pp, level, level, g, mutate="multiply_by_mask"), want, gates)
    print("multiply_by_mask under poison", dict(zip(lg.NAMES, share)))
    assert np.isinf(share[2:]).all(), share  # (the two L1 tensors survive it: sign(NaN) is 0)
    assert set(MUTANT_LEAVES_GATE_ON) | {"multiply_by_mask"} == set(lg.MUTANTS)


def test_empty_selection_has_zero_gradients():
    inputs, predictions = lc.random_case(2, 5, 7, 2, mel_lens=[0, 0], seed=3)
    got = lg.closed_form(inputs, predictions, "frame_level", "frame_level", lg.G_TOTAL)
    for n, a in zip(lg.NAMES, got):
        assert np.isfinite(a).all() and (n == "log_d") == bool(a.any()), n


# ---- the C ABI's host side ----------------------------------------------------------------------------------------------------------
def test_abi_versions_header_against_lib():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    for macro, fn, want in (("NS_LOSSG_ABI_VERSION", lib.ns_lossg_abi_version, 1), ("NS_LOSS_ABI_VERSION", lib.ns_loss_abi_version, 1),
                            ("NS_ABI_VERSION", lib.ns_abi_version, 6), ("NS_VOC_ABI_VERSION", lib.ns_voc_abi_version, 1),
                            ("NS_ALN_ABI_VERSION", lib.ns_aln_abi_version, 1), ("NS_MEL_ABI_VERSION", lib.ns_mel_abi_version, 1),
                            ("NS_GL_ABI_VERSION", lib.ns_gl_abi_version, 1), ("NS_VT_ABI_VERSION", lib.ns_vt_abi_version, 1),
                            ("NS_OPT_ABI_VERSION", lib.ns_opt_abi_version, 1)):
        header = int(re.search(rf"#define {macro} (\d+)", text).group(1))
        assert header == fn() == want, macro
    assert int(re.search(r"#define NS_LOSSG_RECORD_BYTES (\d+)", text).group(1)) == lib.ns_lossg_record_bytes() == 32


def test_structs_match_header():
    text = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ns_lossg_grads \{(.*?)\} ns_lossg_grads;", text, flags=re.S).group(1), flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", f.strip().lstrip("*")) for decl in re.findall(r"float\*? ([^;]+);", body) for f in decl.split(",")]
    assert fields == [f for f, _ in _lib.NsLossgGrads._fields_] == ["mel", "postnet", "pitch", "energy", "log_d", "attn"]
    assert C.sizeof(_lib.NsLossgGrads) == 9 * 8
    assert C.sizeof(_lib.NsLossArgs) == 4 * 8 + 2 * 8 + 13 * 8 + 4 * 8, "ns_loss_args is untouched"


def _args(**over):
    """A well-formed argument block over made-up (never dereferenced) device addresses: validation runs before any HIP call."""
    a = _lib.NsLossArgs()
    a.B, a.L, a.T, a.H, a.n_mel, a.pitch_frame_level, a.energy_frame_level = 2, 12, 40, 2, 80, 1, 1
    a.mel_targets_stride, a.d_targets_stride = 40 * 80, 12
    for i, (f, _) in enumerate(_lib.NsLossArgs._fields_[9:22]):
        setattr(a, f, 0x10000 * (i + 1))
    for k in range(4):
        a.attn[k] = 0x1000000 * (k + 1)
    for k, v in over.items():
        if k.startswith("attn"):
            a.attn[int(k[4:])] = v
        else:
            setattr(a, k, v)
    return a


ARG_REFUSALS = ([(dict([(f, -1)]), "negative size") for f in ("B", "L", "T")]
                + [(dict(n_mel=n), "n_mel must be a positive multiple of 4") for n in (0, 81, 82, -4)]
                + [(dict(H=0), "H must be >= 1")]
                + [(dict([(f, None)]), what) for f, what in (
                    ("src_lens", "src_lens or mel_lens"), ("mel_lens", "src_lens or mel_lens"), ("mel", "null mel"), ("postnet", "null mel"),
                    ("mel_targets", "null mel"), ("mel_masks", "null mel"), ("log_d", "null log_d"), ("d_targets", "null log_d"),
                    ("src_masks", "null log_d"), ("pitch", "null pitch"), ("pitch_targets", "null pitch"), ("energy", "null energy"),
                    ("energy_targets", "null energy"), ("attn0", r"attn\[0\] is null"), ("attn3", r"attn\[3\] is null"))]
                + [(dict(attn2=0x1000002), r"attn\[2\] is null or not 4-byte aligned"), (dict(mel=0x10004), "16-byte aligned"),
                   (dict(mel_targets_stride=40 * 80 - 4), "mel_targets_stride"), (dict(mel_targets_stride=40 * 80 + 2), "mel_targets_stride"),
                   (dict(d_targets_stride=11), "d_targets_stride"), (dict(B=1 << 20, T=1 << 12), "problem too large")])


def test_forward_refusals_are_reached_without_a_gpu():
    lib = _lib.load()
    ws, out, rec = C.c_void_p(0x2000000), C.c_void_p(0x3000000), C.c_void_p(0x4000000)
    need = lib.ns_loss_ws_bytes(2, 12, 40)

    def refused(a, match, ws=ws, n=need, out=out, rec=rec):
        rc = lib.ns_lossg_forward(C.byref(a) if a is not None else None, ws, n, out, rec, None)
        msg = lib.ns_last_error().decode()
        assert rc != 0 and msg.startswith("ns_lossg_forward: ") and re.search(match, msg), (match, rc, msg)

    refused(None, "null argument")
    for null in ("ws", "out", "rec"):
        refused(_args(), "null argument", **{null: None})
    for over, match in ARG_REFUSALS:
        refused(_args(**over), match, n=1 << 40)
    refused(_args(), r"workspace too small \(ns_loss_ws_bytes\)", n=need - 1)
    refused(_args(), "workspace must be 16-byte aligned", ws=C.c_void_p(0x2000008))
    refused(_args(), "out7 4-byte aligned", out=C.c_void_p(0x3000002))
    refused(_args(), "record must be 8-byte aligned", rec=C.c_void_p(0x4000004))


def _grads(**over):
    d = _lib.NsLossgGrads()
    for i, f in enumerate(("mel", "postnet", "pitch", "energy", "log_d")):
        setattr(d, f, 0x5000000 + 0x100000 * i)
    for k in range(4):
        d.attn[k] = 0x6000000 + 0x100000 * k
    for k, v in over.items():
        if k.startswith("attn"):
            d.attn[int(k[4:])] = v
        else:
            setattr(d, k, v)
    return d


def test_backward_refusals_are_reached_without_a_gpu():
    lib = _lib.load()
    rec, g7 = C.c_void_p(0x4000000), C.c_void_p(0x4100000)

    def call(a, d, rec=rec, g7=g7):
        return lib.ns_lossg_backward(C.byref(a) if a is not None else None, rec, g7, C.byref(d) if d is not None else None, None)

    def refused(a, d, match, **kw):
        rc = call(a, d, **kw)
        msg = lib.ns_last_error().decode()
        assert rc != 0 and msg.startswith("ns_lossg_backward: ") and re.search(match, msg), (match, rc, msg)

    refused(None, _grads(), "null argument")
    refused(_args(), None, "null argument")
    refused(_args(), _grads(), "null argument", rec=None)
    refused(_args(), _grads(), "null argument", g7=None)
    for over, match in ARG_REFUSALS:
        refused(_args(**over), _grads(), match)
    refused(_args(B=1 << 10, T=1 << 10, H=1 << 11, mel_targets_stride=80 << 10), _grads(), "problem too large")  # B * H * T = 2^31: the maps' rows are 32-bit
    refused(_args(), _grads(), "record must be 8-byte aligned", rec=C.c_void_p(0x4000004))
    refused(_args(), _grads(), "g7 4-byte aligned", g7=C.c_void_p(0x4100002))
    for f, shown in (("mel", "mel"), ("postnet", "postnet"), ("pitch", "pitch"), ("energy", "energy"), ("log_d", "log_d"),
                     ("attn0", r"attn\[0\]"), ("attn1", r"attn\[1\]"), ("attn2", r"attn\[2\]"), ("attn3", r"attn\[3\]")):
        for off in (4, 8):
            refused(_args(), _grads(**{f: 0x7000000 + off}), rf"grads->{shown} must be 16-byte aligned")
    # nine null outputs: nothing to write, nothing is launched — legal, and no HIP call is made
    none = _lib.NsLossgGrads()
    assert call(_args(), none) == 0


def test_python_surface_without_a_gpu():
    import smart_nar_fast_tts_amd
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss

    assert smart_nar_fast_tts_amd.FastSpeech2TrainingLoss is FastSpeech2TrainingLoss and issubclass(FastSpeech2TrainingLoss, FastSpeech2Loss)
    assert len(GRAD_NAMES) == len(lg.NAMES) == 9
    loss = FastSpeech2TrainingLoss(wl.preprocess_config(), wl.model_config("tiny"))
    assert loss.train() is loss and loss.training and loss.eval() is loss and not loss.training and loss.train(False) is loss and loss.to("cuda") is loss
    inputs, predictions = lc.random_case(2, 5, 7, 2, seed=1)
    for mode in (loss.train(), loss.eval()):
        with pytest.raises(RuntimeError, match="must live on the MI355X"):
            mode(inputs, (predictions[0].clone().requires_grad_(True),) + predictions[1:])
    for i, name in ((6, "mel_targets"), (9, "pitch_targets"), (10, "energy_targets")):
        bad = inputs[:i] + (inputs[i].clone().requires_grad_(True),) + inputs[i + 1:]
        with pytest.raises(ValueError, match=rf"{name}\.requires_grad: targets, masks and lengths get no gradient"):
            loss(bad, predictions)
    # the value-only class keeps refusing both, as before
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        FastSpeech2Loss(wl.preprocess_config(), wl.model_config("tiny")).train()


def test_lossgrad_kernel_does_not_spill():
    """Register hygiene of csrc/lossgrad.hip: no VGPR / SGPR spill, no scratch, no LDS (tools/kernel_resources.py cross-compiles for
    gfx950 and reads the code object's metadata; no GPU needed)."""
    stdout = assert_no_spill("lossgrad.hip")
    row = [ln for ln in stdout.splitlines() if "k_lossg_backward" in ln]
    assert len(row) == 1, stdout
    cols = dict(zip(stdout.splitlines()[0].split(), row[0].split()))
    assert cols["lds"] == "0" and cols["scratch"] == "0", row
