"""Validation loss, everything that needs no GPU: the torch-CPU restatement (tests/loss_cpu.py) against the values captured from the
imported reference, the gate proven both ways (fp32 evaluations use a small share of it, every mutant is rejected), the ns_loss_*
C ABI's host side (versions, size function, every refusal) and the kernels' register hygiene."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from smart_nar_fast_tts_amd import _lib
from tests import loss_cpu as lc
from tests.util import assert_no_spill, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = (("loss_tiny", "teacher_tiny"), ("loss_tiny_phoneme_level", "teacher_tiny_phoneme_level"))


@pytest.mark.parametrize("name,source", FIXTURES)
def test_restatement_reproduces_the_reference(name, source):
    """loss_cpu in float64 equals the reference's float64 values to 1e-12 relative; loss_cpu in fp32 AND the reference's own fp32
    values stay below a third of every gate (measured: at most 0.030 — energy at phoneme_level; mel 0.010, pitch 0.001-0.005)."""
    meta, z = load_golden(name)
    ms, zs = load_golden(source)
    assert meta["names"] == list(lc.NAMES)
    i64, p64 = lc.fixture_case(zs, ms, "_f64")
    v64 = lc.loss(i64, p64, ms["pitch"], ms["energy"], torch.float64)
    rel = np.abs(v64 - z["values_f64"]) / np.abs(z["values_f64"])
    print(name, "float64 restatement, relative distance:", rel)
    assert (rel <= 1e-12).all(), rel
    gate = lc.gates(i64, p64, ms["pitch"], ms["energy"])
    i32, p32 = lc.fixture_case(zs, ms, "")
    v32 = lc.loss(i32, p32, ms["pitch"], ms["energy"], torch.float32)
    for who, v in (("the reference's fp32", z["values"]), ("loss_cpu fp32", v32)):
        share = lc.shares(v, z["values_f64"], gate)
        print(name, who, "share of the gate:", dict(zip(lc.NAMES, share.round(4))))
        assert (share < 1 / 3).all(), (who, share)


@pytest.mark.parametrize("level", lc.LEVELS)
@pytest.mark.parametrize("name", list(lc.CASES))
def test_fp32_restatement_uses_under_a_third_of_the_gate(name, level):
    """The gate's constants are derived, not measured; torch's fp32 evaluation of the same closed form must sit well inside them."""
    inputs, predictions, want, gate = lc.case(name, level)
    share = lc.shares(lc.loss(inputs, predictions, level, level, torch.float32), want, gate)
    print(name, level, "loss_cpu fp32 share of the gate:", dict(zip(lc.NAMES, share.round(4))))
    assert (share < 1 / 3).all(), share


def test_gate_rejects_every_mutant():
    """Every deliberately wrong variant of loss_cpu leaves the gate on the part it changes: on the tiny fixture, and — for the two
    that need them — on a case with an utterance of src_lens == 0 and NaN in every masked-out position."""
    ms, zs = load_golden("teacher_tiny")
    i64, p64 = lc.fixture_case(zs, ms, "_f64")
    want, gate = lc.loss(i64, p64, "frame_level", "frame_level"), lc.gates(i64, p64, "frame_level", "frame_level")
    part = {"mask_off_by_one": ("mel", "postnet", "pitch", "energy", "duration", "attn"), "log_without_plus_one": ("duration",),
            "l2_for_l1": ("mel", "postnet")}
    for m in lc.MUTANTS:
        if m == "multiply_by_mask":
            continue
        share = lc.shares(lc.loss(i64, p64, "frame_level", "frame_level", mutate=m), want, gate)
        print(f"{m:22s}", dict(zip(lc.NAMES, share.round(1))))
        for p in part.get(m, ("attn",)):
            assert share[lc.NAMES.index(p)] > 1.0, (m, p, share)
    # multiply-by-mask: finite on clean data (equal to the selection), NaN as soon as a padded position holds one
    inputs, predictions, want, gate = lc.case("unaligned_prime_T_empty_utterances", "frame_level")
    pi, pp = lc.poison(inputs, predictions, "frame_level", "frame_level")
    assert np.array_equal(lc.loss(pi, pp, "frame_level", "frame_level"), want)  # the selection does not see the poison
    share = lc.shares(lc.loss(pi, pp, "frame_level", "frame_level", mutate="multiply_by_mask"), want, gate)
    print("multiply_by_mask      ", dict(zip(lc.NAMES, share)))
    assert (share > 1.0).all(), share


def test_olen_from_slot_9_is_the_same_function():
    """The issue lists "olen taken from slot 9 on a case with src_lens == 0" among the mutants the gate must reject.  It cannot: slot 9
    (the durations' row sums) differs from the input mel_lens only for an utterance with src_lens == 0, and that
    utterance has ilen == 0 — its attention region {t < olen, l < ilen} is empty and its cell count ilen * olen is 0 whatever olen
    is.  So the variant computes the same value, bit for bit; this test pins that down on such a case (slot 9 really differs there)."""
    inputs, predictions, want, _ = lc.case("unaligned_prime_T_empty_utterances", "frame_level")
    assert not np.array_equal(np.asarray(predictions[9]), np.asarray(inputs[7]))
    assert np.array_equal(lc.loss(inputs, predictions, "frame_level", "frame_level", olen_from_slot9=True), want)


def test_empty_selection_is_nan():
    inputs, predictions = lc.random_case(2, 5, 7, 2, mel_lens=[0, 0], seed=3)
    v = lc.loss(inputs, predictions, "frame_level", "frame_level")
    assert np.isnan(v[[0, 1, 2, 3, 4, 6]]).all() and np.isfinite(v[5]), v


# ---- the C ABI's host side ----------------------------------------------------------------------------------------------------------
def test_abi_versions_header_against_lib():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    for macro, fn, want in (("NS_LOSS_ABI_VERSION", lib.ns_loss_abi_version, 1), ("NS_ABI_VERSION", lib.ns_abi_version, 6),
                            ("NS_VOC_ABI_VERSION", lib.ns_voc_abi_version, 1), ("NS_ALN_ABI_VERSION", lib.ns_aln_abi_version, 1)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == want == fn(), macro


def test_args_struct_matches_header():
    text = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ns_loss_args \{(.*?)\} ns_loss_args;", text, flags=re.S).group(1), flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", f.strip().lstrip("*")) for decl in re.findall(r"(?:const )?\w+\*? ([^;]+);", body) for f in decl.split(",")]
    assert fields == [f for f, _ in _lib.NsLossArgs._fields_]
    assert C.sizeof(_lib.NsLossArgs) == 4 * 8 + 2 * 8 + 13 * 8 + 4 * 8  # 7 int32 + padding, 2 int64, 13 + 4 pointers


def test_ws_bytes_positive_and_monotone():
    lib = _lib.load()
    assert lib.ns_loss_ws_bytes(0, 0, 0) > 0 and lib.ns_loss_ws_bytes(1, 0, 0) > 0
    base = lib.ns_loss_ws_bytes(2, 12, 40)
    assert base > 0 and base % 64 == 0
    for B, L, T in ((3, 12, 40), (2, 13, 40), (2, 12, 41), (2, 1025, 40), (2, 12, 1500), (16, 128, 1030)):
        assert lib.ns_loss_ws_bytes(B, L, T) >= base, (B, L, T)
    for axis in range(3):
        prev = 0
        for v in (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4000):
            dims = [4, 96, 300]
            dims[axis] = v
            n = lib.ns_loss_ws_bytes(*dims)
            assert n >= prev, (axis, v)
            prev = n


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


def test_every_refusal_is_reached_without_a_gpu():
    lib = _lib.load()
    ws, out = C.c_void_p(0x2000000), C.c_void_p(0x3000000)
    need = lib.ns_loss_ws_bytes(2, 12, 40)

    def refused(a, match, ws=ws, n=need, out=out):
        rc = lib.ns_loss_forward(C.byref(a) if a is not None else None, ws, n, out, None)
        msg = lib.ns_last_error().decode()
        assert rc != 0 and re.search(match, msg), (match, rc, msg)

    refused(None, "null argument")
    refused(_args(), "null argument", ws=None)
    refused(_args(), "null argument", out=None)
    for f in ("B", "L", "T"):
        refused(_args(**{f: -1}), "negative size")
    for n_mel in (0, 81, 82, -4):
        refused(_args(n_mel=n_mel), "n_mel must be a positive multiple of 4")
    refused(_args(H=0), "H must be >= 1")
    for f, what in (("src_lens", "src_lens or mel_lens"), ("mel_lens", "src_lens or mel_lens"), ("mel", "null mel"), ("postnet", "null mel"),
                    ("mel_targets", "null mel"), ("mel_masks", "null mel"), ("log_d", "null log_d"), ("d_targets", "null log_d"),
                    ("src_masks", "null log_d"), ("pitch", "null pitch"), ("pitch_targets", "null pitch"), ("energy", "null energy"),
                    ("energy_targets", "null energy"), ("attn0", r"attn\[0\] is null"), ("attn3", r"attn\[3\] is null")):
        refused(_args(**{f: None}), what)
    refused(_args(attn2=0x1000002), r"attn\[2\] is null or not 4-byte aligned")
    refused(_args(mel=0x10004), "16-byte aligned")
    refused(_args(mel_targets_stride=40 * 80 - 4), "mel_targets_stride")
    refused(_args(mel_targets_stride=40 * 80 + 2), "mel_targets_stride")
    refused(_args(d_targets_stride=11), "d_targets_stride")
    refused(_args(), r"workspace too small \(ns_loss_ws_bytes\)", n=need - 1)
    refused(_args(), "workspace too small", n=0)
    refused(_args(), "workspace must be 16-byte aligned", ws=C.c_void_p(0x2000008))
    refused(_args(B=1 << 20, T=1 << 12), "problem too large", n=1 << 40)


def test_python_surface_without_a_gpu():
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss

    loss = FastSpeech2Loss(wl.preprocess_config(), wl.model_config("tiny"))
    assert loss.eval() is loss and loss.train(False) is loss and loss.to("cuda") is loss
    with pytest.raises(NotImplementedError, match=r"training is out of scope for this path \(SURVEY.md §2\); only eval\(\) is supported"):
        loss.train()
    inputs, predictions = lc.random_case(2, 5, 7, 2, seed=1)
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        loss(inputs, predictions)
    with pytest.raises(ValueError, match=r"layers 0-3 \(model/loss.py:233-236\); got 3 map"):
        loss(inputs, predictions[:10] + (predictions[10][:3], predictions[11]))
    grad = predictions[0].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="requires_grad: training is out of scope"):
        loss(inputs, (grad,) + predictions[1:])


def test_loss_kernels_do_not_spill():
    """Register hygiene of csrc/loss.hip: no VGPR / SGPR spill, no scratch (tools/kernel_resources.py cross-compiles for gfx950 and
    reads the code object's metadata; no GPU needed)."""
    assert_no_spill("loss.hip", kernels=("k_loss_partial", "k_loss_final"))
