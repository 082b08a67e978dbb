"""The yardstick of tests/test_gpu_train_align.py proven on the CPU, every refusal of the ns_mh_* family and the Python surface of
smart_nar_fast_tts_amd.training (no GPU).

On the fixture (tests/golden/train_align_tiny.npz: the reference's own FastSpeech2Align and FastSpeech2Loss, one training step at dropout
0) the float64 restatement agrees with the reference's float64 predictions, losses and gradients to <= 1e-12 relative, and the fp32
restatement stays inside the project gate (tests/util.gate_value's rule) taken from the fixture's own fp32 and float64 values.  A
gradient that is zero in exact arithmetic (the key bias of an attention: the softmax does not see it; a conv bias ahead of a train-mode
BatchNorm) is rounding noise in both evaluations: the relative bound gets an absolute floor of 1e-12 of the largest stored gradient.

The mutants: each one is caught on the case tests/train_align_cpu.CATCHER names, by the check the GPU test makes there (bit-equality
with the kernel's emulation, colsum_bound, or the gate on the fixture)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import train_align_cpu as tc
from tests.util import assert_no_spill, built_lib, expect_refusals, gate_value, load_golden, run_c_caller, share_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return built_lib()


@pytest.fixture(scope="module")
def fixture():
    meta, z = load_golden("train_align_tiny")
    return meta, z, tc.fixture_state_dict(meta), tc.fixture_config(meta), tc.fixture_batch(meta)


grad_gate = tc.grad_gate  # the one gate of a stored gradient, shared with tests/test_gpu_train_align.py


def _evaluate(fixture, dtype, mutate=None):
    meta, z, sd, cfgs, batch = fixture
    res = tc.statement(sd, cfgs, batch, dtype, forced_d=z["d_targets"] if dtype == torch.float64 else None, mutate=mutate)
    return res, tc.stored_gradients(tc.backward(res), sd)


# ---------------------------------------------------------------------------------------------------- the whole model's yardstick
def test_restatement_reproduces_the_reference(fixture):
    meta, z, sd, _, _ = fixture
    r64, g64 = _evaluate(fixture, torch.float64)
    r32, g32 = _evaluate(fixture, torch.float32)
    assert np.array_equal(r32["predictions"][11].numpy(), z["d_targets"]), "the fp32 restatement's own durations are the reference's"
    assert np.array_equal(r32["predictions"][9].numpy(), z["d_targets"].sum(1))
    for i, n in enumerate(tc.PRED_NAMES):
        a64, a32, want = r64["predictions"][i].detach().numpy(), r32["predictions"][i].detach().numpy(), z[n + "_f64"]
        assert np.abs(a64 - want).max() <= 1e-12 * np.abs(want).max(), n
        assert share_of(a32, want, gate_value(z[n], want))[0] <= 1.0, n
    s64, s32 = r64["seven"].detach().numpy(), r32["seven"].detach().numpy()
    for i in range(7):
        assert abs(s64[i] - z["seven_f64"][i]) <= 1e-12 * abs(z["seven_f64"][i]), i
        assert abs(float(s32[i]) - z["seven_f64"][i]) <= gate_value(z["seven"][i], z["seven_f64"][i]), i
    stored = sorted(k[3:] for k in z.files if k.startswith("g__"))
    assert sorted(g64) == stored == sorted(meta["grad_dist"]) and "mel_linear.weight" in stored and "mel_linear.bias" in stored
    floor = 1e-12 * max(np.abs(z["g__" + k]).max() for k in stored)
    for k in stored:
        want = z["g__" + k]
        assert np.abs(g64[k] - want).max() <= 1e-12 * np.abs(want).max() + floor, k
        assert share_of(g32[k], want, grad_gate(meta, z, k))[0] <= 1.0, k
    assert tuple(z["g__mel_linear.weight"].shape) == (80, 256)
    assert z["g__txt_encoder.layer_stack.0.slf_attn.w_qs.weight"].shape == (len(tc.ROWS), 256)


def test_the_fixture_records_its_hazards(fixture):
    meta = fixture[0]
    assert meta["min_top2_gap_f64"] >= meta["gap_factor"] * meta["head_sum_dist_fp32_f64"]
    for n in ("output", "postnet_output"):
        assert meta[f"{n}_min_abs_error_f64"] >= meta["gap_factor"] * meta[f"{n}_dist_fp32_f64"], n
    # the one-element gradients: the recorded distance is not below one standard deviation of the error the sum collects
    floors = meta["one_element_grad_floor"]
    assert sorted(floors) == sorted(f"variance_adaptor.{p}_predictor.linear_layer.bias" for p in ("duration", "pitch", "energy"))
    for k, floor in floors.items():
        assert floor > 0 and meta["grad_dist"][k] >= floor, k
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "train_align_tiny.npz"))
    assert size < os.path.getsize(os.path.join(ROOT, "tests", "golden", "mel_encoder_tiny.npz"))


@pytest.mark.parametrize("mutate", ["residual_grad_one_operand", "d_targets_attached"])
def test_model_level_mutants_leave_the_gate_on_the_fixture(fixture, mutate):
    meta, z = fixture[:2]
    assert tc.CATCHER[mutate] in ("fixture", "mel_head")
    _, gm = _evaluate(fixture, torch.float64, mutate)
    worst = max(share_of(gm[k], z["g__" + k], grad_gate(meta, z, k))[0] for k in gm)
    assert worst > 100.0, (mutate, worst)
    # where: the residual's gradient reaches mel_linear and everything below it, the attached durations reach the aligner alone
    probe = "mel_linear.bias" if mutate == "residual_grad_one_operand" else "mel_encoder.layer_stack.3.crs_attn.w_qs.bias"
    assert share_of(gm[probe], z["g__" + probe], grad_gate(meta, z, probe))[0] > 100.0
    if mutate == "d_targets_attached":
        assert share_of(gm["mel_linear.bias"], z["g__mel_linear.bias"], grad_gate(meta, z, "mel_linear.bias"))[0] <= 1.0


# ---------------------------------------------------------------------------------------------------- the kernels' yardstick
@pytest.mark.parametrize("n_mel", tc.KERNEL_N_MEL)
@pytest.mark.parametrize("M", tc.KERNEL_M)
def test_kernel_emulation_against_plain_numpy(n_mel, M):
    c = tc.kernel_case(n_mel, M)
    dz, part = tc.pad_colsum(c["g"], n_mel, dz_before=c["dz_before"])
    assert dz.shape == (M, 128) and np.array_equal(dz[:, :n_mel].view(np.uint32), c["g"].view(np.uint32))
    assert not dz[:, n_mel:].any() and not np.signbit(dz[:, n_mel:]).any()
    assert part.shape == ((M + 63) // 64, n_mel) and part.dtype == np.float64
    exact = c["g"].astype(np.float64).sum(0)
    db = tc.d_bias(c["g"], n_mel)
    assert db.dtype == np.float32 and (np.abs(db.astype(np.float64) - exact) <= tc.colsum_bound(c["g"])).all()
    assert np.array_equal(tc.residual(c["p"], c["x"]), c["p"] + c["x"])
    dp, dx = tc.residual_backward(c["g"])
    assert dp is dx


def test_kernel_level_mutants_are_caught_on_their_named_case():
    for mutate in ("pad_columns_unwritten", "bias_fp32", "bias_valid_rows_only"):
        n_mel, M = tc.CATCHER[mutate]
        assert n_mel in tc.KERNEL_N_MEL and M in tc.KERNEL_M
        c = tc.kernel_case(n_mel, M)
        if mutate == "pad_columns_unwritten":
            good, _ = tc.pad_colsum(c["g"], n_mel, dz_before=c["dz_before"])
            bad, _ = tc.pad_colsum(c["g"], n_mel, dz_before=c["dz_before"], mutate=mutate)
            assert not np.array_equal(good.view(np.uint32), bad.view(np.uint32)) and np.isnan(bad[:, n_mel:]).all()
            continue
        v = tc.VALID_LENS
        assert v["B"] * v["T"] == M
        valid = tc.valid_rows(v["B"], v["T"], v["lens"])
        good, bad = tc.d_bias(c["g"], n_mel), tc.d_bias(c["g"], n_mel, mutate=mutate, valid=valid)
        assert not np.array_equal(good.view(np.uint32), bad.view(np.uint32)), mutate
        over = np.abs(bad.astype(np.float64) - c["g"].astype(np.float64).sum(0)) > tc.colsum_bound(c["g"])
        assert over.any(), (mutate, "colsum_bound must reject it as well")
    g = tc.kernel_case(80, 65)["g"]
    assert not np.array_equal(tc.residual_backward(g, "residual_grad_one_operand")[1], tc.residual_backward(g)[1])


@pytest.mark.parametrize("d", [256, 512])
def test_mel_head_closed_form_is_autograd(d):
    rs = np.random.RandomState(5)
    w = tc.seeded_mel_head(d, 80, 6)
    x, g = rs.standard_normal((2, 35, d)).astype(np.float32), rs.standard_normal((2, 35, 80)).astype(np.float32)
    leaves = dict(x=torch.as_tensor(x).double().requires_grad_(True), w=torch.as_tensor(w["w"]).double().requires_grad_(True),
                  b=torch.as_tensor(w["b"]).double().requires_grad_(True))
    y = tc.mel_head_statement(None, None, torch.float64, leaves)
    assert np.array_equal(y.detach().numpy(), tc.mel_head_statement(x, w).numpy())
    grads = torch.autograd.grad(y, [leaves["x"], leaves["w"], leaves["b"]], grad_outputs=torch.as_tensor(g).double())
    cf = tc.mel_head_closed_form(x, w, g)
    for n, t in zip(("dx", "w", "b"), grads):
        assert np.abs(cf[n] - t.numpy()).max() <= 1e-12 * np.abs(t.numpy()).max(), n
    valid = tc.valid_rows(2, 35, (35, 20))
    bad = tc.mel_head_closed_form(x, w, g, mutate="bias_valid_rows_only", valid=valid)
    assert np.abs(bad["b"] - cf["b"]).max() > 1e-3  # the reference sums the bias gradient over the padded rows too


# ---------------------------------------------------------------------------------------------------- the C ABI
NAMES = ("ns_mh_abi_version", "ns_mh_last_launches", "ns_mh_ws_bytes", "ns_mh_forward", "ns_mh_backward", "ns_mh_op_pad_colsum",
         "ns_mh_op_residual")


def test_abi_is_declared_everywhere(lib):
    L, so = lib
    assert so.ns_mh_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    assert re.findall(r"^#define NS_MH_ABI_VERSION (\d+)\b", header, re.M) == ["1"]
    for name in NAMES:
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    assert L.MH_NAMES == ("w", "b")
    assert [f for f, _ in L.NsMhShape._fields_] == ["B", "T", "d", "n_mel"] and [f for f, _ in L.NsMhGrads._fields_] == ["dx", "w", "b"]
    build = open(os.path.join(ROOT, "smart-nar_fast_tts_amd", "build.py")).read()
    assert '"melheadgrad.hip"' in build and '"melheadgrad_api.hip"' in build
    # the padded weight gradient lives in the shared core now, and the PostNet's ABI reaches it there
    core = open(os.path.join(ROOT, "smart-nar_fast_tts_amd", "csrc", "train_api.h")).read()
    pn = open(os.path.join(ROOT, "smart-nar_fast_tts_amd", "csrc", "postnetgrad_api.hip")).read()
    assert "int wgrad_narrow(" in core and "int wgrad_narrow(" not in pn and pn.count("counted.wgrad_narrow(") == 2


def _shape(L, B=2, T=8, d=256, n_mel=80):
    s = L.NsMhShape()
    s.B, s.T, s.d, s.n_mel = B, T, d, n_mel
    return s


DIMS = ((dict(B=0), "must be positive"), (dict(T=-2), "must be positive"), (dict(d=128), "d must be 256 or 512"), (dict(d=384), "d must be 256 or 512"),
        (dict(d=1024), "d must be 256 or 512"), (dict(n_mel=0), "n_mel must be a multiple of 16 in [16, 128]"), (dict(n_mel=-16), "n_mel must be"),
        (dict(n_mel=84), "n_mel must be a multiple of 16 in [16, 128]"), (dict(n_mel=144), "n_mel must be a multiple of 16 in [16, 128]"),
        (dict(B=1 << 12, T=1 << 11), "B * T * d must stay below 2^31"))


def test_sizes(lib):
    L, so = lib
    n = so.ns_mh_ws_bytes(C.byref(_shape(L)))
    assert n > 0 and n % 256 == 0
    for kw, msg in DIMS:
        assert so.ns_mh_ws_bytes(C.byref(_shape(L, **kw))) == 0 and msg in so.ns_last_error().decode(), kw
    assert so.ns_mh_ws_bytes(None) == 0 and "null argument" in so.ns_last_error().decode()
    for n_mel in (16, 48, 80, 96, 128):
        for d in (256, 512):
            assert so.ns_mh_ws_bytes(C.byref(_shape(L, n_mel=n_mel, d=d))) > 0, (n_mel, d)
    assert so.ns_mh_ws_bytes(C.byref(_shape(L, B=16, T=1000))) > so.ns_mh_ws_bytes(C.byref(_shape(L)))


def test_every_refusal_precedes_the_first_hip_call(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    ws_bytes = so.ns_mh_ws_bytes(C.byref(_shape(L)))

    def blocks(w, dg):
        k, d = L.NsMhWeights(), L.NsMhGrads()
        for i, f in enumerate(L.MH_NAMES):
            setattr(k, f, (w or {}).get(f, 0x1000000 + 0x100000 * i) or None)
            setattr(d, f, (dg or {}).get(f, 0x2000000 + 0x100000 * i) or None)
        d.dx = (dg or {}).get("dx", 0x2800000) or None
        return k, d

    def forward(shape=None, weights=None, w=None, x=0x3000000, y=0x5000000, ws=0x7000000, nbytes=None, **dims):
        k, _ = blocks(w, None)
        return so.ns_mh_forward(C.byref(_shape(L, **dims)) if shape is None else None, C.byref(k) if weights is None else None, P(x), P(y), P(ws),
                                ws_bytes if nbytes is None else nbytes, None)

    def backward(shape=None, weights=None, grads=None, w=None, dg=None, x=0x3000000, g=0x5000000, ws=0x7000000, nbytes=None, **dims):
        k, d = blocks(w, dg)
        return so.ns_mh_backward(C.byref(_shape(L, **dims)) if shape is None else None, C.byref(k) if weights is None else None, P(x), P(g),
                                 C.byref(d) if grads is None else None, P(ws), ws_bytes if nbytes is None else nbytes, None)

    def pad(g=0x1000000, M=16, n_mel=80, dz=0x3000000, d_bias=0x4000000, ws=0x7000000, nbytes=1 << 20):
        return so.ns_mh_op_pad_colsum(P(g), M, n_mel, P(dz), P(d_bias), P(ws), nbytes, None)

    def residual(p=0x1000000, x=0x2000000, M=16, n_mel=80, out=0x3000000):
        return so.ns_mh_op_residual(P(p), P(x), M, n_mel, P(out), None)

    both = DIMS + ((dict(shape=0), "null argument"), (dict(weights=0), "null argument"), (dict(ws=0), "null argument"), (dict(x=0), "null argument"),
                   (dict(w=dict(w=0)), "null weights->w"), (dict(w=dict(b=0)), "null weights->b"),
                   (dict(w=dict(w=0x1000004)), "weights->w must be 16-byte aligned"), (dict(w=dict(b=0x1100008)), "weights->b must be 16-byte aligned"),
                   (dict(x=0x3000004), "x must be 16-byte aligned"), (dict(ws=0x7000008), "the workspace must be 16-byte aligned"),
                   (dict(nbytes=ws_bytes - 1), "workspace too small (ns_mh_ws_bytes)"), (dict(nbytes=0), "workspace too small"))
    expect_refusals(err, forward, both + ((dict(y=0), "null argument"), (dict(y=0x500000c), "y must be 16-byte aligned")))
    expect_refusals(err, backward, both + (
        (dict(g=0), "null argument"), (dict(grads=0), "null argument"), (dict(g=0x5000004), "g must be 16-byte aligned"),
        (dict(dg=dict(dx=0x2800004)), "every gradient must be 16-byte aligned"), (dict(dg=dict(b=0x2100008)), "every gradient must be 16-byte aligned")))
    expect_refusals(err, pad, (
        (dict(g=0), "null argument"), (dict(dz=0), "null argument"), (dict(ws=0), "null argument"), (dict(M=0), "M must be positive"),
        (dict(n_mel=8), "n_mel must be a multiple of 16 in [16, 128]"), (dict(n_mel=132), "n_mel must be a multiple of 16"),
        (dict(M=1 << 24), "M * 128 must stay below 2^31"), (dict(dz=0x1000000), "out of place"), (dict(g=0x1000004), "g must be 16-byte aligned"),
        (dict(dz=0x3000008), "dz must be 16-byte aligned"), (dict(d_bias=0x4000004), "d_bias must be 16-byte aligned"),
        (dict(ws=0x7000004), "the workspace must be 16-byte aligned"), (dict(nbytes=16), "workspace too small: ")))
    expect_refusals(err, residual, (
        (dict(p=0), "null argument"), (dict(x=0), "null argument"), (dict(out=0), "null argument"), (dict(M=-1), "M must be positive"),
        (dict(n_mel=20), "n_mel must be a multiple of 16 in [16, 128]"), (dict(out=0x1000000), "out of place"), (dict(out=0x2000000), "out of place"),
        (dict(p=0x1000004), "p must be 16-byte aligned"), (dict(x=0x2000008), "x must be 16-byte aligned"), (dict(out=0x3000004), "out must be 16-byte aligned")))
    assert so.ns_mh_last_launches() == 0


def test_backward_with_no_output_wanted_launches_nothing(lib):
    L, so = lib
    s, k, d = _shape(L), L.NsMhWeights(), L.NsMhGrads()
    k.w, k.b = 0x1000000, 0x1100000
    P = C.c_void_p
    rc = so.ns_mh_backward(C.byref(s), C.byref(k), P(0x3000000), P(0x5000000), C.byref(d), P(0x7000000), so.ns_mh_ws_bytes(C.byref(s)), None)
    assert rc == 0 and so.ns_mh_last_launches() == 0  # every pointer of grads is null: validated, then nothing to do and no HIP call


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("mh_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("melheadgrad.hip", kernels=("k_mh_pad_colsum", "k_mh_residual"))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_state_dict_is_a_reference_checkpoint(lib, fixture):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import sublayers, training

    assert pkg.training is training and pkg.MelLinear is sublayers.MelLinear and "training" in pkg.__all__ and "MelLinear" in pkg.__all__
    meta, _, sd, (pcfg, cfg), _ = fixture
    m = training.FastSpeech2Align(pcfg, cfg)
    assert [n for n, _ in m.named_children()] == ["txt_encoder", "variance_adaptor", "mel_encoder", "mel_decoder", "mel_linear", "postnet"]
    # the reference's own names and shapes, in its order (recorded by the generator from the reference's state_dict())
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in meta["state_dict"]]
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert np.array_equal(m.mel_linear.weight.detach().numpy(), sd["mel_linear.weight"]) and m.training
    # workload's tables list the same entries: the inference subset, the aligner's, the two position tables the inference
    # subset regenerates, and the five num_batches_tracked
    cfg = wl.model_config("tiny")
    m = training.FastSpeech2Align(wl.preprocess_config(), cfg)
    want = dict(wl.inference_shapes(cfg))
    want.update(wl.aligner_shapes(cfg))
    want.update({f"{s}.position_enc": (1, cfg["max_seq_len"] + 1, 256) for s in ("txt_encoder", "mel_decoder")})
    want.update({f"postnet.convolutions.{i}.1.num_batches_tracked": () for i in range(5)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    # (workload.inference_shapes lists fc ahead of layer_norm, a module's state dict the other way round: the order is judged above)
    assert [k for k in m.state_dict() if k.startswith("mel_encoder.")] == list(wl.aligner_shapes(cfg))
    full = wl.synth_state_dict(cfg, seed=0)
    full.update(wl.synth_aligner_state_dict(cfg, seed=0))
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in full.items()}, strict=True)
    lin = sublayers.MelLinear(256)
    assert sorted(lin.state_dict()) == ["bias", "weight"] and tuple(lin.weight.shape) == (80, 256) and tuple(lin.bias.shape) == (80,)
    assert float(lin.weight.detach().abs().max()) <= 256 ** -0.5 and float(lin.bias.detach().abs().max()) <= 256 ** -0.5  # nn.Linear's initialisation


def test_python_raises_name_the_alternative(lib, fixture):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import checkpoint, sublayers, training

    _, _, _, (pcfg, cfg), batch = fixture
    m = training.FastSpeech2Align(pcfg, cfg)
    args = [torch.as_tensor(a) if isinstance(a, np.ndarray) else a for a in batch[2:]]
    with pytest.raises(NotImplementedError, match="model.FastSpeech2Align"):
        m(*args[:4])
    with pytest.raises(NotImplementedError, match="model.FastSpeech2Align"):
        m(*args[:5], None, *args[6:])
    with pytest.raises(NotImplementedError, match="inference path only"):
        m(*args, p_control=1.1)
    with pytest.raises(NotImplementedError, match="inference path only"):
        m(*args, e_control=0.9)
    with pytest.raises(ValueError, match="keep_masks takes the keys"):
        m(*args, keep_masks={"decoder": None})
    long = list(args)
    long[4], long[6] = torch.zeros(2, cfg["max_seq_len"] + 1, 80), cfg["max_seq_len"] + 1
    with pytest.raises(ValueError, match="must not exceed max_seq_len"):
        m(*long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(*args)
    with pytest.raises(NotImplementedError, match="multi_speaker"):
        training.FastSpeech2Align(pcfg, dict(cfg, multi_speaker=True))
    with pytest.raises(ValueError, match="decoder_hidden must be 256.*model.FastSpeech2Align"):
        training.FastSpeech2Align(wl.preprocess_config(), wl.model_config("tiny512"))
    with pytest.raises(NotImplementedError, match="checkpoint.get_model"):
        training.get_model(None, (pcfg, cfg, {}), "cpu", train=False)
    with pytest.raises(NotImplementedError):
        checkpoint.get_model(None, (pcfg, cfg, {}), "cpu", train=True)  # the inference module keeps refusing
    for kw, msg in ((dict(d=128), "d must be 256 or 512"), (dict(d=256, n_mel=84), "n_mel must be a multiple of 16")):
        with pytest.raises(ValueError, match=msg):
            sublayers.MelLinear(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sublayers.MelLinear(256)(torch.zeros(2, 3, 256))
    with pytest.raises(RuntimeError, match="no CPU path"):
        training.add_residual(torch.zeros(2, 3, 80), torch.zeros(2, 3, 80))
