"""The yardstick of tests/test_gpu_mel_encoder.py proven on the CPU, and every refusal of the ns_me_* family (no GPU).

On the fixture (tests/golden/mel_encoder_tiny.npz, the reference's own MelEncoder at dropout 0) the float64 restatement agrees with the
reference's float64 forward and autograd to <= 1e-12 relative, and the fp32 restatement stays inside the project gate
(tests/util.gate_value) taken from the fixture's own fp32 and float64 values.  (d_bk of an attention is zero in exact arithmetic — the
softmax does not see a key bias — so its bounds are taken from d_bq's, as tests/test_stacks_host.py does.)  Frame 0 of d_mels and the rows
past the truncation are exactly 0.

The mutants: each leaves bit-equality with the yardstick on the case tests/mel_encoder_cpu.CATCHER names (the Prenet-level one,
frame0_not_zeroed, on the fixture's "train" inputs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mel_encoder_cpu as mc
from tests import stacks_cpu as sc
from tests.util import assert_no_spill, built_lib, expect_refusals, gate_value, load_golden, run_c_caller, share_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def _stack(meta):
    return mc.seeded_stack(meta["d"], meta["d_hid"], meta["kernel"], meta["n_layers"], meta["seed"])


# ---------------------------------------------------------------------------------------------------- the stack's yardstick
@pytest.mark.parametrize("c", ["train", "eval", "trunc", "long_eval"])
def test_restatement_reproduces_the_reference(c):
    meta, z = load_golden("mel_encoder_tiny")
    case = meta["cases"][c]
    w = _stack(meta)
    src, mels, g, a = mc.fixture_inputs(meta, c)
    stored = sorted(k[len(c) + 3:] for k in z.files if k.startswith(f"{c}_d_") and not k.endswith("_f64"))
    assert bool(stored) == case["training"]
    got = {}
    for dtype in (torch.float32, torch.float64):
        if stored:
            got[dtype] = mc.autograd_ref(w, src, mels, meta["src_lens"], case["mel_lens"], meta["H"], g, a, meta["max_seq_len"], True, dtype=dtype)
        else:
            with torch.no_grad():
                y, attns, _ = mc.statement(mc.leaves_of(w, dtype, src, mels), meta["src_lens"], case["mel_lens"], meta["H"], meta["max_seq_len"],
                                           False, dtype=dtype)
            got[dtype] = (y.numpy(), [t.numpy() for t in attns], {})
    y64 = got[torch.float64][0]
    rows = y64.shape[1]
    assert y64.shape == z[f"{c}_y_f64"].shape
    pad = sc.pad_of([min(n, rows) for n in case["mel_lens"]], rows)
    assert not y64[pad].any() and not z[f"{c}_y"][pad].any()

    def check(key, a32, a64, gate_key=None, scale=None):
        want32, want64 = z[key], z[key + "_f64"]
        gate = gate_value(z[gate_key or key], z[(gate_key or key) + "_f64"])
        s32 = share_of(a32, want64, gate)[0]
        e64 = np.abs(a64 - want64).max()
        print(f"{key}: fp32 share of the gate {s32:.3g}, float64 {e64:.3g}")
        assert a32.shape == want32.shape and s32 <= 1.0, key
        assert e64 <= 1e-12 * (scale if scale is not None else np.abs(want64).max()), key

    check(f"{c}_y", got[torch.float32][0], y64)
    for i in range(meta["n_layers"]):
        check(f"{c}_attn{i}", got[torch.float32][1][i], got[torch.float64][1][i])
        key_pad = sc.pad_of(meta["src_lens"], meta["L"])
        assert not np.moveaxis(z[f"{c}_attn{i}"], 3, 1)[key_pad].any()  # exact 0 at padded phonemes
    if stored:
        scale = max(np.abs(z[f"{c}_d_{n}_f64"]).max() for n in stored)
        rows_of = lambda n, t: t[list(mc.ROWS)] if t.ndim == 2 else t  # noqa: E731  (a weight matrix: the stored rows)
        for n in stored:
            bk = n.endswith("_a_bk")  # zero up to rounding: bounds from d_bq, relative to the gradients' common scale
            check(f"{c}_d_{n}", rows_of(n, got[torch.float32][2][n]), rows_of(n, got[torch.float64][2][n]), f"{c}_d_{n[:-1]}q" if bk else None,
                  scale if bk else None)
        for dtype in got:
            assert not got[dtype][2]["dmels"][:, 0].any() and not got[dtype][2]["dmels"][:, rows:].any()
        assert not z[f"{c}_d_dmels"][:, 0].any() and not z[f"{c}_d_dmels_f64"][:, 0].any()
        want = [n for n in mc.grad_names(meta["n_layers"]) if not re.search(r"_(wq|wk|wv|wfc|w1|w2)$", n) or n in ("P_w1", "P_w2", "L0_a_wq")]
        assert sorted(stored) == sorted(want)
    if c == "trunc":
        assert rows == meta["max_seq_len"] < mels.shape[1] and not z["trunc_d_dmels"][:, rows:].any()
        assert np.abs(z["trunc_d_dmels"][:, 1:rows]).max() > 0
    if c == "long_eval":
        assert rows == mels.shape[1] > meta["max_seq_len"]


def test_prenet_closed_form_is_the_autograd_of_its_statement():
    meta, _ = load_golden("mel_encoder_tiny")
    w = _stack(meta)["prenet"]
    _, mels, g, _ = mc.fixture_inputs(meta, "train")
    B, T, _ = mels.shape
    rs = np.random.RandomState(5)
    keep = (rs.random_sample((B, T, mc.D_PRENET)) >= 0.2).astype(np.uint8)
    pos = sc.position_table(T, mc.D_PRENET, meta["max_seq_len"], True)[0]
    for k, p in ((None, 0.0), (keep, 0.2)):
        leaves = {n: v.clone().requires_grad_(True) for n, v in mc._pw(w, torch.float64).items()}
        leaves["mels"] = torch.from_numpy(mels).double().requires_grad_(True)
        out = mc.prenet_statement(None, None, pos, k, p, torch.float64, leaves)
        grads = torch.autograd.grad(out["y"], [leaves[n] for n in ("w1", "b1", "w2", "b2", "mels")], grad_outputs=torch.from_numpy(g).double())
        cf = mc.prenet_closed_form(mels, w, g, (out["h1"].detach().numpy(), out["h2"].detach().numpy()), k, p)
        for n, t in zip(mc.PRENET_NAMES, grads):
            assert np.abs(cf[n] - t.numpy()).max() <= 1e-12 * np.abs(t.numpy()).max(), n
        assert not cf["dmels"][:, 0].any()
        # the two kernels' statements are the same expressions, rounded once
        y32 = mc.drop_pos(out["h2"].detach().numpy().astype(np.float32).reshape(B * T, -1), pos, None if k is None else k.reshape(B * T, -1), p, T)
        h2_32 = out["h2"].detach().numpy().astype(np.float32).astype(np.float64)
        want = h2_32 * (1.0 if k is None else k * np.float64(mc.scale_of(p))) + pos[None].astype(np.float64)
        assert np.array_equal(y32.reshape(B, T, -1), want.astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the mutants
@pytest.mark.parametrize("mutant", [m for m in mc.MUTANTS if m != "frame0_not_zeroed"])
def test_bit_equality_rejects_the_kernel_mutants(mutant):
    B, T = 3, 33
    for F in mc.KERNEL_WIDTHS:
        changed = set()
        for case in mc.KERNEL_CASES:
            k = mc.kernel_case(case, B, T, F)
            y, ym = mc.drop_pos(k["h2"], k["pos"], k["keep"], k["p"], T), mc.drop_pos(k["h2"], k["pos"], k["keep"], k["p"], T, mutant)
            (dh, s), (dhm, sm) = mc.drop_relu_gate(k["g"], k["h2"], k["keep"], k["p"]), mc.drop_relu_gate(k["g"], k["h2"], k["keep"], k["p"], mutant)
            if case != "nan_h2":
                assert np.isfinite(dh).all() and np.isfinite(s).all(), "nothing behind a dropped or gated element reaches dh or a sum"
            same = np.array_equal(y.view(np.uint32), ym.view(np.uint32)) and np.array_equal(dh.view(np.uint32), dhm.view(np.uint32))
            if not same:
                changed.add(case)
        print(f"{mutant} F {F}: other bits on {sorted(changed)}")
        assert mc.CATCHER[mutant] in changed
        if mutant == "multiply_not_select":  # a multiply lets the planted NaN through, and writes -0.0 where g < 0 even on finite data
            assert changed == set(mc.KERNEL_CASES)


def test_kernel_cases_hold_what_they_promise():
    k = mc.kernel_case("nan_g", 2, 70, 256)
    closed = (k["keep"] == 0) | ~(k["h2"] > 0)
    assert not np.isfinite(k["g"][closed]).any() and np.isfinite(k["g"][~closed]).all() and closed.any() and (~closed).any()
    dh, s = mc.drop_relu_gate(k["g"], k["h2"], k["keep"], k["p"])
    assert not dh[closed].any() and not np.signbit(dh[closed]).any() and (dh[~closed] != 0).all()
    assert (np.abs(s.astype(np.float32).astype(np.float64) - s) <= mc.colsum_bound(dh)).all()
    k = mc.kernel_case("nan_h2", 3, 33, 512)
    dh, _ = mc.drop_relu_gate(k["g"], k["h2"], k["keep"], k["p"])
    assert np.isnan(k["h2"]).any() and np.isfinite(dh).all() and not dh[np.isnan(k["h2"])].any()
    assert float(mc.scale_of(0.0)) == 1.0 and float(mc.scale_of(0.5)) == 2.0


def test_frame0_mutant_leaves_bit_equality():
    meta, _ = load_golden("mel_encoder_tiny")
    w = _stack(meta)["prenet"]
    _, mels, g, _ = mc.fixture_inputs(meta, "train")
    pos = sc.position_table(mels.shape[1], mc.D_PRENET, meta["max_seq_len"], True)[0]
    out = mc.prenet_statement(mels, w, pos, dtype=torch.float32)
    saved = (out["h1"].numpy(), out["h2"].numpy())
    good, bad = (mc.prenet_closed_form(mels, w, g, saved, dtype=torch.float32, mutate=m) for m in (None, "frame0_not_zeroed"))
    assert not good["dmels"][:, 0].any() and bad["dmels"][:, 0].any()
    assert np.array_equal(good["dmels"][:, 1:], bad["dmels"][:, 1:]) and all(np.array_equal(good[n], bad[n]) for n in mc.PRENET_NAMES[:4])


# ---------------------------------------------------------------------------------------------------- versions and refusals (no device work)
NAMES = ("ns_me_abi_version", "ns_me_last_launches", "ns_me_ws_bytes", "ns_me_saved_bytes", "ns_me_forward", "ns_me_backward", "ns_me_op_drop_pos",
         "ns_me_op_drop_relu_gate")


def test_version(lib):
    L, so = lib
    assert so.ns_me_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    assert re.findall(r"^#define NS_ME_ABI_VERSION (\d+)\b", header, re.M) == ["1"]
    for name in NAMES:
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    assert L.ME_NAMES == ("w1", "b1", "w2", "b2")
    assert [f for f, _ in L.NsMeShape._fields_] == ["B", "T", "n_mel", "d"] and [f for f, _ in L.NsMeGrads._fields_] == ["dmels", "w1", "b1", "w2", "b2"]


def _shape(L, B=2, T=8, n_mel=80, d=256):
    s = L.NsMeShape()
    s.B, s.T, s.n_mel, s.d = B, T, n_mel, d
    return s


def test_sizes(lib):
    L, so = lib
    s = _shape(L)
    assert so.ns_me_saved_bytes(C.byref(s)) == 2 * 8 * (80 + 2 * 256) * 4
    assert so.ns_me_ws_bytes(C.byref(s)) > 0 and so.ns_me_ws_bytes(C.byref(s)) % 256 == 0
    for kw, msg in ((dict(d=128), "d must be 256 or 512"), (dict(n_mel=82), "n_mel must be a positive multiple of 4"), (dict(n_mel=0), "n_mel must be"),
                    (dict(B=0), "must be positive"), (dict(T=-1), "must be positive"), (dict(B=1 << 12, T=1 << 11), "B * T * d must stay below 2^31"),
                    (dict(B=1 << 10, T=1 << 11, n_mel=1024), "B * T * n_mel must stay below 2^31"),
                    # multiples of 4 that pass check_dims and reach the carve: the GEMM dispatch takes Cin only as a multiple of 16
                    (dict(n_mel=4), "the Conv1D-as-GEMM dispatch refuses this shape"), (dict(n_mel=20), "the Conv1D-as-GEMM dispatch refuses this shape"),
                    (dict(n_mel=84), "the Conv1D-as-GEMM dispatch refuses this shape")):
        s = _shape(L, **kw)
        assert so.ns_me_ws_bytes(C.byref(s)) == 0 and msg in so.ns_last_error().decode(), kw
        assert so.ns_me_saved_bytes(C.byref(s)) == 0 and msg in so.ns_last_error().decode(), kw
    assert so.ns_me_ws_bytes(None) == 0 and "null argument" in so.ns_last_error().decode()
    for n_mel in (16, 48, 80, 96):  # the multiples of 16 pass
        assert so.ns_me_ws_bytes(C.byref(_shape(L, n_mel=n_mel))) > 0, n_mel


def test_every_refusal_precedes_the_first_hip_call(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    ws_bytes = so.ns_me_ws_bytes(C.byref(_shape(L)))

    def blocks(w, dg):
        k, d = L.NsMeWeights(), L.NsMeGrads()
        for i, f in enumerate(L.ME_NAMES):
            setattr(k, f, (w or {}).get(f, 0x1000000 + 0x100000 * i) or None)
            setattr(d, f, (dg or {}).get(f, 0x2000000 + 0x100000 * i) or None)
        d.dmels = (dg or {}).get("dmels", 0x2800000) or None
        return k, d

    def forward(shape=None, w=None, mels=0x3000000, pos=0x4000000, keep=0, p=0.0, y=0x5000000, saved=0x6000000, ws=0x7000000, nbytes=None, **dims):
        k, _ = blocks(w, None)
        s = _shape(L, **dims)
        return so.ns_me_forward(C.byref(s) if shape is None else None, C.byref(k), P(mels), P(pos), P(keep), p, P(y), P(saved), P(ws),
                                ws_bytes if nbytes is None else nbytes, None)

    def backward(shape=None, w=None, dg=None, keep=0, p=0.0, saved=0x6000000, g=0x5000000, ws=0x7000000, nbytes=None, **dims):
        k, d = blocks(w, dg)
        s = _shape(L, **dims)
        return so.ns_me_backward(C.byref(s) if shape is None else None, C.byref(k), P(keep), p, P(saved), P(g), C.byref(d), P(ws),
                                 ws_bytes if nbytes is None else nbytes, None)

    def drop_pos(h2=0x1000000, pos=0x2000000, keep=0, p=0.0, B=2, T=8, d=256, y=0x3000000):
        return so.ns_me_op_drop_pos(P(h2), P(pos), P(keep), p, B, T, d, P(y), None)

    def gate(g=0x1000000, h2=0x2000000, keep=0, p=0.0, M=16, d=256, dh=0x3000000, d_b2=0x4000000, ws=0x7000000, nbytes=1 << 20):
        return so.ns_me_op_drop_relu_gate(P(g), P(h2), P(keep), p, M, d, P(dh), P(d_b2), P(ws), nbytes, None)

    dims = ((dict(B=0), "must be positive"), (dict(T=-2), "must be positive"), (dict(d=128), "d must be 256 or 512"), (dict(d=384), "d must be 256 or 512"),
            (dict(d=1024), "d must be 256 or 512"), (dict(n_mel=0), "n_mel must be a positive multiple of 4"), (dict(n_mel=-4), "n_mel must be"),
            (dict(n_mel=81), "n_mel must be a positive multiple of 4"), (dict(B=1 << 12, T=1 << 11), "B * T * d must stay below 2^31"),
            (dict(B=1 << 10, T=1 << 11, n_mel=1024), "B * T * n_mel must stay below 2^31"),
            (dict(n_mel=4), "the Conv1D-as-GEMM dispatch refuses this shape"), (dict(n_mel=20), "the Conv1D-as-GEMM dispatch refuses this shape"))
    drop = ((dict(p=-0.1), "p_drop must lie in [0, 1)"), (dict(p=1.0), "p_drop must lie in [0, 1)"), (dict(p=float("nan")), "p_drop must lie in [0, 1)"),
            (dict(p=0.2), "p_drop > 0 needs a keep-mask"), (dict(keep=0x8000000), "keep-mask given although p_drop == 0"),
            (dict(p=0.2, keep=0x8000004), "the keep-mask must be 16-byte aligned"))
    both = dims + drop + ((dict(shape=0), "null argument"), (dict(ws=0), "null argument"), (dict(w=dict(w1=0)), "null weights->w1"),
                          (dict(w=dict(b2=0)), "null weights->b2"), (dict(w=dict(w2=0x1000004)), "weights->w2 must be 16-byte aligned"),
                          (dict(saved=0x6000004), "saved must be 16-byte aligned"), (dict(ws=0x7000008), "the workspace must be 16-byte aligned"),
                          (dict(nbytes=ws_bytes - 1), "workspace too small (ns_me_ws_bytes)"), (dict(nbytes=0), "workspace too small"))
    expect_refusals(err, forward, both + (
        (dict(mels=0), "null argument"), (dict(pos=0), "null argument"), (dict(y=0), "null argument"), (dict(mels=0x3000004), "mels must be 16-byte aligned"),
        (dict(pos=0x4000008), "pos must be 16-byte aligned"), (dict(y=0x500000c), "y must be 16-byte aligned")))
    expect_refusals(err, backward, both + (
        (dict(saved=0), "null argument"), (dict(g=0), "null argument"), (dict(g=0x5000004), "g must be 16-byte aligned"),
        (dict(dg=dict(dmels=0x2800004)), "every gradient must be 16-byte aligned"), (dict(dg=dict(b1=0x2000008)), "every gradient must be 16-byte aligned")))
    expect_refusals(err, drop_pos, drop + (
        (dict(h2=0), "null argument"), (dict(pos=0), "null argument"), (dict(y=0), "null argument"), (dict(B=0), "must be positive"),
        (dict(T=0), "must be positive"), (dict(d=128), "d must be 256 or 512"), (dict(B=1 << 12, T=1 << 11), "must stay below 2^31"),
        (dict(y=0x1000000), "out of place"), (dict(h2=0x1000004), "h2 must be 16-byte aligned"), (dict(pos=0x2000008), "pos must be 16-byte aligned"),
        (dict(y=0x3000004), "y must be 16-byte aligned")))
    expect_refusals(err, gate, drop + (
        (dict(g=0), "null argument"), (dict(h2=0), "null argument"), (dict(dh=0), "null argument"), (dict(ws=0), "null argument"),
        (dict(M=0), "M must be positive"), (dict(d=768), "d must be 256 or 512"), (dict(M=1 << 23), "must stay below 2^31"),
        (dict(dh=0x1000000), "out of place"), (dict(g=0x1000004), "g must be 16-byte aligned"), (dict(d_b2=0x4000004), "d_b2 must be 16-byte aligned"),
        (dict(nbytes=16), "workspace too small: ")))
    assert so.ns_me_last_launches() == 0


def test_backward_with_no_output_wanted_launches_nothing(lib):
    L, so = lib
    s, k, d = _shape(L), L.NsMeWeights(), L.NsMeGrads()
    for i, f in enumerate(L.ME_NAMES):
        setattr(k, f, 0x1000000 + 0x100000 * i)
    P = C.c_void_p
    rc = so.ns_me_backward(C.byref(s), C.byref(k), None, 0.0, P(0x6000000), P(0x5000000), C.byref(d), P(0x7000000), so.ns_me_ws_bytes(C.byref(s)), None)
    assert rc == 0 and so.ns_me_last_launches() == 0  # every pointer of grads is null: validated, then nothing to do and no HIP call


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("me_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("melencgrad.hip", kernels=("k_me_drop_pos", "k_me_drop_relu_gate"))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_modules_have_the_reference_names_and_no_cpu_path(lib):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import stacks, sublayers

    assert pkg.MelEncoder is stacks.MelEncoder and pkg.Prenet is sublayers.Prenet and pkg.FFTBlock2 is sublayers.FFTBlock2
    meta, _ = load_golden("mel_encoder_tiny")
    t = dict(conv_filter_size=256, conv_kernel_size=meta["kernel"], decoder_hidden=256, decoder_head=meta["H"], decoder_layer=meta["n_layers"], decoder_dropout=0.1)
    m = stacks.MelEncoder({"max_seq_len": meta["max_seq_len"], "transformer": t})
    # the reference's own names, in its order, and its shapes with the fixture's d_inner (64) replaced by one the kernels are built for
    want = [(k, tuple({meta["d_hid"]: 256}.get(n, n) for n in shape)) for k, shape in meta["state_dict"]]
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == ["position_enc"] and not list(m.named_buffers())
    # workload.aligner_shapes lists the same names and shapes, and the seeded mel_encoder.* slice loads strictly
    cfg = wl.model_config("tiny")
    m = stacks.MelEncoder(cfg)
    shapes = wl.aligner_shapes(cfg)
    assert {"mel_encoder." + k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(shapes)
    assert ["mel_encoder." + k for k in m.state_dict()] == list(shapes)
    built = m.position_enc.detach().numpy().copy()
    asd = wl.synth_aligner_state_dict(cfg, seed=0)
    assert built.tobytes() == np.asarray(asd["mel_encoder.position_enc"]).tobytes()
    m.load_state_dict({k[len("mel_encoder."):]: torch.as_tensor(np.asarray(v)) for k, v in asd.items()})  # strict
    assert m.position_enc.detach().numpy().tobytes() == built.tobytes() and m.training
    assert np.array_equal(m.prenet.w_1.weight.detach().numpy(), np.asarray(asd["mel_encoder.prenet.w_1.weight"]))
    p = sublayers.Prenet()
    assert sorted(p.state_dict()) == ["w_1.bias", "w_1.weight", "w_2.bias", "w_2.weight"] and p.p_drop == 0.2
    assert tuple(p.w_1.weight.shape) == (256, 80) and tuple(p.w_2.weight.shape) == (256, 256)
    p.load_state_dict({k[len("mel_encoder.prenet."):]: torch.as_tensor(np.asarray(v)) for k, v in asd.items() if k.startswith("mel_encoder.prenet.")})
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 5, 256), torch.zeros(2, 7, 80), torch.zeros(2, 5, dtype=torch.bool), torch.zeros(2, 7, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        p(torch.zeros(2, 7, 80), torch.zeros(7, 256))
    wide = {"max_seq_len": 12, "transformer": dict(t, decoder_hidden=512)}
    with pytest.raises(ValueError, match="decoder_hidden must be 256"):
        stacks.MelEncoder(wide)
    # the older stacks keep their parameter names after the shared base learnt about a second kind of block
    assert "layer_stack.0.slf_attn.w_qs.weight" in stacks.MelDecoder(cfg).state_dict() and "src_word_emb.weight" in stacks.TxtEncoder(cfg).state_dict()
