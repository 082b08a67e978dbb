"""The trainable FastSpeech2Align on the GPU (csrc/melheadgrad.hip through ns_mh_*, sublayers.MelLinear, smart_nar_fast_tts_amd.training).

The two new kernels alone first, bit-equal to tests/train_align_cpu.py's emulations at n_mel in {16, 80, 128} and M in {1, 63, 64, 65,
140}: dz pre-filled with NaN bytes, the partials wanted and not wanted, d_bias bit-equal to the replayed order and inside
``colsum_bound`` of the exact column sum, two runs bit-equal.

Then MelLinear through ns_mh_forward / ns_mh_backward at d in {256, 512} and (B, T) in {(1, 1), (3, 33), (2, 70)}: y and the three
gradients against float64 at the project gate (tests/util.gate_value), the launch counts include/nar_fs2.h states, and every
needs_input_grad combination dropping what the header says it drops.

Then the whole model: in eval() on teacher_tiny.npz (the reference's own forward, full ljspeech config) at the fixture's gates; in
train() at dropout 0 on train_align_tiny.npz (the reference's own training step) — the seven losses and every stored gradient at the
gate; in train() with given keep-masks against the hand chain, bit for bit; two optimiser steps through ``train_step``; and the round
trip of the trained state dict into the inference class.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/train_step.md is written from one)."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from tests import mel_encoder_cpu as mc
from tests import optim_cpu as oc
from tests import train_align_cpu as tc
from tests.util import ROOT, dev, gate_value, gates, load_golden, native_lib, report, share_of, shares, weights_for

pytestmark = pytest.mark.gpu
SHAPES = mc.KERNEL_SHAPES  # (1, 1), (3, 33), (2, 70): one row, a partial 64-row block, past one block


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _G(lib, M, N, Cin):
    """G(M, N, Cin) of include/nar_fs2.h: the Conv1D-as-GEMM dispatch's own launch count at KW = 1"""
    n = lib.ns_plan_gemm_launches(M, N, Cin, 1, 0, None)
    assert n in (1, 2)
    return n


def _nan_bytes(*shape):
    n = int(np.prod(shape))
    return torch.full((n * 4,), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32).reshape(*shape)


# ---------------------------------------------------------------------------------------------------- the two kernels alone
@pytest.mark.parametrize("M", tc.KERNEL_M)
@pytest.mark.parametrize("n_mel", tc.KERNEL_N_MEL)
def test_kernels_alone(so, n_mel, M):
    L, lib = so
    c = tc.kernel_case(n_mel, M)
    want_dz, part = tc.pad_colsum(c["g"], n_mel, dz_before=c["dz_before"])
    want_b = tc.bias_finish(part)
    exact, bound = c["g"].astype(np.float64).sum(0), tc.colsum_bound(c["g"])
    want_out = tc.residual(c["p"], c["x"])
    nblk = (M + 63) // 64
    runs = []
    for _ in range(2):
        g_d, out = dev(c["g"]), {}
        for with_bias in (True, False):
            dz = _nan_bytes(M, 128)
            assert torch.isnan(dz).all()
            db = _nan_bytes(n_mel) if with_bias else None
            ws = torch.full((nblk * n_mel * 8,), 0xFF, dtype=torch.uint8, device="cuda") if with_bias else None
            L.check(lib.ns_mh_op_pad_colsum(L.ptr(g_d), M, n_mel, L.ptr(dz), L.ptr(db), L.ptr(ws), 0 if ws is None else ws.numel(), L.stream_ptr()),
                    "ns_mh_op_pad_colsum")
            assert lib.ns_mh_last_launches() == (2 if with_bias else 1)  # the pad, and the finish of d_bias
            out["dz" if with_bias else "dz_alone"] = dz.cpu().numpy()
            if with_bias:
                out["b"] = db.cpu().numpy()
        p_d, x_d, o = dev(c["p"]), dev(c["x"]), _nan_bytes(M, n_mel)
        L.check(lib.ns_mh_op_residual(L.ptr(p_d), L.ptr(x_d), M, n_mel, L.ptr(o), L.stream_ptr()), "ns_mh_op_residual")
        assert lib.ns_mh_last_launches() == 1
        out["out"] = o.cpu().numpy()
        assert g_d.cpu().numpy().tobytes() == c["g"].tobytes() and p_d.cpu().numpy().tobytes() == c["p"].tobytes() and \
            x_d.cpu().numpy().tobytes() == c["x"].tobytes(), "g, p and x are only read"
        runs.append(out)
    got = runs[0]
    for n in ("dz", "dz_alone"):
        assert got[n].view(np.uint32).tobytes() == want_dz.view(np.uint32).tobytes(), "dz is g, then +0.0 up to column 128, bit for bit"
    assert got["b"].view(np.uint32).tobytes() == want_b.view(np.uint32).tobytes(), "d_bias is the replayed order's, bit for bit"
    err = np.abs(got["b"].astype(np.float64) - exact)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    report(test="mh_kernels", n_mel=n_mel, M=M, d_bias=worst)
    assert np.isfinite(got["b"]).all() and (err <= bound).all(), worst
    assert got["out"].view(np.uint32).tobytes() == want_out.view(np.uint32).tobytes(), "out = p + x, one rounding"
    for n in got:
        assert got[n].tobytes() == runs[1][n].tobytes(), ("two runs are bit-equal", n)


# ---------------------------------------------------------------------------------------------------- mel_linear through the two C calls
def _head_inputs(Bc, Tc, d, n_mel=80, seed=0):
    rs = np.random.RandomState(1200 + seed + 31 * Bc + Tc + d)
    return rs.standard_normal((Bc, Tc, d)).astype(np.float32), rs.standard_normal((Bc, Tc, n_mel)).astype(np.float32), tc.seeded_mel_head(d, n_mel, 1300 + d)


def _head_raw(L, lib, x, g, w, want=(True, True, True)):
    """ns_mh_forward + ns_mh_backward by hand: (y, {dx, w, b: gradient or None}, launches)"""
    Bc, Tc, d = x.shape
    n_mel = g.shape[2]
    s = L.NsMhShape()
    s.B, s.T, s.d, s.n_mel = Bc, Tc, d, n_mel
    wd = {n: dev(w[n]) for n in L.MH_NAMES}
    k = L.NsMhWeights()
    k.w, k.b = wd["w"].data_ptr(), wd["b"].data_ptr()
    ws = torch.full((lib.ns_mh_ws_bytes(C.byref(s)),), 0xFF, dtype=torch.uint8, device="cuda")
    x_d, g_d = dev(x), dev(g)
    y = _nan_bytes(Bc, Tc, n_mel)
    L.check(lib.ns_mh_forward(C.byref(s), C.byref(k), L.ptr(x_d), L.ptr(y), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_mh_forward")
    launches = {"forward": lib.ns_mh_last_launches()}
    shapes = dict(dx=(Bc, Tc, d), w=(n_mel, d), b=(n_mel,))
    outs = {n: _nan_bytes(*shapes[n]) if wanted else None for n, wanted in zip(("dx", "w", "b"), want)}
    dg = L.NsMhGrads()
    for n, o in outs.items():
        setattr(dg, n, None if o is None else o.data_ptr())
    L.check(lib.ns_mh_backward(C.byref(s), C.byref(k), L.ptr(x_d), L.ptr(g_d), C.byref(dg), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_mh_backward")
    launches["backward"] = lib.ns_mh_last_launches()
    assert x_d.cpu().numpy().tobytes() == x.tobytes() and g_d.cpu().numpy().tobytes() == g.tobytes(), "x and g are only read"
    return y.cpu().numpy(), {n: None if o is None else o.cpu().numpy() for n, o in outs.items()}, launches


def _head_counts(lib, M, d, n_mel, want=(True, True, True)):
    """the table of include/nar_fs2.h"""
    dx, w, b = want
    return _G(lib, M, n_mel, d), (1 if (w or b) else 0) + (1 if b else 0) + (3 if w else 0) + ((1 + _G(lib, M, d, n_mel)) if dx else 0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("d", [256, 512])
def test_mel_linear_forward_and_backward(so, d, shape):
    L, lib = so
    Bc, Tc = shape
    x, g, w = _head_inputs(Bc, Tc, d)
    y, grads, launches = _head_raw(L, lib, x, g, w)
    ref = {}
    for dt in (torch.float32, torch.float64):
        ref[dt] = dict(tc.mel_head_closed_form(x, w, g, dt), y=tc.mel_head_statement(x, w, dt).numpy())
    sh = shares(dict(grads, y=y), ref[torch.float64], gates(ref[torch.float32], ref[torch.float64], ("y", "dx", "w", "b")))
    report(test="mh_linear", d=d, shape=f"{Bc}x{Tc}", launches=launches, shares=sh)
    assert max(sh.values()) <= 1.0, sh
    # d_bias is the kernel's replayed order on g, bit for bit
    assert grads["b"].view(np.uint32).tobytes() == tc.d_bias(g.reshape(Bc * Tc, -1), 80).view(np.uint32).tobytes()
    assert launches == dict(zip(("forward", "backward"), _head_counts(lib, Bc * Tc, d, 80))), launches
    assert launches["backward"] == 6 + _G(lib, Bc * Tc, d, 80)


def test_mel_linear_module_needs_input_grad_and_run_to_run_bits(so):
    from smart_nar_fast_tts_amd import sublayers

    L, lib = so
    Bc, Tc, d = 3, 33, 256
    M = Bc * Tc
    x, g, w = _head_inputs(Bc, Tc, d, seed=1)
    m = sublayers.MelLinear(d)
    m.load_state_dict({"weight": torch.from_numpy(w["w"]), "bias": torch.from_numpy(w["b"])})
    m = m.cuda()
    params = m.ordered_parameters()
    raw = _head_raw(L, lib, x, g, w)

    def once(x_grad, need_w, need_b):
        for p, need in zip(params, (need_w, need_b)):
            p.requires_grad_(need)
            p.grad = None
        xd = dev(x).requires_grad_(x_grad)
        y = m(xd)
        y.backward(dev(g))
        return y.detach().cpu().numpy(), xd.grad, params[0].grad, params[1].grad, dict(m.last_launches)

    try:
        for want in itertools.product((True, False), repeat=3):
            if not any(want):
                continue  # (no autograd node: the plain forward; the all-null backward is a host test)
            for rep in range(2 if all(want) else 1):  # two runs give identical bits
                y, dx, dw, db, launches = once(*want)
                assert y.tobytes() == raw[0].tobytes(), "the module is the two C calls"
                for n, t, wanted in zip(("dx", "w", "b"), (dx, dw, db), want):
                    assert (t is not None) == wanted and (t is None or t.cpu().numpy().tobytes() == raw[1][n].tobytes()), (want, n)
                assert launches == dict(zip(("forward", "backward"), _head_counts(lib, M, d, 80, want))), (want, launches)
        with torch.no_grad():
            quiet = m(dev(x))
        assert quiet.cpu().numpy().tobytes() == raw[0].tobytes() and not quiet.requires_grad
        assert m.last_launches["forward"] == _G(lib, M, 80, d)
    finally:
        for p in params:
            p.requires_grad_(True)
            p.grad = None


def test_wgrad_narrow_of_the_postnet_still_counts_three(so):
    """the helper moved into the shared core: ns_pn_op_wgrad_narrow makes the same three launches and counts them into ns_pn's counter"""
    L, lib = so
    Bc, S, N, Cin, K = 2, 37, 80, 256, 5
    rs = np.random.RandomState(77)
    dz = np.zeros((Bc * S, 128), dtype=np.float32)
    dz[:, :N] = rs.standard_normal((Bc * S, N))
    X = rs.standard_normal((Bc * S, Cin)).astype(np.float32)
    dW = _nan_bytes(N, Cin, K)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    dz_d, x_d = dev(dz), dev(X)
    L.check(lib.ns_pn_op_wgrad_narrow(L.ptr(dz_d), L.ptr(x_d), Bc, S, N, Cin, K, L.ptr(dW), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pn_op_wgrad_narrow")
    assert lib.ns_pn_last_launches() == 3
    assert torch.isfinite(dW).all()


# ---------------------------------------------------------------------------------------------------- the whole model
_MODELS = {}


def _zero_dropout(cfg):
    cfg = dict(cfg, transformer=dict(cfg["transformer"], encoder_dropout=0.0, decoder_dropout=0.0),
               variance_predictor=dict(cfg["variance_predictor"], dropout=0.0))
    return cfg


def _build(pcfg, cfg, sd, no_dropout=False):
    from smart_nar_fast_tts_amd import training

    m = training.FastSpeech2Align(pcfg, _zero_dropout(cfg) if no_dropout else cfg)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    if no_dropout:
        m.mel_encoder.prenet.p_drop, m.postnet.dropout = 0.0, 0.0
    return m.cuda()


def _teacher():
    """(meta, z, preprocess config, model config, state dict, batch on the device) of teacher_tiny: the full ljspeech config"""
    if "teacher" not in _MODELS:
        meta, z = load_golden("teacher_tiny")
        cfg, sd = weights_for(meta)
        sd = dict(sd)
        sd.update(wl.synth_aligner_state_dict(cfg, seed=meta["aligner_seed"]))
        batch = (None, None, torch.zeros(meta["B"], dtype=torch.long, device="cuda"), dev(z["texts"]), dev(z["src_lens"]), int(meta["L"]), dev(z["mels"]),
                 dev(z["mel_lens"]), int(meta["T"]), dev(z["p_targets"]), dev(z["e_targets"]))
        _MODELS["teacher"] = (meta, z, wl.preprocess_config(meta["pitch"], meta["energy"]), cfg, sd, batch)
    return _MODELS["teacher"]


def _tiny():
    """(meta, z, (preprocess config, model config), state dict, batch on the device) of train_align_tiny"""
    if "tiny" not in _MODELS:
        meta, z = load_golden("train_align_tiny")
        b = tc.fixture_batch(meta)
        batch = tuple(dev(a) if isinstance(a, np.ndarray) else a for a in b)
        _MODELS["tiny"] = (meta, z, tc.fixture_config(meta), tc.fixture_state_dict(meta), batch)
    return _MODELS["tiny"]


PRED = tc.PRED_NAMES


def _unused(m):
    """the parameters no output of the training forward depends on: the feed-forward of the aligner's LAST layer (only its alignment
    maps are used, fastspeech2_align.py:56-58); autograd leaves their .grad None, here as in the reference"""
    last = len(m.mel_encoder.layer_stack) - 1
    return sorted(n for n, _ in m.named_parameters() if n.startswith(f"mel_encoder.layer_stack.{last}.pos_ffn."))


def _zero_in_exact_arithmetic(m):
    """the parameters whose gradient is zero in exact arithmetic, so that a step may leave them where they are: the key bias of every
    attention (the softmax does not see it), a conv bias ahead of a train-mode BatchNorm, and what the aligner's last layer has
    behind its map (w_vs, fc, layer_norm feed the unused tgt_output alone; one Function with the map, so zeros come back, not None)"""
    last = len(m.mel_encoder.layer_stack) - 1
    tail = tuple(f"mel_encoder.layer_stack.{last}.crs_attn.{n}" for n in ("w_vs.", "fc.", "layer_norm."))
    return {n for n, _ in m.named_parameters() if n.endswith("w_ks.bias") or (n.startswith("postnet.") and n.endswith(".0.conv.bias")) or n.startswith(tail)}


def _teacher_gates(z, n_layer):
    names = list(PRED) + [f"attn{i}" for i in range(n_layer)]
    return gates(z, {n: z[n + "_f64"] for n in names}, names), names


def test_eval_forward_on_the_reference_fixture():
    meta, z, pcfg, cfg, sd, batch = _teacher()
    m = _build(pcfg, cfg, sd).eval()
    with torch.no_grad():
        out = m(*batch[2:])
    torch.cuda.synchronize()
    assert len(out) == 12 and out[5] is out[11] and len(out[10]) == meta["n_layer"] >= 4
    assert meta["exact_durations"], "the fixture must clear its argmax gap: d_targets are judged exactly"
    assert np.array_equal(out[11].cpu().numpy(), z["d_targets"])
    assert np.array_equal(out[9].cpu().numpy(), z["out_mel_lens"]) and out[8] is batch[4]
    assert np.array_equal(out[6].cpu().numpy(), z["src_masks"]) and np.array_equal(out[7].cpu().numpy(), z["mel_masks"])
    g, names = _teacher_gates(z, meta["n_layer"])
    got = {n: out[i].cpu().numpy() for i, n in enumerate(PRED)}
    got.update({f"attn{i}": a.cpu().numpy() for i, a in enumerate(out[10])})
    sh = shares(got, {n: z[n + "_f64"] for n in names}, g)
    report(test="ta_eval", shares=sh)
    assert max(sh.values()) <= 1.0, sh


_grad_gate = tc.grad_gate  # the one gate of a stored gradient, shared with tests/test_train_align_host.py


def test_training_step_on_the_reference_fixture():
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    meta, z, (pcfg, cfg), sd, batch = _tiny()
    m = _build(pcfg, cfg, sd, no_dropout=True).train()
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    out = m(*batch[2:])
    seven = loss(batch, out)
    seven[0].backward()
    torch.cuda.synchronize()
    assert np.array_equal(out[11].cpu().numpy(), z["d_targets"]) and not out[11].requires_grad
    assert np.array_equal(out[9].cpu().numpy(), z["d_targets"].sum(1))
    sh = {}
    for i, n in enumerate(PRED):
        sh[n] = share_of(out[i].detach().cpu().numpy(), z[n + "_f64"], gate_value(z[n], z[n + "_f64"]))[0]
    vals = torch.stack(list(seven)).detach().cpu().numpy()
    for i, n in enumerate(("total", "mel", "postnet", "pitch", "energy", "duration", "attn")):
        sh["loss_" + n] = share_of(vals[i], z["seven_f64"][i], gate_value(z["seven"][i], z["seven_f64"][i]))[0]
    named = dict(m.named_parameters())
    stored = sorted(k[3:] for k in z.files if k.startswith("g__"))
    assert sorted(k for k in named if named[k].requires_grad and named[k].grad is None) == _unused(m) and len(_unused(m)) == 6
    grads = tc.stored_gradients({k: (torch.zeros_like(v) if v.grad is None else v.grad).cpu().numpy() for k, v in named.items() if v.requires_grad}, sd)
    assert sorted(grads) == stored and not any(z["g__" + k].any() for k in _unused(m) if "g__" + k in z.files)
    gsh = {k: share_of(grads[k], z["g__" + k], _grad_gate(meta, z, k))[0] for k in stored}
    classes = {}
    for k, v in gsh.items():
        c = k.split(".")[0]
        classes[c] = max(classes.get(c, 0.0), v)
    report(test="ta_train", shares=sh, gradients=classes, worst=max(gsh, key=gsh.get))
    assert max(sh.values()) <= 1.0, sh
    assert max(gsh.values()) <= 1.0, sorted(gsh.items(), key=lambda t: -t[1])[:8]


def _keep_masks(m, B, L, T, seed):
    """given keep-masks for every dropout site of the model, on the device"""
    rs = np.random.RandomState(seed)
    draw = lambda p, *shape: dev((rs.rand(*shape) >= p).astype(np.uint8))  # noqa: E731
    t = m.model_config["transformer"]
    d = t["encoder_hidden"]
    F = m.model_config["variance_predictor"]["filter_size"]
    pe, pd, pv = t["encoder_dropout"], t["decoder_dropout"], m.model_config["variance_predictor"]["dropout"]
    return {"txt_encoder": [[draw(pe, B, L, d) for _ in range(2)] for _ in m.txt_encoder.layer_stack],
            "mel_encoder": [[draw(pd, B, T, d) for _ in range(2)] for _ in m.mel_encoder.layer_stack],
            "prenet": draw(m.mel_encoder.prenet.p_drop, B, T, d),
            "variance_adaptor": {"duration": [draw(pv, B, L, F) for _ in range(2)], "pitch": [draw(pv, B, T, F) for _ in range(2)],
                                 "energy": [draw(pv, B, T, F) for _ in range(2)]},
            "mel_decoder": [[draw(pd, B, T, d) for _ in range(2)] for _ in m.mel_decoder.layer_stack],
            "postnet": [draw(m.postnet.dropout, B, T, c) for c in m.postnet.channels[1:]]}


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _grads(m):
    return {n: None if p.grad is None else _bits(p.grad) for n, p in m.named_parameters()}


def _flat(out):
    """the float tensors and the integer ones of a 12-tuple as bits / arrays, by position"""
    res = []
    for o in out:
        if isinstance(o, (list, tuple)):
            res.append([_bits(a) for a in o])
        elif o.dtype == torch.float32:
            res.append(_bits(o))
        else:
            res.append(o.cpu().numpy())
    return res


def _loss_grads(loss, batch, out):
    seven = loss(batch, out)
    seven[0].backward()
    return torch.stack(list(seven)).detach().cpu().numpy().view(np.uint32)


def _hand_chain(m, batch, km):
    """fastspeech2_align.py:44-100 by hand: the six parts, MelLinear and add_residual in the model's order, the same masks, on the
    model's own parameters"""
    from smart_nar_fast_tts_amd import training

    _, _, _, texts, src_lens, L, mels, mel_lens, T, pt, et = batch
    src_masks = torch.arange(L, device="cuda")[None, :] >= src_lens[:, None]
    mel_masks = torch.arange(T, device="cuda")[None, :] >= mel_lens[:, None]
    src_output = m.txt_encoder(texts, src_masks, lens=src_lens, keep_masks=km["txt_encoder"])
    _, attns = m.mel_encoder(src_output, mels, src_masks, mel_masks, src_lens=src_lens, mel_lens=mel_lens, keep_masks=km["mel_encoder"],
                             prenet_keep_mask=km["prenet"])
    with torch.no_grad():
        d_targets = m.mel_encoder.durations(attns[-1], src_lens, mel_lens)
    x, p_pred, e_pred, log_d, d_rounded, mel_lens_out, mel_masks2 = m.variance_adaptor(src_output, src_masks, mel_masks, T, pt, et, d_targets,
                                                                                      keep_masks=km["variance_adaptor"])
    x, mel_masks3 = m.mel_decoder(x, mel_masks2, lens=mel_lens, keep_masks=km["mel_decoder"])
    mel = m.mel_linear(x)
    post = training.add_residual(m.postnet(mel, keep_masks=km["postnet"]), mel)
    return (mel, post, p_pred, e_pred, log_d, d_rounded, src_masks, mel_masks3, src_lens, mel_lens_out, attns, d_targets)


def _bn_state(m):
    return {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}


def test_train_mode_equals_the_hand_chain():
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    meta, z, (pcfg, cfg), sd, batch = _tiny()
    cfg = dict(cfg, transformer=dict(cfg["transformer"], encoder_dropout=0.2, decoder_dropout=0.2), variance_predictor=dict(cfg["variance_predictor"], dropout=0.5))
    m = _build(pcfg, cfg, sd).train()
    B, L, T = meta["B"], meta["L"], meta["T"]
    km = _keep_masks(m, B, L, T, seed=31)
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    spec = importlib.util.spec_from_file_location("_ns_tools_bench", os.path.join(ROOT, "tools", "_bench.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    bn = _bn_state(m)

    def restore():
        m.load_state_dict(bn, strict=False)  # the PostNet's forward moves its running statistics: both runs start from the same ones

    try:
        _clear(m)
        before = m.launches
        out = m(*batch[2:], keep_masks=km)
        got_seven = _loss_grads(loss, batch, out)
        spent, last = m.launches - before, m.last_launches
        got, got_grads, bn_after = _flat(out), _grads(m), _bn_state(m)
        parts = [m.txt_encoder, m.mel_encoder, m.mel_decoder]
        counted = list(m.variance_adaptor.hip_modules()) + [m.mel_linear, m.postnet]
        for which in ("forward", "backward"):
            want = sum(s.last_launches[which] for s in parts) + sum(c.last_launches.get(which, 0) for c in counted) + (1 if which == "forward" else 0)
            assert last[which] == want, (which, last, want)
        assert spent == last["forward"] + last["backward"]
        restore()
        _clear(m)
        want_out = _hand_chain(m, batch, km)
        want_seven = _loss_grads(loss, batch, want_out)
        want, want_grads = _flat(want_out), _grads(m)
        assert np.array_equal(got_seven, want_seven), "the seven losses"
        for i, (a, b) in enumerate(zip(got, want)):
            if isinstance(a, list):
                assert len(a) == len(b) == 4 and all(np.array_equal(p, q) for p, q in zip(a, b)), ("maps", i)
            else:
                assert np.array_equal(a, b), ("tuple entry", i)
        assert got_grads.keys() == want_grads.keys()
        for n in got_grads:
            assert (got_grads[n] is None) == (want_grads[n] is None) and (got_grads[n] is None or np.array_equal(got_grads[n], want_grads[n])), n
        frozen = [n for n, v in got_grads.items() if v is None]
        assert sorted(frozen) == sorted([n for n, p in m.named_parameters() if not p.requires_grad] + _unused(m)) and len(frozen) == 5 + 6
        assert all(torch.equal(v, _bn_state(m)[k]) for k, v in bn_after.items())
        # padded rows: the stacks' outputs are +0.0 there, so mel equals the bias on them (the reference masks nothing behind the decoder)
        pad = out[7].cpu().numpy()
        mel = out[0].detach().cpu().numpy()
        assert pad.any() and np.array_equal(mel[pad], np.broadcast_to(m.mel_linear.bias.detach().cpu().numpy(), mel[pad].shape))
        restore()
        with torch.no_grad():
            dec_in = m.txt_encoder(batch[3], out[6], lens=batch[4], keep_masks=km["txt_encoder"])
        assert not _bits(dec_in)[out[6].cpu().numpy()].any(), "padded rows of a stack's output are +0.0 by their bits"
        # lengths and max_mel_len given: no device-to-host read in forward, loss and backward
        restore()
        _clear(m)
        torch.cuda.synchronize()

        def step():
            o = m(*batch[2:], keep_masks=km)
            loss(batch, o)[0].backward()

        n_reads, msgs = tb.host_reads(step)
        assert n_reads == 0, msgs
        # the no_grad forward: the same bits, nothing kept
        restore()
        with torch.no_grad():
            quiet = m(*batch[2:], keep_masks=km)
        assert all(not t.requires_grad for t in quiet[:5]) and m.last_launches["backward"] == 0
        for i in range(5):
            assert np.array_equal(_bits(quiet[i]), got[i]), i
        # frozen submodules drop their backward launches
        restore()
        _clear(m)
        for p in list(m.postnet.parameters()) + list(m.mel_linear.parameters()):
            p.requires_grad_(False)
        o = m(*batch[2:], keep_masks=km)
        loss(batch, o)[0].backward()
        fz = m.last_launches
        # the data gradients still run (the decoder below wants them); the parameter gradients' launches are gone: 1 + 1 + 3 of mel_linear
        assert m.mel_linear.last_launches["backward"] == 1 + _G(native_lib()[1], B * T, 256, 80), m.mel_linear.last_launches
        assert fz["backward"] < last["backward"] and fz["forward"] == last["forward"], (fz, last)
        assert all(p.grad is None for p in m.postnet.parameters()) and m.mel_linear.weight.grad is None
        g2 = _grads(m)
        for n in got_grads:
            if not n.startswith(("postnet.", "mel_linear.")) and got_grads[n] is not None:
                assert np.array_equal(g2[n], got_grads[n]), n
    finally:
        for p in list(m.postnet.parameters()) + list(m.mel_linear.parameters()):
            p.requires_grad_(True)
        _clear(m)


# ---------------------------------------------------------------------------------------------------- the loop
OCFG = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, grad_clip_thresh=oc.GRAD_CLIP, grad_acc_step=1, **oc.SHIPPED)}


def _param_bits(m):
    return {n: _bits(p).copy() for n, p in m.named_parameters()}


def test_training_loop_two_steps_and_one_step_against_float64():
    from smart_nar_fast_tts_amd import optim, training
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    meta, z, (pcfg, cfg), sd, batch = _tiny()
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    mcfg = {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}
    # grad_acc_step = 2: the first call accumulates, the second steps and zeroes
    m = _build(pcfg, cfg, sd, no_dropout=True).train()
    opt = optim.ScheduledOptim(m, OCFG, mcfg, 0)
    p0 = _param_bits(m)
    l1 = training.train_step(m, loss, opt, batch, 1, 2, oc.GRAD_CLIP)
    assert len(l1) == 7 and all(t.is_cuda and t.dim() == 0 for t in l1)
    p1 = _param_bits(m)
    assert all(np.array_equal(p0[n], p1[n]) for n in p0), "step 1 of 2 leaves the parameters untouched"
    trainable = [n for n, p in m.named_parameters() if p.requires_grad and n not in _unused(m)]
    assert all(dict(m.named_parameters())[n].grad is None for n in _unused(m))
    assert all(dict(m.named_parameters())[n].grad is not None for n in trainable)
    assert {n for n in trainable if not bool(dict(m.named_parameters())[n].grad.abs().max() > 0)} <= _zero_in_exact_arithmetic(m)
    g1 = {n: dict(m.named_parameters())[n].grad.clone() for n in trainable}
    training.train_step(m, loss, opt, batch, 2, 2, oc.GRAD_CLIP)
    p2 = _param_bits(m)
    moved = [n for n in trainable if not np.array_equal(p1[n], p2[n])]
    # the first Adam step moves an element by at most lr (2.5e-7 here): a tensor all of whose elements have half an ulp above that
    # stays where it is (the pitch predictor's output bias, one element of 250)
    lr = opt._optimizer.param_groups[0]["lr"]
    heavy = {n for n in trainable if float(np.abs(p1[n].view(np.float32)).min()) * 2.0 ** -24 > lr}
    assert heavy <= {"variance_adaptor.pitch_predictor.linear_layer.bias"}
    allowed = _zero_in_exact_arithmetic(m) | heavy
    assert set(trainable) - set(moved) <= allowed, sorted(set(trainable) - set(moved) - allowed)
    assert len(moved) >= len(trainable) - len(allowed) and len(_zero_in_exact_arithmetic(m)) == 9 + 5 + 6
    assert all(not dict(m.named_parameters())[n].grad.any() for n in trainable), "the step zeroes the gradients"
    assert all(np.array_equal(p1[n], p2[n]) for n in p1 if n not in trainable)
    assert opt.current_step == 1
    del g1

    # one step (grad_acc_step = 1) against optim_cpu's float64 step from the device's own gradients; two runs from one state bit-equal
    runs = []
    for _ in range(2):
        m = _build(pcfg, cfg, sd, no_dropout=True).train()
        opt = optim.ScheduledOptim(m, OCFG, mcfg, 3998)
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad and n not in _unused(m)]
        before = [p.detach().cpu().numpy().reshape(-1).copy() for _, p in named]
        bn = _bn_state(m)
        out = m(*batch[2:])
        loss(batch, out)[0].backward()
        grads = [p.grad.detach().cpu().numpy().reshape(-1).copy() for _, p in named]
        opt.zero_grad()
        m.load_state_dict(bn, strict=False)
        seven = training.train_step(m, loss, opt, batch, 1, 1, oc.GRAD_CLIP)
        runs.append((named, before, grads, [p.detach().cpu().numpy().reshape(-1).copy() for _, p in named],
                     torch.stack(list(seven)).detach().cpu().numpy(), opt._optimizer.param_groups[0]["lr"]))
    named, before, grads, got, seven, lr = runs[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, runs[1][3])) and seven.tobytes() == runs[1][4].tobytes(), "two runs, one state: equal bits"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(grads, runs[1][2]))
    assert abs(lr - oc.lr_at(3999, **oc.SHIPPED)) <= 1e-12 * lr
    c = dict(params=before, grads=[grads], lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=oc.GRAD_CLIP)
    p64, p32 = oc.run(c)[0]["p"], oc.torch_run(c)[0]["p"]
    sh = {}
    for (n, _), a, t32, w64 in zip(named, got, p32, p64):
        err = np.abs(a.astype(np.float64) - w64).max()
        sh[n] = float(err / oc.gate_of(t32, w64)) if np.isfinite(err) else float("inf")
    report(test="ta_native_step", shares={"worst": max(sh.values())})
    assert max(sh.values()) <= 1.0, sorted(sh.items(), key=lambda t: -t[1])[:5]
    assert any(not np.array_equal(a, b) for a, b in zip(got, before))


def test_round_trip_into_the_inference_class(tmp_path):
    """two optimiser steps on teacher_tiny's batch (the full ljspeech config, dropout 0), save_checkpoint, checkpoint.load_checkpoint
    into model.FastSpeech2Align: its forward_teacher_forced() and the trainable module in eval() agree on the batch.  Each side is
    within one gate of the same truth (test_eval_forward_on_the_reference_fixture; tests/test_gpu_teacher.py), so the two differ by at
    most the sum of the two gates; the learning rate of steps 1 and 2 (2.5e-7, 4.9e-7) moves no weight by more than that.  The inference
    class computes valid rows only, so the frame-level outputs are compared on the valid frames."""
    from smart_nar_fast_tts_amd import checkpoint, optim, training
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss
    from smart_nar_fast_tts_amd.model import FastSpeech2Align as Inference

    meta, z, pcfg, cfg, sd, batch = _teacher()
    m = _build(pcfg, cfg, sd, no_dropout=True).train()
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    opt = optim.ScheduledOptim(m, OCFG, cfg, 0)
    w0 = _bits(m.mel_linear.weight).copy()
    for step in (1, 2):
        training.train_step(m, loss, opt, batch, step, 1, oc.GRAD_CLIP)
    assert not np.array_equal(_bits(m.mel_linear.weight), w0) and opt.current_step == 2
    path = str(tmp_path / "2.pth.tar")
    training.save_checkpoint(m, opt, path)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(ckpt) == ["model", "optimizer"] and list(ckpt["model"]) == list(m.state_dict())
    inf = Inference(pcfg, cfg).to("cuda").eval()
    checkpoint.load_checkpoint(inf, path)
    a = inf.forward_teacher_forced(None, *batch[3:])
    m.eval()
    with torch.no_grad():
        b = m(*batch[2:])
    torch.cuda.synchronize()
    assert torch.equal(a[11], b[11]) and torch.equal(a[9], b[9]), "d_targets and mel_lens are exact"
    g, _ = _teacher_gates(z, meta["n_layer"])
    valid_t = ~z["mel_masks"]
    valid_l = ~z["src_masks"]
    sh = {}
    for i, n in enumerate(PRED):
        x, y = a[i].cpu().numpy().astype(np.float64), b[i].cpu().numpy().astype(np.float64)
        sel = valid_l if n == "log_d_predictions" else valid_t
        sh[n] = float(np.abs(x - y)[sel].max() / (2.0 * g[n]))
    # the four alignment maps, on the frames and phonemes both sides compute (t < mel_len, l < src_len)
    assert len(a[10]) == len(b[10]) == meta["n_layer"]
    valid_tl = valid_t[:, None, :, None] & valid_l[:, None, None, :]
    for i, (p, q) in enumerate(zip(a[10], b[10])):
        x, y = p.cpu().numpy().astype(np.float64), q.cpu().numpy().astype(np.float64)
        assert x.shape == y.shape == z[f"attn{i}"].shape
        sh[f"attn{i}"] = float(np.abs(x - y)[np.broadcast_to(valid_tl, x.shape)].max() / (2.0 * g[f"attn{i}"]))
    report(test="ta_round_trip", shares=sh)
    assert max(sh.values()) <= 1.0, sh
    # and a restored trainable model continues from the checkpoint: get_model reads what save_checkpoint wrote
    class Args:
        restore_step = 2

    m2, opt2 = training.get_model(Args, (pcfg, cfg, dict(OCFG, path={"ckpt_path": str(tmp_path)})), torch.device("cuda"), train=True)
    assert m2.training and opt2.current_step == 2
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
