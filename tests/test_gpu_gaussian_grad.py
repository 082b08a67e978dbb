"""The Gaussian length regulator's training side on the GPU (csrc/gaussgrad.hip through ns_va_op_gu_* and adaptor.GaussianUpsampling)
against the float64 yardstick of tests/gaussian_grad_cpu.py, which tests/test_gaussian_grad_host.py proves both ways.

  launches alone   k_gu_prepare: the fp32 durations' effect (the centres), mel_len and the clamp of a negative duration, exact.
                   k_gu_denominators + k_gu_bwd on every case of gaussian_grad_cpu.CASES: w_out bit-equal to the FORWARD's weight output
                   (ns_op_gaussian_upsampling) on the live rows and +0.0 past them, d_x inside the bound and exactly +0.0 where the
                   bound is zero, the unbanded hook and a second run the same bits, nothing written next to d_x.
  NaN              planted in g at and past lim_b, and between the disjoint bands of the long-pause case: the same bits.
  the module       out and mel_len bit-equal to ops.gaussian_regulate, autograd's d_x bit-equal to the hook, needs_input_grad, counts.
  VarianceAdaptor  with the key, on the reference's recorded results (tests/golden/gaussian_grad_tiny.npz) under the gates of
                   tests/variance_adaptor_grad_cpu.py; all four mixes run twice bit-equal.
  the model        training.FastSpeech2Align with the key at the train_align_tiny shape: two runs bit-equal, one finite train_step,
                   text-encoder gradients that differ from the hard regulator's, and the saved checkpoint in model.FastSpeech2Align
                   with the key — whose forward_teacher_forced honours it (phase 2 is shared, csrc/api.hip) — within the round-trip
                   gates of tests/test_gpu_train_align.py.

Every output and workspace starts as 0xFF bytes.  NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line
(profiles/gaussian_grad.md quotes them).

Measured on the MI355X: d_x at most 0.078 of its bound (L = 257; 0.073 at L = 256, 0.062 over three LDS chunks, 0.01 ... 0.06 elsewhere),
each within 0.02 of the CPU emulation's share; through the module 0.02 ... 0.06; the adaptor on the fixture at most 0.53 of its gate
(d_pitch_emb), d_x 0.41; the round trip at most 0.23 of two gates (log_d), the mel 0.14."""
import ctypes as C

import numpy as np
import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from tests import gaussian_cpu as gc
from tests import gaussian_grad_cpu as gg
from tests import optim_cpu as oc
from tests import train_align_cpu as tc
from tests import variance_adaptor_grad_cpu as vc
from tests.util import dev, gate_value, load_golden, native_lib, report

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def so():
    return native_lib()


def ff(*shape, dtype=torch.float32):
    """a device tensor of a 4- or 8-byte type, every byte 0xFF"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def forward_plain(lib, x, d):
    """ns_op_gaussian_upsampling: (out [B, T, D], centres [B, L], w [B, L, T]) on the device"""
    B, L, D = x.shape
    T = gc.frames(d)
    out, s, w = ff(B, T, D), ff(B * (L + 1)), ff(B, L, T)
    assert lib.ns_op_gaussian_upsampling(P(dev(x)), P(dev(d)), B, L, D, T, T, P(out), P(s), P(w), _st()) == 0, lib.ns_last_error()
    return out, s[B:].clone().view(B, L), w


def backward(lib, g, centres, own_len, L, w_out=True, entry="ns_va_op_gu_bwd"):
    """one of the two backward entry points on pre-filled buffers: (d_x with one spare row, w_out or None)"""
    B, T, D = g.shape
    n = lib.ns_va_gu_ws_bytes(B, L, T)
    assert n > 0, lib.ns_last_error()
    ws, dx = ff(n // 4), ff(B * L + 1, D)
    w = ff(B, L, T) if w_out else None
    own = None if own_len is None else torch.tensor(own_len, dtype=torch.long, device="cuda")
    assert getattr(lib, entry)(P(g), P(centres), P(own), B, L, D, T, P(dx), P(w), P(ws), n, _st()) == 0, lib.ns_last_error()
    assert lib.ns_va_last_launches() == 2
    return dx, w


def case(lib, name):
    """(x, d, own_len, g, Reference, the forward's (out, centres, w) on the device), once per case"""
    if name not in _CACHE:
        x, d, own_len, g = gg.CASES[name]()
        _CACHE[name] = (x, d, own_len, g, gg.reference(x, d, g, own_len), forward_plain(lib, x, d))
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------------- each launch alone
@pytest.mark.parametrize("name", ["odd_L_partial_tile 2x7x24", "padded_odd_tail 1x257x64", "zero_utterance T=128 2x12x24", "long_pause 2x40x8"])
def test_prepare_alone(so, name):
    L_, lib = so
    x, d, *_ = gg.CASES[name]()
    di = np.floor(d).astype(np.int64)
    di[0, 0] = -3   # max(d, 0)
    B, L = di.shape
    n = lib.ns_va_gu_ws_bytes(B, L, 1)
    ws, saved, mel_len = ff(n // 4), ff(B * L + 1), ff(B + 1, dtype=torch.int64)
    assert lib.ns_va_op_gu_fwd(None, P(dev(di)), B, L, 4, 0, None, P(saved), P(mel_len), P(ws), n, _st()) == 0, lib.ns_last_error()
    assert lib.ns_va_last_launches() == 1
    clamped = np.maximum(di, 0)
    c, total = gc.centres(clamped.astype(np.float32))
    assert np.array_equal(saved[:-1].cpu().numpy().reshape(B, L), c) and mel_len[:-1].cpu().tolist() == clamped.sum(1).tolist() == total.astype(np.int64).tolist()
    assert np.array_equal(ws[:B * L].cpu().numpy().reshape(B, L), clamped.astype(np.float32)), "the fp32 durations the forward launch reads"
    assert bits(saved[-1:]) == b"\xff" * 4 and mel_len[-1] == -1, "nothing is written next to the outputs"


@pytest.mark.parametrize("name", list(gg.CASES))
def test_backward_alone_against_float64(so, name):
    L_, lib = so
    x, d, own_len, g, ref, (_, centres, w_fwd) = case(lib, name)
    B, L, D = x.shape
    T = ref.T
    assert np.array_equal(centres.cpu().numpy(), gc.centres(d)[0])
    dx, w = backward(lib, dev(g), centres, own_len, L)
    torch.cuda.synchronize()
    for b, lim in enumerate(ref.lim):
        assert bits(w[b, :, :lim]) == bits(w_fwd[b, :, :lim]), (name, b, "a weight the backward used differs from the forward's")
        assert not w[b, :, lim:].contiguous().view(torch.int32).any(), (name, b, "a row at or past lim_b has a weight other than +0.0")
    got = dx[:B * L].view(B, L, D).cpu().numpy()
    s = gg.share(got, ref)
    report(test="gaussian_grad", case=name, T=T, gpu_dx=round(s, 4))
    assert s <= 1.0, (name, s)
    zero = ref.bound == 0
    assert not got[zero].view(np.int32).any(), "exactly +0.0 where the bound is zero"
    assert bits(dx[B * L:]) == b"\xff" * 4 * D, "the row after d_x was written"
    full, w_full = backward(lib, dev(g), centres, own_len, L, entry="ns_va_op_gu_bwd_unbanded")
    assert bits(full) == bits(dx) and bits(w_full) == bits(w), (name, "the band changed a bit")
    again, _ = backward(lib, dev(g), centres, own_len, L, w_out=False)
    assert bits(again) == bits(dx), (name, "a second run, or w_out = NULL, changed a bit")


def test_nan_outside_the_live_rows_and_outside_every_band_reaches_nothing(so):
    L_, lib = so
    for name in ("forwards_dense 5x9x24", "forwards_packed 5x9x24", "long_pause 2x40x8"):
        x, d, own_len, g, ref, (_, centres, _) = case(lib, name)
        L = d.shape[1]
        clean, _ = backward(lib, dev(g), centres, own_len, L, w_out=False)
        gn = g.copy()
        for b, lim in enumerate(ref.lim):
            gn[b, lim:] = np.nan
        if name.startswith("long_pause"):
            c, _ = gc.centres(d)
            (lo0, hi0), (lo1, hi1) = gg.band(c[0, :32], ref.lim[0]), gg.band(c[0, 32:], ref.lim[0])
            assert hi0 < lo1
            gn[0, hi0:lo1] = np.nan
        assert np.isnan(gn).any()
        got, _ = backward(lib, dev(gn), centres, own_len, L, w_out=False)
        assert bits(got) == bits(clean), name


# ---------------------------------------------------------------------------------------------------- the module
def _int_case(name, T=None):
    x, d, *_ = gg.CASES[name]()
    di = np.floor(d).astype(np.int64)
    return x, di, int(di.sum(1).max()) if T is None else T


@pytest.mark.parametrize("name,T", [("odd_L_partial_tile 2x7x24", None), ("tile_plus_one 2x33x36", 40), ("long_pause 2x40x8", None), ("T=32k+1 3x10x40", 130)])
def test_module_equals_the_inference_launch_and_the_hook(so, name, T):
    from smart_nar_fast_tts_amd import adaptor, ops

    L_, lib = so
    x, di, T = _int_case(name, T)
    B, L, D = x.shape
    m = adaptor.GaussianUpsampling()
    xt = dev(x).requires_grad_(True)
    out, mel_len = m(xt, dev(di), T)
    assert m.last_launches["forward"] == 3 and not mel_len.requires_grad and mel_len.dtype == torch.int64
    assert mel_len.cpu().tolist() == di.sum(1).tolist()
    want, s = ff(B, T, D), ff(B * (L + 1))
    ops.gaussian_regulate(dev(x), dev(di.astype(np.float32)), mel_len, T, want, s)
    assert bits(out) == bits(want), "the training forward is the inference side's launch"
    g = torch.from_numpy(np.random.default_rng(5).standard_normal((B, T, D)).astype(np.float32)).cuda()
    n0 = m.launches
    out.backward(g)
    assert m.last_launches["backward"] == 2 and m.launches == n0 + 2
    hook, _ = backward(lib, g, s[B:].clone().view(B, L), mel_len.cpu().tolist(), L, w_out=False)
    assert bits(xt.grad) == bits(hook[:B * L]), "autograd's d_x is the hook's"
    # float64 of the same: the yardstick's bound at these integer durations
    ref = gg.reference(x, di.astype(np.float32), _fit(g.cpu().numpy(), gc.frames(di.astype(np.float32))), [min(int(n), T) for n in di.sum(1)])
    s_dx = gg.share(xt.grad.cpu().numpy(), ref)
    report(test="gaussian_grad_module", case=name, T=T, gpu_dx=round(s_dx, 4))
    assert s_dx <= 1.0
    # nothing upstream wants a gradient: no Function, no backward launch; an int32 duration is converted
    n1 = m.launches
    plain_out, _ = m(dev(x), dev(di.astype(np.int32)), T)
    assert bits(plain_out) == bits(out) and not plain_out.requires_grad and m.launches == n1 + 3
    y = dev(x).requires_grad_(True)
    o2, _ = m(y.detach(), dev(di), T)
    assert not o2.requires_grad


def _fit(a, T):
    """g [B, T_call, D] cut or zero-padded to the yardstick's T = the batch maximum (frames past it are past every lim_b)"""
    out = np.zeros((a.shape[0], T, a.shape[2]), dtype=a.dtype)
    n = min(T, a.shape[1])
    out[:, :n] = a[:, :n]
    return out


def test_max_len_none_reads_the_batch_maximum_once(so):
    from smart_nar_fast_tts_amd import adaptor

    x, di, T = _int_case("odd_L_partial_tile 2x7x24")
    m = adaptor.GaussianUpsampling()
    xt = dev(x).requires_grad_(True)
    out, mel_len = m(xt, dev(di), None)
    assert tuple(out.shape) == (2, T, 24) and m.last_launches["forward"] == 4
    fixed, _ = m(xt, dev(di), T)
    assert bits(fixed) == bits(out)
    with pytest.raises(ValueError, match="no frame to pad to"):
        m(xt, dev(np.zeros_like(di)), None)
    with pytest.raises(ValueError, match="multiple of 4"):
        m(dev(x[:, :, :6]), dev(di), T)


# ---------------------------------------------------------------------------------------------------- VarianceAdaptor with the key
def _adaptor(cfg, w, mix):
    from smart_nar_fast_tts_amd import adaptor

    mc = wl.model_config("tiny+gaussian")
    mc["transformer"]["encoder_hidden"] = cfg["d"]
    mc["variance_predictor"].update(filter_size=cfg["F"], kernel_size=cfg["K"], dropout=0.0)
    mc["variance_embedding"]["n_bins"] = cfg["n_bins"]
    m = adaptor.VarianceAdaptor(wl.preprocess_config(vc.LEVEL[mix[0]], vc.LEVEL[mix[1]]), mc)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in vc.state_dict(w).items()}, strict=True)
    assert type(m.length_regulator) is adaptor.GaussianUpsampling
    return m.cuda().eval()


def _run_adaptor(m, inp):
    src_mask, mel_mask, _ = vc.masks(inp)
    x = dev(inp["x"]).requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    y, p, e, log_d, d_r, mel_len, mm = m(x, dev(src_mask), dev(mel_mask), int(inp["T"]), dev(inp["pitch_t"]), dev(inp["energy_t"]), dev(inp["duration"]))
    torch.autograd.backward([y, p, e, log_d], [dev(inp[k]) for k in ("g_out", "g_pitch", "g_energy", "g_log_d")])
    named = dict(m.named_parameters())
    got = dict(y=y, pitch=p, energy=e, log_d=log_d, dx=x.grad)
    for k in vc.NAMES[5:]:
        got[k] = named[vc.grad_key(k)].grad
    return {k: v.detach().cpu().numpy() for k, v in got.items()}, mel_len.cpu().numpy()


@pytest.mark.parametrize("mix", vc.MIXES)
def test_variance_adaptor_with_the_key(so, mix):
    meta, z = load_golden("gaussian_grad_tiny")
    w = vc.synth_weights(meta["cfg"], meta["seeds"][0])
    inp = vc.inputs_for(z, mix)
    m = _adaptor(meta["cfg"], w, mix)
    got, mel_len = _run_adaptor(m, inp)
    assert np.array_equal(mel_len, z["duration"].sum(1)) and m.length_regulator.last_launches == {"forward": 3, "backward": 2}
    assert all(np.isfinite(v).all() for v in got.values())
    again, _ = _run_adaptor(m, inp)
    assert all(again[k].tobytes() == got[k].tobytes() for k in got), "run to run, bit for bit"
    if mix in meta["mixes"]:  # the reference's own recorded results, under the gate built from them
        ref64 = {k: z[f"{mix}_{k}_f64"] for k in vc.FIXTURE_NAMES}
        gates = vc.gate({k: z[f"{mix}_{k}"] for k in vc.FIXTURE_NAMES}, ref64)
        sh = vc.shares(got, ref64, gates)
        assert set(sh) == set(vc.FIXTURE_NAMES)
        report(test="gaussian_grad_adaptor", mix=mix, shares=vc.classes(sh))
        assert max(sh.values()) <= 1.0, sh
        assert np.array_equal(mel_len, z[f"{mix}_mel_len"])


# ---------------------------------------------------------------------------------------------------- the whole model
OCFG = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, grad_clip_thresh=oc.GRAD_CLIP, grad_acc_step=1, **oc.SHIPPED)}


def _model(pcfg, cfg, sd):
    from smart_nar_fast_tts_amd import training

    m = training.FastSpeech2Align(pcfg, cfg)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m.mel_encoder.prenet.p_drop, m.postnet.dropout = 0.0, 0.0
    return m.cuda().train()


def _encoder_grads(m, loss, batch):
    for p in m.parameters():
        p.grad = None
    loss(batch, m(*batch[2:]))[0].backward()
    return {n: bits(p.grad) for n, p in m.named_parameters() if n.startswith("txt_encoder.") and p.grad is not None}


def test_training_model_with_the_key(so, tmp_path):
    from smart_nar_fast_tts_amd import adaptor, checkpoint, optim, training
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss
    from smart_nar_fast_tts_amd.model import FastSpeech2Align as Inference

    meta, z = load_golden("train_align_tiny")
    pcfg, hard = tc.fixture_config(meta)
    cfg = dict(hard, length_regulator="gaussian")
    sd = tc.fixture_state_dict(meta)
    batch = tuple(dev(a) if isinstance(a, np.ndarray) else a for a in tc.fixture_batch(meta))
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    m = _model(pcfg, cfg, sd)
    assert type(m.variance_adaptor.length_regulator) is adaptor.GaussianUpsampling
    first = _encoder_grads(m, loss, batch)
    assert first and first == _encoder_grads(_model(pcfg, cfg, sd), loss, batch), "two runs from one state: equal bits"
    assert m.variance_adaptor.length_regulator.last_launches == {"forward": 3, "backward": 2}
    hard_grads = _encoder_grads(_model(pcfg, hard, sd), loss, batch)
    assert set(hard_grads) == set(first) and sum(hard_grads[n] != first[n] for n in first) > len(first) // 2, "the blended frames reach the text encoder"
    # one optimiser step
    m = _model(pcfg, cfg, sd)
    opt = optim.ScheduledOptim(m, OCFG, cfg, 0)
    before = {n: bits(p) for n, p in m.named_parameters()}
    seven = training.train_step(m, loss, opt, batch, 1, 1, oc.GRAD_CLIP)
    assert all(bool(torch.isfinite(t)) for t in seven) and all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert sum(before[n] != bits(p) for n, p in m.named_parameters()) > len(before) // 2 and opt.current_step == 1
    # the checkpoint in the inference class, built with the same key
    path = str(tmp_path / "1.pth.tar")
    training.save_checkpoint(m, opt, path)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert list(ckpt["model"]) == list(m.state_dict()) == list(_model(pcfg, hard, sd).state_dict())
    inf = Inference(pcfg, cfg).to("cuda").eval()
    checkpoint.load_checkpoint(inf, path)   # strict
    a = inf.forward_teacher_forced(None, *batch[3:])
    m.eval()
    with torch.no_grad():
        b = m(*batch[2:])
    torch.cuda.synchronize()
    assert torch.equal(a[11], b[11]) and torch.equal(a[9], b[9]), "d_targets and mel_lens are exact"
    T, L = int(meta["T"]), int(meta["L"])
    valid_t = np.arange(T)[None, :] < b[9].cpu().numpy()[:, None]
    valid_l = np.arange(L)[None, :] < np.asarray(meta["src_lens"])[:, None]
    sh = {}
    level = {"p_predictions": meta["pitch"], "e_predictions": meta["energy"], "log_d_predictions": "phoneme_level"}
    for i, n in enumerate(tc.PRED_NAMES):   # each side within one gate of the same truth: the two differ by at most two
        u, v = a[i].cpu().numpy().astype(np.float64), b[i].cpu().numpy().astype(np.float64)
        sel = valid_l if level.get(n) == "phoneme_level" else valid_t
        sh[n] = float(np.abs(u - v)[sel].max() / (2.0 * gate_value(z[n], z[n + "_f64"])))
    report(test="gaussian_grad_round_trip", shares=sh)
    assert max(sh.values()) <= 1.0, sh
    # and the key matters on the inference side too: the hard regulator gives another mel
    inf_hard = Inference(pcfg, hard).to("cuda").eval()
    checkpoint.load_checkpoint(inf_hard, path)
    h = inf_hard.forward_teacher_forced(None, *batch[3:])
    assert not torch.equal(h[0], a[0])
