"""The VarianceAdaptor's training path on the GPU (csrc/adaptorgrad.hip through ns_va_* and smart_nar_fast_tts_amd/adaptor.py).

Each new kernel alone against float64 of its own fp32 inputs: a stored value is a float64 sum rounded once, so the bound is one fp32 ulp
of the value plus 1e-13 of the sum's absolute terms (the bound of tests/test_gpu_postnet_grad.py); copies, bucket indices, prefix sums
and lengths are exact.  Every workspace and output starts as 0xFF bytes.  Then determinism (bits), the module against the float64
yardstick (tests/variance_adaptor_grad_cpu.py) under the project gate — the fixture's four mixes against the reference's own recorded
results too — needs_input_grad with the launch counters, and one native step: loss.FastSpeech2TrainingLoss -> the adaptor's backward
-> optim.ScheduledOptim.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/variance_adaptor_grad.md was written from one)."""
import ctypes as C

import numpy as np
import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from tests import lossgrad_cpu as lg
from tests import optim_cpu as oc
from tests import variance_adaptor_grad_cpu as vc
from tests.util import dev, load_golden, native_lib, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _poison(shape, dtype):
    """a tensor whose every byte is 0xFF (NaN as a float, -1 as an integer)"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)
    return t


def _ulp(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _share(got, want, absum):
    """max |got - want| / (one fp32 ulp of want + 1e-13 of the absolute terms); inf for a NaN / Inf"""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - want) / (_ulp(want) + 1e-13 * absum + 1e-300)).max(initial=0.0))


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- the embedding alone
# (M, D, n_bins, targets): a row block's remainder and half-wide slabs; the smallest legal shape; several row blocks; a 64-wide slab
# and two float4 strides; every row in one bin; edges, outside the range, infinities and NaN
EMBED = [(74, 256, 256, "normal"), (2, 16, 2, "normal"), (650, 256, 256, "normal"), (650, 512, 8, "normal"), (650, 256, 256, "one_bin"),
         (37, 36, 8, "edges")]


def _embed_case(M, D, n_bins, kind, seed=7):
    rs = np.random.RandomState(seed + M + D + n_bins)
    bins = np.sort(rs.standard_normal(n_bins - 1)).astype(np.float32)
    if kind == "one_bin":
        target = np.zeros(M, np.float32)  # what every padded frame carries
    else:
        target = (rs.standard_normal(M) * 1.5).astype(np.float32)
    if kind == "edges":
        target[:7] = bins[:7]
        target[7:13] = [bins[0] - 1, bins[-1] + 1, np.inf, -np.inf, np.nan, np.nextafter(bins[2], np.float32(np.inf))]
    x = rs.standard_normal((M, D)).astype(np.float32)
    table = rs.standard_normal((n_bins, D)).astype(np.float32)
    g = rs.standard_normal((M, D)).astype(np.float32)
    return bins, target, x, table, g


def _embed_fwd(lib, x, target, bins, table, n_bins):
    M, D = x.shape
    y, idx = _poison((M, D), torch.float32), _poison((M,), torch.int32)
    assert lib.ns_va_op_embed_fwd(C.c_void_p(x.data_ptr()), C.c_void_p(target.data_ptr()), C.c_void_p(bins.data_ptr()), C.c_void_p(table.data_ptr()),
                                  M, D, n_bins, C.c_void_p(y.data_ptr()), C.c_void_p(idx.data_ptr()), _st()) == 0, lib.ns_last_error()
    assert lib.ns_va_last_launches() == 1
    return y, idx


def _embed_bwd(lib, g, idx, n_bins):
    M, D = g.shape
    n = lib.ns_va_embed_ws_bytes(M, D, n_bins)
    assert n > 0
    ws, dt = _poison((n,), torch.uint8), _poison((n_bins, D), torch.float32)
    assert lib.ns_va_op_embed_bwd(C.c_void_p(g.data_ptr()), C.c_void_p(idx.data_ptr()), M, D, n_bins, C.c_void_p(dt.data_ptr()), C.c_void_p(ws.data_ptr()),
                                  n, _st()) == 0, lib.ns_last_error()
    assert lib.ns_va_last_launches() == 2
    return dt


def test_the_large_embedding_case_has_several_row_blocks(so):
    L, lib = so
    out = (C.c_int32 * 8)()
    assert lib.ns_va_plan_embed(650, 256, 256, out) == 0 and out[0] > 1 and out[2] < 64 and out[3] > 1
    assert lib.ns_va_plan_embed(650, 512, 8, out) == 0 and out[0] > 1 and out[2] == 64 and out[3] == 8
    assert lib.ns_va_plan_embed(74, 256, 256, out) == 0 and out[0] == 1 and 74 % out[1] != 0


@pytest.mark.parametrize("M,D,n_bins,kind", EMBED)
def test_embedding_alone(so, M, D, n_bins, kind):
    L, lib = so
    bins, target, x, table, g = _embed_case(M, D, n_bins, kind)
    y, idx = _embed_fwd(lib, dev(x), dev(target), dev(bins), dev(table), n_bins)
    want_idx = torch.empty(M, dtype=torch.int64, device="cuda")
    assert lib.ns_op_bucketize(C.c_void_p(dev(target).data_ptr()), M, C.c_void_p(dev(bins).data_ptr()), n_bins - 1, C.c_void_p(want_idx.data_ptr()), _st()) == 0
    k = idx.cpu().numpy()
    assert np.array_equal(k, want_idx.cpu().numpy())  # ns_op_bucketize's index, bit for bit
    ref = torch.bucketize(torch.from_numpy(target), torch.from_numpy(bins)).numpy()  # right=False; NaN -> n_bins - 1
    assert np.array_equal(k, ref) and k.min() >= 0 and k.max() <= n_bins - 1
    if kind == "one_bin":
        assert len(set(k.tolist())) == 1
    if kind == "edges":
        assert k[4] == 4 and k[7] == 0 and k[8] == k[9] == k[11] == n_bins - 1 and k[10] == 0 and k[12] == 3
    want_y = x.astype(np.float64) + table.astype(np.float64)[k]
    s_y = _share(y.cpu().numpy(), want_y, np.abs(x) + np.abs(table[k]))
    # backward: float64 sums per bin over ALL rows
    dt = _embed_bwd(lib, dev(g), idx, n_bins)
    want = np.zeros((n_bins, D))
    absum = np.zeros((n_bins, D))
    np.add.at(want, k, g.astype(np.float64))
    np.add.at(absum, k, np.abs(g.astype(np.float64)))
    got = dt.cpu().numpy()
    s_t = _share(got, want, absum)
    empty = np.setdiff1d(np.arange(n_bins), k)
    assert (kind, len(empty)) != ("one_bin", 0) and (M >= n_bins or len(empty) > 0)
    assert not got[empty].any() and not np.signbit(got[empty]).any()  # a bin no row hits: +0.0
    report(test="va_embedding_alone", M=M, D=D, n_bins=n_bins, kind=kind, y=s_y, d_table=s_t)
    assert s_y <= 1.0 and s_t <= 1.0, (s_y, s_t)
    assert _bits(_embed_bwd(lib, dev(g), idx, n_bins)) == _bits(dt)  # run to run, bit for bit


def test_embedding_backward_ignores_an_index_outside_the_table(so):
    L, lib = so
    bins, target, x, table, g = _embed_case(74, 16, 8, "normal")
    idx = np.random.RandomState(3).randint(0, 8, size=74).astype(np.int32)
    clean = _embed_bwd(lib, dev(g), dev(idx), 8)
    bad = idx.copy()
    bad[5], bad[40] = -1, 8
    got = _embed_bwd(lib, dev(g), dev(bad), 8).cpu().numpy().astype(np.float64)
    want = clean.cpu().numpy().astype(np.float64)
    want[idx[5]] -= g[5]
    want[idx[40]] -= g[40]
    assert np.abs(got - want).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------- the length regulator alone
def _lr_cases():
    rs = np.random.RandomState(11)
    c = {}
    d = rs.randint(0, 9, size=(2, 5))
    c["2x5_T37_D256"] = (d, 37, 256)
    d = rs.randint(0, 6, size=(3, 7))
    c["3x7_T_exact_D16"] = (d, int(d.sum(1).max()), 16)
    d = rs.randint(1, 6, size=(2, 6))
    d[:, 0] = 0
    c["leading_zero"] = (d, int(d.sum(1).max()) + 2, 32)
    d = rs.randint(1, 5, size=(3, 4))
    d[1] = 0
    d[2, 1] = -3  # max(d, 0)
    c["all_zero_utterance"] = (d, 14, 32)
    d = rs.randint(1, 4, size=(2, 5))
    d[0, 2] = 300
    c["one_of_300_frames"] = (d, int(d.sum(1).max()), 256)
    d = rs.randint(2, 7, size=(3, 6))
    c["T_below_the_total"] = (d, int(d.sum(1).min()) - 3, 64)
    c["T_above_the_total"] = (d, int(d.sum(1).max()) + 9, 520)
    return c


LR = _lr_cases()


def _lr_fwd(lib, x, duration, T):
    B, L, D = x.shape
    out, cum, mel_len = _poison((B, T, D), torch.float32), _poison((B, L), torch.int32), _poison((B,), torch.int64)
    assert lib.ns_va_op_lr_fwd(C.c_void_p(x.data_ptr()), C.c_void_p(duration.data_ptr()), B, L, D, T, C.c_void_p(out.data_ptr()), C.c_void_p(cum.data_ptr()),
                               C.c_void_p(mel_len.data_ptr()), _st()) == 0, lib.ns_last_error()
    assert lib.ns_va_last_launches() == 2
    return out, cum, mel_len


def _lr_bwd(lib, g, cum, L):
    B, T, D = g.shape
    dx = _poison((B, L, D), torch.float32)
    assert lib.ns_va_op_lr_bwd(C.c_void_p(g.data_ptr()), C.c_void_p(cum.data_ptr()), B, L, D, T, C.c_void_p(dx.data_ptr()), _st()) == 0, lib.ns_last_error()
    assert lib.ns_va_last_launches() == 1
    return dx


@pytest.mark.parametrize("name", list(LR))
def test_length_regulator_alone(so, name):
    L_, lib = so
    d, T, D = LR[name]
    B, L = d.shape
    rs = np.random.RandomState(23)
    x = rs.standard_normal((B, L, D)).astype(np.float32)
    g = rs.standard_normal((B, T, D)).astype(np.float32)
    out, cum, mel_len = _lr_fwd(lib, dev(x), dev(d.astype(np.int64)), T)
    want_cum = np.cumsum(np.maximum(d, 0), axis=1)
    total = want_cum[:, -1]
    assert np.array_equal(cum.cpu().numpy(), want_cum) and np.array_equal(mel_len.cpu().numpy(), total) and mel_len.dtype == torch.int64
    want = vc.regulate(torch.from_numpy(x), d, T).numpy()
    got = out.cpu().numpy()
    assert np.array_equal(got, want) and not np.signbit(got[want == 0]).any()  # copies; +0.0 at and past the total
    if name == "all_zero_utterance":
        assert total[1] == 0 and not got[1].any()
    if name == "T_below_the_total":
        assert (total > T).all()
    # backward: float64 sums over each phoneme's frames below T
    dx = _lr_bwd(lib, dev(g), cum, L)
    want_dx = vc.lr_backward(torch.from_numpy(g).double(), want_cum, L, T).numpy()
    absum = vc.lr_backward(torch.from_numpy(g).double().abs(), want_cum, L, T).numpy()
    got_dx = dx.cpu().numpy()
    s = _share(got_dx, want_dx, absum)
    zero = np.maximum(d, 0) == 0
    assert not got_dx[zero].any() and not np.signbit(got_dx[zero]).any()  # duration 0: exactly +0.0
    report(test="va_length_regulator_alone", case=name, d_x=s)
    assert s <= 1.0, s
    assert _bits(_lr_bwd(lib, dev(g), cum, L)) == _bits(dx)
    # NaN at every frame at or past an utterance's total never reaches d_x
    gn = g.copy()
    gn[np.arange(T)[None, :] >= total[:, None]] = np.nan
    assert name not in ("T_above_the_total", "leading_zero", "all_zero_utterance") or np.isnan(gn).any()
    dn = _lr_bwd(lib, dev(gn), cum, L)
    assert np.isfinite(dn.cpu().numpy()).all() and _bits(dn) == _bits(dx)


def test_identical_utterances_get_identical_gradients(so):
    L_, lib = so
    rs = np.random.RandomState(5)
    d = np.tile(rs.randint(0, 40, size=(1, 9)), (4, 1))
    T, D = int(d[0].sum()), 256
    g = np.tile(rs.standard_normal((1, T, D)).astype(np.float32), (4, 1, 1))
    x = np.tile(rs.standard_normal((1, 9, D)).astype(np.float32), (4, 1, 1))
    out, cum, _ = _lr_fwd(lib, dev(x), dev(d.astype(np.int64)), T)
    dx = _lr_bwd(lib, dev(g), cum, 9).cpu().numpy()
    assert all(dx[b].tobytes() == dx[0].tobytes() for b in range(4)) and all(_bits(out[b]) == _bits(out[0]) for b in range(4))


# ---------------------------------------------------------------------------------------------------- the module
BIG = dict(B=5, L=26, T=130, src_lens=[26, 19, 26, 7, 22], cfg=vc.config(d=256, F=256, K=3, n_bins=256))
_CASES = {}


def _case(name):
    """(cfg, weights, both-levels inputs), once: "tiny" is the fixture, "big" is B 5, L 26, T 130, d 256, n_bins 256"""
    if name not in _CASES:
        if name == "tiny":
            meta, z = load_golden("variance_adaptor_grad_tiny")
            _CASES[name] = (meta["cfg"], vc.synth_weights(meta["cfg"], meta["seeds"][0]), z)
        else:
            # Seeds chosen on the CPU so that the gate stays sharp: at weight seed 77 (inputs 78) one ReLU of the energy predictor sits so
            # close to zero that torch's fp32 CPU run takes the other branch, and |ref fp32 - ref f64| — the gate — grows from 1e-6 to 1e-2
            # of the tensor for dx and every energy gradient.  At 80 / 81 every tensor's fp32 reference is within 1e-6 relative.
            w = vc.synth_weights(BIG["cfg"], 80)
            _CASES[name] = (BIG["cfg"], w, vc.synth_inputs(BIG["cfg"], BIG["B"], BIG["L"], BIG["T"], BIG["src_lens"], 81, max_dur=11))
    return _CASES[name]


_REFS = {}


def _yardstick(name, mix):
    """(inputs, float64 reference, fp32 reference, gates) of one case and mix, computed once and left unchanged"""
    if (name, mix) not in _REFS:
        cfg, w, z = _case(name)
        inp = vc.inputs_for(z, mix)
        r64, r32 = vc.autograd_ref(inp, w, mix, torch.float64), vc.autograd_ref(inp, w, mix, torch.float32)
        _REFS[name, mix] = (inp, r64, r32, vc.gate(r32, r64))
    return _REFS[name, mix]


def _module(cfg, w, mix, train=False):
    from smart_nar_fast_tts_amd import adaptor

    mc = wl.model_config("tiny")
    mc["transformer"]["encoder_hidden"] = cfg["d"]
    mc["variance_predictor"].update(filter_size=cfg["F"], kernel_size=cfg["K"], dropout=0.0)
    mc["variance_embedding"]["n_bins"] = cfg["n_bins"]
    m = adaptor.VarianceAdaptor(wl.preprocess_config(vc.LEVEL[mix[0]], vc.LEVEL[mix[1]]), mc)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in vc.state_dict(w).items()}, strict=True)  # reference-named keys
    assert not res.missing_keys and not res.unexpected_keys
    return m.cuda().train(train)


def _run(m, inp, x_grad=True):
    """every tensor of vc.NAMES (None where no gradient came back), mel_len, and the launches of the forward and of the backward"""
    src_mask, mel_mask, _ = vc.masks(inp)
    x = dev(inp["x"]).requires_grad_(x_grad)
    for p in m.parameters():
        p.grad = None
    n0 = m.launches()
    y, p, e, log_d, d_r, mel_len, mm = m(x, dev(src_mask), dev(mel_mask), int(inp["T"]), dev(inp["pitch_t"]), dev(inp["energy_t"]), dev(inp["duration"]))
    n1 = m.launches()
    torch.autograd.backward([y, p, e, log_d], [dev(inp[k]) for k in ("g_out", "g_pitch", "g_energy", "g_log_d")])
    n2 = m.launches()
    named = dict(m.named_parameters())
    got = dict(y=y, pitch=p, energy=e, log_d=log_d, dx=x.grad)
    for k in vc.NAMES[5:]:
        got[k] = named[vc.grad_key(k)].grad
    got = {k: (None if v is None else v.detach().cpu().numpy()) for k, v in got.items()}
    return got, mel_len.cpu().numpy(), (n1 - n0, n2 - n1), (d_r, mm)


@pytest.mark.parametrize("name,mix", [("tiny", m) for m in vc.MIXES] + [("big", "pp"), ("big", "ff")])
def test_module_forward_and_backward(so, name, mix):
    cfg, w, z = _case(name)
    inp, r64, r32, gates = _yardstick(name, mix)
    m = _module(cfg, w, mix)
    got, mel_len, launches, (d_r, mm) = _run(m, inp)
    assert np.array_equal(mel_len, vc.masks(inp)[2]) and mel_len.dtype == np.int64
    assert np.array_equal(d_r.cpu().numpy(), inp["duration"]) and mm.dtype == torch.bool  # duration_target itself; mel_mask passed through
    sh = vc.shares(got, r64, gates)
    assert set(sh) == set(vc.NAMES)
    report(test="va_module", case=name, mix=mix, launches=list(launches), shares=vc.classes(sh))
    assert max(sh.values()) <= 1.0, sh
    if name == "tiny":  # the reference's own recorded results, under the gate built from them
        ref64 = {k: z[f"{mix}_{k}_f64"] for k in vc.FIXTURE_NAMES}
        fg = vc.gate({k: z[f"{mix}_{k}"] for k in vc.FIXTURE_NAMES}, ref64)
        fs = vc.shares(got, ref64, fg)
        assert max(fs.values()) <= 1.0, fs
        assert np.array_equal(mel_len, z[f"{mix}_mel_len"])
    again, *_ = _run(m, inp)
    assert all(again[k].tobytes() == got[k].tobytes() for k in vc.NAMES)  # run to run, bit for bit


def test_max_len_none_pads_to_the_batch_maximum(so):
    from smart_nar_fast_tts_amd import adaptor

    d, _, D = LR["2x5_T37_D256"]
    x = dev(np.random.RandomState(1).standard_normal((2, 5, D)).astype(np.float32)).requires_grad_(True)
    lr = adaptor.LengthRegulator()
    out, mel_len = lr(x, dev(d.astype(np.int64)), None)
    T = int(d.sum(1).max())
    assert tuple(out.shape) == (2, T, D) and mel_len.cpu().tolist() == d.sum(1).tolist() and lr.last_launches["forward"] == 2
    fixed, _ = lr(x, dev(d.astype(np.int32)), T)  # an int32 duration is converted
    assert _bits(fixed) == _bits(out) and not mel_len.requires_grad
    out.sum().backward()
    assert np.array_equal(x.grad.cpu().numpy(), np.broadcast_to(np.maximum(d, 0)[..., None].astype(np.float32), (2, 5, D))) and lr.last_launches["backward"] == 1


def test_needs_input_grad_drops_launches_and_returns_none(so):
    cfg, w, z = _case("tiny")
    inp, r64, r32, gates = _yardstick("tiny", "pf")
    m = _module(cfg, w, "pf")
    full, _, (f_all, b_all), _ = _run(m, inp)
    # a frozen table: no gradient, its two launches gone, everything else the same bits
    m.energy_embedding.weight.requires_grad_(False)
    got, _, (f1, b1), _ = _run(m, inp)
    assert got["d_energy_emb"] is None and f1 == f_all and b1 == b_all - 2
    assert all(got[k].tobytes() == full[k].tobytes() for k in vc.NAMES if k != "d_energy_emb")
    assert m.energy_embedding.last_launches["forward"] == 1
    m.energy_embedding.weight.requires_grad_(True)
    # a frozen predictor: its ten gradients are None and its backward launches shrink to the data gradient's
    for p in m.pitch_predictor.parameters():
        p.requires_grad_(False)
    got, _, (f2, b2), _ = _run(m, inp)
    assert all(got[f"pitch.{n}"] is None for n in vc.pg.NAMES[:10]) and f2 == f_all and b2 < b_all
    sh = vc.shares(got, r64, gates)
    assert max(sh.values()) <= 1.0 and got["dx"].tobytes() == full["dx"].tobytes()
    # nothing upstream wants a gradient: the input's is None, the parameters' are the same bits
    for p in m.pitch_predictor.parameters():
        p.requires_grad_(True)
    got, _, (f3, b3), _ = _run(m, inp, x_grad=False)
    assert got["dx"] is None and b3 < b_all
    assert all(got[k].tobytes() == full[k].tobytes() for k in vc.NAMES if k != "dx")
    report(test="va_launches", mix="pf", forward=f_all, backward=b_all, frozen_table_backward=b1, frozen_predictor_backward=b2, no_dx_backward=b3)


def test_one_native_training_step_from_the_loss_through_the_adaptor(so):
    """pitch, energy and log_d of the adaptor go into loss.FastSpeech2TrainingLoss (with seeded mel, postnet and attention tensors, which
    do not meet the adaptor); total + (g_out * x_out).sum() is differentiated, so the loss's d_pitch, d_energy and d_log_d and a random
    d_out run through the adaptor's backward; one optim.ScheduledOptim step moves all of the adaptor's trainable parameters.  The updated
    parameters against the float64 chain at optim_cpu.gate_of of the fp32 CPU chain plus the gradient's own gate carried through the
    float64 step (the rule and the reason of tests/test_gpu_postnet_grad.py); x.grad at the project gate."""
    from smart_nar_fast_tts_amd import loss as loss_mod
    from smart_nar_fast_tts_amd import optim

    mix, cfg = "pf", vc.config()
    B, L, T, H, n_mel = 2, 5, 37, 2, 80
    w = vc.synth_weights(cfg, 501)
    z = vc.synth_inputs(cfg, B, L, T, [5, 3], 502, max_dur=7)
    inp = vc.inputs_for(z, mix)
    src_mask, mel_mask, mel_len = vc.masks(inp)
    assert mel_len.max() <= T
    rs = np.random.RandomState(503)
    mel, post, mel_t = (rs.standard_normal((B, T, n_mel)).astype(np.float32) for _ in range(3))
    attn = [rs.rand(B, H, T, L).astype(np.float32) for _ in range(4)]
    t = torch.from_numpy
    inputs = (None, None, None, None, t(inp["src_lens"]), L, t(mel_t), t(mel_len), T, t(inp["pitch_t"]), t(inp["energy_t"]), t(inp["duration"]))

    def predictions(p, e, log_d, up=lambda a: a):
        return (up(t(mel)), up(t(post)), p, e, log_d, None, up(t(src_mask)), up(t(mel_mask)), up(t(inp["src_lens"])), up(t(mel_len)),
                [up(t(a)) for a in attn], up(t(inp["duration"])))

    names = [k for k in vc.NAMES[5:]]
    m = _module(cfg, w, mix)
    start = 3998
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    sched = optim.ScheduledOptim(m, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, start)
    crit = loss_mod.FastSpeech2TrainingLoss(wl.preprocess_config(vc.LEVEL[mix[0]], vc.LEVEL[mix[1]]), wl.model_config("tiny"))
    x = dev(inp["x"]).requires_grad_(True)
    y, p, e, log_d, *_ = m(x, dev(src_mask), dev(mel_mask), T, dev(inp["pitch_t"]), dev(inp["energy_t"]), dev(inp["duration"]))
    cuda = lambda a: a.cuda()  # noqa: E731
    out = crit(tuple(cuda(a) if torch.is_tensor(a) else a for a in inputs), predictions(p, e, log_d, cuda))
    (out[0] + (y * dev(inp["g_out"])).sum()).backward()
    sched.step_and_update_lr()
    lr = sched._optimizer.param_groups[0]["lr"]
    named = dict(m.named_parameters())
    got = [named[vc.grad_key(k)].detach().cpu().numpy().reshape(-1) for k in names]
    before = {vc.grad_key(k): np.asarray(v, dtype=np.float32).reshape(-1) for k, v in zip(names, [vc.state_dict(w)[vc.grad_key(k)] for k in names])}

    def case_of(grads):
        return dict(params=[before[vc.grad_key(k)] for k in names], grads=[[np.asarray(grads[k]).reshape(-1) for k in names]],
                    lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=None)

    chain, gr = {}, {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        fwd, _ = vc.forward_form(inp, w, mix, dtype)
        preds = predictions(t(fwd["pitch"]), t(fwd["energy"]), t(fwd["log_d"]))
        nine = lg.autograd_ref(inputs, preds, vc.LEVEL[mix[0]], vc.LEVEL[mix[1]], lg.G_TOTAL, dtype)
        chained = dict(inp, g_pitch=nine[2], g_energy=nine[3], g_log_d=nine[4])
        gr[name] = vc.autograd_ref(chained, w, mix, dtype)
        chain[name] = oc.run(case_of(gr[name]))[0]["p"] if name == "f64" else oc.torch_run(case_of(gr[name]))[0]["p"]
    g_gate = vc.gate(gr["f32"], gr["f64"], names + ["dx"])
    hi = oc.run(case_of({k: gr["f64"][k] + g_gate[k] for k in names}))[0]["p"]
    lo = oc.run(case_of({k: gr["f64"][k] - g_gate[k] for k in names}))[0]["p"]
    sh = {}
    for k, a, t32, w64, h_, l_ in zip(names, got, chain["f32"], chain["f64"], hi, lo):
        bound = oc.gate_of(t32, w64) + np.maximum(np.abs(h_ - w64), np.abs(l_ - w64))
        err = np.abs(a.astype(np.float64) - w64)
        sh[k] = float((err / bound).max()) if np.isfinite(err).all() else float("inf")
    sh["x_grad"] =vc.shares({"dx": x.grad.cpu().numpy()}, gr["f64"], g_gate, ["dx"])["dx"]
    assert all(np.abs(a - before[vc.grad_key(k)]).max() > 0 for k, a in zip(names, got))  # every parameter moved
    report(test="va_native_step", mix=mix, shares=vc.classes(sh))
    assert max(sh.values()) <= 1.0, sh
