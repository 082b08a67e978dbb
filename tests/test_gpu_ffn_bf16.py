"""The opt-in "bf16" feed-forward training mode on the GPU (csrc/ffngrad_bf16.hip through ns_fg_*_bf16, sublayers.PositionwiseFeedForward
with matmul="bf16", sublayers.set_ffn_matmul).  The yardstick is float64 with rounded operands (tests/ffn_bf16_emu.py, proven in
tests/test_ffn_bf16_host.py); the reference has no bf16 mode, so there is no fixture.

Each new launch alone first — the weight gradient against wgrad_check on both weight shapes of every config, random-sign and same-sign
operands, a case with several ranges whose last range and last stage are partial, a case with S < pad whose dead taps must be exactly
+0.0; the pack + bf16 GEMM hook in forward form (bias, ReLU) and in transposed form (resid) against gemm_check, the pack alone on exact
ties — then the module: the saved h bit-equal to the forward hook, z and y held to float64 of the device's own h and z, every gradient
bit-equal to the hand chain of the hooks on the device's own tensors (each link is held to float64 elementwise above, so no
rounding-flip allowance is needed), needs_input_grad and the launch counts, and training.FastSpeech2Align with its decoder switched.

The replica property (an utterance placed twice in a batch gets identical bits) is a property of rows, so it is checked where rows come
out: the two conv forms and the module's y and dx.  A weight gradient sums over every utterance and has no per-utterance output.

Configs and cases are those of tests/test_gpu_ffn_grad.py.  NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line
(profiles/ffn_bf16.md is written from one).

Measured on the MI355X (profiles/ffn_bf16.md): the weight gradient alone at most 0.029 of its bound (0.0094 on the several-range case),
the conv hook 0.013 forward and 0.015 transposed, the module's z 0.0099 and y 0.015 of theirs; every gradient bit-equal to the hand
chain; with the decoder's four feed-forwards switched the mel moves by 1.4e-3 of its largest magnitude."""
import numpy as np
import pytest
import torch

from tests import bf16_emu as B16
from tests import ffn_bf16_emu as E
from tests import ffn_grad_cpu as fc
from tests.util import dev, native_lib, report

pytestmark = pytest.mark.gpu
CONFIGS, CASES = E.CONFIGS, E.CASES
_cid = lambda c: f"{c[0]}x{c[1]}"  # noqa: E731
_fid = lambda c: f"d{c[0]}i{c[1]}k{c[2]}{c[3]}"  # noqa: E731
GRADS = ("dx", "w1", "b1", "w2", "b2", "ln_g", "ln_b")


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _op_ws(lib, B, S, N, Cin, KW):
    n = lib.ns_fg_op_bf16_ws_bytes(B, S, N, Cin, KW)
    assert n > 0, lib.ns_last_error()
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")


def _wgrad(so, dz, x, KW):
    """ns_fg_op_wgrad_bf16 on CPU tensors dz [B, S, N], x [B, S, Cin]: dW [N, Cin, KW] on the CPU, pre-filled with NaN"""
    L, lib = so
    (B, S, N), Cin = dz.shape, x.shape[2]
    dW, ws = torch.full((N, Cin, KW), float("nan"), device="cuda"), _op_ws(lib, B, S, N, Cin, KW)
    dz_d, x_d = dz.cuda(), x.cuda()  # (held until the result is read)
    L.check(lib.ns_fg_op_wgrad_bf16(L.ptr(dz_d), L.ptr(x_d), B, S, N, Cin, KW, L.ptr(dW), L.ptr(ws), ws.numel(), L.stream_ptr()),
            "ns_fg_op_wgrad_bf16")
    assert lib.ns_fg_last_launches() == 2  # the GEMM and its reduce
    return dW.cpu()


def _conv(so, x, w, bias, resid, transposed, act):
    """ns_fg_op_conv_bf16 on CPU tensors: x [B, S, Cin] -> [B, S, N] (forward form) or x [B, S, N] -> [B, S, Cin] (transposed)"""
    L, lib = so
    B, S, _ = x.shape
    N, Cin, KW = w.shape
    y, ws = torch.full((B, S, Cin if transposed else N), float("nan"), device="cuda"), _op_ws(lib, B, S, N, Cin, KW)
    x_d, w_d, bias_d, resid_d = (None if t is None else t.cuda() for t in (x, w, bias, resid))  # (held until the result is read)
    L.check(lib.ns_fg_op_conv_bf16(L.ptr(x_d), L.ptr(w_d), L.ptr(bias_d), L.ptr(resid_d), B, S, N, Cin, KW, int(transposed), act, L.ptr(y),
                                   L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_fg_op_conv_bf16")
    assert lib.ns_fg_last_launches() == 2  # the pack and the GEMM
    return y.cpu()


# ---------------------------------------------------------------------------------------------------- the weight gradient alone
@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_wgrad_alone(so, cfg, case):
    B, S = case
    for i, (N, Cin, KW) in enumerate(E.weight_shapes(cfg)):
        pl = E.plan(so[1], B * S, N, Cin, KW)  # (asserts rows per range <= 2816)
        for same_sign in (False, True):
            dz, x = E.operands(B, S, N, Cin, seed=31 * B * S + N + KW + same_sign, same_sign=same_sign)
            got = _wgrad(so, dz, x, KW)
            c = E.wgrad_check(got, dz, x, KW)
            print(f"{_fid(cfg)} w{i + 1} {_cid(case)} same_sign={same_sign} ranges={pl['ranges']}: {c}")
            report(test="fgb_wgrad", cfg=_fid(cfg), weight=i + 1, case=_cid(case), same_sign=same_sign, ranges=pl["ranges"], share=c.worst)
            assert c.ok, str(c)
            if not same_sign:
                assert _bits(_wgrad(so, dz, x, KW)) == _bits(got), "two runs give identical bits"


def test_wgrad_several_ranges_partial_last_range_and_stage(so):
    """3 x 55 rows on one 128 x 32 tile: the plan gives 3 ranges of 64 rows, the last of 37 = one full stage and 5 rows"""
    B, S, N, Cin, KW = 3, 55, 128, 32, 1
    pl = E.plan(so[1], B * S, N, Cin, KW)
    last = B * S - (pl["ranges"] - 1) * pl["rows"]
    assert pl["ranges"] >= 2 and 0 < last < pl["rows"] and last % 32 != 0 and last > 32, pl
    for KW in (1, 5):  # (5 taps on the same rows: 2 tiles of columns, the second 32 wide)
        E.plan(so[1], B * S, N, Cin, KW)
        dz, x = E.operands(B, S, N, Cin, seed=9 + KW)
        got = _wgrad(so, dz, x, KW)
        c = E.wgrad_check(got, dz, x, KW)
        print(f"KW={KW}: {c}")
        report(test="fgb_wgrad_ranges", KW=KW, ranges=pl["ranges"], share=c.worst)
        assert c.ok, str(c)
        assert _bits(_wgrad(so, dz, x, KW)) == _bits(got)


def test_wgrad_short_utterances_dead_taps_are_plus_zero(so):
    """S = 2 < pad = 4: a tap reads t + j - 4 with t in {0, 1}, so only the taps 3, 4, 5 are ever inside an utterance; the six others
    must come out as +0.0 from a NaN-filled dW"""
    B, S, N, Cin, KW = 5, 2, 128, 64, 9
    E.plan(so[1], B * S, N, Cin, KW)
    dz, x = E.operands(B, S, N, Cin, seed=3)
    got = _wgrad(so, dz, x, KW)
    unit = E.wgrad_unit(dz, x, KW)
    dead = [0, 1, 2, 6, 7, 8]
    assert bool((unit[:, :, dead] == 0).all()) and bool((unit[:, :, 3:6] > 0).all())
    c = E.wgrad_check(got, dz, x, KW, unit=unit)
    print(c)
    assert c.ok and c.zeros_ok and not got[:, :, dead].contiguous().view(torch.int32).any(), str(c)


# ---------------------------------------------------------------------------------------------------- the pack + GEMM hook alone
def _weight(N, Cin, KW, seed):
    return (torch.randn(N, Cin, KW, generator=torch.Generator().manual_seed(seed)) / (Cin * KW) ** 0.5).float()


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_conv_alone(so, cfg, case):
    B, S = case
    for i, (N, Cin, KW) in enumerate(E.weight_shapes(cfg)):
        w = _weight(N, Cin, KW, seed=N + KW)
        dz, x = E.operands(B, S, N, Cin, seed=17 * B * S + Cin + KW)
        if B > 1:
            dz[B - 1], x[B - 1] = dz[0], x[0]  # a replica of utterance 0 placed last
        bias = torch.randn(N, generator=torch.Generator().manual_seed(i)).float()
        resid = x * 0.5
        fwd = _conv(so, x, w, bias, None, False, 1)
        c1 = B16.gemm_check(fwd, x, w, bias, act="relu")
        back = _conv(so, dz, w, None, resid, True, 0)
        c2 = E.dgrad_check(back, dz, w, resid)
        print(f"{_fid(cfg)} w{i + 1} {_cid(case)}: forward {c1}; transposed {c2}")
        report(test="fgb_conv", cfg=_fid(cfg), weight=i + 1, case=_cid(case), forward=c1.worst, transposed=c2.worst)
        assert c1.ok and c2.ok, (str(c1), str(c2))
        if B > 1:
            assert _bits(fwd[B - 1]) == _bits(fwd[0]) and _bits(back[B - 1]) == _bits(back[0]), "a replica gets the original's bits"


def test_pack_rounds_ties_to_even(so):
    """weights that are exact ties between two bf16 values (low half 0x8000), even and odd upper halves, both signs, through both
    planes: against one-hot rows the GEMM returns the rounded weight itself (one product with 1.0, the rest exact zeros)"""
    N = Cin = 64
    rs = np.random.RandomState(4)
    hi = (rs.randint(0x3C00, 0x4100, size=(N, Cin)).astype(np.uint32) | (rs.randint(0, 2, size=(N, Cin)).astype(np.uint32) << 15))
    hi[0, :4] = [0x3F80, 0x3F81, 0xBF80, 0xBF81]  # +-1.0 (even) and the next bf16 (odd)
    bits = (hi << 16) | np.uint32(0x8000)
    w = torch.from_numpy(bits.view(np.float32).copy()).reshape(N, Cin, 1)
    want_hi = np.where(hi & 1, hi + 1, hi).astype(np.uint32)  # ties to even: an odd upper half goes up, an even one stays
    want = torch.from_numpy((want_hi << 16).view(np.float32).copy())  # [N, Cin]
    assert bool((B16.bf(w[:, :, 0]) == want).all())  # (torch's own cast agrees with the statement)
    eye = torch.eye(N).reshape(1, N, N)
    fwd = _conv(so, eye, w, None, None, False, 0)[0]   # y[m = c, n] = bf(w[n][c])
    back = _conv(so, eye, w, None, None, True, 0)[0]   # y[m = n, c] = bf(w[n][c])
    assert _bits(fwd) == _bits(want.T.contiguous()), "the forward plane rounds ties to even"
    assert _bits(back) == _bits(want), "the transposed plane rounds ties to even"
    assert (want_hi != hi).any() and (want_hi == hi).any()


# ---------------------------------------------------------------------------------------------------- the whole module
_MODULES = {}


def module(cfg, dropout=0.5):
    from smart_nar_fast_tts_amd import sublayers

    d, di, K1, K2 = cfg
    if cfg not in _MODULES:
        w = fc.seeded_weights(d, di, K1, K2, seed=200 + d + di + K1)
        m = sublayers.PositionwiseFeedForward(d, di, (K1, K2), dropout=dropout, matmul="bf16")
        m.load_state_dict({n: torch.from_numpy(w[k]) for n, k in zip(sublayers.FFN_PARAM_NAMES, fc.NAMES[:6])})
        _MODULES[cfg] = (m.cuda(), w)
    return _MODULES[cfg]


def _inputs(cfg, case, seed=0):
    d = cfg[0]
    B, S = case
    rs = np.random.RandomState(B * S + d + cfg[1] + seed)
    return rs.standard_normal((B, S, d)).astype(np.float32), rs.standard_normal((B, S, d)).astype(np.float32)


def _run(m, x, g, keep=None, need=None):
    """one forward + backward through the module's own marshalling: (y, saved, grads by GRADS, launches), all on the device"""
    m.train(keep is not None)
    call = m._marshal(dev(x), None if keep is None else dev(keep))
    y, saved = m._forward(call, save=True)
    outs = m._backward(call, saved, dev(g), [True] * 7 if need is None else need)
    return y, saved, dict(zip(GRADS, outs)), dict(m.last_launches)


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_module_forward_and_backward(so, cfg, case):
    L, lib = so
    m, w = module(cfg)
    d, di, K1, K2 = cfg
    B, S = case
    M = B * S
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    wd = {k: dev(w[k]) for k in ("w1", "w2", "ln_g")}
    x, g = _inputs(cfg, case)
    xt = torch.from_numpy(x)
    h_hook = _conv(so, xt, wt["w1"], wt["b1"], None, False, 1)
    for mode, keep in (("eval", None), ("train_p0.5", (np.random.RandomState(M + 3).rand(B, S, d) >= m.p_drop).astype(np.uint8))):
        y, saved, grads, launches = _run(m, x, g, keep)
        p = 0.0 if keep is None else m.p_drop
        s = saved.cpu()
        h, z = s[:M * di].reshape(B, S, di), s[M * di:].reshape(B, S, d)
        assert _bits(h) == _bits(h_hook), "the saved h is the forward hook's, bit for bit (dropout sits behind w_2)"
        # z against float64 of the device's own h at the GEMM bound, the fp32 row arithmetic on top
        u64, unit = B16.gemm_emu(h, wt["w2"], wt["b2"]), B16.gemm_unit(h, wt["w2"], wt["b2"])
        kf = 1.0 if keep is None else torch.from_numpy(keep).double() / (1.0 - p)
        z64 = u64 * kf + xt.double()
        z_share = float(((z.double() - z64).abs() / (E.GEMM_REL * unit * kf + E.FP32_REL * z64.abs())).max())
        y64 = B16.layernorm_emu(z, wt["ln_g"], wt["ln_b"])
        y_share = float(((y.cpu().double() - y64).abs() / (E.FP32_REL * (y64.abs() + wt["ln_b"].double().abs()))).max())
        assert z_share <= 1.0 and y_share <= 1.0 and bool(torch.isfinite(y).all()), (mode, z_share, y_share)
        # every gradient against the hand chain of the hooks on the device's own tensors
        chain = E.hand_chain(L, lib, cfg, case, dev(x), saved, dev(g), None if keep is None else dev(keep), p, wd)
        for n in GRADS:
            assert _bits(grads[n]) == _bits(chain[n]), (mode, n)
            assert bool(torch.isfinite(grads[n]).all()), (mode, n)
        report(test="fgb_module", cfg=_fid(cfg), case=_cid(case), mode=mode, launches=launches, z=z_share, y=y_share)
        assert launches == dict(forward=4, backward=11), launches  # the counts include/nar_fs2.h states


def test_needs_input_grad_bits_replicas_and_a_nan_behind_the_gate(so):
    cfg, (B, S) = CONFIGS[0], CASES[4]
    m, w = module(cfg)
    m.eval()
    d, di, K1, K2 = cfg
    x, g = _inputs(cfg, (B, S))
    x[2], g[2] = x[0], g[0]  # utterances 0 and 2 are replicas
    params = m.ordered_parameters()

    def once(x_grad=True, frozen=()):
        for i, p in enumerate(params):
            p.requires_grad_(i not in frozen)
            p.grad = None
        xd = dev(x).requires_grad_(x_grad)
        y = m(xd)
        y.backward(dev(g))
        bits = [None if p.grad is None else _bits(p.grad) for p in params]
        return _bits(y), bits, None if xd.grad is None else xd.grad.cpu().numpy(), dict(m.last_launches), y.detach().cpu().numpy()

    try:
        a, b = once(), once()
        assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), "two runs give identical bits"
        assert all(v is not None for v in a[1])
        assert a[4][0].tobytes() == a[4][2].tobytes() and a[2][0].tobytes() == a[2][2].tobytes(), "replicas get bit-identical y and dx rows"
        assert a[3] == dict(forward=4, backward=11), a[3]
        same = lambda r, skip=(): all(r[1][i] == a[1][i] for i in range(6) if i not in skip)  # noqa: E731
        nx = once(x_grad=False)
        assert nx[2] is None and same(nx) and nx[0] == a[0] and nx[3]["backward"] == 10, nx[3]  # no dx GEMM
        for i, drop in ((0, 2), (1, 1), (2, 2)):  # w1: its GEMM and reduce; b1: its column finish; w2: its GEMM and reduce
            fz = once(frozen=(i,))
            assert fz[1][i] is None and same(fz, (i,)) and fz[2].tobytes() == a[2].tobytes(), i
            assert fz[3]["backward"] == 11 - drop, (i, fz[3])
        fz = once(frozen=(3, 4, 5))  # none of b2, ln_g, ln_b: no finish at width d
        assert fz[1][3:] == [None] * 3 and same(fz, (3, 4, 5)) and fz[2].tobytes() == a[2].tobytes() and fz[3]["backward"] == 10, fz[3]
        tail = once(x_grad=False, frozen=(0, 1))  # nothing behind the ReLU: no pack, no da, no gate
        assert same(tail, (0, 1)) and tail[3]["backward"] == 4, tail[3]  # row backward, dW2's GEMM + reduce, the finish
        only_g = once(x_grad=False, frozen=(0, 1, 2, 3, 5))
        assert only_g[1][4] == a[1][4] and only_g[3]["backward"] == 2, only_g[3]  # exactly the row backward and the finish
        with torch.no_grad():
            quiet = m(dev(x))
        assert _bits(quiet) == a[0] and not quiet.requires_grad, "a forward that saves nothing gives the same y bits"
        assert m.last_launches["forward"] == 4
        report(test="fgb_launches", forward=a[3]["forward"], backward=a[3]["backward"], backward_no_dx=nx[3]["backward"],
               backward_tail_only=tail[3]["backward"], backward_ln_g_only=only_g[3]["backward"])
    finally:
        for p in params:
            p.requires_grad_(True)
            p.grad = None

    # a NaN in da behind the gate reaches nothing: channel c of h is dead in every row (b1[c] far below zero), and between the forward and
    # the backward w2[:, c] turns NaN — the backward reads the live weights, so da[:, c] is NaN, and the gate selects +0.0 there
    from smart_nar_fast_tts_amd import sublayers

    n = sublayers.PositionwiseFeedForward(d, di, (K1, K2), dropout=0.0, matmul="bf16")
    n.load_state_dict(m.state_dict())
    n = n.cuda().eval()
    c = 5
    with torch.no_grad():
        n.w_1.bias[c] = -1e30
    call = n._marshal(dev(x), None)
    y, saved = n._forward(call, save=True)
    assert not bool(saved[:B * S * di].reshape(B * S, di)[:, c].any())
    clean = n._backward(call, saved, dev(g), [True] * 7)
    with torch.no_grad():
        n.w_2.weight[:, c, :] = float("nan")
    call2 = n._marshal(dev(x), None)
    dirty = n._backward(call2, saved, dev(g), [True] * 7)
    for name, a_, b_ in zip(GRADS, clean, dirty):
        assert bool(torch.isfinite(b_).all()), name
        assert _bits(a_) == _bits(b_), name


# ---------------------------------------------------------------------------------------------------- the whole model
def test_fastspeech2_align_with_the_decoder_switched():
    from smart_nar_fast_tts_amd import optim, sublayers, training
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss
    from tests import optim_cpu as oc
    from tests import train_align_cpu as tc
    from tests.util import load_golden

    meta, z = load_golden("train_align_tiny")
    pcfg, cfg = tc.fixture_config(meta)
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in tc.fixture_state_dict(meta).items()}
    batch = tuple(dev(a) if isinstance(a, np.ndarray) else a for a in tc.fixture_batch(meta))

    def build():
        mdl = training.FastSpeech2Align(pcfg, cfg)
        mdl.load_state_dict(sd, strict=True)
        return mdl.cuda().eval()

    def forward(mdl):
        with torch.no_grad():
            out = mdl(*batch[2:])
        return out

    ref, plain, mixed = forward(build()), build(), build()
    assert sublayers.set_ffn_matmul(plain.txt_encoder.layer_stack[0].slf_attn, "bf16") == 0  # nothing switched
    n_dec = len(mixed.mel_decoder.layer_stack)
    assert sublayers.set_ffn_matmul(mixed.mel_decoder, "bf16") == n_dec > 0
    assert list(mixed.state_dict().keys()) == list(plain.state_dict().keys())
    out_plain, out = forward(plain), forward(mixed)
    for i in range(5):
        assert _bits(out_plain[i]) == _bits(ref[i]), ("a model with nothing switched gives the fp32 bits", i)
    for i in (2, 3, 4):  # p_predictions, e_predictions, log_d_predictions: upstream of the decoder
        assert _bits(out[i]) == _bits(ref[i]), i
    assert len(out[10]) >= 1 and all(_bits(a) == _bits(b) for a, b in zip(out[10], ref[10])), "the attention maps are upstream too"
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
    assert _bits(out[0]) != _bits(ref[0]), "the switch took effect"
    close = float((out[0] - ref[0]).abs().max() / ref[0].abs().max())
    report(test="fgb_model", decoder_layers=n_dec, output_rel_distance=close)
    # one training step (of two accumulation steps: the gradients stay) leaves every gradient and all seven losses finite
    mixed.train()
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, grad_clip_thresh=oc.GRAD_CLIP, grad_acc_step=2, **oc.SHIPPED)}
    opt = optim.ScheduledOptim(mixed, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, 0)
    seven = training.train_step(mixed, loss, opt, batch, 1, 2, oc.GRAD_CLIP)
    assert len(seven) == 7 and all(bool(torch.isfinite(t)) for t in seven)
    got = [(k, p.grad) for k, p in mixed.named_parameters() if p.grad is not None]
    assert len(got) > 100 and all(bool(torch.isfinite(gr).all()) for _, gr in got), [k for k, gr in got if not bool(torch.isfinite(gr).all())]
    dec = [gr for k, gr in got if k.startswith("mel_decoder.") and ".pos_ffn.w_" in k and k.endswith("weight")]
    assert len(dec) == 2 * n_dec and all(bool(gr.abs().max() > 0) for gr in dec)
