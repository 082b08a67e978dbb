"""The trainable MelEncoder on the GPU (csrc/melencgrad.hip through ns_me_*, sublayers.Prenet / FFTBlock2 and stacks.MelEncoder).

The two new kernels alone first, bit-equal to the numpy float64 statements of tests/mel_encoder_cpu.py (one rounding), at F in {256, 512}
and (B, T) in {(1, 1), (3, 33), (2, 70)}: one row, a partial 64-row block, past one block; with and without a keep-mask; NaN and
infinities planted in g behind dropped and gated elements (they reach neither dh nor d_b2); NaN planted in h2 (it gates like a zero);
d_b2 inside ``colsum_bound`` of the exact float64 column sum; two runs bit-equal.

Then the Prenet alone through ns_me_forward / ns_me_backward at the same three shapes with p in {0, 0.2 with a given mask}: h1, h2 and
y against the float64 statement at the project gate (tests/util.gate_value), the gradients against ``prenet_closed_form`` in float64 on
the DEVICE's saved h1 / h2 at the same gate (a pre-activation within a rounding of zero can change sign in float64: DESIGN.md section
28), NaN in frame 0 of mels reaching nothing, frame 0 of d_mels +0.0 by its bits, the launch counts include/nar_fs2.h states, and every
needs_input_grad combination dropping what the header says it drops.

Then the stack at d 256, H 2, d_inner 256, kernels (9, 1), 2 layers, B 3, L 9 with source lengths [9, 1, 8], T 33 with mel lengths
[33, 1, 32], in train() with given keep-masks (0.5 in the blocks, 0.2 in the Prenet): every bit of y, of both maps and of every gradient
equal to the hand chain (the Prenet op, FFTBlock2's sublayers twice by hand on a source leaf of their own each, dsrc the fp32 sum of the
two), and what the module docstring promises around it.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/mel_encoder_grad.md is written from one)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import aligner_cpu as alc
from tests import attention_grad_cpu as ac
from tests import ffn_grad_cpu as fc
from tests import mel_encoder_cpu as mc
from tests import optim_cpu as oc
from tests import stacks_cpu as sc
from tests.util import ROOT, dev, gates, native_lib, report, shares

pytestmark = pytest.mark.gpu
D, H, DI, KS, NL, B, L_SRC, SRC_LENS, T, MEL_LENS, P = 256, 2, 256, (9, 1), 2, 3, 9, [9, 1, 8], 33, [33, 1, 32], 0.5


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


def _prenet_counts(lib, M):
    return 3 + _G(lib, M, 256, 80) + _G(lib, M, 256, 256), 10 + _G(lib, M, 256, 256) + _G(lib, M, 80, 256)


# ---------------------------------------------------------------------------------------------------- the two kernels alone
def _same_with_nan(got, want):
    """bit-equal where ``want`` is a number, NaN where it is NaN (a NaN's payload is the hardware's)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("case", mc.KERNEL_CASES)
@pytest.mark.parametrize("shape", mc.KERNEL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("F", mc.KERNEL_WIDTHS)
def test_kernels_alone(so, F, shape, case):
    L, lib = so
    Bc, Tc = shape
    M = Bc * Tc
    k = mc.kernel_case(case, Bc, Tc, F)
    want_y = mc.drop_pos(k["h2"], k["pos"], k["keep"], k["p"], Tc)
    want_dh, col = mc.drop_relu_gate(k["g"], k["h2"], k["keep"], k["p"])
    assert np.isfinite(want_dh).all() and np.isfinite(col).all()
    bound = mc.colsum_bound(want_dh)
    runs = []
    for _ in range(2):
        g_d, h_d, p_d, keep_d = dev(k["g"]), dev(k["h2"]), dev(k["pos"]), None if k["keep"] is None else dev(k["keep"])
        y = torch.full((M, F), float("nan"), device="cuda")
        L.check(lib.ns_me_op_drop_pos(L.ptr(h_d), L.ptr(p_d), L.ptr(keep_d), k["p"], Bc, Tc, F, L.ptr(y), L.stream_ptr()), "ns_me_op_drop_pos")
        assert lib.ns_me_last_launches() == 1
        out = {"y": y.cpu().numpy()}
        for with_bias in (True, False):
            dh = torch.full((M, F), float("nan"), device="cuda")
            b2 = torch.full((F,), float("nan"), device="cuda") if with_bias else None
            ws = torch.full((((M + 63) // 64) * 5 * F * 8,), 0xFF, dtype=torch.uint8, device="cuda")
            L.check(lib.ns_me_op_drop_relu_gate(L.ptr(g_d), L.ptr(h_d), L.ptr(keep_d), k["p"], M, F, L.ptr(dh), L.ptr(b2), L.ptr(ws), ws.numel(),
                                                L.stream_ptr()), "ns_me_op_drop_relu_gate")
            assert lib.ns_me_last_launches() == (2 if with_bias else 1)  # the gate, and the column finish of d_b2
            out["dh" if with_bias else "dh_alone"] = dh.cpu().numpy()
            if with_bias:
                out["b2"] = b2.cpu().numpy()
        assert g_d.cpu().numpy().tobytes() == k["g"].tobytes() and h_d.cpu().numpy().tobytes() == k["h2"].tobytes(), "g and h2 are only read"
        runs.append(out)
    got = runs[0]
    assert _same_with_nan(got["y"], want_y), "y = fl32(f64(h2) k + f64(pos[m % T]))"
    for n in ("dh", "dh_alone"):
        assert got[n].view(np.uint32).tobytes() == want_dh.view(np.uint32).tobytes(), "dh is the select, bit for bit (+0.0 behind the gate)"
    err = np.abs(got["b2"].astype(np.float64) - col)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    report(test="me_kernels", F=F, shape=f"{Bc}x{Tc}", case=case, d_b2=worst)
    assert np.isfinite(got["b2"]).all() and (err <= bound).all(), worst
    for n in got:
        assert got[n].tobytes() == runs[1][n].tobytes(), ("two runs are bit-equal", n)


# ---------------------------------------------------------------------------------------------------- the Prenet alone
W_PRENET = mc.seeded_prenet(610)


def _prenet_inputs(Bc, Tc, seed=0):
    rs = np.random.RandomState(700 + seed + 31 * Bc + Tc)
    mels = (rs.standard_normal((Bc, Tc, mc.N_MEL)) * 2.0 - 3.0).astype(np.float32)
    g = rs.standard_normal((Bc, Tc, mc.D_PRENET)).astype(np.float32)
    pos = sc.position_table(Tc, mc.D_PRENET, 1000, True)[0]
    keep = (rs.random_sample((Bc, Tc, mc.D_PRENET)) >= mc.P_PRENET).astype(np.uint8)
    return mels, g, np.ascontiguousarray(pos), keep


def _prenet_raw(L, lib, mels, g, pos, keep, p, want=(True,) * 5):
    """ns_me_forward + ns_me_backward by hand: (y, (xin, h1, h2), {name: gradient or None}, launches)"""
    Bc, Tc, _ = mels.shape
    M = Bc * Tc
    s = L.NsMeShape()
    s.B, s.T, s.n_mel, s.d = Bc, Tc, mc.N_MEL, mc.D_PRENET
    wd = {n: dev(W_PRENET[n]) for n in L.ME_NAMES}
    k = L.NsMeWeights()
    for n in L.ME_NAMES:
        setattr(k, n, wd[n].data_ptr())
    ws = torch.full((lib.ns_me_ws_bytes(C.byref(s)),), 0xFF, dtype=torch.uint8, device="cuda")
    saved = torch.full((lib.ns_me_saved_bytes(C.byref(s)) // 4,), float("nan"), device="cuda")
    m_d, g_d, p_d, keep_d = dev(mels), dev(g), dev(pos), None if keep is None else dev(keep)
    y = torch.full((Bc, Tc, mc.D_PRENET), float("nan"), device="cuda")
    L.check(lib.ns_me_forward(C.byref(s), C.byref(k), L.ptr(m_d), L.ptr(p_d), L.ptr(keep_d), p, L.ptr(y), L.ptr(saved), L.ptr(ws), ws.numel(),
                              L.stream_ptr()), "ns_me_forward")
    launches = {"forward": lib.ns_me_last_launches()}
    shapes = dict(dmels=(Bc, Tc, mc.N_MEL), w1=(256, 80), b1=(256,), w2=(256, 256), b2=(256,))
    outs = {n: torch.full(shapes[n], float("nan"), device="cuda") if w else None for n, w in zip(("dmels",) + L.ME_NAMES, want)}
    d = L.NsMeGrads()
    for n, o in outs.items():
        setattr(d, n, None if o is None else o.data_ptr())
    L.check(lib.ns_me_backward(C.byref(s), C.byref(k), L.ptr(keep_d), p, L.ptr(saved), L.ptr(g_d), C.byref(d), L.ptr(ws), ws.numel(),
                               L.stream_ptr()), "ns_me_backward")
    launches["backward"] = lib.ns_me_last_launches()
    sv = saved.cpu().numpy()
    parts = (sv[:M * 80].reshape(Bc, Tc, 80), sv[M * 80:M * 336].reshape(Bc, Tc, 256), sv[M * 336:].reshape(Bc, Tc, 256))
    assert m_d.cpu().numpy().tobytes() == mels.tobytes() and g_d.cpu().numpy().tobytes() == g.tobytes(), "mels and g are only read"
    return y.cpu().numpy(), parts, {n: None if o is None else o.cpu().numpy() for n, o in outs.items()}, launches


@pytest.mark.parametrize("p", [0.0, mc.P_PRENET])
@pytest.mark.parametrize("shape", mc.KERNEL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_prenet_forward_and_backward(so, shape, p):
    L, lib = so
    Bc, Tc = shape
    mels, g, pos, keep = _prenet_inputs(Bc, Tc)
    keep = keep if p else None
    poisoned = mels.copy()
    poisoned[:, 0] = np.nan  # frame 0 is replaced, not read
    y, (xin, h1, h2), grads, launches = _prenet_raw(L, lib, poisoned, g, pos, keep, p)
    ref = {dt: {n: v.numpy() for n, v in mc.prenet_statement(mels, W_PRENET, pos, keep, p, dt).items()} for dt in (torch.float32, torch.float64)}
    assert xin.tobytes() == ref[torch.float32]["xin"].tobytes() and not xin[:, 0].view(np.uint32).any()
    fwd = shares(dict(y=y, h1=h1, h2=h2), ref[torch.float64], gates(ref[torch.float32], ref[torch.float64], ("y", "h1", "h2")))
    # y from the device's own h2 is the forward kernel's statement, bit for bit
    assert np.array_equal(y.view(np.uint32).reshape(Bc * Tc, -1),
                          mc.drop_pos(h2.reshape(Bc * Tc, -1), pos, None if keep is None else keep.reshape(Bc * Tc, -1), p, Tc).view(np.uint32))
    r64 = mc.prenet_closed_form(mels, W_PRENET, g, (h1, h2), keep, p, torch.float64)
    r32 = mc.prenet_closed_form(mels, W_PRENET, g, (h1, h2), keep, p, torch.float32)
    sh = shares(grads, r64, gates(r32, r64, mc.PRENET_NAMES))
    report(test="me_prenet", shape=f"{Bc}x{Tc}", p=p, launches=launches, forward=fwd, shares=sh)
    assert max(fwd.values()) <= 1.0, fwd
    assert max(sh.values()) <= 1.0, sh
    assert not grads["dmels"][:, 0].view(np.uint32).any(), "frame 0 of d_mels is +0.0 by its bits"
    assert launches == dict(zip(("forward", "backward"), _prenet_counts(lib, Bc * Tc))), launches  # the counts include/nar_fs2.h states


def test_prenet_module_needs_input_grad_and_run_to_run_bits(so):
    from smart_nar_fast_tts_amd import sublayers

    L, lib = so
    Bc, Tc = 3, 33
    M = Bc * Tc
    m = sublayers.Prenet()
    m.load_state_dict({n: torch.from_numpy(W_PRENET[k]) for n, k in zip(sublayers.PRENET_PARAM_NAMES, L.ME_NAMES)})
    m = m.cuda().train()
    mels, g, pos, keep = _prenet_inputs(Bc, Tc, seed=1)
    params = m.ordered_parameters()
    pos_d, keep_d = dev(pos), dev(keep)

    def once(x_grad=True, frozen=()):
        for i, p in enumerate(params):
            p.requires_grad_(i not in frozen)
            p.grad = None
        xd = dev(mels).requires_grad_(x_grad)
        y = m(xd, pos_d, keep_mask=keep_d)
        y.backward(dev(g))
        bits = [None if p.grad is None else p.grad.cpu().numpy().tobytes() for p in params]
        return y.detach().cpu().numpy(), bits, None if xd.grad is None else xd.grad.cpu().numpy(), dict(m.last_launches)

    try:
        a, b = once(), once()
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), "two runs give identical bits"
        assert all(v is not None for v in a[1]) and pos_d.grad is None
        raw = _prenet_raw(L, lib, mels, g, pos, keep, mc.P_PRENET)
        assert raw[0].tobytes() == a[0].tobytes() and raw[2]["dmels"].tobytes() == a[2].tobytes(), "the module is the two C calls"
        assert [raw[2][n].tobytes() for n in L.ME_NAMES] == a[1]
        fwd, bwd = _prenet_counts(lib, M)
        assert a[3] == dict(forward=fwd, backward=bwd), a[3]
        same = lambda r, skip=(): all(r[1][i] == a[1][i] for i in range(4) if i not in skip)  # noqa: E731
        nx = once(x_grad=False)
        assert nx[2] is None and same(nx) and nx[0].tobytes() == a[0].tobytes()
        assert nx[3]["backward"] == bwd - _G(lib, M, 80, 256) - 1, (nx[3], a[3])  # no data-gradient GEMM, no frame-0 select
        for i, drop in ((0, 2), (1, 1), (2, 2), (3, 1)):  # w1, w2: GEMM and reduce; b1, b2: the column finish
            fz = once(frozen=(i,))
            assert fz[1][i] is None and same(fz, (i,)) and fz[2].tobytes() == a[2].tobytes(), i
            assert fz[3]["backward"] == bwd - drop, (i, fz[3], a[3])
        tail = once(x_grad=False, frozen=(0, 1))  # nothing behind the first ReLU: no pack, no da1, no second gate
        assert same(tail, (0, 1)) and tail[3]["backward"] == 4, tail[3]  # the gate, d_b2's finish, dW2's GEMM + reduce
        only_b2 = once(x_grad=False, frozen=(0, 1, 2))
        assert only_b2[1][3] == a[1][3] and only_b2[3]["backward"] == 2, only_b2[3]
        only_x = once(frozen=(0, 1, 2, 3))
        assert only_x[2].tobytes() == a[2].tobytes() and only_x[3]["backward"] == bwd - 6, only_x[3]
        with torch.no_grad():
            quiet = m(dev(mels), pos_d, keep_mask=keep_d)
        assert quiet.cpu().numpy().tobytes() == a[0].tobytes() and not quiet.requires_grad and m.last_launches["forward"] == fwd
        m.eval()
        with torch.no_grad():
            plain = m(dev(mels), pos_d).cpu().numpy()
        assert plain.tobytes() == _prenet_raw(L, lib, mels, g, pos, None, 0.0)[0].tobytes(), "eval() means p = 0"
        with pytest.raises(ValueError, match="no dropout applies"):
            m(dev(mels), pos_d, keep_mask=keep_d)
        report(test="me_prenet_launches", forward=fwd, backward=bwd, backward_no_dmels=nx[3]["backward"], backward_tail_only=tail[3]["backward"])
    finally:
        for p in params:
            p.requires_grad_(True)
            p.grad = None


# ---------------------------------------------------------------------------------------------------- the stack
def _config(max_seq_len=40, dropout=P):
    t = dict(conv_filter_size=DI, conv_kernel_size=list(KS), decoder_hidden=D, decoder_head=H, decoder_layer=NL, decoder_dropout=dropout)
    return {"max_seq_len": max_seq_len, "transformer": t}


def _state_dict(w):
    from smart_nar_fast_tts_amd import sublayers

    sd = {f"prenet.{n}": torch.from_numpy(w["prenet"][k]) for n, k in zip(sublayers.PRENET_PARAM_NAMES, mc.PRENET_NAMES[:4])}
    for i, (wa, wf) in enumerate(w["layers"]):
        sd.update({f"layer_stack.{i}.crs_attn.{n}": torch.from_numpy(wa[k]) for n, k in zip(sublayers.PARAM_NAMES, ac.NAMES[:10])})
        sd.update({f"layer_stack.{i}.pos_ffn.{n}": torch.from_numpy(wf[k]) for n, k in zip(sublayers.FFN_PARAM_NAMES, fc.NAMES[:6])})
    return sd


_BUILT = {}


def _stack(max_seq_len=40):
    """(module on the GPU, its seeded weights), built once per max_seq_len"""
    from smart_nar_fast_tts_amd import stacks

    if max_seq_len not in _BUILT:
        w = mc.seeded_stack(D, DI, KS, NL, seed=800)
        m = stacks.MelEncoder(_config(max_seq_len))
        missing = m.load_state_dict(_state_dict(w), strict=False)
        assert missing.missing_keys == ["position_enc"] and not missing.unexpected_keys
        _BUILT[max_seq_len] = (m.cuda(), w)
    return _BUILT[max_seq_len]


def _inputs(Tc=T, mel_lens=MEL_LENS, seed=0):
    rs = np.random.RandomState(950 + seed + Tc)
    src = rs.standard_normal((B, L_SRC, D)).astype(np.float32)
    mels = (rs.standard_normal((B, Tc, mc.N_MEL)) * 2.0 - 3.0).astype(np.float32)
    g = rs.standard_normal((B, Tc, D)).astype(np.float32)  # random on every row, padded ones too
    a = [(rs.standard_normal((B, H, Tc, L_SRC)) / Tc).astype(np.float32) for _ in range(NL)]
    keeps = [[dev((rs.rand(B, Tc, D) >= P).astype(np.uint8)) for _ in range(2)] for _ in range(NL)]
    pk = dev((rs.rand(B, Tc, D) >= mc.P_PRENET).astype(np.uint8))
    return dict(src=src, mels=mels, g=g, a=a, keeps=keeps, pk=pk, src_mask=dev(sc.pad_of(SRC_LENS, L_SRC)), tgt_mask=dev(sc.pad_of(mel_lens, Tc)),
                src_lens=dev(np.asarray(SRC_LENS, dtype=np.int64)), mel_lens=dev(np.asarray(mel_lens, dtype=np.int64)))


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _grads(m):
    return {n: None if p.grad is None else _bits(p.grad) for n, p in m.named_parameters()}


def _cut(i, rows, train=True):
    """the inputs of a call that keeps ``rows`` target rows: g, a, the keep-masks and the lengths cut to them"""
    return dict(i, g=i["g"][:, :rows], a=[x[:, :, :rows] for x in i["a"]], pk=None if not train else i["pk"][:, :rows].contiguous(),
                keeps=None if not train else [[k[:, :rows].contiguous() for k in pair] for pair in i["keeps"]])


def _run_stack(m, i, lens=True, rows=None):
    """forward + backward through the module: (y bits, [map bits], {parameter: grad bits}, dsrc bits, d_mels bits, last_launches)"""
    _clear(m)
    src, mels = dev(i["src"]).requires_grad_(True), dev(i["mels"]).requires_grad_(True)
    y, attns = m(src, mels, i["src_mask"], i["tgt_mask"], src_lens=i["src_lens"] if lens else None, mel_lens=i["mel_lens"] if lens else None,
                 keep_masks=i["keeps"], prenet_keep_mask=i["pk"])
    torch.autograd.backward([y] + attns, [dev(i["g"])] + [dev(x) for x in i["a"]])
    return _bits(y), [_bits(x) for x in attns], _grads(m), _bits(src.grad), _bits(mels.grad), m.last_launches


def _run_chain(m, i, pos=None):
    """the hand chain: the Prenet op, then per layer crs_attn on a source leaf of its own, the row mask, pos_ffn, the row mask; dsrc is
    the fp32 sum of the two layers' (two terms: no order to choose)"""
    from smart_nar_fast_tts_amd import stacks

    _clear(m)
    mels = dev(i["mels"]).requires_grad_(True)
    rows = i["g"].shape[1]
    pos = m.position_enc.detach()[0] if pos is None else pos
    cut = mels[:, :rows]
    x = m.prenet(cut, pos, keep_mask=i["pk"])
    pad = i["tgt_mask"][:, :rows].contiguous()
    srcs, attns = [], []
    for n, layer in enumerate(m.layer_stack):
        ka, kf = i["keeps"][n] if i["keeps"] is not None else (None, None)
        s = dev(i["src"]).requires_grad_(True)
        x, attn = layer.crs_attn(x, s, s, lens=i["src_lens"], keep_mask=ka)
        x = stacks.mask_rows(x, mask=pad)
        x = layer.pos_ffn(x, keep_mask=kf)
        x = stacks.mask_rows(x, mask=pad)
        srcs.append(s)
        attns.append(attn)
    torch.autograd.backward([x] + attns, [dev(i["g"])] + [dev(a) for a in i["a"]])
    assert len(srcs) == 2
    return _bits(x), [_bits(a) for a in attns], _grads(m), _bits(srcs[0].grad + srcs[1].grad), _bits(mels.grad), None


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "y")
    assert len(a[1]) == len(b[1]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1])), (what, "maps")
    assert a[2].keys() == b[2].keys()
    for n in a[2]:
        assert (a[2][n] is None) == (b[2][n] is None) and (a[2][n] is None or np.array_equal(a[2][n], b[2][n])), (what, n)
    assert np.array_equal(a[3], b[3]), (what, "dsrc")
    assert np.array_equal(a[4], b[4]), (what, "d_mels")


def _formula(m):
    fwd = m.prenet.last_launches.get("forward", 0) + sum(ly.crs_attn.last_launches["forward"] + 1 + ly.pos_ffn.last_launches["forward"] + 1
                                                          for ly in m.layer_stack)
    bwd = m.prenet.last_launches.get("backward", 0) + sum(1 + ly.pos_ffn.last_launches.get("backward", 0) + 1 + ly.crs_attn.last_launches.get("backward", 0)
                                                           for ly in m.layer_stack)
    return fwd, bwd


def test_stack_equals_the_hand_chain(so):
    L, lib = so
    m, _ = _stack()
    m.train()
    i = _inputs()
    spec = importlib.util.spec_from_file_location("_ns_tools_bench", os.path.join(ROOT, "tools", "_bench.py"))
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    try:
        before = m.launches
        got = _run_stack(m, i)
        spent = m.launches - before
        fwd, bwd = _formula(m)
        assert got[5] == {"forward": fwd, "backward": bwd} and spent == fwd + bwd, (got[5], fwd, bwd, spent)
        assert m.prenet.last_launches == dict(zip(("forward", "backward"), _prenet_counts(lib, B * T)))
        want = _run_chain(m, i)
        _same(got, want, "stack vs chain")
        y = got[0].view(np.float32)
        pad = i["tgt_mask"].cpu().numpy().astype(bool)
        assert np.isfinite(y).all() and not got[0][pad].any() and np.abs(y[~pad]).max() > 0, "padded rows of the output are +0.0 by their bits"
        key_pad = sc.pad_of(SRC_LENS, L_SRC)
        for a in got[1]:
            assert a.shape == (B, H, T, L_SRC) and not np.moveaxis(a, 3, 1)[key_pad].any(), "a map is [B, H, T, L], exact 0 at padded phonemes"
        assert got[2]["position_enc"] is None and all(v is not None for n, v in got[2].items() if n != "position_enc")
        assert not got[4][:, 0].any() and np.abs(got[4].view(np.float32)).max() > 0 and np.abs(got[3].view(np.float32)).max() > 0
        # the masks alone (lengths derived and validated: host reads) give the same bits; both length vectors given: no host read
        _same(_run_stack(m, i, lens=False), got, "masks alone")
        src, mels = dev(i["src"]).requires_grad_(True), dev(i["mels"]).requires_grad_(True)
        gs = [dev(i["g"])] + [dev(x) for x in i["a"]]
        torch.cuda.synchronize()

        def step(lens=True):
            y, attns = m(src, mels, i["src_mask"], i["tgt_mask"], src_lens=i["src_lens"] if lens else None, mel_lens=i["mel_lens"] if lens else None,
                         keep_masks=i["keeps"], prenet_keep_mask=i["pk"])
            torch.autograd.backward([y] + attns, gs)

        n_reads, msgs = tb.host_reads(step)
        assert n_reads == 0, msgs
        assert tb.host_reads(lambda: step(False))[0] >= 2, "the counting sees the two validations of the masks-alone form"
        # the no_grad forward, with and without the maps
        with torch.no_grad():
            y0, a0 = m(dev(i["src"]), dev(i["mels"]), i["src_mask"], i["tgt_mask"], src_lens=i["src_lens"], mel_lens=i["mel_lens"], keep_masks=i["keeps"],
                       prenet_keep_mask=i["pk"])
            fwd0, _ = _formula(m)
            assert m.last_launches == {"forward": fwd0, "backward": 0} and fwd0 <= fwd
            y1, a1 = m(dev(i["src"]), dev(i["mels"]), i["src_mask"], i["tgt_mask"], return_attns=False, src_lens=i["src_lens"], mel_lens=i["mel_lens"],
                       keep_masks=i["keeps"], prenet_keep_mask=i["pk"])
        assert np.array_equal(_bits(y0), got[0]) and all(np.array_equal(_bits(p), q) for p, q in zip(a0, got[1])) and not y0.requires_grad
        assert np.array_equal(_bits(y1), got[0]) and a1 == []
        # durations() on the module's own last map
        dur = m.durations(a0[-1], i["src_lens"], i["mel_lens"]).cpu().numpy()
        assert np.array_equal(dur, alc.durations(a0[-1].cpu().numpy(), SRC_LENS, MEL_LENS)) and dur.sum(1).tolist() == MEL_LENS
    finally:
        _clear(m)


def test_forward_against_float64():
    m, w = _stack()
    m.eval()
    i = _inputs(seed=5)
    with torch.no_grad():
        y, attns = m(dev(i["src"]), dev(i["mels"]), i["src_mask"], i["tgt_mask"], src_lens=i["src_lens"], mel_lens=i["mel_lens"])
    ref = {}
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            yr, ar, _ = mc.statement(mc.leaves_of(w, dtype, i["src"], i["mels"]), SRC_LENS, MEL_LENS, H, 40, training=False, dtype=dtype)
        ref[dtype] = dict(y=yr.numpy(), **{f"attn{n}": a.numpy() for n, a in enumerate(ar)})
    got = dict(y=y.cpu().numpy(), **{f"attn{n}": a.cpu().numpy() for n, a in enumerate(attns)})
    sh = shares(got, ref[torch.float64], gates(ref[torch.float32], ref[torch.float64]))
    report(test="me_forward", shares=sh)
    assert max(sh.values()) <= 1.0, sh


def test_truncates_in_train_and_regenerates_in_eval(so):
    from smart_nar_fast_tts_amd import ops

    m, _ = _stack()  # max_seq_len 40
    Tc, lens = 45, [45, 3, 41]
    i = _inputs(Tc=Tc, mel_lens=lens, seed=9)
    try:
        m.train()
        c = _cut(i, 40)
        got = _run_stack(m, c)
        assert got[0].shape == (B, 40, D) and all(a.shape == (B, H, 40, L_SRC) for a in got[1]), "the maps are [B, H, max_mel_len, L]"
        assert not got[4][:, 40:].any() and not got[4][:, 0].any(), "d_mels past max_seq_len and at frame 0 is exactly 0"
        short = dict(c, mels=i["mels"][:, :40].copy(), tgt_mask=i["tgt_mask"][:, :40].contiguous(), mel_lens=i["mel_lens"].clamp(max=40))
        want = _run_chain(m, short)
        _same((got[0], got[1], got[2], got[3], got[4][:, :40]), want, "truncated vs chain")
        # eval(): the regenerated table, nothing truncated, one more launch
        m.eval()
        e = _cut(i, Tc, train=False)
        got = _run_stack(m, e)
        assert got[0].shape == (B, Tc, D) and all(a.shape == (B, H, Tc, L_SRC) for a in got[1])
        fwd, _ = _formula(m)
        assert got[5]["forward"] == fwd + 1
        want = _run_chain(m, e, pos=ops.sinusoid_table(Tc, D))
        _same(got, want, "regenerated vs chain")
        assert np.abs(got[4][:, 40:].view(np.float32)).max() > 0, "rows past 40 take part"
    finally:
        _clear(m)


def test_one_native_training_step():
    """a loss over y and the last map -> the stack's backward -> optim.ScheduledOptim.step_and_update_lr(): every updated tensor against
    optim_cpu.run on the DEVICE's own gradients, within optim_cpu.gate_of of the fp32 CPU step.  position_enc has no gradient and is
    passed over: its bits do not move."""
    from smart_nar_fast_tts_amd import optim, stacks

    src_m, _ = _stack()
    m = stacks.MelEncoder(_config())
    m.load_state_dict(src_m.state_dict())
    m = m.cuda().eval()
    i = _inputs(seed=13)
    args = (i["src_mask"], i["tgt_mask"])
    kw = dict(src_lens=i["src_lens"], mel_lens=i["mel_lens"])
    with torch.no_grad():
        y0 = m(dev(i["src"]), dev(i["mels"]), *args, **kw)[0].cpu().numpy()
    g = (np.float32(2.0 / (B * T)) * (y0 - i["g"])).astype(np.float32)  # the gradient of an MSE against a random target
    start = 3998
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    so_ = optim.ScheduledOptim(m, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, start)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == ["position_enc"]
    before = [p.detach().cpu().numpy().reshape(-1).copy() for _, p in named]
    pos_before = _bits(m.position_enc).copy()
    y, attns = m(dev(i["src"]), dev(i["mels"]), *args, **kw)
    torch.autograd.backward([y, attns[-1]], [dev(g), dev(i["a"][-1])])
    assert m.position_enc.grad is None and all(p.grad is not None for _, p in named)
    grads = [p.grad.detach().cpu().numpy().reshape(-1).copy() for _, p in named]
    so_.step_and_update_lr()
    lr = so_._optimizer.param_groups[0]["lr"]
    assert abs(lr - oc.lr_at(start + 1, **oc.SHIPPED)) <= 1e-12 * lr
    got = [p.detach().cpu().numpy().reshape(-1) for _, p in named]
    c = dict(params=before, grads=[grads], lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=None)
    p64, p32 = oc.run(c)[0]["p"], oc.torch_run(c)[0]["p"]
    sh = {}
    for (n, _), a, t32, w64 in zip(named, got, p32, p64):
        err = np.abs(a.astype(np.float64) - w64).max()
        sh[n] = float(err / oc.gate_of(t32, w64)) if np.isfinite(err) else float("inf")
    report(test="me_native_step", shares={"worst": max(sh.values())})
    assert max(sh.values()) <= 1.0, sh
    assert np.array_equal(_bits(m.position_enc), pos_before)
    assert any(not np.array_equal(a, b) for a, b in zip(got, before))
