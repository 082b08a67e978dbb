"""The position-wise feed-forward sublayer's training forward and backward on the GPU (csrc/ffngrad.hip through ns_fg_* and
sublayers.PositionwiseFeedForward), and sublayers.FFTBlock.

The one new kernel alone — the ReLU gate with the w_1 bias gradient, da holding NaN wherever h <= 0, dh pre-filled with NaN, the
workspace with 0xFF, some h exactly 0 — then the whole module: the saved h and z and y against float64 of their own inputs at the
existing fp32 bounds (tests/bf16_emu.py), every gradient at the project gate of tests/ffn_grad_cpu.py judged from the DEVICE's saved
tensors (a pre-activation within a rounding of zero may have the other sign in float64: that is the input's property, not an error of
the backward), needs_input_grad, run-to-run bits, replicas, the launch counts include/nar_fs2.h states, FFTBlock against the
hand-chained sublayers, and one native training step into optim.ScheduledOptim.  The yardstick itself is proven in
tests/test_ffn_grad_host.py.

Configs (d, d_inner, K1, K2): (256, 1024, 9, 1), (512, 2048, 9, 1), (256, 512, 3, 3).  Cases (B, S): one row per utterance (every tap
but the centre out of range); S < K1 (the taps must not read the neighbouring utterance); past the 32-row GEMM tile and the 64-row
block; the 64-row block edge from above; several weight-gradient row stages.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/ffn_grad.md is written from one).

Measured on the MI355X (profiles/ffn_grad.md): dh bit-equal, d_b1 of the gate alone at most 0.98 of one fp32 rounding of the float64
column sum (the bound is half an ulp), the saved h 0.012, z 0.012 and y 0.005 of their bounds, every gradient of the module at or
below 0.56 of its gate (d_w1, 2 x 1 rows at d = 256 in train()), the native step 0.42 of optim_cpu.gate_of."""
import numpy as np
import pytest
import torch

from tests import attention_grad_cpu as ac
from tests import bf16_emu as E
from tests import ffn_grad_cpu as fc
from tests import optim_cpu as oc
from tests.util import dev, native_lib, report

pytestmark = pytest.mark.gpu
REL = E.FP32_REL
CONFIGS = [(256, 1024, 9, 1), (512, 2048, 9, 1), (256, 512, 3, 3)]
CASES = [(2, 1), (3, 5), (2, 33), (1, 65), (3, 130)]
_cid = lambda c: f"{c[0]}x{c[1]}"  # noqa: E731
_fid = lambda c: f"d{c[0]}i{c[1]}k{c[2]}{c[3]}"  # noqa: E731


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _G(lib, M, N, Cin, KW):
    """G(M, N, KW Cin) of include/nar_fs2.h: the Conv1D-as-GEMM dispatch's own launch count"""
    n = lib.ns_plan_gemm_launches(M, N, Cin, KW, 0, None)
    assert n in (1, 2)
    return n


def _counts(lib, cfg, M):
    """(forward, full backward) as the header states them"""
    d, di, K1, K2 = cfg
    return 1 + _G(lib, M, di, d, K1) + _G(lib, M, d, di, K2) + 1, 9 + _G(lib, M, di, d, K2) + _G(lib, M, d, di, K1)


_MODULES = {}


def module(cfg, dropout=0.5):
    from smart_nar_fast_tts_amd import sublayers

    d, di, K1, K2 = cfg
    if cfg not in _MODULES:
        w = fc.seeded_weights(d, di, K1, K2, seed=200 + d + di + K1)
        m = sublayers.PositionwiseFeedForward(d, di, (K1, K2), dropout=dropout)
        m.load_state_dict({n: torch.from_numpy(w[k]) for n, k in zip(sublayers.FFN_PARAM_NAMES, fc.NAMES[:6])})
        _MODULES[cfg] = (m.cuda(), w)
    return _MODULES[cfg]


def _inputs(cfg, case, seed=0):
    d = cfg[0]
    B, S = case
    rs = np.random.RandomState(B * S + d + cfg[1] + seed)
    x = rs.standard_normal((B, S, d)).astype(np.float32)
    g = rs.standard_normal((B, S, d)).astype(np.float32)  # random on every row
    return x, g


def _saved_parts(saved, B, S, d, di):
    s = saved.cpu()
    return s[:B * S * di].reshape(B, S, di), s[B * S * di:].reshape(B, S, d)


def _run(m, x, g, keep=None, need=None):
    """one forward + backward through the module's own marshalling: (y, saved tensor, grads by fc.NAMES, launches)"""
    m.train(keep is not None)
    call = m._marshal(dev(x), None if keep is None else dev(keep))
    y, saved = m._forward(call, save=True)
    need = [True] * 7 if need is None else need
    outs = m._backward(call, saved, dev(g), need)
    grads = dict(zip(("dx",) + fc.NAMES[:6], (None if o is None else o.cpu().numpy().reshape(-1) for o in outs)))
    return y.cpu(), saved, grads, dict(m.last_launches)


# ---------------------------------------------------------------------------------------------------- the new kernel alone
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("shape", [(1, 256), (66, 1024), (65, 768), (390, 2048)], ids=_cid)
def test_relu_gate_alone(so, shape, in_place):
    """one row; past the 64-row block (a partial of 2 rows, of 1 row); three, four and eight column slabs; seven blocks"""
    L, lib = so
    M, di = shape
    rs = np.random.RandomState(M + di)
    h = np.maximum(rs.standard_normal((M, di)), 0.0).astype(np.float32)  # about half of it gated, as a ReLU output is
    h[rs.rand(M, di) < 0.05] = 0.0
    h[rs.rand(M, di) < 0.02] = -0.0
    h[0, 0], h[M - 1, di - 1] = 0.0, 1.5
    da = rs.standard_normal((M, di)).astype(np.float32)
    da[h <= 0] = np.nan
    want = np.where(h > 0, da, np.float32(0.0)).astype(np.float32)
    assert np.isfinite(want).all() and (h == 0).sum() > 0
    col = want.astype(np.float64).sum(0)
    for with_bias in (True, False):
        da_d, h_d = dev(da), dev(h)
        dh_d = da_d if in_place else torch.full((M, di), float("nan"), device="cuda")
        b1_d = torch.full((di,), float("nan"), device="cuda") if with_bias else None
        ws = torch.full((((M + 63) // 64) * 5 * di * 8,), 0xFF, dtype=torch.uint8, device="cuda")
        L.check(lib.ns_fg_op_relu_gate(L.ptr(da_d), L.ptr(h_d), M, di, L.ptr(dh_d), L.ptr(b1_d), L.ptr(ws), ws.numel(), L.stream_ptr()),
                "ns_fg_op_relu_gate")
        assert lib.ns_fg_last_launches() == (2 if with_bias else 1)  # the gate, and the column finish of d_b1
        got = dh_d.cpu().numpy()
        assert got.view(np.int32).tobytes() == want.view(np.int32).tobytes(), "dh is the select, bit for bit (+0.0 at gated positions)"
        assert h_d.cpu().numpy().tobytes() == h.tobytes()
        if with_bias:
            err = np.abs(b1_d.cpu().numpy().astype(np.float64) - col)
            bound = 2.0 ** -24 * np.abs(col) + 1e-30
            report(test="fg_relu_gate", shape=_cid(shape), in_place=in_place, d_b1=float((err / bound).max()))
            assert (err <= bound).all(), float((err / bound).max())


# ---------------------------------------------------------------------------------------------------- the whole module
def _grad_shares(cfg, x, g, saved_parts, grads, keep=None, p=0.0):
    _, w = module(cfg)
    r64 = fc.closed_form(x, w, g, saved_parts, keep, p, torch.float64)
    r32 = fc.closed_form(x, w, g, saved_parts, keep, p, torch.float32)
    return fc.shares(grads, r64, fc.gate(r32, r64))


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_module_forward_and_backward(so, cfg, case):
    L, lib = so
    m, w = module(cfg)
    d, di, K1, K2 = cfg
    B, S = case
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    x, g = _inputs(cfg, case)
    xt = torch.from_numpy(x)
    # ---- eval: the saved h and z and y at their bounds, then every gradient at the gate
    y, saved, grads, launches = _run(m, x, g)
    h, z = _saved_parts(saved, B, S, d, di)
    c1 = E.gemm_check(h, xt, wt["w1"], wt["b1"], act="relu", rel=REL, round_fn=E.exact)
    c2 = E.gemm_ln_check(y, h, wt["w2"], wt["b2"], xt, wt["ln_g"], wt["ln_b"], rel=REL, round_fn=E.exact)
    u64, unit = E.gemm_emu(h, wt["w2"], wt["b2"], round_fn=E.exact), E.gemm_unit(h, wt["w2"], wt["b2"], round_fn=E.exact)
    z64 = u64 + xt.double()
    z_share = float(((z.double() - z64).abs() / (REL * unit + REL * z64.abs())).max())
    sh = _grad_shares(cfg, x, g, (h, z), grads)
    fwd, bwd = _counts(lib, cfg, B * S)
    report(test="fg_module", cfg=_fid(cfg), case=_cid(case), mode="eval", launches=launches, h=c1.worst, z=z_share, y=c2.worst, shares=sh)
    assert c1.ok and c2.ok and z_share <= 1.0, (str(c1), str(c2), z_share)
    assert launches == dict(forward=fwd, backward=bwd), (launches, fwd, bwd)  # the counts include/nar_fs2.h states
    assert max(sh.values()) <= 1.0, sh
    # ---- train() at p = 0.5 with a given keep-mask
    keep = np.random.RandomState(B * S + 3).rand(B, S, d) >= m.p_drop
    y, saved, grads, launches = _run(m, x, g, keep.astype(np.uint8))
    h2, z = _saved_parts(saved, B, S, d, di)
    assert h2.numpy().tobytes() == h.numpy().tobytes()  # dropout sits behind w_2
    kf = torch.from_numpy(keep).double() / (1.0 - m.p_drop)
    z64 = u64 * kf + xt.double()
    assert bool(((z.double() - z64).abs() <= REL * unit * kf + REL * z64.abs()).all())
    y64 = E.layernorm_emu(z, wt["ln_g"], wt["ln_b"])
    assert bool(((y.double() - y64).abs() <= REL * (y64.abs() + wt["ln_b"].double().abs())).all())
    sh = _grad_shares(cfg, x, g, (h2, z), grads, keep, m.p_drop)
    report(test="fg_module", cfg=_fid(cfg), case=_cid(case), mode="train_p0.5", launches=launches, shares=sh)
    assert launches == dict(forward=fwd, backward=bwd), (launches, fwd, bwd)
    assert max(sh.values()) <= 1.0, sh


def test_needs_input_grad_run_to_run_bits_and_replicas(so):
    L, lib = so
    cfg, (B, S) = CONFIGS[0], CASES[4]
    m, w = module(cfg)
    m.eval()
    d, di, K1, K2 = cfg
    M = B * S
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
        bits = [None if p.grad is None else p.grad.cpu().numpy().tobytes() for p in params]
        return y.detach().cpu().numpy(), bits, None if xd.grad is None else xd.grad.cpu().numpy(), dict(m.last_launches)

    try:
        a, b = once(), once()
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), "two runs give identical bits"
        assert all(v is not None for v in a[1])
        assert a[0][0].tobytes() == a[0][2].tobytes(), "two replicas of an utterance get bit-identical y rows"
        assert a[2][0].tobytes() == a[2][2].tobytes(), "two replicas of an utterance get bit-identical dx rows"
        assert a[3] == dict(zip(("forward", "backward"), _counts(lib, cfg, M))), a[3]
        same = lambda r, skip=(): all(r[1][i] == a[1][i] for i in range(6) if i not in skip)  # noqa: E731
        nx = once(x_grad=False)
        assert nx[2] is None and same(nx) and nx[0].tobytes() == a[0].tobytes()
        assert nx[3]["backward"] == a[3]["backward"] - _G(lib, M, d, di, K1), (nx[3], a[3])  # no dx GEMM
        for i, drop in ((0, 2), (1, 1), (2, 2)):  # w1: its GEMM and reduce; b1: its column finish; w2: its GEMM and reduce
            fz = once(frozen=(i,))
            assert fz[1][i] is None and same(fz, (i,)) and fz[2].tobytes() == a[2].tobytes(), i
            assert fz[3]["backward"] == a[3]["backward"] - drop, (i, fz[3], a[3])
        fz = once(frozen=(3, 4, 5))  # none of b2, ln_g, ln_b: no finish at width d
        assert fz[1][3:] == [None] * 3 and same(fz, (3, 4, 5)) and fz[2].tobytes() == a[2].tobytes()
        assert fz[3]["backward"] == a[3]["backward"] - 1, (fz[3], a[3])
        tail = once(x_grad=False, frozen=(0, 1))  # nothing behind the ReLU: no pack, no da, no gate
        assert same(tail, (0, 1)) and tail[3]["backward"] == 4, tail[3]  # row backward, dW2's GEMM + reduce, the finish
        only_g = once(x_grad=False, frozen=(0, 1, 2, 3, 5))
        assert only_g[1][4] == a[1][4] and only_g[3]["backward"] == 2, only_g[3]  # exactly the row backward and the finish
        with torch.no_grad():
            quiet = m(dev(x))
        assert quiet.cpu().numpy().tobytes() == a[0].tobytes() and not quiet.requires_grad, "a forward that saves nothing gives the same y bits"
        assert m.last_launches["forward"] == a[3]["forward"]
        report(test="fg_launches", forward=a[3]["forward"], backward=a[3]["backward"], backward_no_dx=nx[3]["backward"],
                backward_tail_only=tail[3]["backward"], backward_ln_g_only=only_g[3]["backward"])
    finally:
        for p in params:
            p.requires_grad_(True)
            p.grad = None


def test_fft_block_equals_the_hand_chained_sublayers():
    from smart_nar_fast_tts_amd import sublayers

    d, H, di, ks, B, S, lens = 256, 2, 1024, (9, 1), 3, 33, [33, 1, 32]
    wa, wf = ac.seeded_weights(d, seed=301), fc.seeded_weights(d, di, ks[0], ks[1], seed=302)
    blk = sublayers.FFTBlock(d, H, d // H, d // H, di, ks, dropout=0.5)
    sd = {"slf_attn." + n: torch.from_numpy(wa[k]) for n, k in zip(sublayers.PARAM_NAMES, ac.NAMES[:10])}
    sd.update({"pos_ffn." + n: torch.from_numpy(wf[k]) for n, k in zip(sublayers.FFN_PARAM_NAMES, fc.NAMES[:6])})
    blk.load_state_dict(sd)
    blk = blk.cuda().train()
    rs = np.random.RandomState(77)
    x = rs.standard_normal((B, S, d)).astype(np.float32)
    g = rs.standard_normal((B, S, d)).astype(np.float32)
    keeps = [dev((rs.rand(B, S, d) >= 0.5).astype(np.uint8)) for _ in range(2)]
    lens_d = dev(np.asarray(lens, dtype=np.int64))
    mask = torch.arange(S, device="cuda")[None, :] >= lens_d[:, None]
    slf_attn_mask = mask[:, None, :].expand(B, S, S)
    params = list(blk.parameters())

    def grads_of(run):
        for p in params:
            p.grad = None
        xd = dev(x).requires_grad_(True)
        y = run(xd)
        y.backward(dev(g))
        return y.detach().cpu().numpy(), [p.grad.cpu().numpy().tobytes() for p in params], xd.grad.cpu().numpy().tobytes()

    def by_hand(xd):
        y, _ = blk.slf_attn(xd, xd, xd, mask=slf_attn_mask, lens=lens_d, keep_mask=keeps[0])
        y = y.masked_fill(mask.unsqueeze(-1), 0)
        y = blk.pos_ffn(y, keep_mask=keeps[1])
        return y.masked_fill(mask.unsqueeze(-1), 0)

    def block(xd):
        y, attn = blk(xd, mask=mask, slf_attn_mask=slf_attn_mask, lens=lens_d, keep_masks=keeps)
        assert attn is None
        return y

    try:
        got, want = grads_of(block), grads_of(by_hand)
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2]
        assert np.isfinite(got[0]).all() and not got[0][mask.cpu().numpy()].view(np.int32).any(), "padded rows of the output are exactly 0"
        assert np.abs(got[0][~mask.cpu().numpy()]).max() > 0
        via_mask = grads_of(lambda xd: blk(xd, mask=mask, slf_attn_mask=slf_attn_mask, keep_masks=keeps)[0])
        assert via_mask[0].tobytes() == got[0].tobytes() and via_mask[1] == got[1], "the mask and the lengths it stands for give the same bits"
    finally:
        for p in params:
            p.grad = None


def test_one_native_training_step():
    """a loss-shaped gradient -> this module's backward -> optim.ScheduledOptim.step_and_update_lr(): the six updated tensors against
    the float64 chain at optim_cpu.gate_of of the fp32 CPU chain.  Both chains take their gradients from ``closed_form`` on the
    device's saved h and z, as every gradient here is judged."""
    from smart_nar_fast_tts_amd import optim, sublayers

    cfg, case = CONFIGS[0], CASES[2]
    d, di, K1, K2 = cfg
    B, S = case
    src, w = module(cfg)
    m = sublayers.PositionwiseFeedForward(d, di, (K1, K2), dropout=0.5)
    m.load_state_dict(src.state_dict())
    m = m.cuda().eval()
    x, target = _inputs(cfg, case, seed=7)
    # loss-shaped: the gradient of an MSE against a random target, averaged over the B * S rows, taken at the fp32 CPU statement's y;
    # every chain below gets the same fp32 g
    y_cpu = fc.statement(x, w, dtype=torch.float32)["y"].numpy()
    g = (np.float32(2.0 / (B * S)) * (y_cpu - target)).astype(np.float32)
    start = 3998
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    so_ = optim.ScheduledOptim(m, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, start)
    _, saved = m._forward(m._marshal(dev(x), None), save=True)  # the same bits the autograd call below keeps
    parts = _saved_parts(saved, B, S, d, di)
    y = m(dev(x))
    y.backward(dev(g))
    so_.step_and_update_lr()
    lr = so_._optimizer.param_groups[0]["lr"]
    assert abs(lr - oc.lr_at(start + 1, **oc.SHIPPED)) <= 1e-12 * lr
    got = [p.detach().cpu().numpy().reshape(-1) for p in m.ordered_parameters()]
    chain = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        grads = fc.closed_form(x, w, g, parts, dtype=dtype)
        c = dict(params=[np.asarray(w[k], dtype=np.float32).reshape(-1) for k in fc.NAMES[:6]], grads=[[grads[k].reshape(-1) for k in fc.NAMES[:6]]],
                 lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=None)
        chain[name] = oc.run(c)[0]["p"] if name == "f64" else oc.torch_run(c)[0]["p"]
    sh = {}
    for k, a, t32, w64 in zip(fc.NAMES[:6], got, chain["f32"], chain["f64"]):
        err = np.abs(a.astype(np.float64) - w64).max()
        sh[k] = float(err / oc.gate_of(t32, w64)) if np.isfinite(err) else float("inf")
    report(test="fg_native_step", shares=sh)
    assert max(sh.values()) <= 1.0, sh
