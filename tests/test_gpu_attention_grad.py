"""The self-attention sublayer's training forward and backward on the GPU (csrc/attngrad.hip through ns_ag_* and
sublayers.MultiHeadAttention).

Each new kernel alone — the row log-sum-exp (also at scores around +90), the flash-style attention backward (workspace filled with
0xFF and the output with NaN beforehand, exact +0.0 at masked keys, NaN planted in the masked K and V rows), the row backward with and
without a keep-mask — then the whole module: the saved qkv and y against float64 of their own inputs at the existing bounds
(tests/bf16_emu.py), every gradient at the project gate of tests/attention_grad_cpu.py judged from the DEVICE's saved tensors,
needs_input_grad, run-to-run bits, replicas, the launch counts include/nar_fs2.h states, and one native training step into
optim.ScheduledOptim.  The yardstick itself is proven in tests/test_attention_grad_host.py.

Configs (d, H): (256, 2), (256, 8), (512, 8), i.e. dk = 128, 32, 64.  Cases (B, S, lens): one key; the 32-key tile edge from both
sides; just past the 128-query tile; several tiles with a skipped tail.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/attention_grad.md is written from one).

Measured on the MI355X (profiles/attention_grad.md): lse at most 0.026 of its bound (0.014 at scores around +90), the attention backward
alone at most 0.86 of the project gate (dV; dQ 0.70, dK 0.60), the row backward alone 0.14, the saved qkv 0.029 and y 0.011 of their
bounds, every gradient of the module at or below 0.80 of its gate (d_bq, 2 x 1 rows at d = 512), the native step 0.56 of
optim_cpu.gate_of."""
import numpy as np
import pytest
import torch

from tests import attention_grad_cpu as ac
from tests import bf16_emu as E
from tests import lossgrad_cpu as lg
from tests import optim_cpu as oc
from tests.util import dev, native_lib, report

pytestmark = pytest.mark.gpu
REL = E.FP32_REL
CONFIGS = [(256, 2), (256, 8), (512, 8)]
CASES = [(2, 1, [1, 1]), (3, 33, [33, 1, 32]), (2, 130, [130, 97]), (3, 343, [343, 129, 3])]
_cid = lambda c: f"{c[0]}x{c[1]}"  # noqa: E731
_fid = lambda c: f"d{c[0]}h{c[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _ws(nbytes, fill=0xFF):
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def _gemm_launches(lib, M, N, K):
    n = lib.ns_plan_gemm_launches(M, N, K, 1, 0, None)
    assert n in (1, 2)
    return n


_MODULES = {}


def module(cfg, dropout=0.5):
    from smart_nar_fast_tts_amd import sublayers

    d, H = cfg
    if cfg not in _MODULES:
        w = ac.seeded_weights(d, seed=100 + d + H)
        m = sublayers.MultiHeadAttention(H, d, d // H, d // H, dropout=dropout)
        m.load_state_dict({n: torch.from_numpy(w[k]) for n, k in zip(sublayers.PARAM_NAMES, ac.NAMES[:10])})
        _MODULES[cfg] = (m.cuda(), w)
    return _MODULES[cfg]


def _inputs(cfg, case, seed=0):
    d, _ = cfg
    B, S, lens = case
    rs = np.random.RandomState(B * S + d + seed)
    x = rs.standard_normal((B, S, d)).astype(np.float32)
    g = rs.standard_normal((B, S, d)).astype(np.float32)  # random on every row, padded ones included
    return x, g


def _saved_parts(saved, B, S, d, H):
    md = B * S * d
    s = saved.cpu()
    return s[:3 * md].reshape(B, S, 3 * d), s[3 * md:4 * md].reshape(B, S, d), s[4 * md:5 * md].reshape(B, S, d), s[5 * md:].reshape(B, H, S)


def _run(m, x, lens, g, keep=None, need=None):
    """one forward + backward through the module's own marshalling: (y, saved tensor, grads by ac.NAMES, launches)"""
    m.train(keep is not None)
    call = m._marshal(dev(x), None, dev(np.asarray(lens, dtype=np.int64)), None if keep is None else dev(keep))
    y, saved = m._forward(call, save=True)
    need = [True] * 11 if need is None else need
    outs = m._backward(call, saved, dev(g), need)
    grads = dict(zip(("dx",) + ac.NAMES[:10], (None if o is None else o.cpu().numpy().reshape(-1) for o in outs)))
    return y.cpu(), saved, grads, dict(m.last_launches)


_FWD = {}


def forward_saved(cfg, case):
    """(x, g, lens, y, the four saved tensors on the CPU) of the eval forward, computed once per (config, case) and left unchanged"""
    key = (cfg, _cid(case))
    if key not in _FWD:
        m, _ = module(cfg)
        B, S, lens = case
        x, g = _inputs(cfg, case)
        m.eval()
        call = m._marshal(dev(x), None, dev(np.asarray(lens, dtype=np.int64)), None)
        y, saved = m._forward(call, save=True)
        _FWD[key] = (x, g, y.cpu(), _saved_parts(saved, B, S, cfg[0], cfg[1]))
    return _FWD[key]


# ---------------------------------------------------------------------------------------------------- each kernel alone
def _lse_check(so, qkv, lens, B, S, d, H):
    L, lib = so
    lse = torch.full((B, H, S), float("nan"), device="cuda")
    q_d, l_d = dev(qkv), dev(np.asarray(lens, dtype=np.int64))
    L.check(lib.ns_ag_op_lse(L.ptr(q_d), L.ptr(l_d), B, S, d, H, L.ptr(lse), L.stream_ptr()), "ns_ag_op_lse")
    assert lib.ns_ag_last_launches() == 1
    ref = ac.lse_of(qkv, lens, H, torch.float64)
    q64 = torch.from_numpy(qkv).double()
    Q, K = ac.split_heads(q64[..., :d], H).abs(), ac.split_heads(q64[..., d:2 * d], H).abs()
    unit = (Q @ K.transpose(-1, -2)).masked_fill(ac.key_mask(lens, S)[:, None], 0.0).amax(-1) * (d // H) ** -0.5
    bound = REL * (1 + ref.abs()) + REL * unit
    got = lse.cpu().double()
    assert bool(torch.isfinite(got).all())
    share = float(((got - ref).abs() / bound).max())
    return share, ref


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_lse_alone_elementwise(so, cfg, case):
    d, H = cfg
    B, S, lens = case
    qkv = np.random.RandomState(B * S + H).standard_normal((B, S, 3 * d)).astype(np.float32)
    share, _ = _lse_check(so, qkv, lens, B, S, d, H)
    report(test="ag_lse", cfg=_fid(cfg), case=_cid(case), share=share)
    assert share <= 1.0, share


@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_lse_at_scores_around_90(so, cfg):
    """exp(90) is past the fp32 range: a kernel without the row maximum gives inf here (so does the naive fp32 statement)"""
    d, H = cfg
    B, S, lens = CASES[2]
    dk = d // H
    rs = np.random.RandomState(d + H)
    qkv = (rs.standard_normal((B, S, 3 * d)) * 0.3).astype(np.float32)
    qkv[..., :2 * d] += np.float32(np.sqrt(90.0 / np.sqrt(dk)))
    share, ref = _lse_check(so, qkv, lens, B, S, d, H)
    assert 80 < float(ref.min()) and float(ref.max()) < 120
    assert not bool(torch.isfinite(ac.lse_of(qkv, lens, H, torch.float32, with_max=False)).all())
    report(test="ag_lse_shifted", cfg=_fid(cfg), share=share)
    assert share <= 1.0, share


def _attention_backward(so, qkv, ctx, lse, dctx, lens, B, S, d, H):
    L, lib = so
    ws = _ws(B * H * S * 4 + 256)
    out = torch.full((B, S, 3 * d), float("nan"), device="cuda")
    t = [dev(a.numpy() if isinstance(a, torch.Tensor) else a) for a in (qkv, ctx, lse, dctx)]
    l_d = dev(np.asarray(lens, dtype=np.int64))
    L.check(lib.ns_ag_op_attention_backward(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(l_d), B, S, d, H, L.ptr(out), L.ptr(ws),
                                            ws.numel(), L.stream_ptr()), "ns_ag_op_attention_backward")
    assert lib.ns_ag_last_launches() == 2
    return out.cpu()


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_attention_backward_alone(so, cfg, case):
    d, H = cfg
    B, S, lens = case
    x, g, y, (qkv, ctx, z, lse) = forward_saved(cfg, case)
    dctx = np.random.RandomState(B * S + 3 * H).standard_normal((B, S, d)).astype(np.float32)
    got = _attention_backward(so, qkv, ctx, lse, dctx, lens, B, S, d, H)
    r64 = ac.attention_backward(qkv, ctx, lse, dctx, lens, H, torch.float64)
    r32 = ac.attention_backward(qkv, ctx, lse, dctx, lens, H, torch.float32)
    sh = {}
    for i, n in enumerate(("dq", "dk", "dv")):
        a, w64, w32 = (t[..., i * d:(i + 1) * d].double() for t in (got, r64, r32))
        gate = 2.0 * float((w32 - w64).abs().max()) + lg.ulp32(float(w64.abs().max()))
        sh[n] = float((a - w64).abs().max() / gate) if bool(torch.isfinite(a).all()) else float("inf")
    report(test="ag_attention_backward", cfg=_fid(cfg), case=_cid(case), shares=sh)
    # dK and dV at keys >= lens[b]: exactly +0.0
    pad = torch.from_numpy(np.arange(S)[None, :] >= np.asarray(lens)[:, None])
    assert not got[..., d:][pad].view(torch.int32).any()
    # a NaN in the K and V rows past lens[b] reaches nothing
    if bool(pad.any()):
        dirty = qkv.clone()
        dirty[..., d:][pad] = float("nan")
        again = _attention_backward(so, dirty, ctx, lse, dctx, lens, B, S, d, H)
        assert again.numpy().tobytes() == got.numpy().tobytes()
    assert max(sh.values()) <= 1.0, sh


@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_row_backward_alone(so, p, d):
    """197 rows: past one workgroup's 64 (four column partials, the last one of 5 rows)"""
    L, lib = so
    M = 197
    rs = np.random.RandomState(23 + d)
    z, dy = rs.standard_normal((M, d)).astype(np.float32), rs.standard_normal((M, d)).astype(np.float32)
    ln_g = (1 + 0.2 * rs.standard_normal(d)).astype(np.float32)
    keep = (rs.rand(M, d) >= p) if p > 0 else None
    outs = {n: torch.full(s, float("nan"), device="cuda") for n, s in (("dz", (M, d)), ("du", (M, d)), ("d_ln_g", (d,)), ("d_ln_b", (d,)), ("d_bfc", (d,)))}
    ws = _ws(4 << 20)
    keep_d = None if keep is None else dev(keep.astype(np.uint8))
    t = {n: dev(a) for n, a in dict(dy=dy, z=z, ln_g=ln_g).items()}
    L.check(lib.ns_ag_op_row_backward(L.ptr(t["dy"]), L.ptr(t["z"]), L.ptr(t["ln_g"]), L.ptr(keep_d), p, M, d,
                                      *[L.ptr(outs[n]) for n in ("dz", "du", "d_ln_g", "d_ln_b", "d_bfc")], L.ptr(ws), ws.numel(), L.stream_ptr()),
            "ns_ag_op_row_backward")
    assert lib.ns_ag_last_launches() == 2

    def ref(dtype):
        c = lambda a: torch.as_tensor(a).to(dtype)  # noqa: E731
        k = None if keep is None else c(keep) * torch.tensor(1.0 / (1.0 - p), dtype=dtype)
        return dict(zip(("dz", "du", "d_ln_g", "d_ln_b", "d_bfc"), (a.numpy() for a in ac.row_backward(c(dy), c(z), c(ln_g), k))))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    gates = ac.gate(r32, r64, names=list(r64))
    sh = ac.shares({n: outs[n].cpu().numpy() for n in r64}, r64, gates, names=list(r64))
    if keep is not None:
        assert not outs["du"][dev(~keep)].any()
    report(test="ag_row_backward", p=p, d=d, shares=sh)
    assert max(sh.values()) <= 1.0, sh


# ---------------------------------------------------------------------------------------------------- the whole module
def _grad_shares(cfg, case, x, g, saved_parts, grads, keep=None, p=0.0):
    _, w = module(cfg)
    _, _, lens = case
    r64 = ac.closed_form(x, w, lens, cfg[1], g, saved_parts, keep, p, torch.float64)
    r32 = ac.closed_form(x, w, lens, cfg[1], g, saved_parts, keep, p, torch.float32)
    return ac.shares(grads, r64, ac.gate(r32, r64))


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_module_forward_and_backward(so, cfg, case):
    L, lib = so
    m, w = module(cfg)
    d, H = cfg
    B, S, lens = case
    M = B * S
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    # ---- eval: the saved qkv and y at their bounds, then every gradient at the gate
    x, g = _inputs(cfg, case)
    y, saved, grads, launches = _run(m, x, lens, g)
    parts = _saved_parts(saved, B, S, d, H)
    qkv, ctx, z, lse = parts
    xt = torch.from_numpy(x)
    c1 = E.gemm_check(qkv, xt, torch.cat([wt["wq"], wt["wk"], wt["wv"]]), torch.cat([wt["bq"], wt["bk"], wt["bv"]]), rel=REL, round_fn=E.exact)
    c2 = E.gemm_ln_check(y, ctx, wt["wfc"], wt["bfc"], xt, wt["ln_g"], wt["ln_b"], rel=REL, round_fn=E.exact)
    assert c1.ok and c2.ok, (str(c1), str(c2))
    sh = _grad_shares(cfg, case, x, g, parts, grads)
    fwd = 1 + _gemm_launches(lib, M, 3 * d, d) + 1 + 1 + _gemm_launches(lib, M, d, d) + 1
    bwd = 14 + _gemm_launches(lib, M, d, d) + _gemm_launches(lib, M, d, 3 * d)
    report(test="ag_module", cfg=_fid(cfg), case=_cid(case), mode="eval", launches=launches, qkv=c1.worst, y=c2.worst, shares=sh)
    assert launches == dict(forward=fwd, backward=bwd), (launches, fwd, bwd)  # the counts include/nar_fs2.h states
    assert max(sh.values()) <= 1.0, sh
    # ---- train() at p = 0.5 with a given keep-mask
    keep = np.random.RandomState(B * S + 3).rand(B, S, d) >= m.p_drop
    y, saved, grads, launches = _run(m, x, lens, g, keep.astype(np.uint8))
    parts = _saved_parts(saved, B, S, d, H)
    qkv, ctx, z, lse = parts
    kf = torch.from_numpy(keep).double() / (1.0 - m.p_drop)
    u64 = E.gemm_emu(ctx, wt["wfc"], wt["bfc"], round_fn=E.exact)
    unit = E.gemm_unit(ctx, wt["wfc"], wt["bfc"], round_fn=E.exact)
    z64 = u64 * kf + xt.double()
    assert bool(((z.double() - z64).abs() <= REL * unit * kf + REL * z64.abs()).all())
    y64 = E.layernorm_emu(z, wt["ln_g"], wt["ln_b"])
    assert bool(((y.double() - y64).abs() <= REL * (y64.abs() + wt["ln_b"].double().abs())).all())
    sh = _grad_shares(cfg, case, x, g, parts, grads, keep, m.p_drop)
    report(test="ag_module", cfg=_fid(cfg), case=_cid(case), mode="train_p0.5", launches=launches, shares=sh)
    assert max(sh.values()) <= 1.0, sh


def test_needs_input_grad_run_to_run_bits_and_replicas(so):
    L, lib = so
    cfg, case = CONFIGS[0], CASES[2]
    m, w = module(cfg)
    m.eval()
    d, H = cfg
    B, S, lens = 3, case[1], [case[2][1], case[2][0], case[2][1]]  # utterances 0 and 2 are replicas
    x, g = _inputs(cfg, (B, S, lens))
    x[2], g[2] = x[0], g[0]
    params = m.ordered_parameters()
    lens_d = dev(np.asarray(lens, dtype=np.int64))

    def once(x_grad=True, frozen=(), with_mask=False):
        for i, p in enumerate(params):
            p.requires_grad_(i not in frozen)
            p.grad = None
        xd = dev(x).requires_grad_(x_grad)
        if with_mask:
            mask = (torch.arange(S, device="cuda")[None, None, :] >= lens_d[:, None, None]).expand(B, S, S)
            y, attn = m(xd, xd, xd, mask=mask)
        else:
            y, attn = m(xd, xd, xd, lens=lens_d)
        assert attn is None
        y.backward(dev(g))
        bits = [None if p.grad is None else p.grad.cpu().numpy().tobytes() for p in params]
        return y.detach().cpu().numpy().tobytes(), bits, None if xd.grad is None else xd.grad.cpu().numpy(), dict(m.last_launches)

    try:
        a, b = once(), once()
        assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), "two runs give identical bits"
        assert all(v is not None for v in a[1])
        assert a[2][0].tobytes() == a[2][2].tobytes(), "two replicas of an utterance get bit-identical dx rows"
        via_mask = once(with_mask=True)
        assert via_mask[0] == a[0] and via_mask[1] == a[1], "the mask and the lengths it stands for give the same bits"
        nx = once(x_grad=False)
        assert nx[2] is None and nx[1] == a[1] and nx[0] == a[0]
        assert nx[3]["backward"] == a[3]["backward"] - _gemm_launches(lib, B * S, d, 3 * d), (nx[3], a[3])  # no dx GEMM
        fz = once(frozen=(0,))
        assert fz[1][0] is None and fz[1][1:] == a[1][1:] and fz[2].tobytes() == a[2].tobytes()
        assert fz[3]["backward"] == a[3]["backward"] - 2, (fz[3], a[3])  # no wgrad, no reduce
        tail = once(x_grad=False, frozen=(0, 1, 2, 3, 4, 5))  # only fc and layer_norm: nothing behind ctx
        assert tail[1][6:] == a[1][6:] and tail[3]["backward"] == 4, tail[3]  # row backward, dWfc's GEMM + reduce, the final column sums: no pack, no dctx
        with torch.no_grad():
            xd = dev(x)
            quiet, _ = m(xd, xd, xd, lens=lens_d)
        assert quiet.cpu().numpy().tobytes() == a[0] and not quiet.requires_grad
        assert m.last_launches["forward"] == a[3]["forward"] - 1  # nothing kept: no lse launch
        with pytest.raises(NotImplementedError, match="self-attention only"):
            m(xd, xd.clone(), xd)
        bad = torch.zeros(B, S, S, dtype=torch.bool, device="cuda")
        bad[0, 1, 2] = True
        with pytest.raises(ValueError, match="not a key-padding mask"):
            m(xd, xd, xd, mask=bad)
        report(test="ag_launches", forward=a[3]["forward"], backward=a[3]["backward"], backward_no_dx=nx[3]["backward"], backward_frozen_wq=fz[3]["backward"],
                backward_tail_only=tail[3]["backward"])
    finally:
        for p in params:
            p.requires_grad_(True)
            p.grad = None


def test_one_native_training_step():
    """a loss-shaped gradient -> this module's backward -> optim.ScheduledOptim.step_and_update_lr(): the ten updated tensors against
    the float64 chain at optim_cpu.gate_of of torch's fp32 CPU chain.  (d_bk is zero in exact arithmetic, so Adam's first step moves
    every element of w_ks.bias by +-lr on the sign of rounding noise, in torch's fp32 chain as here: its gate is 4 lr.)"""
    from smart_nar_fast_tts_amd import optim, sublayers

    cfg, case = CONFIGS[0], CASES[1]
    d, H = cfg
    B, S, lens = case
    src, w = module(cfg)
    m = sublayers.MultiHeadAttention(H, d, d // H, d // H, dropout=0.5)
    m.load_state_dict(src.state_dict())
    m = m.cuda().eval()
    x, target = _inputs(cfg, case, seed=7)
    # loss-shaped: the gradient of an MSE against a random target, averaged over the B * S rows (as the pitch / energy / duration MSEs
    # average over their B * S elements), taken at the fp32 CPU statement's y; every chain below gets the same fp32 g
    y_cpu = ac.statement(x, w, lens, H, dtype=torch.float32)["y"].numpy()
    g = (np.float32(2.0 / (B * S)) * (y_cpu - target)).astype(np.float32)
    start = 3998
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    so_ = optim.ScheduledOptim(m, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, start)
    xd = dev(x)
    y, _ = m(xd, xd, xd, lens=dev(np.asarray(lens, dtype=np.int64)))
    y.backward(dev(g))
    so_.step_and_update_lr()
    lr = so_._optimizer.param_groups[0]["lr"]
    assert abs(lr - oc.lr_at(start + 1, **oc.SHIPPED)) <= 1e-12 * lr
    got = [p.detach().cpu().numpy().reshape(-1) for p in m.ordered_parameters()]
    chain = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        grads, _ = ac.autograd_ref(x, w, lens, H, g, dtype=dtype)
        c = dict(params=[np.asarray(w[k], dtype=np.float32).reshape(-1) for k in ac.NAMES[:10]], grads=[[grads[k].reshape(-1) for k in ac.NAMES[:10]]],
                 lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=None)
        chain[name] = oc.run(c)[0]["p"] if name == "f64" else oc.torch_run(c)[0]["p"]
    sh = {}
    for k, a, t32, w64 in zip(ac.NAMES[:10], got, chain["f32"], chain["f64"]):
        err = np.abs(a.astype(np.float64) - w64).max()
        sh[k] = float(err / oc.gate_of(t32, w64)) if np.isfinite(err) else float("inf")
    report(test="ag_native_step", shares=sh)
    assert max(sh.values()) <= 1.0, sh
