"""The cross-attention sublayer's training forward and backward on the GPU (csrc/xattngrad.hip through ns_xg_* and
sublayers.MultiHeadCrossAttention).

The two new kernels alone (workspace filled with 0xFF and the outputs with NaN beforehand; the map's gradient absent, on head 0 only and
dense; the query split forced and planned; exact +0.0 at masked keys; NaN planted in the masked K and V rows and in the masked columns
of dA), then the forward (the map and ctx at tests/aligner_cpu.py's elementwise bound, q, kv and y at the existing GEMM bounds of
tests/bf16_emu.py), then the whole module: every gradient at the project gate of tests/cross_attention_grad_cpu.py judged from the
DEVICE's saved tensors, needs_input_grad, run-to-run bits, replicas, mask against lens, no host read, the launch counts
include/nar_fs2.h states, and one chain from a loss-shaped map gradient into optim.ScheduledOptim.  The yardstick itself is proven in
tests/test_cross_attention_grad_host.py.

Configs (d, H): (256, 2), (256, 4), (512, 8), i.e. dk = 128, 64, 64.  Cases (B, T, L, src_lens): the smallest shape; T across a 32-row
tile with L under a tile and no multiple of 4; two query workgroups with a length on a tile edge; two key workgroups, one wholly past
its length; a planned query split above 1.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/cross_attention_grad.md is written from one).

Measured on the MI355X (profiles/cross_attention_grad.md): the attention backward alone at most 0.70 of the project gate (dK; dQ 0.57,
dV 0.54), the forward's map 0.037 and ctx 0.018 of the aligner's elementwise bound, q 0.051, kv 0.028 and y 0.011 of their GEMM
bounds, every gradient of the module at or below 0.73 of its gate (dWq at 2 x 1 x 1, d = 256, H = 4: with one key dS is zero in exact
arithmetic, so dWq, d_bq, dWk and d_bk are rounding noise there), the chain 0.50 of optim_cpu.gate_of."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import aligner_cpu as al
from tests import bf16_emu as E
from tests import cross_attention_grad_cpu as xc
from tests import lossgrad_cpu as lg
from tests import optim_cpu as oc
from tests.util import dev, native_lib, report

pytestmark = pytest.mark.gpu
REL = E.FP32_REL
CONFIGS = [(256, 2), (256, 4), (512, 8)]
CASES = [(2, 1, 1, [1, 1]), (3, 33, 5, [5, 1, 4]), (2, 130, 37, [37, 32]), (2, 70, 131, [131, 97]), (3, 343, 40, [40, 9, 33])]
_cid = lambda c: f"{c[0]}x{c[1]}x{c[2]}"  # noqa: E731
_fid = lambda c: f"d{c[0]}h{c[1]}"  # noqa: E731


def lens_d(lens):
    return dev(np.asarray(lens, dtype=np.int64))


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _gemm_launches(lib, M, N, K):
    n = lib.ns_plan_gemm_launches(M, N, K, 1, 0, None)
    assert n in (1, 2)
    return n


def _splits(so, cfg, case):
    L, lib = so
    return lib.ns_xg_kv_splits(C.byref(L.NsXgShape(case[0], case[1], case[2], cfg[0], cfg[1])))


_MODULES = {}


def module(cfg, dropout=0.5):
    from smart_nar_fast_tts_amd import sublayers

    d, H = cfg
    if cfg not in _MODULES:
        w = xc.seeded_weights(d, seed=100 + d + H)
        m = sublayers.MultiHeadCrossAttention(H, d, d // H, d // H, dropout=dropout)
        m.load_state_dict({n: torch.from_numpy(w[k]) for n, k in zip(sublayers.PARAM_NAMES, xc.NAMES[:10])})
        _MODULES[cfg] = (m.cuda(), w)
    return _MODULES[cfg]


def _inputs(cfg, case, seed=0):
    d, H = cfg
    B, T, L, lens = case
    rs = np.random.RandomState(B * T + L + d + seed)
    tgt = rs.standard_normal((B, T, d)).astype(np.float32)
    src = rs.standard_normal((B, L, d)).astype(np.float32)
    g = rs.standard_normal((B, T, d)).astype(np.float32)  # random on every row
    a = rs.standard_normal((B, H, T, L)).astype(np.float32)
    return tgt, src, g, a


def _saved_parts(saved, attn, B, T, L, d, H):
    mt, ml = B * T * d, B * L * 2 * d
    s = saved.cpu()
    return (s[:mt].reshape(B, T, d), s[mt:mt + ml].reshape(B, L, 2 * d), s[mt + ml:2 * mt + ml].reshape(B, T, d),
            s[2 * mt + ml:3 * mt + ml].reshape(B, T, d), attn.cpu())


def _run(m, tgt, src, lens, g, a, keep=None, need=None):
    """one forward + backward through the module's own marshalling: (y, attn, saved tensor, grads by xc.NAMES, launches)"""
    m.train(keep is not None)
    td, sd = dev(tgt), dev(src)
    call = m._marshal(td, sd, None, lens_d(lens), None if keep is None else dev(keep))
    y, attn, saved = m._forward(call, save=True)
    need = [True] * 12 if need is None else need
    outs = m._backward(call, saved, attn, dev(g), None if a is None else dev(a), need)
    grads = dict(zip(("dtgt", "dsrc") + xc.NAMES[:10], (None if o is None else o.cpu().numpy().reshape(-1) for o in outs)))
    return y.cpu(), attn, saved, grads, dict(m.last_launches)


_FWD = {}


def forward_saved(cfg, case):
    """(tgt, src, g, a, y, the five saved tensors on the CPU) of the eval forward, computed once per (config, case) and left unchanged"""
    key = (cfg, _cid(case))
    if key not in _FWD:
        m, _ = module(cfg)
        B, T, L, lens = case
        tgt, src, g, a = _inputs(cfg, case)
        m.eval()
        call = m._marshal(dev(tgt), dev(src), None, lens_d(lens), None)
        y, attn, saved = m._forward(call, save=True)
        _FWD[key] = (tgt, src, g, a, y.cpu(), _saved_parts(saved, attn, B, T, L, cfg[0], cfg[1]), dict(m.last_launches))
    return _FWD[key]


# ---------------------------------------------------------------------------------------------------- the new kernels alone
def _attention_backward(so, q, kv, ctx, attn, dctx, dA, lens, B, T, L, d, H, ks):
    L_, lib = so
    nsplit = ks if ks else lib.ns_xg_kv_splits(C.byref(L_.NsXgShape(B, T, L, d, H)))
    ws = torch.full((B * H * T * 4 + 256 + nsplit * B * L * 2 * d * 4 + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    dq = torch.full((B, T, d), float("nan"), device="cuda")
    dkv = torch.full((B, L, 2 * d), float("nan"), device="cuda")
    t = [None if x is None else dev(x.numpy() if isinstance(x, torch.Tensor) else x) for x in (q, kv, ctx, attn, dctx, dA)]
    l_d = lens_d(lens)
    L_.check(lib.ns_xg_op_attention_backward(*[L_.ptr(x) for x in t], L_.ptr(l_d), B, T, L, d, H, ks, L_.ptr(dq), L_.ptr(dkv), L_.ptr(ws), ws.numel(),
                                             L_.stream_ptr()), "ns_xg_op_attention_backward")
    assert lib.ns_xg_last_launches() == 2 + (nsplit > 1)
    return dq.cpu(), dkv.cpu()


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_attention_backward_alone(so, cfg, case):
    d, H = cfg
    B, T, L, lens = case
    tgt, src, g, a, y, (q, kv, ctx, z, attn), _ = forward_saved(cfg, case)
    if T == 343:
        assert _splits(so, cfg, case) > 1
    dctx = np.random.RandomState(B * T + 3 * H).standard_normal((B, T, d)).astype(np.float32)
    a_h0 = a.copy()
    a_h0[:, 1:] = 0.0
    masked = np.broadcast_to(xc.key_mask(lens, L).numpy()[:, None], a.shape)
    pad = torch.from_numpy(np.arange(L)[None, :] >= np.asarray(lens)[:, None])
    worst = {}
    for name, dA in (("none", None), ("head0", a_h0), ("dense", a)):
        r64 = xc.attention_backward(q, kv, ctx, attn, dctx, dA, lens, H, torch.float64)
        r32 = xc.attention_backward(q, kv, ctx, attn, dctx, dA, lens, H, torch.float32)
        want = {"dq": (r64[0], r32[0]), "dk": (r64[1][..., :d], r32[1][..., :d]), "dv": (r64[1][..., d:], r32[1][..., d:])}
        for ks in ((1, 3) if T == 70 else (0,)):
            dq, dkv = _attention_backward(so, q, kv, ctx, attn, dctx, dA, lens, B, T, L, d, H, ks)
            got = {"dq": dq, "dk": dkv[..., :d], "dv": dkv[..., d:]}
            sh = {}
            for n, (w64, w32) in want.items():
                gate = 2.0 * float((w32.double() - w64).abs().max()) + lg.ulp32(float(w64.abs().max()))
                x = got[n].double()
                sh[n] = float((x - w64).abs().max() / gate) if bool(torch.isfinite(x).all()) else float("inf")
            print(f"{_fid(cfg)} {_cid(case)} dA {name} kv_splits {ks}: {sh}")
            report(test="xg_attention_backward", cfg=_fid(cfg), case=_cid(case), dA=name, kv_splits=ks, shares=sh)
            for n, v in sh.items():
                worst[n] = max(worst.get(n, 0.0), v)
            # dK and dV at keys >= src_lens[b]: exactly +0.0
            assert not dkv[pad].view(torch.int32).any()
            if bool(pad.any()):
                # a NaN in the K and V rows past src_lens[b] reaches nothing
                dirty = kv.clone()
                dirty[pad] = float("nan")
                again = _attention_backward(so, q, dirty, ctx, attn, dctx, dA, lens, B, T, L, d, H, ks)
                assert again[0].numpy().tobytes() == dq.numpy().tobytes() and again[1].numpy().tobytes() == dkv.numpy().tobytes()
                if dA is not None:
                    # nor does a NaN in dA at those keys
                    dirty = dA.copy()
                    dirty[masked] = np.nan
                    again = _attention_backward(so, q, kv, ctx, attn, dctx, dirty, lens, B, T, L, d, H, ks)
                    assert again[0].numpy().tobytes() == dq.numpy().tobytes() and again[1].numpy().tobytes() == dkv.numpy().tobytes()
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_forward(so, cfg, case):
    L_, lib = so
    _, w = module(cfg)
    d, H = cfg
    B, T, L, lens = case
    tgt, src, g, a, y, (q, kv, ctx, z, attn), launches = forward_saved(cfg, case)
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    tt, st = torch.from_numpy(tgt), torch.from_numpy(src)
    c1 = E.gemm_check(q, tt, wt["wq"], wt["bq"], rel=REL, round_fn=E.exact)
    c2 = E.gemm_check(kv, st, torch.cat([wt["wk"], wt["wv"]]), torch.cat([wt["bk"], wt["bv"]]), rel=REL, round_fn=E.exact)
    c3 = E.gemm_ln_check(y, ctx, wt["wfc"], wt["bfc"], tt, wt["ln_g"], wt["ln_b"], rel=REL, round_fn=E.exact)
    rp, rc = al.attention_gate(q, kv, torch.as_tensor(lens), H, ctx, attn)
    print(f"{_fid(cfg)} {_cid(case)}: q {c1.worst:.3g} kv {c2.worst:.3g} y {c3.worst:.3g} attn {rp:.3g} ctx {rc:.3g}")
    report(test="xg_forward", cfg=_fid(cfg), case=_cid(case), q=c1.worst, kv=c2.worst, y=c3.worst, attn=rp, ctx=rc)
    masked = torch.from_numpy(np.broadcast_to(xc.key_mask(lens, L).numpy()[:, None], tuple(attn.shape)).copy())
    assert not attn[masked].view(torch.int32).any(), "masked keys hold exactly +0.0"
    fwd = 1 + _gemm_launches(lib, B * T, d, d) + _gemm_launches(lib, B * L, 2 * d, d) + 1 + _gemm_launches(lib, B * T, d, d) + 1
    assert launches["forward"] == fwd, (launches, fwd)  # the count include/nar_fs2.h states
    assert c1.ok and c2.ok and c3.ok, (str(c1), str(c2), str(c3))
    assert rp <= 1.0 and rc <= 1.0, (rp, rc)


# ---------------------------------------------------------------------------------------------------- the whole module
def _grad_shares(cfg, case, tgt, src, g, a, parts, grads, keep=None, p=0.0):
    _, w = module(cfg)
    lens = case[3]
    r64 = xc.closed_form(tgt, src, w, lens, cfg[1], g, a, parts, keep, p, torch.float64)
    r32 = xc.closed_form(tgt, src, w, lens, cfg[1], g, a, parts, keep, p, torch.float32)
    return xc.shares(grads, r64, xc.gate(r32, r64))


@pytest.mark.parametrize("case", CASES, ids=_cid)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_fid)
def test_module_forward_and_backward(so, cfg, case):
    L_, lib = so
    m, w = module(cfg)
    d, H = cfg
    B, T, L, lens = case
    MT, ML = B * T, B * L
    tgt, src, g, a = _inputs(cfg, case)
    bwd = 16 + (_splits(so, cfg, case) > 1) + 2 * _gemm_launches(lib, MT, d, d) + _gemm_launches(lib, ML, d, 2 * d)
    # ---- eval
    y, attn, saved, grads, launches = _run(m, tgt, src, lens, g, a)
    parts = _saved_parts(saved, attn, B, T, L, d, H)
    sh = _grad_shares(cfg, case, tgt, src, g, a, parts, grads)
    print(f"{_fid(cfg)} {_cid(case)} eval: {sh}")
    report(test="xg_module", cfg=_fid(cfg), case=_cid(case), mode="eval", launches=launches, shares=sh)
    assert launches["backward"] == bwd, (launches, bwd)  # the count include/nar_fs2.h states
    worst = dict(sh)
    # ---- train() at p = 0.5 with a given keep-mask
    keep = np.random.RandomState(B * T + 3).rand(B, T, d) >= m.p_drop
    y, attn, saved, grads, launches = _run(m, tgt, src, lens, g, a, keep.astype(np.uint8))
    parts = _saved_parts(saved, attn, B, T, L, d, H)
    q, kv, ctx, z, _ = parts
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    kf = torch.from_numpy(keep).double() / (1.0 - m.p_drop)
    u64 = E.gemm_emu(ctx, wt["wfc"], wt["bfc"], round_fn=E.exact)
    unit = E.gemm_unit(ctx, wt["wfc"], wt["bfc"], round_fn=E.exact)
    z64 = u64 * kf + torch.from_numpy(tgt).double()
    assert bool(((z.double() - z64).abs() <= REL * unit * kf + REL * z64.abs()).all())
    y64 = E.layernorm_emu(z, wt["ln_g"], wt["ln_b"])
    assert bool(((y.double() - y64).abs() <= REL * (y64.abs() + wt["ln_b"].double().abs())).all())
    sh = _grad_shares(cfg, case, tgt, src, g, a, parts, grads, keep, m.p_drop)
    print(f"{_fid(cfg)} {_cid(case)} train p=0.5: {sh}")
    report(test="xg_module", cfg=_fid(cfg), case=_cid(case), mode="train_p0.5", launches=launches, shares=sh)
    assert launches["backward"] == bwd, (launches, bwd)
    for n, v in sh.items():
        worst[n] = max(worst[n], v)
    assert max(worst.values()) <= 1.0, worst


def test_needs_input_grad_run_to_run_bits_replicas_and_no_host_read(so):
    from smart_nar_fast_tts_amd import sublayers

    L_, lib = so
    cfg = CONFIGS[0]
    m, w = module(cfg)
    m.eval()
    d, H = cfg
    B, T, L, lens = 3, 130, 37, [32, 37, 32]  # utterances 0 and 2 are replicas
    tgt, src, g, a = _inputs(cfg, (B, T, L, lens))
    tgt[2], src[2], g[2], a[2] = tgt[0], src[0], g[0], a[0]
    params = m.ordered_parameters()
    l_d = lens_d(lens)

    def once(tgt_grad=True, src_grad=True, frozen=(), with_mask=False, use_map=True, zero_map=False):
        for i, p in enumerate(params):
            p.requires_grad_(i not in frozen)
            p.grad = None
        td, sd = dev(tgt).requires_grad_(tgt_grad), dev(src).requires_grad_(src_grad)
        if with_mask:
            mask = (torch.arange(L, device="cuda")[None, None, :] >= l_d[:, None, None]).expand(B, T, L)
            y, attn = m(td, sd, sd, mask=mask)
        else:
            y, attn = m(td, sd, sd, lens=l_d)
        assert tuple(attn.shape) == (B, H, T, L) and attn.requires_grad
        if use_map:
            torch.autograd.backward([y, attn], [dev(g), torch.zeros_like(attn) if zero_map else dev(a)])
        else:
            y.backward(dev(g))
        bits = [None if p.grad is None else p.grad.cpu().numpy().tobytes() for p in params]
        ins = [None if t.grad is None else t.grad.cpu().numpy() for t in (td, sd)]
        return (y.detach().cpu().numpy().tobytes(), attn.detach().cpu().numpy().tobytes()), bits, ins, dict(m.last_launches)

    try:
        x, b = once(), once()
        assert x[0] == b[0] and x[1] == b[1] and all(p.tobytes() == q.tobytes() for p, q in zip(x[2], b[2])), "two runs give identical bits"
        assert all(v is not None for v in x[1])
        assert x[2][0][0].tobytes() == x[2][0][2].tobytes() and x[2][1][0].tobytes() == x[2][1][2].tobytes(), \
            "two replicas of an utterance get bit-identical dtgt and dsrc rows"
        via_mask = once(with_mask=True)
        assert via_mask[0] == x[0] and via_mask[1] == x[1], "the mask and the lengths it stands for give the same bits"
        ns = once(src_grad=False)
        assert ns[2][1] is None and ns[1] == x[1] and ns[0] == x[0] and ns[2][0].tobytes() == x[2][0].tobytes()
        assert ns[3]["backward"] == x[3]["backward"] - _gemm_launches(lib, B * L, d, 2 * d), (ns[3], x[3])  # no dsrc GEMM
        fz = once(frozen=(0,))
        assert fz[1][0] is None and fz[1][1:] == x[1][1:] and all(p.tobytes() == q.tobytes() for p, q in zip(fz[2], x[2]))
        assert fz[3]["backward"] == x[3]["backward"] - 2, (fz[3], x[3])  # no wgrad, no reduce
        tail = once(tgt_grad=False, src_grad=False, frozen=(0, 1, 2, 3, 4, 5))  # only fc and layer_norm: nothing behind ctx
        assert tail[1][6:] == x[1][6:] and tail[3]["backward"] == 4, tail[3]  # row backward, dWfc's GEMM + reduce, the final column sums
        unused, zeros = once(use_map=False), once(zero_map=True)
        assert unused[1] == zeros[1] and all(p.tobytes() == q.tobytes() for p, q in zip(unused[2], zeros[2])), \
            "an unused map (dA = NULL) gives the bits of a dense all-zero dA"
        assert unused[1] != x[1]
        with torch.no_grad():
            td, sd = dev(tgt), dev(src)
            quiet, qmap = m(td, sd, sd, lens=l_d)
        assert (quiet.cpu().numpy().tobytes(), qmap.cpu().numpy().tobytes()) == x[0] and not quiet.requires_grad and not qmap.requires_grad
        assert m.last_launches["forward"] == x[3]["forward"]  # nothing kept, nothing extra launched either way
        # no host read with lens
        for p in params:
            p.grad = None
        td, sd = dev(tgt).requires_grad_(True), dev(src).requires_grad_(True)
        gd, ad = dev(g), dev(a)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            y, attn = m(td, sd, sd, lens=l_d)
            torch.autograd.backward([y, attn], [gd, ad])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert td.grad.cpu().numpy().tobytes() == x[2][0].tobytes()
        # refusals
        with pytest.raises(ValueError, match="k and v must be the same tensor"):
            m(td, sd, sd.clone())
        bad = torch.zeros(B, T, L, dtype=torch.bool, device="cuda")
        bad[0, 1, 2] = True
        with pytest.raises(ValueError, match="not a key-padding mask"):
            m(td, sd, sd, mask=bad)
        sa = sublayers.MultiHeadAttention(H, d, d // H, d // H).cuda()
        with pytest.raises(NotImplementedError, match="self-attention only"):
            sa(td, sd, sd)
        report(test="xg_launches", forward=x[3]["forward"], backward=x[3]["backward"], backward_no_dsrc=ns[3]["backward"],
                backward_frozen_wq=fz[3]["backward"], backward_tail_only=tail[3]["backward"])
    finally:
        for p in params:
            p.requires_grad_(True)
            p.grad = None


def test_one_chain_from_a_loss_shaped_map_gradient_into_the_optimiser():
    """A dA shaped exactly like ns_lossg_backward's d_attn (head 0 inside t < olen, l < ilen, +0.0 elsewhere) and an MSE-shaped g ->
    this module's backward -> optim.ScheduledOptim.step_and_update_lr(): the ten updated tensors against the float64 chain at
    optim_cpu.gate_of of torch's fp32 CPU chain.  (d_bk is zero in exact arithmetic, as in tests/test_gpu_attention_grad.py.)"""
    from smart_nar_fast_tts_amd import optim, sublayers

    cfg, case = CONFIGS[0], CASES[1]
    d, H = cfg
    B, T, L, lens = case
    olens = [33, 20, 7]
    srcm, w = module(cfg)
    m = sublayers.MultiHeadCrossAttention(H, d, d // H, d // H, dropout=0.5)
    m.load_state_dict(srcm.state_dict())
    m = m.cuda().eval()
    tgt, src, target, _ = _inputs(cfg, case, seed=7)
    a = xc.loss_shaped_dA(B, H, T, L, lens, olens, seed=5)
    assert a[:, 0].any() and not a[:, 1:].any() and not a[1, 0, olens[1]:].any() and not a[1, 0, :, lens[1]:].any()
    y_cpu = xc.statement(tgt, src, w, lens, H, dtype=torch.float32)["y"].numpy()
    g = (np.float32(2.0 / (B * T)) * (y_cpu - target)).astype(np.float32)
    start = 3998
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    so_ = optim.ScheduledOptim(m, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, start)
    td, sd = dev(tgt), dev(src)
    y, attn = m(td, sd, sd, lens=lens_d(lens))
    torch.autograd.backward([y, attn], [dev(g), dev(a)])
    so_.step_and_update_lr()
    lr = so_._optimizer.param_groups[0]["lr"]
    assert abs(lr - oc.lr_at(start + 1, **oc.SHIPPED)) <= 1e-12 * lr
    got = [p.detach().cpu().numpy().reshape(-1) for p in m.ordered_parameters()]
    chain = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        grads, _ = xc.autograd_ref(tgt, src, w, lens, H, g, a, dtype=dtype)
        c = dict(params=[np.asarray(w[k], dtype=np.float32).reshape(-1) for k in xc.NAMES[:10]], grads=[[grads[k].reshape(-1) for k in xc.NAMES[:10]]],
                 lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=None)
        chain[name] = oc.run(c)[0]["p"] if name == "f64" else oc.torch_run(c)[0]["p"]
    sh = {}
    for k, x, t32, w64 in zip(xc.NAMES[:10], got, chain["f32"], chain["f64"]):
        err = np.abs(x.astype(np.float64) - w64).max()
        sh[k] = float(err / oc.gate_of(t32, w64)) if np.isfinite(err) else float("inf")
    print(sh)
    report(test="xg_chain", shares=sh)
    assert max(sh.values()) <= 1.0, sh
