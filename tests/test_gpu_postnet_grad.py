"""The PostNet training forward and backward with train-mode BatchNorm on the GPU (csrc/postnetgrad.hip through ns_pn_* and
postnet.PostNet).

Each new kernel alone through its ns_pn_op_* entry against float64 of its own fp32 inputs — a stored value is a float64 expression
rounded once, so the bound is one fp32 ulp of the value (plus 1e-13 of a sum's absolute terms) — then the whole module: y, every
gradient and the buffers after a forward against the float64 yardstick tests/postnet_grad_cpu.autograd_ref (the reference's own torch
ops on the CPU) under the project gate, 2 x max |ref fp32 - ref float64| + one fp32 ulp of max |ref float64| per tensor.  The yardstick
itself is proven in tests/test_postnet_grad_host.py.  torch's own Conv1d / BatchNorm1d autograd on the GPU appears once, as a loose sanity
check only: it is not the yardstick.

NS_FP32_OPS_REPORT=<path> appends every measured share as a JSON line (profiles/postnet_grad.md was written from one).

Measured on the MI355X (profiles/postnet_grad.md): every kernel alone at 0.50 of its one-ulp bound, the padded weight gradient 0.049 of
the contraction contract; the module's y 0.61, d_weight 0.64, d_gamma 0.63, d_beta 0.61, dx 0.61, the buffers 0.23 of their gates, the
train-mode d_bias 2.2e-8 and the eval-mode d_bias 0.37; eval() against the folded inference PostNet 1.2e-7; the native step 0.36."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bf16_emu as E
from tests import optim_cpu as oc
from tests import postnet_grad_cpu as pc
from tests.predictor_grad_cpu import wgrad
from tests.util import dev, native_lib, report

pytestmark = pytest.mark.gpu
REL = E.FP32_REL
# (B, T): a row block's remainder; T about K, taps cross every utterance edge; only the centre tap and M / (M - 1) = 2; more than one
# row block and more than one weight-gradient range
CASES = [(2, 37), (3, 5), (2, 1), (5, 130)]
BASE = (80, 512, 5, 3)  # n_mel, emb, K, n
CONFIGS = [(c, BASE) for c in CASES] + [((5, 130), (80, 512, 5, 5)), ((5, 130), (16, 256, 5, 3))]
_id = lambda cc: f"{cc[0][0]}x{cc[0][1]}_mel{cc[1][0]}_emb{cc[1][1]}_n{cc[1][3]}"  # noqa: E731


@pytest.fixture(scope="module")
def so():
    return native_lib()


def _ws(nbytes=64 << 20, fill=0xFF):
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def _ulp(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def test_the_large_case_has_several_row_blocks_and_weight_gradient_ranges(so):
    L, lib = so
    out = (C.c_int32 * 8)()
    for N, Cin in ((512, 80), (512, 512), (128, 512), (256, 16), (256, 256), (128, 256)):
        assert lib.ns_pg_plan_wgrad(650, N, Cin, 5, out) == 0
        assert out[3] >= 2, (N, Cin, list(out))
    assert (650 + 31) // 32 > 1 and 74 % 32 != 0


# ---------------------------------------------------------------------------------------------------- each kernel alone
ALONE = [(74, 80), (15, 512), (2, 80), (650, 512), (650, 16), (650, 256)]


def _stats64(u):
    u = u.astype(np.float64)
    mu = u.mean(0)
    var = ((u - mu) ** 2).mean(0)
    return mu, var, 1.0 / np.sqrt(var + pc.BN_EPS)


@pytest.mark.parametrize("M,Cw", ALONE)
def test_stats_alone(so, M, Cw):
    L, lib = so
    rs = np.random.RandomState(M + Cw)
    u = (rs.standard_normal((M, Cw)) * 1.5 + rs.standard_normal(Cw)).astype(np.float32)
    rm0, rv0 = rs.standard_normal(Cw).astype(np.float32), (0.5 + rs.rand(Cw)).astype(np.float32)
    mu, var, rstd = _stats64(u)
    u_d = dev(u)

    def train():
        ws = _ws(8 << 20)
        rm, rv, nbt = dev(rm0), dev(rv0), torch.tensor(41, dtype=torch.int64, device="cuda")
        st = torch.full((2, Cw), float("nan"), dtype=torch.float64, device="cuda")
        L.check(lib.ns_pn_op_stats(L.ptr(u_d), M, Cw, 1, L.ptr(rm), L.ptr(rv), L.ptr(nbt), L.ptr(st), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pn_op_stats")
        assert lib.ns_pn_last_launches() == 2
        return st.cpu().numpy(), rm.cpu().numpy(), rv.cpu().numpy(), int(nbt)

    st, rm, rv, nbt = train()
    again = train()
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip((st, rm, rv), again[:3])), "two runs give identical bits"
    assert nbt == 42
    e_mu = np.abs(st[0] - mu).max() / np.abs(u).max()
    e_rs = (np.abs(st[1] - rstd) / rstd).max()
    want_rm = 0.9 * rm0.astype(np.float64) + 0.1 * mu
    want_rv = 0.9 * rv0.astype(np.float64) + 0.1 * var * M / (M - 1)
    s_rm = (np.abs(rm - want_rm) / _ulp(want_rm)).max()
    s_rv = (np.abs(rv - want_rv) / _ulp(want_rv)).max()
    report(test="pn_stats", M=M, C=Cw, mu=e_mu, rstd=e_rs, running_mean_ulp=s_rm, running_var_ulp=s_rv)
    # (rstd: the one-pass variance E[u^2] - mu^2 in float64 is off by about 1e-15 E[u^2] absolute, which 1 / (2 (var + 1e-5)) magnifies
    #  to at most 5e-11 E[u^2] relative where a column's variance is far below eps — possible at M = 2; E[u^2] is below 20 here)
    assert e_mu <= 1e-13 and e_rs <= 1e-9 and s_rm <= 1.0 and s_rv <= 1.0
    # eval: mu and rstd from the buffers, which stay as they are; no statistics of u (null here) are taken
    rm_d, rv_d = dev(rm0), dev(rv0)
    st = torch.full((2, Cw), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.ns_pn_op_stats(None, M, Cw, 0, L.ptr(rm_d), L.ptr(rv_d), None, L.ptr(st), None, 0, L.stream_ptr()), "ns_pn_op_stats")
    assert lib.ns_pn_last_launches() == 1
    st = st.cpu().numpy()
    assert np.array_equal(st[0], rm0.astype(np.float64)) and (np.abs(st[1] * np.sqrt(rv0.astype(np.float64) + pc.BN_EPS) - 1.0)).max() <= 1e-14
    assert np.array_equal(rm_d.cpu().numpy(), rm0) and np.array_equal(rv_d.cpu().numpy(), rv0)


def _layer_inputs(M, Cw, p, seed):
    rs = np.random.RandomState(seed)
    u = (rs.standard_normal((M, Cw)) * 1.5).astype(np.float32)
    gam, bet = (1 + 0.2 * rs.standard_normal(Cw)).astype(np.float32), (0.1 * rs.standard_normal(Cw)).astype(np.float32)
    keep = (rs.rand(M, Cw) >= p).astype(np.uint8) if p > 0 else None
    dh = rs.standard_normal((M, Cw)).astype(np.float32)
    mu, var, rstd = _stats64(u)
    return u, gam, bet, keep, dh, np.stack([mu, rstd])


def _apply64(u, st, gam, bet, keep, p, last):
    v = gam.astype(np.float64) * ((u.astype(np.float64) - st[0]) * st[1]) + bet.astype(np.float64)
    v = v if last else np.tanh(v)
    return v if keep is None else v * keep / (1.0 - p)


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M,Cw", ALONE)
def test_apply_alone(so, M, Cw, p, last):
    L, lib = so
    u, gam, bet, keep, _, st = _layer_inputs(M, Cw, p, M + Cw + last)
    want = _apply64(u, st, gam, bet, keep, p, last)
    h = torch.full((M + 1, Cw), float("nan"), device="cuda")  # one row more: the kernel stops at M
    t = [dev(a) for a in (u, st, gam, bet)]
    k_d = None if keep is None else dev(keep)
    L.check(lib.ns_pn_op_apply(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(k_d), p, last, M, Cw, L.ptr(h), L.stream_ptr()), "ns_pn_op_apply")
    assert lib.ns_pn_last_launches() == 1
    got = h.cpu().numpy()
    assert np.isnan(got[M]).all() and np.isfinite(got[:M]).all()
    share = (np.abs(got[:M] - want) / _ulp(want)).max()
    report(test="pn_apply", M=M, C=Cw, p=p, last=last, ulps=share)
    assert share <= 1.0
    if keep is not None:
        assert not got[:M][keep == 0].any()


def _dy64(dh, u, h, st, keep, p, last):
    xh = (u.astype(np.float64) - st[0]) * st[1]
    scale = 1.0 / (1.0 - p)
    dy = dh.astype(np.float64) * (1.0 if keep is None else keep * scale)
    if not last:
        t = h.astype(np.float64) / scale
        dy = dy * (1.0 - t * t)
    return dy, xh


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("M,Cw", ALONE)
def test_backward_kernels_alone(so, M, Cw, p, last):
    L, lib = so
    u, gam, bet, keep, dh, st = _layer_inputs(M, Cw, p, M + Cw + 7 * last)
    h = _apply64(u, st, gam, bet, keep, p, last).astype(np.float32)
    dy, xh = _dy64(dh, u, h, st, keep, p, last)
    t = {k: dev(v) for k, v in dict(dh=dh, u=u, h=h, st=st, gam=gam).items()}
    k_d = None if keep is None else dev(keep)
    h_ptr = None if last else L.ptr(t["h"])  # the last layer never reads h
    # ---- the reduction
    ws = _ws(8 << 20)
    d_g, d_b = torch.full((Cw,), float("nan"), device="cuda"), torch.full((Cw,), float("nan"), device="cuda")
    means = torch.full((2, Cw), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.ns_pn_op_bwd_reduce(L.ptr(t["dh"]), L.ptr(t["u"]), h_ptr, L.ptr(t["st"]), L.ptr(k_d), p, last, M, Cw, L.ptr(d_g), L.ptr(d_b), L.ptr(means),
                                    L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pn_op_bwd_reduce")
    assert lib.ns_pn_last_launches() == 2
    s0, s1, a0, a1 = dy.sum(0), (dy * xh).sum(0), np.abs(dy).sum(0), np.abs(dy * xh).sum(0)
    mn = means.cpu().numpy()
    assert (np.abs(mn[0] * M - s0) <= 1e-13 * a0 + 1e-300).all() and (np.abs(mn[1] * M - s1) <= 1e-13 * a1 + 1e-300).all()
    sh_b = (np.abs(d_b.cpu().numpy() - s0) / (_ulp(s0) + 1e-13 * a0)).max()
    sh_g = (np.abs(d_g.cpu().numpy() - s1) / (_ulp(s1) + 1e-13 * a1)).max()
    assert sh_b <= 1.0 and sh_g <= 1.0, (sh_b, sh_g)
    # ---- the apply: train (with the means), eval (without), dense and padded to 128 columns
    worst = {}
    for mode in ("train", "eval"):
        m1, m2 = (s0 / M, s1 / M) if mode == "train" else (0.0, 0.0)
        dz = gam.astype(np.float64) * st[1] * (dy - m1 - xh * m2)
        unit = np.abs(gam.astype(np.float64) * st[1]) * (np.abs(dy) + np.abs(m1) + np.abs(xh * m2))
        for ldz in ([Cw, 128] if Cw < 128 else [Cw]):
            out = torch.full((M + 1, ldz), float("nan"), device="cuda")
            db = torch.full((Cw + 16,), float("nan"), device="cuda")
            mean_d = dev(np.stack([s0 / M, s1 / M])) if mode == "train" else None
            ws = _ws(8 << 20)
            L.check(lib.ns_pn_op_bwd_apply(L.ptr(t["dh"]), L.ptr(t["u"]), h_ptr, L.ptr(t["st"]), L.ptr(mean_d), L.ptr(t["gam"]), L.ptr(k_d), p, last, M, Cw,
                                           ldz, L.ptr(out), L.ptr(db), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pn_op_bwd_apply")
            assert lib.ns_pn_last_launches() == 2
            got, gb = out.cpu().numpy(), db.cpu().numpy()
            assert np.isnan(got[M]).all() and np.isnan(gb[Cw:]).all(), "nothing past the M rows and the C bias columns is written"
            assert not got[:M, Cw:].any(), "the padding columns are zeros"
            sh = (np.abs(got[:M, :Cw] - dz) / (_ulp(dz) + 1e-14 * unit)).max()
            want_b, abs_b = dz.sum(0), unit.sum(0)
            # d_bias is the sum of the UNROUNDED dz: in train() it is zero in exact arithmetic and only float64 noise is left.  That
            # noise scales with the terms dz is the difference of (unit), not with dz: at M = 2 every dz is itself a near-total cancellation
            sb = (np.abs(gb[:Cw] - want_b) / (_ulp(want_b) + 1e-13 * abs_b)).max()
            worst[f"{mode}_{ldz}"] = (float(sh), float(sb))
            assert sh <= 1.0 and sb <= 1.0, (mode, ldz, sh, sb)
            if mode == "train" and M > 2:
                assert (np.abs(gb[:Cw]) <= 1e-12 * abs_b + 1e-30).all(), "train-mode d_bias is float64 rounding noise"
    report(test="pn_backward_kernels", M=M, C=Cw, p=p, last=last, d_beta=sh_b, d_gamma=sh_g, dz=worst)


@pytest.mark.parametrize("B,S,N,Cin", [(3, 5, 80, 512), (5, 130, 80, 512), (5, 130, 16, 256), (2, 1, 80, 512)])
def test_wgrad_narrow_alone(so, B, S, N, Cin):
    L, lib = so
    K, M = 5, B * S
    rs = np.random.RandomState(B * S + N)
    dz = np.zeros((B, S, 128), np.float32)
    dz[..., :N] = rs.standard_normal((B, S, N))
    x = rs.standard_normal((B, S, Cin)).astype(np.float32)
    dW = torch.full((N + 8, Cin, K), float("nan"), device="cuda")  # eight rows more: only the first N rows are the caller's
    ws = _ws()
    dz_d, x_d = dev(dz), dev(x)
    L.check(lib.ns_pn_op_wgrad_narrow(L.ptr(dz_d), L.ptr(x_d), B, S, N, Cin, K, L.ptr(dW), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pn_op_wgrad_narrow")
    assert lib.ns_pn_last_launches() == 3
    got = dW.cpu().double()
    assert bool(torch.isnan(got[N:]).all()) and bool(torch.isfinite(got[:N]).all()), "the padding rows of the 128-wide scratch never reach the caller"
    dz64, x64 = torch.from_numpy(dz[..., :N]).double(), torch.from_numpy(x).double()
    ref, unit = wgrad(dz64, x64, K, 2), wgrad(dz64.abs(), x64.abs(), K, 2)
    share = float(((got[:N] - ref).abs() / (REL * unit).clamp_min(1e-300)).max())
    report(test="pn_wgrad_narrow", case=f"{B}x{S}", N=N, Cin=Cin, share=share)
    assert share <= 1.0
    if B > 1 and S > 1:
        cross = wgrad(dz64, x64, K, 2, cross=True)
        assert not bool(((cross - ref).abs() <= REL * unit).all())


# ---------------------------------------------------------------------------------------------------- the whole module
_MODULES, _REFS = {}, {}


def module(cfg, seed=300):
    """(the module on the GPU, its seeded weights); the buffers are put back before every use (_reset)"""
    from smart_nar_fast_tts_amd import postnet

    if cfg not in _MODULES:
        n_mel, emb, K, n = cfg
        w = pc.seeded_weights(n_mel, emb, K, n, seed + n_mel + emb + n)
        m = postnet.PostNet(n_mel, emb, K, n)
        _MODULES[cfg] = (m.cuda(), w)
        _reset(cfg)
    return _MODULES[cfg]


def _state_dict(w, n):
    sd = {}
    for i in range(n):
        for q, key in (("w", "0.conv.weight"), ("b", "0.conv.bias"), ("g", "1.weight"), ("be", "1.bias"), ("rm", "1.running_mean"), ("rv", "1.running_var"),
                       ("nbt", "1.num_batches_tracked")):
            sd[f"convolutions.{i}.{key}"] = torch.as_tensor(np.asarray(w[f"{q}{i}"]))
    return sd


def _reset(cfg):
    m, w = _MODULES[cfg]
    m.load_state_dict(_state_dict(w, cfg[3]))  # strict
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None


def _inputs(case, cfg):
    B, T = case
    rs = np.random.RandomState(B * T + cfg[0])
    return rs.standard_normal((B, T, cfg[0])).astype(np.float32), rs.standard_normal((B, T, cfg[0])).astype(np.float32)


def _buffers(m, n):
    out = {}
    for i in range(n):
        bn = m.convolutions[i][1]
        out[f"rm{i}"], out[f"rv{i}"] = bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy()
        out[f"nbt{i}"] = int(bn.num_batches_tracked)
    return out


def _yardstick(case, cfg, mode, p):
    """autograd_ref in float64 and fp32 and the gates, once per (case, config, mode, p); shared, never modified"""
    key = (case, cfg, mode, p)
    if key not in _REFS:
        _, w = module(cfg)
        x, g = _inputs(case, cfg)
        B, T = case
        keeps = pc.keep_masks(B, T, cfg[0], cfg[1], cfg[3], p, B * T + 11) if p > 0 else None
        r64, _ = pc.autograd_ref(x, w, g, keeps, p, mode == "train", torch.float64)
        r32, _ = pc.autograd_ref(x, w, g, keeps, p, mode == "train", torch.float32)
        _REFS[key] = (x, g, keeps, r64, r32, pc.gate(r32, r64))
    return _REFS[key]


def _run(cfg, x, g, keeps, mode, need=None):
    """one forward + backward through the module's own marshalling: every tensor of pc.all_names by name, and the launches"""
    m, _ = module(cfg)
    _reset(cfg)
    m.train(mode == "train")
    n = cfg[3]
    call = m._marshal(dev(x), None if keeps is None else [dev(k) for k in keeps])
    y, saved = m._forward(call, save=True)
    need = [True] * (4 * n + 1) if need is None else need
    outs = m._backward(call, saved, dev(g), need)
    got = dict(zip(("dx",) + pc.grad_names(n)[:-1], (None if o is None else o.cpu().numpy() for o in outs)))
    got["y"] = y.cpu().numpy()
    got.update(_buffers(m, n))
    return got, dict(m.last_launches)


def _gemm_launches(so, M, N, Cin, K=5):
    from smart_nar_fast_tts_amd import ops

    return len(ops.plan_gemm_launches(M, N, Cin, K))


@pytest.mark.parametrize("mode,p", [("train", 0.0), ("train", 0.5), ("eval", 0.0)])
@pytest.mark.parametrize("cc", CONFIGS, ids=_id)
def test_module_forward_and_backward(so, cc, mode, p):
    case, cfg = cc
    n_mel, emb, K, n = cfg
    M = case[0] * case[1]
    x, g, keeps, r64, r32, gates = _yardstick(case, cfg, mode, p)
    m, w = module(cfg)
    m.dropout = p if p > 0 else 0.0
    try:
        got, launches = _run(cfg, x, g, keeps, mode)
    finally:
        m.dropout = 0.5
    sh = pc.shares(got, r64, gates)
    cl = pc.classes(sh)
    print(_id(cc), mode, p, "worst share per class", {k: f"{v:.3g}" for k, v in cl.items()}, launches)
    report(test="pn_module", case=_id(cc), mode=mode, p=p, launches=launches, classes=cl)
    chans = [n_mel] + [emb] * (n - 1) + [n_mel]
    fwd = (n + 1) // 2 + sum(_gemm_launches(so, M, chans[i + 1], chans[i]) + (3 if mode == "train" else 2) for i in range(n))
    bwd = (n + 1) // 2 + 1 + sum(3 + 2 + _gemm_launches(so, M, chans[i], chans[i + 1]) for i in range(n)) + 1
    assert launches == {"forward": fwd, "backward": bwd}
    for i in range(n):
        assert got[f"nbt{i}"] == int(w[f"nbt{i}"]) + (1 if mode == "train" else 0)
        if mode == "eval":
            assert np.array_equal(got[f"rm{i}"], w[f"rm{i}"]) and np.array_equal(got[f"rv{i}"], w[f"rv{i}"])
    assert max(sh.values()) <= 1.0, sh
    if keeps is not None:
        assert not got["y"][keeps[-1] == 0].any()


def test_buffers_after_one_and_two_forwards_also_under_no_grad(so):
    case, cfg = CASES[0], BASE
    x, g, _, r64, r32, gates = _yardstick(case, cfg, "train", 0.0)
    m, w = module(cfg)
    n = cfg[3]
    _reset(cfg)
    m.train()
    m.dropout = 0.0
    try:
        with torch.no_grad():
            y = m(dev(x))
        assert not y.requires_grad
        one = _buffers(m, n)
        sh1 = pc.shares(one, r64, gates, pc.buffer_names(n))
        assert max(sh1.values()) <= 1.0 and all(one[f"nbt{i}"] == int(w[f"nbt{i}"]) + 1 for i in range(n)), sh1
        assert pc.shares({"y": y.cpu().numpy()}, r64, gates, ["y"])["y"] <= 1.0
        # a second forward, this time with autograd on, starts from the updated buffers; the backward touches none of them
        xd = dev(x).requires_grad_(True)
        y2 = m(xd)
        two = _buffers(m, n)
        y2.backward(dev(g))
        assert all(np.array_equal(two[k], v) if isinstance(v, np.ndarray) else two[k] == v for k, v in _buffers(m, n).items())
        w2 = dict(w)
        for i in range(n):
            w2[f"rm{i}"], w2[f"rv{i}"] = r32[f"rm{i}"], r32[f"rv{i}"]  # the yardstick's second step from ITS first step, per dtype
        q32, _ = pc.autograd_ref(x, w2, g, None, 0.0, True, torch.float32)
        w2 = {k: (r64[k] if k[:2] in ("rm", "rv") else v) for k, v in w.items()}
        q64, _ = pc.autograd_ref(x, w2, g, None, 0.0, True, torch.float64)
        sh2 = pc.shares(two, q64, pc.gate(q32, q64), pc.buffer_names(n))
        report(test="pn_buffers", one=pc.classes(sh1), two=pc.classes(sh2))
        assert max(sh2.values()) <= 1.0 and all(two[f"nbt{i}"] == int(w[f"nbt{i}"]) + 2 for i in range(n)), sh2
        assert y2.detach().cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), "train-mode output does not depend on the running statistics"
    finally:
        m.dropout = 0.5


def test_needs_input_grad_launch_counts_and_run_to_run_bits(so):
    case, cfg = CASES[3], BASE
    n = cfg[3]
    x, g, *_ = _yardstick(case, cfg, "train", 0.0)
    m, w = module(cfg)
    params = m.ordered_parameters()
    M = case[0] * case[1]
    G = lambda N, Cin: _gemm_launches(so, M, N, Cin)  # noqa: E731

    def once(x_grad=True, wanted=None):
        _reset(cfg)
        m.train()
        for i, p in enumerate(params):
            p.requires_grad_(wanted is None or i in wanted)
        xd = dev(x).requires_grad_(x_grad)
        y = m(xd)
        y.backward(dev(g))
        bits = [None if p.grad is None else p.grad.cpu().numpy().tobytes() for p in params]
        return y.detach().cpu().numpy().tobytes(), bits, None if xd.grad is None else xd.grad.cpu().numpy().tobytes(), dict(m.last_launches)

    m.dropout = 0.0
    try:
        a, b = once(), once()
        assert a[:3] == b[:3], "two runs give identical bits"
        assert a[2] is not None and all(v is not None for v in a[1])
        full = a[3]["backward"]
        # only dx: every layer's reduction, finish, dz and data gradient; no weight gradient, no d_bias finish
        dx = once(wanted=())
        assert dx[2] == a[2] and all(v is None for v in dx[1])
        assert dx[3]["backward"] == 2 + n * 3 + G(512, 80) + G(512, 512) + G(80, 512), (dx[3], a[3])
        # only the last layer's parameters: the walk stops there — no pack, no data gradient
        last = once(x_grad=False, wanted=range(4 * (n - 1), 4 * n))
        assert last[2] is None and last[1][:4 * (n - 1)] == [None] * (4 * (n - 1)) and last[1][4 * (n - 1):] == a[1][4 * (n - 1):]
        assert last[3]["backward"] == 3 + 3 + 1, last[3]
        # nothing wanted for layer 0: its visit is dropped, and with it the data gradient into it
        no0 = once(x_grad=False, wanted=range(4, 4 * n))
        assert no0[1][:4] == [None] * 4 and no0[1][4:] == a[1][4:]
        # (layer 0's five launches and its data gradient, the data gradient out of layer 1, and the pack launches of n - 2 weights, not n)
        assert no0[3]["backward"] == full - (3 + 2 + G(80, 512)) - G(512, 512) - ((n + 1) // 2 - (n - 1) // 2), (no0[3], a[3])
        with torch.no_grad():
            _reset(cfg)
            m.train()
            quiet = m(dev(x))
        assert quiet.cpu().numpy().tobytes() == a[0] and not quiet.requires_grad
        report(test="pn_launches", forward=a[3]["forward"], backward=full, only_dx=dx[3]["backward"], only_last=last[3]["backward"], no_layer0=no0[3]["backward"])
    finally:
        m.dropout = 0.5
        _reset(cfg)


def test_unwanted_gradients_are_never_written(so):
    """ns_pn_backward with sentinel-filled outputs: what is not asked for is not written, what is asked for is written in full"""
    L, lib = so
    case, cfg = CASES[1], BASE
    n = cfg[3]
    x, g, *_ = _yardstick(case, cfg, "train", 0.0)
    m, _ = module(cfg)
    _reset(cfg)
    m.train()
    m.dropout = 0.0
    try:
        call = m._marshal(dev(x), None)
        y, saved = m._forward(call, save=True)
        names = ("dx",) + tuple(m.FIELDS)
        shapes = [call.x.shape] + [p.shape for p in call.params]
        for wanted in ({"dx"}, {"w2", "beta1"}, set(names)):
            bufs = {k: torch.full((int(np.prod(s)) + 16,), float("nan"), device="cuda") for k, s in zip(names, shapes)}
            d = m.GRADS()  # ns_pn_grads, which takes d.w2 for d.layer[2].w
            for k in wanted:
                setattr(d, k, bufs[k].data_ptr())
            ws = m.WORKSPACES.get(lib, call.shape, call.device)
            g_d = dev(g)
            L.check(lib.ns_pn_backward(C.byref(call.shape), C.byref(call.weights), 1, L.ptr(call.x), None, 0.0, L.ptr(saved), L.ptr(g_d), C.byref(d),
                                       L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pn_backward")
            for k, s in zip(names, shapes):
                v, numel = bufs[k].cpu().numpy(), int(np.prod(s))
                assert np.isnan(v[numel:]).all(), k
                assert np.isfinite(v[:numel]).all() if k in wanted else np.isnan(v).all(), (sorted(wanted), k)
    finally:
        m.dropout = 0.5


def test_eval_forward_equals_the_folded_inference_postnet_and_a_trained_state_dict_loads_into_it():
    """eval() against ns_op_postnet (BatchNorm folded into the convolution weights at load time) on the same weights at the existing
    per-operator tolerance of tests/test_gpu_parity.py; then one train-mode forward moves the running statistics, the module's
    state_dict() goes into the inference model and the two agree again"""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import ops, postnet
    from smart_nar_fast_tts_amd.model import FastSpeech2Align
    from tests.test_gpu_parity import OP_TOL

    cfg = wl.model_config("tiny")
    sd = wl.synth_state_dict(cfg, seed=0)
    model = FastSpeech2Align(wl.preprocess_config(), cfg).to("cuda").eval()
    model.load_state_dict(sd)
    pn = postnet.PostNet().cuda()
    pn.load_state_dict({k[len("postnet."):]: torch.as_tensor(np.asarray(v)) for k, v in sd.items() if k.startswith("postnet.")})  # strict
    B, T = 2, 37
    x = dev((np.random.RandomState(5).standard_normal((B, T, 80)) * 0.5).astype(np.float32))
    pn.eval()
    with torch.no_grad():
        e1 = float((pn(x) - ops.postnet(model, x)).abs().max())
    pn.train()
    with torch.no_grad():
        pn(x)
    pn.eval()
    sd2 = dict(sd)
    sd2.update({"postnet." + k: v.cpu().numpy() for k, v in pn.state_dict().items()})
    assert float(np.abs(sd2["postnet.convolutions.0.1.running_mean"] - sd["postnet.convolutions.0.1.running_mean"]).max()) > 1e-3
    model.load_state_dict(sd2)
    with torch.no_grad():
        e2 = float((pn(x) - ops.postnet(model, x)).abs().max())
    report(test="pn_eval_vs_folded", before=e1, after_training_forward=e2)
    assert e1 <= OP_TOL and e2 <= OP_TOL, (e1, e2)


def test_torch_autograd_on_the_gpu_agrees_loosely(so):
    """every gradient of the n_mel = 16, emb = 256 case against torch's own Conv1d / BatchNorm1d autograd on the same GPU: a sanity
    check at 1e-3 of each tensor's largest magnitude (torch's fp32 kernels are not the yardstick; d_bias, zero in exact arithmetic, is
    held to 1e-3 of d_beta's scale)"""
    case, cfg = CONFIGS[-1]
    n_mel, emb, K, n = cfg
    x, g, _, r64, *_ = _yardstick(case, cfg, "train", 0.0)
    m, w = module(cfg)
    m.dropout = 0.0
    try:
        got, _ = _run(cfg, x, g, None, "train")
    finally:
        m.dropout = 0.5
    chans = [n_mel] + [emb] * (n - 1) + [n_mel]
    layers = []
    for i in range(n):
        conv, bn = torch.nn.Conv1d(chans[i], chans[i + 1], K, padding=2), torch.nn.BatchNorm1d(chans[i + 1])
        conv.weight.data, conv.bias.data = torch.as_tensor(w[f"w{i}"]), torch.as_tensor(w[f"b{i}"])
        bn.weight.data, bn.bias.data = torch.as_tensor(w[f"g{i}"]), torch.as_tensor(w[f"be{i}"])
        layers += [conv, bn] + ([torch.nn.Tanh()] if i < n - 1 else [])
    net = torch.nn.Sequential(*layers).cuda().train()
    xd = dev(x).requires_grad_(True)
    net(xd.transpose(1, 2)).transpose(1, 2).backward(dev(g))
    mods = [l for l in layers if not isinstance(l, torch.nn.Tanh)]
    theirs = {"dx": xd.grad}
    for i in range(n):
        theirs[f"w{i}"], theirs[f"b{i}"] = mods[2 * i].weight.grad, mods[2 * i].bias.grad
        theirs[f"g{i}"], theirs[f"be{i}"] = mods[2 * i + 1].weight.grad, mods[2 * i + 1].bias.grad
    for k, t in theirs.items():
        scale = np.abs(r64[f"be{k[1:]}" if k[0] == "b" and k[1:].isdigit() else k]).max()
        assert np.abs(got[k] - t.cpu().numpy()).max() <= 1e-3 * scale, k


def test_one_native_training_step_through_the_residual_and_an_l1_loss(so):
    """mel.requires_grad_(), post = PostNet(mel) + mel, an L1 loss over the valid frames, backward(), one ScheduledOptim step: the
    updated PostNet parameters against the float64 chain at optim_cpu.gate_of of torch's fp32 CPU chain plus the gradient's own gate carried
    through the float64 step (see below; with gate_of alone the last layer's weight measured 3.1 at ONE element whose gradient is within
    1e-9 of zero, every other tensor at most 0.27), mel.grad at the project gate.
    The targets sit at least 0.1 away from the float64 output, so no sign of the L1 gradient hangs on fp32 noise."""
    from smart_nar_fast_tts_amd import optim, postnet

    case, cfg = CASES[0], BASE
    n_mel, emb, K, n = cfg
    B, T = case
    lens = np.array([T, T - 9])
    valid = (np.arange(T)[None, :] < lens[:, None])
    x, _, _, r64, *_ = _yardstick(case, cfg, "train", 0.0)
    _, w = module(cfg)
    rs = np.random.RandomState(91)
    target = (r64["y"] + x + np.where(rs.rand(B, T, n_mel) < 0.5, -1.0, 1.0) * (0.1 + rs.rand(B, T, n_mel))).astype(np.float32)
    count = float(valid.sum() * n_mel)
    m = postnet.PostNet(n_mel, emb, K, n, dropout=0.0)
    m.load_state_dict(_state_dict(w, n))
    m = m.cuda().train()
    start = 3998
    ocfg = {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, **oc.SHIPPED)}
    sched = optim.ScheduledOptim(m, ocfg, {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}, start)
    mel = dev(x).requires_grad_(True)
    post = m(mel) + mel
    loss = ((post - dev(target)).abs() * dev(valid)[..., None]).sum() / count
    loss.backward()
    sched.step_and_update_lr()
    lr = sched._optimizer.param_groups[0]["lr"]
    got = [p.detach().cpu().numpy().reshape(-1) for p in m.ordered_parameters()]
    names = pc.grad_names(n)[:-1]
    chain, dmel, gr = {}, {}, {}

    def case_of(grads):
        return dict(params=[np.asarray(w[k], dtype=np.float32).reshape(-1) for k in names], grads=[[np.asarray(grads[k]).reshape(-1) for k in names]],
                    lrs=[lr], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, max_norm=None)

    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        y, _ = pc.forward_form(x, w, None, 0.0, True, dtype)
        g = np.sign((y["y"].astype(np.float64) + x - target)) * valid[..., None] / count
        gr[name], _ = pc.autograd_ref(x, w, g, None, 0.0, True, dtype)
        dmel[name] = gr[name]["dx"].astype(np.float64) + g
        chain[name] = oc.run(case_of(gr[name]))[0]["p"] if name == "f64" else oc.torch_run(case_of(gr[name]))[0]["p"]
    assert np.array_equal(np.sign(post.detach().cpu().numpy() - target), np.sign(r64["y"] + x - target))
    # Adam's first step moves an element by lr g / (|g| + 1e-9): where |g| is within a few 1e-9 of zero — one or two elements of a
    # tensor — the step has the gain lr / eps on g, and the largest |torch fp32 - float64| of a tensor is the gradient's fp32 noise AT
    # THAT ELEMENT, which no second fp32 evaluation reproduces within a factor of two.  So the gradient's own per-tensor gate is carried
    # through the float64 step as well: the step from g64 + gate and from g64 - gate, element by element (the step is monotonic in g).
    g_gate = pc.gate(gr["f32"], gr["f64"], names)
    hi = oc.run(case_of({k: gr["f64"][k] + g_gate[k] for k in names}))[0]["p"]
    lo = oc.run(case_of({k: gr["f64"][k] - g_gate[k] for k in names}))[0]["p"]
    sh = {}
    for k, a, t32, w64, h_, l_ in zip(names, got, chain["f32"], chain["f64"], hi, lo):
        bound = oc.gate_of(t32, w64) + np.maximum(np.abs(h_ - w64), np.abs(l_ - w64))
        err = np.abs(a.astype(np.float64) - w64)
        sh[k] = float((err / bound).max()) if np.isfinite(err).all() else float("inf")
    sh["mel.grad"] = pc.shares({"dx": mel.grad.cpu().numpy()}, {"dx": dmel["f64"]}, pc.gate({"dx": dmel["f32"]}, {"dx": dmel["f64"]}))["dx"]
    report(test="pn_native_step", shares=pc.classes(sh))
    assert max(sh.values()) <= 1.0, sh
