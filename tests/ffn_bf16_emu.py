"""The yardstick of the opt-in "bf16" feed-forward training mode (csrc/ffngrad_bf16.hip, ns_fg_*_bf16): float64
with rounded operands.  Shared by tests/test_ffn_bf16_host.py (the gate proven on the CPU: the fp32 evaluation passes, wrong variants
fail) and tests/test_gpu_ffn_bf16.py (the kernels against it).  The reference has no bf16 mode, so there is no fixture.

Contract of the weight gradient: dW[n][c][j] = sum_m bf(dz[m, n]) bf(X[m + j - pad, c]), both operands rounded to bf16 (nearest, ties to
even), products summed in fp32, a tap outside the utterance's [0, S) rows reads zero.  An evaluation differs from the float64 one only
by its summation, so the bound is elementwise: |dW - f64| <= GEMM_REL * sum_m |bf dz| |bf X|, and an element whose every tap lies
outside its utterance (unit == 0) is exactly +0.0.  GEMM_REL is the project's bound for this MFMA, stated for sequential sums of up to
2816 products: MAX_RANGE_ROWS is what the tests hold every case's rows per range to, through the plan hook.

The forward and the data gradient are tests/bf16_emu.py's contraction (gemm_check) on the torch-layout weight; ``transposed_weight``
states the data gradient's weight in that form."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from tests.bf16_emu import FP32_REL, GEMM_REL, bf, bf_trunc, conv_rows, gemm_check  # noqa: F401  (re-exported for the two test files)

MAX_RANGE_ROWS = 2816
CONFIGS = [(256, 1024, 9, 1), (512, 2048, 9, 1), (256, 512, 3, 3)]  # (d, d_inner, K1, K2) of tests/test_gpu_ffn_grad.py
CASES = [(2, 1), (3, 5), (2, 33), (1, 65), (3, 130)]                 # (B, S)


def exact(t):
    return t


def weight_shapes(cfg):
    """(N, Cin, KW) of w_1 and of w_2"""
    d, di, K1, K2 = cfg
    return [(di, d, K1), (d, di, K2)]


def operands(B, S, N, Cin, seed, same_sign=False):
    """ragged data: random magnitudes over three decades, random or one sign"""
    rs = np.random.RandomState(seed)
    dz = (rs.standard_normal((B, S, N)) * 10.0 ** rs.uniform(-2, 1, (B, S, 1))).astype(np.float32)
    x = (rs.standard_normal((B, S, Cin)) * 10.0 ** rs.uniform(-2, 1, (B, S, 1))).astype(np.float32)
    if same_sign:
        dz, x = np.abs(dz), np.abs(x)
    return torch.from_numpy(dz), torch.from_numpy(x)


# ---------------------------------------------------------------------------------------------------- weight gradient
def wgrad_emu(dz, x, KW, round_fn=bf, dtype=torch.float64, drop_tap=None, cross_utterance=False, drop_rows=None):
    """dW [N, Cin, KW] from dz [B, S, N] and x [B, S, Cin], operands rounded by round_fn, evaluated in dtype.
    The WRONG variants, for the proof of the gate: drop_tap = j leaves tap j out; cross_utterance lets a tap past an utterance's edge
    read the neighbouring utterance's row; drop_rows = (m0, m1) leaves the flat rows [m0, m1) out of the contraction."""
    B0, S0, N = dz.shape
    Cin = x.shape[2]
    pad = (KW - 1) // 2
    dz, x = round_fn(dz).to(dtype), round_fn(x).to(dtype)
    B, S = (1, B0 * S0) if cross_utterance else (B0, S0)
    dzf = dz.reshape(B0 * S0, N).clone()
    if drop_rows is not None:
        dzf[drop_rows[0]:drop_rows[1]] = 0
    xp = torch.zeros(B, S + 2 * pad, Cin, dtype=dtype)
    xp[:, pad:pad + S] = x.reshape(B, S, Cin)
    dW = torch.zeros(N, Cin, KW, dtype=dtype)
    for j in range(KW):
        if j != drop_tap:
            dW[:, :, j] = dzf.T @ xp[:, j:j + S].reshape(B * S, Cin)
    return dW


def wgrad_unit(dz, x, KW, round_fn=bf):
    """sum_m |bf dz| |bf x| in float64: what one rounding of the running sum is relative to"""
    return wgrad_emu(round_fn(dz).abs(), round_fn(x).abs(), KW, round_fn=exact)


@dataclass
class WgradCheck:
    ok: bool
    worst: float     # worst |dW - f64| / (GEMM_REL * unit) over the elements with unit > 0: <= 1 passes
    zeros_ok: bool   # every element with unit == 0 is exactly +0.0

    def __str__(self):
        return f"worst |dW - f64| / (GEMM_REL * sum |bf dz| |bf x|) = {self.worst:.3g}, dead elements exactly +0.0: {self.zeros_ok}"


def wgrad_check(got, dz, x, KW, rel=GEMM_REL, ref=None, unit=None):
    """every element of `got` [N, Cin, KW] against the float64 emulation; where no tap is inside the utterance the element is +0.0"""
    ref = wgrad_emu(dz, x, KW) if ref is None else ref
    unit = wgrad_unit(dz, x, KW) if unit is None else unit
    got32 = torch.as_tensor(got).reshape(ref.shape).float().contiguous()
    g = got32.double()
    err = (g - ref).abs()
    live = unit > 0
    inside = bool((err <= rel * unit).all()) and bool(torch.isfinite(g).all())
    zeros_ok = not bool(got32.view(torch.int32)[~live].any())  # all 32 bits clear: +0.0, not -0.0
    worst = float((err[live] / (rel * unit[live])).max()) if bool(live.any()) else 0.0
    return WgradCheck(inside and zeros_ok, worst, zeros_ok)


def plan(lib, M, N, Cin, KW):
    """ns_fg_plan_wgrad_bf16 as a dict; the rows of every range are at most MAX_RANGE_ROWS (the bound's own statement)"""
    out = (C.c_int32 * 8)()
    assert lib.ns_fg_plan_wgrad_bf16(M, N, Cin, KW, out) == 0, lib.ns_last_error()
    p = dict(zip(("tile_n", "tile_c", "rows", "ranges", "tiles", "ws_floats", "chunk"), out))
    assert p["rows"] <= MAX_RANGE_ROWS, p
    return p


def last_partial_stage(M, stage=32):
    """the flat rows [m0, M) of the last range's last, partial stage (a range's rows are a multiple of the stage, so the stages start
    at multiples of it whatever the split); None when every stage is full"""
    full = M // stage * stage
    return None if full == M else (full, M)


# ---------------------------------------------------------------------------------------------------- data gradient
def transposed_weight(w):
    """the data gradient as a forward contraction: dX = conv_rows(dz, wt) with wt [Cin, N, KW], wt[c][n][j] = w[n][c][KW - 1 - j]"""
    return w.permute(1, 0, 2).flip(2).contiguous()


def dgrad_emu(dz, w, resid=None, dtype=torch.float64, round_fn=bf, no_flip=False, resid_before_rounding=False):
    """dX [B, S, Cin] = conv(bf dz, bf w transposed, tap-flipped) + resid, resid added in fp32 behind the sum.
    WRONG variants: no_flip leaves the taps as they are; resid_before_rounding adds resid ahead of a bf16 rounding of the sum, not in the
    fp32 epilogue (the residual branch then carries a bf16 rounding it must not)."""
    wt = w.permute(1, 0, 2).contiguous() if no_flip else transposed_weight(w)
    y = conv_rows(round_fn(dz), round_fn(wt), None, dtype)
    if resid is not None:
        y = y + resid.to(dtype)
        if resid_before_rounding:
            y = bf(y)
    return y


def dgrad_check(got, dz, w, resid=None, rel=GEMM_REL):
    """every element of `got` [B, S, Cin] against float64 at rel * (conv(|bf dz|, |bf wt|) + |resid|): resid is an fp32 addend of the
    epilogue, as a bias is in gemm_check"""
    wt = transposed_weight(w)
    unit = conv_rows(bf(dz).abs(), bf(wt).abs(), None)
    if resid is not None:
        unit = unit + resid.double().abs()
    return gemm_check(got, dz, wt, None, rel=rel, ref=dgrad_emu(dz, w, resid), unit=unit)


# ---------------------------------------------------------------------------------------------------- the module from its hooks
def hand_chain(L, lib, cfg, case, x, saved, g, keep, p, w):
    """Every gradient of the "bf16" module from the single-launch hooks, on the device's own tensors: ns_ag_op_row_backward -> wgrad
    hook (dW2) -> transposed conv hook (da) -> ns_fg_op_relu_gate (dh, d_b1) -> wgrad hook (dW1) -> transposed conv hook with resid = dz
    (dx).  x [B, S, d], saved (h | z), g, keep (uint8 or None) and the weights w (dict of device tensors w1, w2, ln_g) live on the GPU.
    Returns a dict of device tensors named as ns_fg_grads."""
    d, di, K1, K2 = cfg
    B, S = case
    M = B * S
    dev = x.device
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    h, z = saved[:M * di], saved[M * di:]
    dz, du, out = new(M, d), new(M, d), {}
    out["ln_g"], out["ln_b"], out["b2"] = new(d), new(d), new(d)
    ws = torch.empty(((M + 63) // 64) * 5 * max(d, di) * 8, dtype=torch.uint8, device=dev)
    L.check(lib.ns_ag_op_row_backward(L.ptr(g), L.ptr(z), L.ptr(w["ln_g"]), L.ptr(keep), p, M, d, L.ptr(dz), L.ptr(du), L.ptr(out["ln_g"]),
                                      L.ptr(out["ln_b"]), L.ptr(out["b2"]), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_ag_op_row_backward")

    def op_ws(N, Cin, KW):
        n = lib.ns_fg_op_bf16_ws_bytes(B, S, N, Cin, KW)
        assert n > 0, lib.ns_last_error()
        return torch.empty(n, dtype=torch.uint8, device=dev)

    def wgrad(dzz, X, N, Cin, KW):
        dW, o = new(N, Cin, KW), op_ws(N, Cin, KW)
        L.check(lib.ns_fg_op_wgrad_bf16(L.ptr(dzz), L.ptr(X), B, S, N, Cin, KW, L.ptr(dW), L.ptr(o), o.numel(), L.stream_ptr()), "ns_fg_op_wgrad_bf16")
        return dW

    def dgrad(dzz, W, resid, N, Cin, KW):
        y, o = new(M, Cin), op_ws(N, Cin, KW)
        L.check(lib.ns_fg_op_conv_bf16(L.ptr(dzz), L.ptr(W), None, L.ptr(resid), B, S, N, Cin, KW, 1, 0, L.ptr(y), L.ptr(o), o.numel(),
                                       L.stream_ptr()), "ns_fg_op_conv_bf16")
        return y

    out["w2"] = wgrad(du, h, d, di, K2)
    da = dgrad(du, w["w2"], None, d, di, K2)
    dh, out["b1"] = new(M, di), new(di)
    L.check(lib.ns_fg_op_relu_gate(L.ptr(da), L.ptr(h), M, di, L.ptr(dh), L.ptr(out["b1"]), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_fg_op_relu_gate")
    out["w1"] = wgrad(dh, x.reshape(M, d), di, d, K1)
    out["dx"] = dgrad(dh, w["w1"], dz, di, d, K1).reshape(B, S, d)
    return out
