"""CPU emulation of the opt-in "bf16" mel path's two kernels taken ONE AT A TIME, and the gates that hold the kernels to it.
Shared by tests/test_bf16_ops_host.py (the gates proven on the CPU: the fp32 evaluation passes, wrong variants fail) and
tests/test_gpu_bf16_ops.py (the kernels against the float64 evaluation).

Contract of one contraction (csrc/gemm_bf16.hip): both operands rounded to bf16 (round to nearest, ties to even), products
summed in fp32, zero padding per utterance of S rows; bias and activation in fp32.  An evaluation differs from the float64 one
only by its summation, so the bound is elementwise:  |y - f64| <= REL * (conv(|bf x|, |bf w|) + |bias|).

Contract of the attention (csrc/attention.hip, BF = true): scores from rounded Q, K, scaled by log2(e) / sqrt(d_k) in fp32,
masked; p = exp2(s - ceil(max s)); P V from p ROUNDED to bf16 and V rounded, divided by the sum of the UNROUNDED p.  A score
that differs in its last bits can put a p on the other side of a bf16 rounding boundary, which moves that p by one bf16 ulp; the
attention gate budgets such flips explicitly (attention_check).

The GEMM half also serves the exact-fp32 path (tests/test_fp32_ops_host.py, tests/test_gpu_fp32_ops.py): round_fn = exact takes
the operands as they are, which with rel = FP32_REL is the contract of csrc/gemm_conv.hip."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

GEMM_REL = 1.5e-5   # v_mfma_f32_32x32x16_bf16 with fp32 accumulation, K up to 2816: the bound of tests/test_gpu_vocoder_bf16.py
FP32_REL = 4e-6     # fp32 row arithmetic: the bound of tests/test_gpu_vocoder.py
ATT_FLIPS = 3       # flips of a rounded p one output element may carry
ATT_PAIR_CAP = 0.05  # share of (query row, head) pairs that may hold an element above the fp32 tier
LN_EPS = 1e-5
LOG2E = 1.4426950408889634


def bf(t):
    """round to bf16 (nearest, ties to even) and back, in t's dtype; float64 goes through fp32 first, as the kernels' values do"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def bf_trunc(t):
    """the WRONG rounding: bf16 by truncation of the fp32 bits"""
    bits = t.float().contiguous().view(torch.int32) & np.int32(-65536)
    return bits.view(torch.float32).to(t.dtype)


ACTS = {None: lambda t: t, "none": lambda t: t, "relu": torch.relu, "tanh": torch.tanh}


def conv_rows(x, w, b, dtype=torch.float64, cross_utterance=False):
    """sum_j x[b, t + j - pad, :] @ w[:, :, j].T + bias on operands taken as they are: x [B, S, Cin], w [N, Cin, KW] (the
    checkpoint's layout; [N, Cin] for a linear layer), evaluated in dtype; rows outside an utterance read as zero.
    cross_utterance: the WRONG padding, a tap past an utterance's edge reads the neighbouring utterance's row."""
    if w.dim() == 2:
        w = w[:, :, None]
    B0, S0, Cin = x.shape
    N, _, KW = w.shape
    pad = (KW - 1) // 2
    x, w = x.to(dtype), w.to(dtype)
    B, S = (1, B0 * S0) if cross_utterance else (B0, S0)
    xp = torch.zeros(B, S + 2 * pad, Cin, dtype=dtype)
    xp[:, pad:pad + S] = x.reshape(B, S, Cin)
    y = torch.zeros(B, S, N, dtype=dtype)
    for j in range(KW):
        y += xp[:, j:j + S] @ w[:, :, j].T
    if b is not None:
        y += b.to(dtype)
    return y.reshape(B0, S0, N)


def exact(t):
    """the operand rounding of the exact-fp32 contract (csrc/gemm_conv.hip): none, the operands are taken as they are"""
    return t


def gemm_emu(x, w, b, KW=None, act=None, dtype=torch.float64, round_fn=bf):
    """the contraction of the contract: both operands rounded (round_fn = exact: the fp32 path's contract, operands as they are),
    evaluated in dtype, the layer's activation on top"""
    assert KW is None or KW == (1 if w.dim() == 2 else w.shape[2])
    y = conv_rows(round_fn(x), round_fn(w), b, dtype)
    return ACTS[act](y)


def gemm_unit(x, w, b, round_fn=bf):
    """conv(|bf x|, |bf w|) + |bias| in float64: what one rounding of the running sum is relative to"""
    return conv_rows(round_fn(x).abs(), round_fn(w).abs(), None if b is None else b.abs(), torch.float64)


@dataclass
class GemmCheck:
    ok: bool
    worst: float  # worst |y - f64| / (rel * unit): <= 1 passes

    def __str__(self):
        return f"worst |y - f64| / (REL * (conv(|bf x|, |bf w|) + |b|)) = {self.worst:.3g}"


def gemm_check(got, x, w, b, act=None, rel=GEMM_REL, ref=None, unit=None, round_fn=bf):
    """every element of `got` against the float64 emulation.  The bound is on the pre-activation sum; ReLU and tanh are
    1-Lipschitz, so it holds for the stored output too."""
    ref = gemm_emu(x, w, b, act=act, round_fn=round_fn) if ref is None else ref
    unit = gemm_unit(x, w, b, round_fn=round_fn) if unit is None else unit
    got = got.reshape(ref.shape).double()
    err = (got - ref).abs()
    bound = rel * unit
    ok = bool((err <= bound).all()) and bool(torch.isfinite(got).all())
    return GemmCheck(ok, float((err / bound.clamp_min(1e-300)).max()))


# ---------------------------------------------------------------------------------------------------- LayerNorm epilogue
def layernorm_emu(z, g, b, dtype=torch.float64):
    z = z.to(dtype)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + LN_EPS) * g.to(dtype) + b.to(dtype)


@dataclass
class LnCheck:
    ok: bool
    worst: float

    def __str__(self):
        return f"worst |y - f64| / bound = {self.worst:.3g}"


def _ln_ref_bound(x, w, b, resid, g, beta, rel, round_fn, act):
    """(float64 LayerNorm(act(gemm(x)) + resid), its first-order elementwise bound): see gemm_ln_check"""
    z = gemm_emu(x, w, b, act=act, round_fn=round_fn)
    if resid is not None:
        z = z + resid.double()
    ref = layernorm_emu(z, g, beta)
    e = rel * gemm_unit(x, w, b, round_fn=round_fn)
    mean = z.mean(-1, keepdim=True)
    sigma = torch.sqrt(((z - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    yhat = (z - mean) / sigma
    bound = g.double().abs() / sigma * (e + e.mean(-1, keepdim=True) + yhat.abs() * torch.sqrt((e ** 2).mean(-1, keepdim=True)))
    return ref, bound + FP32_REL * (ref.abs() + beta.double().abs())


def gemm_ln_check(got, x, w, b, resid, g, beta, rel=GEMM_REL, round_fn=bf, act=None):
    """got = LayerNorm(act(gemm(x)) + resid) against float64, the GEMM's bound e = rel * unit propagated through the LayerNorm to
    first order: with yhat = (z - mean) / sigma, d y_n = g_n / sigma * (d z_n - mean(d z) - yhat_n * mean(yhat d z)) and
    |mean(yhat d z)| <= rms(yhat) rms(d z) = rms(e); plus FP32_REL * (|ref| + |ln_b|) for the fp32 row arithmetic.  act (ReLU, tanh)
    is 1-Lipschitz, so the GEMM's bound holds on act(z); resid = None is no residual."""
    ref, bound = _ln_ref_bound(x, w, b, resid, g, beta, rel, round_fn, act)
    got = got.reshape(ref.shape).double()
    err = (got - ref).abs()
    ok = bool((err <= bound).all()) and bool(torch.isfinite(got).all())
    return LnCheck(ok, float((err / bound.clamp_min(1e-300)).max()))


# ---------------------------------------------------------------------------------------------------- predictor tail
def pred_tail_ref(h, w2, b2, g2, beta2, wlin, blin, lens, control=1.0, target_given=False, rel=FP32_REL):
    """(float64 pred [B, S], its first-order bound) of the second launch of a VariancePredictor on hidden rows h [B, S, F]:
    (LayerNorm(relu(conv_rows(h, w2, b2))) . wlin + blin), zero at t >= lens[b], * control unless a target is given.
    bound = sum_n |wlin_n| (LayerNorm bound)_n + FP32_REL (sum_n |y_n wlin_n| + |blin|), scaled like the value."""
    y, yb = _ln_ref_bound(h, w2, b2, None, g2, beta2, rel, exact, "relu")
    wl = wlin.double().reshape(-1)
    pred = y @ wl + blin.double().reshape(())
    bound = yb @ wl.abs() + FP32_REL * ((y * wl).abs().sum(-1) + blin.double().abs().reshape(()))
    c = 1.0 if target_given else float(control)
    valid = torch.arange(h.shape[1])[None, :] < torch.as_tensor(lens)[:, None]
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(valid, pred * c, zero), torch.where(valid, bound * abs(c), zero)


def pred_tail_fp32(h, w2, b2, g2, beta2, wlin, blin, lens, control=1.0, target_given=False):
    """torch's fp32 CPU evaluation of the same tail (what "as close to float64 as fp32 gets" means for it)"""
    y = layernorm_emu(gemm_emu(h, w2, b2, act="relu", dtype=torch.float32, round_fn=exact), g2, beta2, dtype=torch.float32)
    pred = y @ wlin.float().reshape(-1) + blin.float().reshape(())
    valid = torch.arange(h.shape[1])[None, :] < torch.as_tensor(lens)[:, None]
    pred = torch.where(valid, pred, torch.zeros((), dtype=torch.float32))
    return pred if target_given else pred * torch.tensor(float(control), dtype=torch.float32)


def pred_check(got, ref, bound, tight):
    """every pred against float64 at tight x the first-order bound; a masked row (bound 0) must be exactly zero.  worst is in units
    of the gate (<= 1 passes); worst * tight is the share of the first-order bound."""
    got = got.reshape(ref.shape).double()
    err = (got - ref).abs()
    ok = bool((err <= tight * bound).all()) and bool(torch.isfinite(got).all())
    live = bound > 0
    worst = float((err[live] / (tight * bound[live])).max()) if bool(live.any()) else 0.0
    if bool((err[~live] != 0).any()):
        worst = float("inf")
    return LnCheck(ok, worst)


# ---------------------------------------------------------------------------------------------------- attention
def attention_emu(qkv, lens, H, dtype=torch.float64, drop_key=None, mask_shift=0, normalised_p=False, round_fn=bf):
    """(out [B, S, d], unit, flip) of the bf16 attention contract on head-packed qkv [B, S, 3 d] (Q | K | V, head h at h * dk),
    evaluated in dtype.  unit[b, q, (h, c)] = sum_j P_j |bf v_jc| and flip = 2^-8 max_j P_j |bf v_jc| with P_j = bf(p_j) / sum p.
    A zero-length utterance gives NaN (softmax over an empty set), as the kernels do.
    The WRONG variants, for the proof of the gate: drop_key = j leaves key j out of every row; mask_shift = 1 admits one key too
    many (-1: one too few); normalised_p rounds p / sum p instead of p; round_fn replaces the operand rounding."""
    B, S, d3 = qkv.shape
    d = d3 // 3
    dk = d // H
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, S, H, dk).permute(0, 2, 1, 3) for i in range(3))
    scale = float(np.float32(LOG2E / np.sqrt(dk)))
    s = (round_fn(q).to(dtype) @ round_fn(k).to(dtype).transpose(-1, -2)) * torch.tensor(scale, dtype=dtype)
    dead = torch.arange(S)[None, :] >= (lens[:, None] + mask_shift)
    if drop_key is not None:
        dead = dead.clone()
        dead[:, drop_key] = True
    s = s.masked_fill(dead[:, None, None, :], -np.inf)
    mx = torch.ceil(s.max(dim=-1, keepdim=True).values)
    p = torch.exp2(s - mx)
    l = p.sum(dim=-1, keepdim=True)
    vr = round_fn(v).to(dtype)
    if normalised_p:
        P = bf(p / l)
        out = P @ vr
    else:
        P = bf(p) / l
        out = (bf(p) @ vr) / l
    unit = P.double() @ vr.double().abs()
    flip = _flip(P.double(), vr.double().abs())
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, S, d)  # noqa: E731
    return back(out), back(unit), back(flip)


def _flip(P, va):
    """2^-8 max_j P[..., q, j] va[..., j, c], a block of query rows at a time (never the whole [S, S, dk] product)"""
    out = torch.empty(P.shape[:-1] + (va.shape[-1],), dtype=torch.float64)
    rows = max(1, 2 ** 22 // max(1, va.numel()))
    for q0 in range(0, P.shape[-2], rows):
        out[..., q0:q0 + rows, :] = (P[..., q0:q0 + rows, :, None] * va[..., None, :, :]).amax(dim=-2)
    return 2.0 ** -8 * out


@dataclass
class AttentionCheck:
    ok: bool
    worst_flips: float   # worst (err - FP32_REL * unit) / flip over all elements: <= ATT_FLIPS passes
    worst_fp32: float    # worst err / (FP32_REL * unit)
    pair_share: float    # share of (query row, head) pairs with an element above FP32_REL * unit: <= ATT_PAIR_CAP passes
    elem_share: float    # share of elements above the first tier (0 passes)

    def __str__(self):
        return (f"worst element {self.worst_flips:.3g} flips beyond the fp32 tier (allowed {ATT_FLIPS}), {100 * self.elem_share:.3g} % of elements "
                f"above the first tier; {100 * self.pair_share:.3g} % of (row, head) pairs above the fp32 tier (cap {100 * ATT_PAIR_CAP:g} %), "
                f"worst err / (4e-6 unit) = {self.worst_fp32:.3g}")


def attention_check(got, ref, unit, flip, H):
    """two tiers per output element of a (query row, head): every element within FP32_REL * unit + ATT_FLIPS * flip, and at most
    ATT_PAIR_CAP of the (row, head) pairs with any element above FP32_REL * unit.  Utterances whose reference is NaN (zero
    length) are the caller's to check; they are left out here."""
    live = ~torch.isnan(ref).reshape(ref.shape[0], -1).any(dim=1)
    got, ref, unit, flip = (t[live].double() for t in (got.reshape(ref.shape), ref, unit, flip))
    B, S, d = ref.shape
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, np.inf))
    fp = FP32_REL * unit
    over1 = err > fp + ATT_FLIPS * flip
    over2 = (err > fp).reshape(B, S, H, d // H).any(dim=-1)
    pair_share = float(over2.double().mean()) if over2.numel() else 0.0
    worst_flips = float(((err - fp) / flip.clamp_min(1e-300)).max()) if err.numel() else 0.0
    worst_fp32 = float((err / fp.clamp_min(1e-300)).max()) if err.numel() else 0.0
    ok = not bool(over1.any()) and pair_share <= ATT_PAIR_CAP
    return AttentionCheck(ok, worst_flips, worst_fp32, pair_share, float(over1.double().mean()) if err.numel() else 0.0)
