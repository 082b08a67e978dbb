"""One launch of the vocoder's implicit GEMM (csrc/vocoder.hip k_voc_gemm, csrc/vocoder_bf16.hip k_voc_gemm_bf16) evaluated on the
CPU, the gate that holds the kernels to it, and the table of cases.  Shared by tests/test_vocoder_ops_host.py (the gate proven on
the CPU both ways, the geometry of the table) and tests/test_gpu_vocoder_ops.py (the kernels against the float64 evaluation).

THE LAUNCH (what stage() in csrc/vocoder_api.hip builds, and ns_voc_op_conv_form / ns_voc_op_upsample alone), x [B, S, C]:
    a = in_act ? lrelu(x, 0.1) : x          bf16 mode: lrelu in fp32 (one fp32 multiply), then a rounded to bf16 (nearest even)
    v = conv(a, W) + bias                   W the folded fp32 weights; bf16 mode: W rounded to bf16
    v = out_act ? lrelu(v, 0.1) : v
    v = v + resid                           when there is a residual
    y = v | acc + v | (acc + v) / n_rb      mrf 0 | 1 | 2
The reference is this, written plainly with F.conv1d / F.conv_transpose1d, in float64.

THE GATE, elementwise:  |got - ref| <= REL * (conv(|a|, |W|) + |bias|) + E.
REL is the project's figure for one contraction: 4e-6 fp32 (bf16_emu.FP32_REL), 1.5e-5 bf16 against the emulation
(bf16_emu.GEMM_REL): an evaluation differs from the float64 one only by the order and the roundings of its sum.  That bound is on
the pre-activation v; the output lrelu is 1-Lipschitz, the residual and the acc are added exactly in the reference, so it carries
to the output unchanged.  E is what the epilogue's own fp32 operations add after `tot + bias` (which REL's |bias| covers), one
half-ulp (u = 2^-24 relative) of each value it forms, from the epilogue lines of both kernels:
    if (p.out_act) v = lrelu(v, p.out_slope);            v < 0: one product, and the slope is the fp32 0.1f, not 0.1 (1.5e-8
                                                         relative):  (u + |0.1f / 0.1 - 1|) * |0.1 v|
    if (p.R) v = v + p.R[at];                            u * |v + resid|
    if (p.mrf == 1) v = p.Y[at] + v;                     u * |acc + v|
    else if (p.mrf == 2) v = (p.Y[at] + v) / p.mrf_div;  u * |acc + v| + u * |(acc + v) / n_rb|
Each magnitude is taken from the float64 reference and widened by the error bound accumulated up to that line (the computed value
is that close to the reference's), so the inequality is exact, not first-order.  For mrf 2 the terms ahead of the division are
NOT divided by n_rb: the gate is the one written above, looser there by at most n_rb.  Nothing is tuned: against REL * unit of
about 4e-6 ... 6e-5 per element, E is about 6e-8 of the output's magnitude per line.

THE CASES.  k_voc_gemm tiles 128 rows, k_voc_gemm_bf16 256 (tile() restates the two dispatch rules); every case has at least three
row tiles, a partial last one, a tile boundary strictly inside an utterance and an utterance boundary strictly inside a later tile
at a row that is no multiple of 32 (geometry(); asserted on every CPU run by tests/test_vocoder_ops_host.py)."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

import smart_nar_fast_tts_amd.workload as wl
from tests import bf16_emu as E
from tests import hifigan_cpu
from tests.hifigan_bf16_emu import bf, lrelu32

MODES = ("fp32", "bf16")
REL = {"fp32": E.FP32_REL, "bf16": E.GEMM_REL}
U = 2.0 ** -24                                   # half an ulp of an fp32 value, relative
SLOPE = 0.1
SLOPE_ERR = abs(float(np.float32(SLOPE)) / SLOPE - 1.0)  # the kernels multiply by 0.1f
N_RB = 3
TILE_M = {"fp32": 128, "bf16": 256}


def tile(mode, N):
    """(rows, columns) of the tile a launch with N output columns takes: launch_voc_gemm / launch_voc_gemm_bf16"""
    if mode == "fp32":
        return 128, (128 if N % 128 == 0 else 64 if N % 64 == 0 else 32)
    return 256, (256 if N % 256 == 0 else 128 if N % 128 == 0 else 64 if N % 64 == 0 else 32)


# ---------------------------------------------------------------------------------------------------- the forms
@dataclass(frozen=True)
class Form:
    key: str
    j: int        # resblock of the stage (kernel 3, 7, 11)
    which: int    # convs1 / convs2
    n: int        # dilation index (convs1: d = 1, 3, 5; convs2: d = 1)
    in_act: bool = True
    out_act: bool = False
    resid: bool = False
    mrf: int = 0

    def name(self, stage):
        return f"resblocks.{N_RB * stage + self.j}.convs{self.which}.{self.n}"


# plain: what ns_voc_op_conv launches.  The rest: ns_voc_op_conv_form, each on the conv stage() gives that form (the last c2 of
# resblock j carries mrf = j).  act_res is NOT a form of stage(): the entry point admits it, and it is the only one that tells
# "residual after the output lrelu" (the epilogue's order) from "before".
PLAIN = [Form("plain_k3_d1", 0, 1, 0), Form("plain_k11_d5", 2, 1, 2)]
EPILOGUES = [Form("c1", 2, 1, 2, out_act=True),
             Form("c2_mid", 1, 2, 1, in_act=False, resid=True),
             Form("c2_last_mrf0", 0, 2, 2, in_act=False, resid=True, mrf=0),
             Form("c2_last_mrf1", 1, 2, 2, in_act=False, resid=True, mrf=1),
             Form("c2_last_mrf2", 2, 2, 2, in_act=False, resid=True, mrf=2),
             Form("act_res", 0, 1, 1, out_act=True, resid=True)]
FORMS = {f.key: f for f in PLAIN + EPILOGUES}


@dataclass(frozen=True)
class Case:
    kind: str     # "conv" | "up"
    form: str     # a key of FORMS; "up" for an upsampler
    stage: int    # conv: the stage whose resblocks it belongs to; up: the upsampler's index
    mode: str
    B: int
    S: int

    @property
    def id(self):
        return f"{self.form}-stage{self.stage}-{self.mode}-{self.B}x{self.S}"


def channels(h, stage):
    return h["upsample_initial_channel"] >> (stage + 1)


def grid(h, c: Case):
    """(grid rows per utterance Sg, output columns N, contraction length K) of the case's launch"""
    ch = channels(h, c.stage)
    if c.kind == "up":
        return c.S + 1, h["upsample_rates"][c.stage] * ch, 2 * 2 * ch
    return c.S, ch, h["resblock_kernel_sizes"][FORMS[c.form].j] * ch


def geometry(mode, N, B, Sg):
    """what the case table promises of a launch of B utterances of Sg grid rows: the tile, the number of row tiles, the rows of
    the last one, the first tile boundary strictly inside an utterance, and the first utterance boundary strictly inside a tile
    other than the first at a row that is no multiple of 32 (None where there is none)"""
    BM, BN = tile(mode, N)
    M = B * Sg
    inside = next((r for r in range(BM, M, BM) if r % Sg), None)
    edge = next((r for r in range(Sg, M, Sg) if r > BM and r % BM and r % 32), None)
    return dict(BM=BM, BN=BN, M=M, tiles=-(-M // BM), last=M % BM, tile_boundary=inside, utt_boundary=edge)


def geometry_ok(g):
    return g["tiles"] >= 3 and g["last"] != 0 and g["tile_boundary"] is not None and g["utt_boundary"] is not None


CONV_LONG = {"fp32": (3, 97), "bf16": (3, 181)}   # 291 / 543 rows; S > 2 * 25, the reach of k = 11, d = 5
CONV_SHORT = {"fp32": (40, 7), "bf16": (80, 7)}   # 280 / 560 rows, Sg < 28: several utterances inside one 32-row block
UP_B = 3


def smallest_up_S(mode, N):
    """the smallest S whose B = 3 upsampler grid of S + 1 rows per utterance passes geometry_ok"""
    return next(S for S in range(1, 4096) if geometry_ok(geometry(mode, N, UP_B, S + 1)))


UP_LONG = {"fp32": (UP_B, 85), "bf16": (UP_B, 170)}  # = smallest_up_S for every upsampler width (asserted by the host test)
UP_SHORT = {"fp32": (40, 6), "bf16": (80, 6)}        # S = 7 would make Sg = 8 and every tile boundary an utterance boundary

PLAIN_CASES = ([Case("conv", f.key, st, m, *CONV_LONG[m]) for m in MODES for st in range(4) for f in PLAIN]
               + [Case("conv", "plain_k11_d5", st, m, *CONV_SHORT[m]) for m in MODES for st in (0, 3)])
EPILOGUE_CASES = [Case("conv", f.key, st, m, *sz[m]) for m in MODES for st in (0, 3) for f in EPILOGUES for sz in (CONV_LONG, CONV_SHORT)]
UP_CASES = [Case("up", "up", i, m, *sz[m]) for m in MODES for i in range(4) for sz in (UP_LONG, UP_SHORT)]
CASES = PLAIN_CASES + EPILOGUE_CASES + UP_CASES


# ---------------------------------------------------------------------------------------------------- weights and inputs
@functools.lru_cache(maxsize=None)
def model():
    """(config, checkpoint-form state dict, the folded fp32 generator on the CPU)"""
    h = wl.hifigan_config("v1")
    sd = wl.synth_vocoder_state_dict(h, seed=0)
    return h, sd, hifigan_cpu.folded(h, sd, torch.float32)


@dataclass
class Launch:
    kind: str
    mode: str
    w: torch.Tensor      # folded fp32: Conv1d [N, Cin, k]; ConvTranspose1d [Cin, Cout, 2 u]
    b: torch.Tensor
    k: int = 1
    d: int = 1
    u: int = 1
    in_act: bool = True
    out_act: bool = False
    mrf: int = 0


def launch_of(c: Case) -> Launch:
    h, _, m = model()
    if c.kind == "up":
        up = m.ups[c.stage]
        return Launch("up", c.mode, up.weight.detach(), up.bias.detach(), u=h["upsample_rates"][c.stage])
    f = FORMS[c.form]
    conv = getattr(m.resblocks[N_RB * c.stage + f.j], f"convs{f.which}")[f.n]
    return Launch("conv", c.mode, conv.weight.detach(), conv.bias.detach(), k=conv.kernel_size[0], d=conv.dilation[0],
                  in_act=f.in_act, out_act=f.out_act, mrf=f.mrf)


def inputs(c: Case):
    """(x, resid or None, acc or None): N(0, 1) scaled so that the pre-activation output has a standard deviation near 1 with the
    synthetic weights (resblock weights are U(+-1 / sqrt(K)): variance 1 / (3 K); an lrelu halves the input's power; of a short
    utterance's taps only the share inside it counts; the upsamplers carry the He gain already), residual and acc N(0, 1); the
    last utterance a copy of the first."""
    h = model()[0]
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    ch = channels(h, c.stage)
    if c.kind == "up":
        cin, scale, f = 2 * ch, 1.0, None
    else:
        f = FORMS[c.form]
        L = launch_of(c)
        live = sum(0 <= t + (j - L.k // 2) * L.d < c.S for t in range(c.S) for j in range(L.k)) / (c.S * L.k)  # taps inside the utterance
        cin, scale = ch, ((3.0 / 0.505 if f.in_act else 3.0) / live) ** 0.5
    x = torch.randn(c.B, c.S, cin, generator=g) * scale
    resid = torch.randn(c.B, c.S, ch, generator=g) if f is not None and f.resid else None
    acc = torch.randn(c.B, c.S, ch, generator=g) if f is not None and f.mrf else None
    for t in (x, resid, acc):
        if t is not None:
            t[c.B - 1] = t[0]
    return x, resid, acc


# ---------------------------------------------------------------------------------------------------- the evaluation
def _lrelu(t, slope=SLOPE):
    """in float64 the exact slope; in fp32 the kernels' own product with the fp32 slope"""
    return lrelu32(t, slope) if t.dtype == torch.float32 else torch.where(t > 0, t, t * slope)


def operands(L: Launch, x, dtype, in_act=None):
    """(a, W) as the mode's contract takes them, in dtype"""
    in_act = L.in_act if in_act is None else in_act
    if L.mode == "bf16":
        return bf(lrelu32(x) if in_act else x).to(dtype), bf(L.w).to(dtype)
    a = x.to(dtype)
    return (_lrelu(a) if in_act else a), L.w.to(dtype)


def contract(L: Launch, a, w, b, cross_utterance=False):
    """conv(a, w) + b on time-major a [B, S, C].  cross_utterance: the WRONG padding, a tap past an utterance's edge reads the
    neighbouring utterance's row (the batch evaluated as one utterance of B S rows)"""
    B, S, C = a.shape
    at = (a.reshape(1, B * S, C) if cross_utterance else a).transpose(1, 2)
    if L.kind == "up":
        y = F.conv_transpose1d(at, w, b, stride=L.u, padding=L.u // 2)
    else:
        y = F.conv1d(at, w, b, padding=L.d * (L.k - 1) // 2, dilation=L.d)
    return y.transpose(1, 2).reshape(B, -1, y.shape[1]).contiguous()


@dataclass
class Eval:
    out: torch.Tensor
    v: torch.Tensor = None       # conv + bias, before the output lrelu
    unit: torch.Tensor = None    # conv(|a|, |W|) + |bias|
    bound: torch.Tensor = None   # REL * unit + E (float64 evaluations only)
    extra: dict = field(default_factory=dict)


def evaluate(L: Launch, x, resid=None, acc=None, dtype=torch.float64, *, cross_utterance=False, drop_chunk=False, in_act=None,
             out_act=None, out_slope=SLOPE, resid_mode="after", mrf_mode=None, swap_halves=False, with_bound=True) -> Eval:
    """the launch in dtype.  Every keyword past dtype is a MUTATION for the proof of the gate (the default is the launch itself):
    drop_chunk zeroes one 32-wide K chunk of W; in_act / out_act override the switches; out_slope the output slope; resid_mode
    "omit" | "next_row" (row t + 1 of the flat [B S] grid) | "before_act"; mrf_mode "store" | "no_div" | "div2"; swap_halves exchanges
    the upsampler's two taps (W[:, :, r] and W[:, :, r + u])."""
    a, w = operands(L, x, dtype, in_act)
    if drop_chunk:
        w = w.clone()
        if L.kind == "up":
            w[:32, :, L.u:] = 0  # the first 32 channels of the x[q - 1] tap
        else:
            w[:, :32, L.k // 2] = 0  # the first 32 channels of the centre tap
    if swap_halves:
        w = torch.cat([w[:, :, L.u:], w[:, :, :L.u]], dim=2)
    b = L.b.to(dtype)
    v = contract(L, a, w, b, cross_utterance)
    r = None if resid is None else resid.to(dtype)
    if resid_mode == "next_row" and r is not None:
        r = r.reshape(-1, r.shape[-1]).roll(-1, 0).reshape(r.shape)
    if resid_mode == "omit":
        r = None
    o = v
    if resid_mode == "before_act" and r is not None:
        o, r = o + r, None
    if L.out_act if out_act is None else out_act:
        o = _lrelu(o, out_slope)
    if r is not None:
        o = o + r
    mrf = {None: L.mrf, "store": 0, "no_div": 1, "div2": 2}[mrf_mode]
    if mrf:
        o = acc.to(dtype) + o
    if mrf == 2:
        o = o / (2 if mrf_mode == "div2" else N_RB)
    ev = Eval(o, v)
    if with_bound and dtype == torch.float64:
        ev.unit = contract(L, a.abs(), w.abs(), b.abs())
        ev.bound = _bound(L, ev, resid, acc)
    return ev


def _bound(L: Launch, ev: Eval, resid, acc):
    """REL * unit + E, the epilogue's lines one at a time (module docstring); e is the bound accumulated so far"""
    e = REL[L.mode] * ev.unit
    o = ev.v
    if L.out_act:
        o = _lrelu(o)
        e = e + torch.where(ev.v < e, (U + SLOPE_ERR) * SLOPE * (ev.v.abs() + e), torch.zeros_like(e))
    if resid is not None:
        o = o + resid.double()
        e = e + U * (o.abs() + e)
    if L.mrf:
        o = acc.double() + o
        e = e + U * (o.abs() + e)
    if L.mrf == 2:
        o = o / N_RB
        e = e + U * (o.abs() + e)
    return e


@dataclass
class Check:
    ok: bool
    worst: float  # worst |got - ref| / bound: <= 1 passes; inf for a value that is not finite

    def __str__(self):
        return f"worst |got - f64| / (REL * (conv(|a|, |W|) + |bias|) + E) = {self.worst:.3g}"


def check(got, ref: Eval, rows=None) -> Check:
    """every element of got against the float64 evaluation (rows: a slice of the flat [B S] output grid, else all of it)"""
    got = got.reshape(ref.out.shape).double()
    err = (got - ref.out).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = err / ref.bound.clamp_min(1e-300)
    if rows is not None:
        ratio = ratio.reshape(-1, ratio.shape[-1])[rows]
    return Check(bool((ratio <= 1).all()), float(ratio.max()))
