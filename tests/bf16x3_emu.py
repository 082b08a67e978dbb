"""The yardstick of the opt-in "bf16x3" mode's GEMM (csrc/gemm_bf16x3.hip k_conv_gemm_b3) taken ALONE: the kernel's contract
restated in numpy / torch, the wrong kernels the gate must reject, and the case tables.  Shared by tests/test_bf16x3_ops_host.py (the
gate proven on the CPU, both ways; the tables checked against the dispatch through ns_plan_gemm_b3) and
tests/test_gpu_bf16x3_ops.py (the three instantiations against float64).

Contract: every fp32 operand is split by TRUNCATION into three bf16 pieces, x = hi + mid + lo exactly (split3); six of the nine
piece products are kept (TERMS, in the kernel's order) and summed in fp32 on the matrix cores; zero padding per utterance of S
rows; bias and activation in fp32.  Every kept product is exact in fp32, so the kernel differs from the float64 evaluation of the
UNSPLIT operands by its summation and by the three dropped products.  The gate is the exact-fp32 path's own,
    |y - f64| <= FP32_REL * (conv(|x|, |w|) + |bias|)        (tests/bf16_emu.py gemm_check, round_fn = exact),
and it is all the mode's promise of "fp32-sized error" can mean per element.

Why SAME-SIGN operands.  The pieces are taken by truncation, so each carries its operand's sign and each partial product the
sign of x * w.  With random-sign operands a lost lo*hi, hi*lo or mid*mid term is a random walk over K and stays inside the gate
(at K >= 1024 at every element, at K = 256 at all but a stray one: tests/test_bf16x3_ops_host.py asserts exactly that); with
x >= 0 and w >= 0 the same loss shifts every output one way, by more than the gate.  So the plain cases run twice, and the same-sign run also bounds the signed mean of (y - f64) / unit by half
of what the gentlest lost term would shift it by (min_mutant_bias, computed, not written down).

The dropped products mid*lo, lo*mid and lo*lo share that sign rule: each of the first two is up to 2^-22 of a product (mid < 2^-7,
lo < 2^-15 of its operand), not "below 2^-32", and on same-sign data they add up to about 2^-24 of conv(|x|, |w|) — the six-term
sum sits at about 0.015 of the gate there (dropped_share measures it).

Out of scope: Inf / NaN operands (split3 turns an Inf into NaN through Inf - Inf, on the device as here).  A value whose residue
x - hi is subnormal (|x| < 2^-103) loses that residue's low bits when the kernel packs the pieces; split3 here keeps them, and no
case comes near."""
from __future__ import annotations

import numpy as np
import torch

from tests import bf16_emu as E
from tests.bf16_emu import conv_rows, exact, gemm_check, gemm_emu, gemm_ln_check, gemm_unit  # noqa: F401  (the yardstick's other half)

REL = E.FP32_REL
PIECES = ("hi", "mid", "lo")
# (piece of x, piece of w) of the six MFMAs of `compute`, in the kernel's order: smallest terms first
TERMS = (("lo", "hi"), ("hi", "lo"), ("mid", "mid"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi"))
SMALL_TERMS = TERMS[:3]   # about 2^-16 of a product each: invisible on random-sign data
DROPPED = (("mid", "lo"), ("lo", "mid"), ("lo", "lo"))


def _trunc16(t):
    return (t.contiguous().view(torch.int32) & np.int32(-65536)).view(torch.float32)


def split3(x):
    """the truncation split of csrc/gemm_bf16x3.hip split3 / split_weights_b3: (hi, mid, lo) as fp32, hi + mid + lo == x"""
    x = x.float().contiguous()
    hi = _trunc16(x)
    r = x - hi
    mid = _trunc16(r)
    return hi, mid, r - mid


def _pieces(t):
    return dict(zip(PIECES, split3(t)))


def six_term(x, w, b, dtype=torch.float64, drop=None, swap_w_mid_lo=False, cross_utterance=False):
    """the kernel's contract: the sum of the six kept piece products over conv_rows, in dtype, plus the bias.
    The WRONG variants, for the proof of the gate: drop = one of TERMS left out; swap_w_mid_lo = the weight's mid and lo planes
    exchanged; cross_utterance = conv_rows' wrong padding."""
    xp, wp = _pieces(x), _pieces(w)
    if swap_w_mid_lo:
        wp["mid"], wp["lo"] = wp["lo"], wp["mid"]
    assert drop is None or drop in TERMS
    y = None
    for a, c in TERMS:
        if (a, c) != drop:
            t = conv_rows(xp[a], wp[c], None, dtype, cross_utterance=cross_utterance)
            y = t if y is None else y + t
    return y if b is None else y + b.to(dtype)


def term_drop_mutants():
    return {f"x_{a} * w_{c} dropped": (lambda x, w, b, t=(a, c): six_term(x, w, b, drop=t)) for a, c in TERMS}


def mutants(KW):
    """name -> the output of a WRONG kernel in float64 (its only error is the mutation): each of the six terms dropped, the
    weight's mid and lo planes exchanged, and (KW > 1) a tap past an utterance's edge reading the neighbouring utterance"""
    out = term_drop_mutants()
    out["w mid and lo planes exchanged"] = lambda x, w, b: six_term(x, w, b, swap_w_mid_lo=True)
    if KW > 1:
        out["neighbour's row for zero"] = lambda x, w, b: six_term(x, w, b, cross_utterance=True)
    return out


def kernel_order_fp32(x, w, b):
    """six_term accumulated as the kernel does, in fp32: one 16-wide K block after another (channel block major, tap minor, as
    dma_chunk walks them), within a block the six terms in TERMS order, each term's 16 products summed exactly and then added to
    the running fp32 sum with one rounding.  (The order INSIDE one MFMA is not specified; this is the emulation a failing
    same-sign case is compared with first.)  x [B, S, Cin], w [N, Cin, KW] -> fp32 [B, S, N]"""
    if w.dim() == 2:
        w = w[:, :, None]
    B, S, Cin = x.shape
    N, _, KW = w.shape
    pad = (KW - 1) // 2
    xp, wp = _pieces(x), _pieces(w)
    xpad = {}
    for k, v in xp.items():
        z = torch.zeros(B, S + 2 * pad, Cin, dtype=torch.float64)
        z[:, pad:pad + S] = v.double()
        xpad[k] = z
    wd = {k: v.double() for k, v in wp.items()}
    acc = torch.zeros(B, S, N, dtype=torch.float32)
    for c0 in range(0, Cin, 32):
        for j in range(KW):
            for k0 in (c0, c0 + 16):
                for a, c in TERMS:
                    acc = (acc.double() + xpad[a][:, j:j + S, k0:k0 + 16] @ wd[c][:, k0:k0 + 16, j].T).float()
    return acc if b is None else acc + b.float()


def same_sign(x):
    return x.abs()


def layer_keys(name):
    """the state-dict keys a contraction's weight and bias are packed from"""
    if name.endswith(".qkv"):
        p = name[:-len(".qkv")]
        return [f"{p}.{k}.{s}" for k in ("w_qs", "w_ks", "w_vs") for s in ("weight", "bias")]
    if name.startswith("postnet."):
        return [name + ".0.conv.weight", name + ".0.conv.bias"]
    return [name + ".weight", name + ".bias"]


def same_sign_weights(sd, name):
    """a state-dict override with |w| and |b| for one layer (the planes are split when the model loads)"""
    return {k: np.abs(np.asarray(sd[k])) for k in layer_keys(name)}


def signed_mean(y, ref, unit):
    """mean((y - f64) / unit): a lost term moves it one way at every element; a nearest-even accumulator's rounding averages out"""
    return float(((y.double().reshape(ref.shape) - ref) / unit).mean())


# ---------------------------------------------------------------------------------------------------- reduced shapes (CPU)
# (Cin, KW) of every contraction that has planes, with a few dozen rows and columns: real contraction lengths and utterance edges
HOST_SHAPES = [(256, 9), (256, 1), (512, 5), (1024, 1), (512, 1)]   # w_1, qkv / fc, PostNet, w_2, tiny512 fc
HOST_B, HOST_S, HOST_N = 3, 13, 48
# the plain same-sign cases' contractions (P1 / P4 / Q2, P2 / Q1): what min_mutant_bias is taken over
SAME_SIGN_SHAPES = [(256, 9), (256, 1)]


def host_case(Cin, KW, same):
    g = torch.Generator().manual_seed(7 * Cin + KW)
    x = torch.randn(HOST_B, HOST_S, Cin, generator=g)
    w = torch.randn(HOST_N, Cin, KW, generator=g) * 0.05
    b = torch.randn(HOST_N, generator=g) * 0.05
    return (x.abs(), w.abs(), b.abs()) if same else (x, w, b)


_BIAS = {}


def mutant_biases(Cin, KW):
    """(signed mean of six_term, {term-drop mutant: signed mean}) on the same-sign reduced case of this contraction"""
    if (Cin, KW) not in _BIAS:
        x, w, b = host_case(Cin, KW, True)
        ref, unit = conv_rows(x, w, b), gemm_unit(x, w, b, round_fn=exact)
        _BIAS[(Cin, KW)] = (signed_mean(six_term(x, w, b), ref, unit), {k: signed_mean(f(x, w, b), ref, unit) for k, f in term_drop_mutants().items()})
    return _BIAS[(Cin, KW)]


def min_mutant_bias():
    """the smallest |signed mean| any lost term gives on the same-sign shapes: a same-sign GPU case may carry half of it"""
    return min(abs(v) for s in SAME_SIGN_SHAPES for v in mutant_biases(*s)[1].values())


# ---------------------------------------------------------------------------------------------------- the case tables (GPU)
L0 = "mel_decoder.layer_stack.0"
TINY1056 = "tiny1056"   # config tiny with conv_filter_size 1056 = 4 * 256 + 32: the only width with a partial last column tile
D_MODEL = {"tiny": 256, TINY1056: 256, "tiny512": 512}
D_INNER = {"tiny": 1024, TINY1056: 1056, "tiny512": 1024}


def shape_of(name, config):
    """(Cin, N, KW) of a contraction of the cases"""
    d = D_MODEL[config]
    if name.startswith("postnet."):
        return 512, 512, 5
    return {"qkv": (d, 3 * d, 1), "fc": (d, d, 1), "w_1": (d, D_INNER[config], 9), "w_2": (D_INNER[config], d, 1)}[name.rsplit(".", 1)[1]]


# (case, contraction, config, B, S, tile rows, (row tiles, column tiles), same-sign variant too).  The smallest the gates admit:
# 128-row cases at the first M with 200 tiles (conv_gemm_b3_ok), 256-row cases at the first with 240 (conv_gemm_b3_tile), every
# M leaving a partial last row tile.  P3 is random-sign only: tanh saturates on same-sign sums.
PLAIN_CASES = [
    ("P1", L0 + ".pos_ffn.w_1", "tiny", 19, 331, 128, (50, 4), True),
    ("P2", L0 + ".slf_attn.qkv", "tiny", 25, 339, 128, (67, 3), True),
    ("P3", "postnet.convolutions.1", "tiny", 37, 343, 128, (100, 2), False),
    ("P4", L0 + ".pos_ffn.w_1", TINY1056, 15, 333, 128, (40, 5), True),
    ("Q1", L0 + ".slf_attn.qkv", "tiny", 59, 343, 256, (80, 3), True),
    ("Q2", L0 + ".pos_ffn.w_1", "tiny", 44, 344, 256, (60, 4), True),
]
# (case, op, config, B, S, what ns_plan_gemm_b3(epi = 1) must answer): L = the 64 x 256 full-row tile with the LayerNorm epilogue,
# T = the plain 128 x 256 tile followed by k_layernorm (N = 512 has no full-row tile)
LN_CASES = [
    ("L1", "ffn", "tiny", 37, 345, (64, 256, 1, 200)),
    ("L2", "mha", "tiny", 37, 345, (64, 256, 1, 200)),
    ("T1", "mha", "tiny512", 37, 343, (128, 256, 0, 200)),
]
HANDOVER = (L0 + ".pos_ffn.w_1", "tiny", 19, 330, 331)   # 49 x 4 = 196 tiles: fp32; 50 x 4: the mode


def judged_utterances(B, S, BM):
    """the utterances the float64 reference is evaluated on (they are independent: zero padding per utterance): the first, the
    last, the ones holding the first and the last row-tile boundary, one in the middle"""
    ntm = (B * S + BM - 1) // BM
    return sorted({0, B - 1, BM // S, (ntm - 1) * BM // S, B // 2})


def ragged_lens(B, S):
    """valid lengths with S, S - 1, the halves, tile edges and a single frame among them"""
    head = [S, S - 1, S // 2 + 1, S // 2, 129, 65, 64, 33, 1]
    return (head + [1 + (97 * b) % S for b in range(len(head), B)])[:B]
