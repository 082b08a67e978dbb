"""Every launch form of the opt-in "bf16x3" GEMM (csrc/gemm_bf16x3.hip k_conv_gemm_b3: the 128 x 256 and 256 x 256 plain tiles, the
64 x 256 full-row tile with the LayerNorm epilogue, and the two-launch and fall-back branches of gemm_ln) ALONE on the MI355X
against a float64 evaluation of the same contraction, elementwise: |gpu - f64| <= 4e-6 * (conv(|x|, |w|) + |bias|) — the exact-fp32
path's own gate, which is what the mode's "fp32-sized error" promises.  The gate, the wrong kernels it rejects and the case tables
are tests/bf16x3_emu.py; tests/test_bf16x3_ops_host.py proves the gate on the CPU and asserts through ns_plan_gemm_b3 that every
case takes the form it names.

Plain forms run through ops.gemm of a model built with matmul = "bf16x3" on inputs the test supplies; the last utterance is a copy
of the first and the two outputs must be the same BITS.  P1, P2, P4, Q1 and Q2 run twice: with random-sign inputs, and with
x >= 0 against a model whose layer holds |w| and |b| — only there does a lost lo*hi, hi*lo or mid*mid term (or exchanged mid / lo
planes) shift every element one way by more than the gate; the same-sign run also holds the signed mean of (gpu - f64) / unit to
half of the gentlest such shift (bf16x3_emu.min_mutant_bias, computed on the CPU).  P4 is the column edge: conv_filter_size 1056
leaves a fifth column tile 32 wide.  The float64 reference is evaluated on a subset of utterances (the first, the last, the ones
holding the first and the last row-tile boundary, one in the middle); replica and finiteness cover all rows.

L1, L2 (full-row tile) and T1 (plain tile + k_layernorm at N = 512) take the GPU's own hidden / attention tensor as the input of the
contraction under test and hold LayerNorm(gemm + x) to the first-order bound of tests/bf16_emu.py gemm_ln_check at FP32_REL.
LayerNorm cancels a uniform relative bias, so the six terms are proven on the plain forms; L1 and L2 prove the ROWEPI epilogue (the
tile parked in the weight-plane buffers, masked rows), which shares the `compute` body.

Measured on one MI355X (profiles/bf16x3_ops.md).  As the kernel stood — all six MFMAs of a K block fed the running accumulator —
the three same-sign cases at K = 2304 failed on both plain tiles: P1 1.73, P4 1.67, Q2 1.71 x the bound, every element SHORT, signed
mean -3.7e-6 of the unit against an allowance of 3.5e-6, while the CPU emulation of that order with nearest-even fp32 adds
(bf16x3_emu.kernel_order_fp32) sits at 0.51 x and +3e-8 on the same data: late in a long contraction the matrix core aligns the
small products away against the accumulator.  The kernel now sums the terms of each K block from zero and adds the block's sum to
the total on the VALU (all six terms on the 128 x 256 and the full-row tile, all but hi*hi on the 256 x 256 tile, which has no
registers for more): P1 0.23, P4 0.25, Q2 0.38 x the bound, signed mean -4.5e-8 (the three dropped products' own).  The other
cases: random-sign 0.011 ... 0.028 x, same-sign at K = 256 0.085 (128 x 256) and 0.15 (256 x 256), LayerNorm forms 0.011 ... 0.040
of their bound.  Against a library with the lo*hi MFMA removed, or with the weight's mid and lo planes exchanged, all five
same-sign cases fail (2.1 ... 2.6 x, signed mean -7.3e-6 or worse) while the whole-model parity test still passes.

Every case reports torch's fp32 CPU figure beside the GPU's (reported, not gated).  NS_FP32_OPS_REPORT=<path> appends every figure
to a JSON-lines file (profiles/bf16x3_ops.md was written from one).  Inf / NaN operands are out of scope (the split makes an Inf a
NaN through Inf - Inf)."""
import numpy as np
import pytest
import torch

import tests.test_gpu_bf16_ops as BO
from tests import bf16_emu as E
from tests import bf16x3_emu as X
from tests.util import report as _report
from tests.util import weights_for

pytestmark = pytest.mark.gpu

REL = E.FP32_REL
METAS = {"tiny": BO.METAS["tiny"], "tiny512": dict(config="tiny512", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25)}
SAME_SIGN_LAYERS = [X.L0 + ".pos_ffn.w_1", X.L0 + ".slf_attn.qkv"]
_MODELS = {}


def models(config, same=False, fp32=False):
    """(cfg, state dict as tensors, {mode: model}), each built once.  same: |w| and |b| in the layers of the same-sign cases."""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    key = (config, same)
    if key not in _MODELS:
        if config == X.TINY1056:
            cfg = wl.model_config("tiny")
            cfg["transformer"]["conv_filter_size"] = X.D_INNER[config]
            sd = wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25)
        else:
            cfg, sd = weights_for(METAS[config])
        if same:
            over = {}
            for name in SAME_SIGN_LAYERS:
                over.update(X.same_sign_weights(sd, name))
            sd = dict(sd, **over)
        _MODELS[key] = (cfg, sd, {})
    cfg, sd, ms = _MODELS[key]
    for mode in ("bf16x3",) + (("fp32",) if fp32 else ()):
        if mode not in ms:
            m = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul=mode)).to("cuda").eval()
            m.load_state_dict(sd)
            ms[mode] = m
    return cfg, {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, ms


def _form(plan, then_layernorm=False):
    return f"{plan[0]}x{plan[1]}" + (" full-row" if plan[2] else "") + f" {plan[3]} workgroups" + (" + k_layernorm" if then_layernorm else "")


PLAIN = [(c, v) for c in X.PLAIN_CASES for v in (("random-sign", "same-sign") if c[7] else ("random-sign",))]


@pytest.mark.parametrize("case,variant", PLAIN, ids=lambda v: v if isinstance(v, str) else v[0])
def test_plain_form_elementwise_replica_and_signed_mean(case, variant):
    from smart_nar_fast_tts_amd import ops

    label, name, config, B, S, BM, tiles, _ = case
    same = variant == "same-sign"
    cfg, sd, ms = models(config, same)
    mb3 = ms["bf16x3"]
    assert mb3._cfg.matmul_bf16x3 == 1
    w, b, act = BO.contraction(cfg, sd, name)
    Cin, N, KW = X.shape_of(name, config)
    assert (w.shape[1], w.shape[0], w.shape[2]) == (Cin, N, KW) == ops.gemm_shape(mb3, name)
    plan = ops.plan_gemm_b3(B * S, N, Cin, KW)
    assert plan == (BM, 256, 0, tiles[0] * tiles[1]), "a threshold of the dispatch moved: tests/test_bf16x3_ops_host.py says where to"
    x = BO._x(B, S, Cin, seed=B * S + N)
    if same:
        x = X.same_sign(x)
        assert bool((w >= 0).all()) and bool((b >= 0).all()) and act in (None, "relu")  # (ReLU is the identity on these sums)
    x[B - 1] = x[0]
    got = ops.gemm(mb3, name, x.cuda()).cpu()
    finite = bool(torch.isfinite(got).all())
    replica = torch.equal(got[B - 1], got[0])
    utts = X.judged_utterances(B, S, BM)
    xs, gs = x[utts], got[utts]
    ref, unit = E.gemm_emu(xs, w, b, act=act, round_fn=E.exact), E.gemm_unit(xs, w, b, round_fn=E.exact)
    res = E.gemm_check(gs, xs, w, b, act=act, rel=REL, ref=ref, unit=unit)
    y32 = E.gemm_emu(xs, w, b, act=act, dtype=torch.float32, round_fn=E.exact)
    cpu = E.gemm_check(y32, xs, w, b, act=act, rel=REL, ref=ref, unit=unit)
    row = dict(test="b3_gemm", case=label, variant=variant, form=_form(plan), name=name, config=config, Cin=Cin, N=N, KW=KW, B=B, S=S, judged=utts,
               gpu_over_bound=res.worst, cpu_fp32_over_bound=cpu.worst, replica_bits=replica, finite=finite)
    if same:
        floor = X.min_mutant_bias()
        row.update(gpu_signed_mean=X.signed_mean(gs, ref, unit), cpu_fp32_signed_mean=X.signed_mean(y32, ref, unit), min_mutant_bias=floor)
    _report(**row)
    assert finite
    assert replica, f"{label} {variant}: the copy of utterance 0 differs in {int((got[B - 1] != got[0]).sum())} values"
    assert res.ok, f"{label} {variant} {_form(plan)}: {res.worst:.3g} x the fp32 bound (torch fp32 on the CPU: {cpu.worst:.3g} x)"
    if same:
        assert abs(row["gpu_signed_mean"]) <= floor / 2, (f"{label} {_form(plan)}: signed mean {row['gpu_signed_mean']:.3g} of the unit, a lost term starts at "
                                                          f"{floor:.3g} (torch fp32 on the CPU: {row['cpu_fp32_signed_mean']:.3g})")


@pytest.mark.parametrize("case,op,config,B,S,form", X.LN_CASES, ids=lambda v: v if isinstance(v, str) and len(v) == 2 else None)
def test_layernorm_form_elementwise(case, op, config, B, S, form):
    """LayerNorm(w_2(hid) + x) with hid = the GPU's own relu(w_1(x)) (ffn), LayerNorm(fc(att) + x) with att = the GPU's own attention
    of its own QKV projection under ragged lengths, 1 and S among them (mha): every row against float64"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, ms = models(config)
    mb3 = ms["bf16x3"]
    d, H = cfg["transformer"]["decoder_hidden"], cfg["transformer"]["decoder_head"]
    M = B * S
    K = d if op == "mha" else X.D_INNER[config]
    plan = ops.plan_gemm_b3(M, d, K, 1, 1)
    assert plan == form, "a threshold of the dispatch moved: tests/test_bf16x3_ops_host.py says where to"
    x = BO._x(B, S, d, seed=M + d + K)
    lens = torch.tensor(X.ragged_lens(B, S))
    if op == "ffn":
        p = X.L0 + ".pos_ffn"
        a = ops.gemm(mb3, p + ".w_1", x.cuda()).cpu()
        got = ops.positionwise_ffn(mb3, p, x.cuda()).cpu()
        w, b, _ = BO.contraction(cfg, sd, p + ".w_2")
    else:
        p = X.L0 + ".slf_attn"
        qkv = ops.gemm(mb3, p + ".qkv", x.cuda())
        a = ops.attention_core(qkv, lens.cuda(), H, split_scratch="workspace").cpu()
        got = ops.multi_head_attention(mb3, p, x.cuda(), lens.cuda()).cpu()
        w, b, _ = BO.contraction(cfg, sd, p + ".fc")
    assert (w.shape[1], w.shape[0], w.shape[2]) == (K, d, 1)
    g, beta = sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"]
    res = E.gemm_ln_check(got, a, w, b, x, g, beta, rel=REL, round_fn=E.exact)
    z32 = E.gemm_emu(a, w, b, dtype=torch.float32, round_fn=E.exact) + x
    cpu = E.gemm_ln_check(E.layernorm_emu(z32, g, beta, dtype=torch.float32), a, w, b, x, g, beta, rel=REL, round_fn=E.exact)
    _report(test="b3_" + op + "_ln", case=case, form=_form(plan, not plan[2]), config=config, Cin=K, N=d, B=B, S=S, gpu_over_bound=res.worst,
            cpu_fp32_over_bound=cpu.worst)
    assert res.ok, f"{case} {op} {config} B={B} S={S} {_form(plan, not plan[2])}: {res} (torch fp32 on the CPU: {cpu.worst:.3g})"


def test_full_row_tile_masks_rows_exactly():
    """fft_block masks both LayerNorms (L1's and L2's launches, both on the full-row tile): rows at t >= lens[b] are exactly zero, valid
    rows finite and non-zero"""
    from smart_nar_fast_tts_amd import ops

    _, _, config, B, S, form = X.LN_CASES[0]
    cfg, sd, ms = models(config)
    d = cfg["transformer"]["decoder_hidden"]
    assert all(ops.plan_gemm_b3(B * S, d, K, 1, 1) == form and form[2] == 1 for K in (d, X.D_INNER[config]))
    x = BO._x(B, S, d, seed=S + d + 2).cuda()
    lens = torch.tensor(X.ragged_lens(B, S)).cuda()
    valid = (torch.arange(S, device="cuda")[None, :] < lens[:, None])[:, :, None]
    got = ops.fft_block(ms["bf16x3"], X.L0, x, lens)
    assert bool((got.masked_select(~valid.expand_as(got)) == 0).all())
    live = got.masked_select(valid.expand_as(got)).reshape(-1, d)
    assert bool(torch.isfinite(live).all()) and bool((live != 0).any(dim=1).all())
    _report(test="b3_masked_rows", case="L1+L2", form=_form(form), config=config, B=B, S=S, masked_rows=int((~valid).sum()), valid_rows=int(valid.sum()))


def test_handover_to_fp32_is_at_200_tiles():
    """w_1 at 19 x 330 rows is 49 x 4 = 196 tiles: the mode stays out and the bf16x3 model's output is the fp32 model's, bit for bit;
    at 19 x 331 (200 tiles) the mode runs and some bit differs"""
    from smart_nar_fast_tts_amd import ops

    name, config, B, S0, S1 = X.HANDOVER
    cfg, sd, ms = models(config, fp32=True)
    Cin, N, KW = X.shape_of(name, config)
    same_bits = {}
    for S in (S0, S1):
        x = BO._x(B, S, Cin, seed=S).cuda()
        same_bits[S] = torch.equal(ops.gemm(ms["bf16x3"], name, x), ops.gemm(ms["fp32"], name, x))
        _report(test="b3_handover", name=name, config=config, B=B, S=S, form="fp32" if ops.plan_gemm_b3(B * S, N, Cin, KW) is None else _form(ops.plan_gemm_b3(B * S, N, Cin, KW)),
                same_bits_as_fp32_model=same_bits[S])
    assert ops.plan_gemm_b3(B * S0, N, Cin, KW) is None and ops.plan_gemm_b3(B * S1, N, Cin, KW) == (128, 256, 0, 200)
    assert same_bits == {S0: True, S1: False}, same_bits
