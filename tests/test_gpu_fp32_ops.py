"""Every launch form of the exact-fp32 Conv1D-as-GEMM (csrc/gemm_conv.hip k_conv_gemm, the default path) ALONE on the MI355X
against a float64 evaluation of the same contraction, elementwise: |gpu - f64| <= 4e-6 * (conv(|x|, |w|) + |bias|) (the gate is
proven on the CPU in tests/test_fp32_ops_host.py, which also holds the case table and asserts, through ns_plan_gemm_launches, that
every form launch_conv_gemm_impl can dispatch is one of these cases or a reasoned entry of UNREACHED).  Plain forms run through
ops.gemm on inputs the test supplies; the last utterance of every input is a copy of the first and the two outputs must be the
same BITS (one GEMM sums all its rows in one order, cut plans included: a row- or tile-position-dependent error shows there even
below any tolerance).  LayerNorm forms — full-row tiles and the ticketed ladder — run through ops.positionwise_ffn and
ops.multi_head_attention on the GPU's own hidden / attention input, so only the one contraction plus LayerNorm is under test.

Every case also reports the same figure for torch's fp32 CPU evaluation of the same inputs (reported, not gated): what "as close to
float64 as the reference's own fp32" means per kernel form.  NS_FP32_OPS_REPORT=<path> appends every figure (form, shape, GPU and
CPU-fp32 worst ratios) to a JSON-lines file, from which a per-form table under profiles/ is written."""
import pytest
import torch

import tests.test_fp32_ops_host as T
import tests.test_gpu_bf16_ops as BO
from tests import bf16_emu as E
from tests.util import report as _report

pytestmark = pytest.mark.gpu

REL = E.FP32_REL
METAS = dict(BO.METAS, tiny512=dict(config="tiny512", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25))
_MODELS = {}


def models(config):
    """(cfg, state dict as tensors, fp32 model), each config built once"""
    if config not in _MODELS:
        cfg, sd, (m32,) = BO._build(METAS[config], modes=("fp32",))
        _MODELS[config] = (cfg, sd, m32)
    return _MODELS[config]


def _by_config(cases):
    return sorted(cases, key=lambda c: ["tiny", "tiny512", "ljspeech", "d512"].index(c[1]))


def _form_str(forms):
    return " + ".join(f"{f[0]}x{f[1]}" + (f" BK{f[2]}" if f[2] != 32 else "") + (f" KS{f[3]}" if f[3] > 1 else "") + (" MF16" if f[4] == 16 else "")
                      + (" full-row" if f[5] else "") + (f" ticket{256 * f[6]}" if f[6] else "") for f in forms)


@pytest.mark.parametrize("name,config,B,S,forms,utts", _by_config(T.GEMM_CASES), ids=lambda v: None if isinstance(v, list) else str(v))
def test_gemm_form_elementwise_and_replica_bits(name, config, B, S, forms, utts):
    from smart_nar_fast_tts_amd import ops

    cfg, sd, m32 = models(config)
    w, b, act = BO.contraction(cfg, sd, name)
    assert (w.shape[1], w.shape[0], w.shape[2]) == T.shape_of(name, config) == ops.gemm_shape(m32, name)
    assert [l[:7] for l in T.launches(B * S, T.shape_of(name, config))] == forms
    x = BO._x(B, S, w.shape[1], seed=B * S + w.shape[0])
    x[B - 1] = x[0]
    got = ops.gemm(m32, name, x.cuda()).cpu()
    finite = bool(torch.isfinite(got).all())
    replica = torch.equal(got[B - 1], got[0])
    xs, gs = (x, got) if utts is None else (x[utts], got[utts])  # (utterances are independent: zero padding per utterance)
    ref, unit = E.gemm_emu(xs, w, b, act=act, round_fn=E.exact), E.gemm_unit(xs, w, b, round_fn=E.exact)
    res = E.gemm_check(gs, xs, w, b, act=act, rel=REL, ref=ref, unit=unit)
    cpu = E.gemm_check(E.gemm_emu(xs, w, b, act=act, dtype=torch.float32, round_fn=E.exact), xs, w, b, act=act, rel=REL, ref=ref, unit=unit)
    _report(test="gemm", form=_form_str(forms), name=name, config=config, Cin=w.shape[1], N=w.shape[0], KW=w.shape[2], B=B, S=S,
            gpu_err_over_unit=res.worst * REL, cpu_fp32_err_over_unit=cpu.worst * REL, gpu_over_bound=res.worst, replica_bits=replica, finite=finite)
    assert finite
    assert replica, f"{name} B={B} S={S} {_form_str(forms)}: the copy of utterance 0 differs in {int((got[B - 1] != got[0]).sum())} values"
    assert res.ok, f"{name} B={B} S={S} {_form_str(forms)}: {res.worst:.3g} x the fp32 bound (torch fp32 on the CPU: {cpu.worst:.3g} x)"


def _layer(config):
    return f"mel_decoder.layer_stack.{T.LAST_LAYER[config]}"


@pytest.mark.parametrize("op,config,B,S,form", _by_config(T.LN_CASES), ids=str)
def test_layernorm_form_elementwise(op, config, B, S, form):
    """LayerNorm(w_2(hid) + x) with hid = the GPU's own relu(w_1(x)) (ffn), LayerNorm(fc(att) + x) with att = the GPU's own attention
    of its own QKV projection (mha): the first-order bound of tests/bf16_emu.py gemm_ln_check at FP32_REL"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, m32 = models(config)
    d, H = cfg["transformer"]["decoder_hidden"], cfg["transformer"]["decoder_head"]
    M = B * S
    (l,) = T.launches(M, (d if op == "mha" else T.D_INNER, d, 1), T.ln_epi(M))
    assert l[:7] == form
    x = BO._x(B, S, d, seed=M + d)
    lens = torch.tensor(T._lens(B, S))
    if op == "ffn":
        p = _layer(config) + ".pos_ffn"
        a = ops.gemm(m32, p + ".w_1", x.cuda()).cpu()
        got = ops.positionwise_ffn(m32, p, x.cuda()).cpu()
        w, b, _ = BO.contraction(cfg, sd, p + ".w_2")
    else:
        p = _layer(config) + ".slf_attn"
        qkv = ops.gemm(m32, p + ".qkv", x.cuda())
        a = ops.attention_core(qkv, lens.cuda(), H, split_scratch="workspace").cpu()
        got = ops.multi_head_attention(m32, p, x.cuda(), lens.cuda()).cpu()
        w, b, _ = BO.contraction(cfg, sd, p + ".fc")
    g, beta = sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"]
    res = E.gemm_ln_check(got, a, w, b, x, g, beta, rel=REL, round_fn=E.exact)
    z32 = E.gemm_emu(a, w, b, dtype=torch.float32, round_fn=E.exact) + x
    cpu = E.gemm_ln_check(E.layernorm_emu(z32, g, beta, dtype=torch.float32), a, w, b, x, g, beta, rel=REL, round_fn=E.exact)
    _report(test=op + "_ln", form=_form_str([form]), config=config, Cin=w.shape[1], N=d, B=B, S=S, gpu_over_bound=res.worst, cpu_fp32_over_bound=cpu.worst)
    assert res.ok, f"{op} {config} B={B} S={S} {_form_str([form])}: {res} (torch fp32 on the CPU: {cpu.worst:.3g})"


@pytest.mark.parametrize("config,B,S", T.MASKED_ROW_CASES)
def test_masked_rows_are_exactly_zero(config, B, S):
    """fft_block masks both LayerNorms: rows at t >= lens[b] are exactly zero, on the full-row tile and on the ticketed ladder"""
    from smart_nar_fast_tts_amd import ops

    cfg, sd, m32 = models(config)
    d = cfg["transformer"]["decoder_hidden"]
    forms = {T.launches(B * S, (K, d, 1), T.ln_epi(B * S))[0][:7] for K in (d, T.D_INNER)}
    assert all(f[5] == 1 for f in forms) if T.ln_epi(B * S) == 1 else all(f[6] > 0 for f in forms)
    x = BO._x(B, S, d, seed=S + d + 2).cuda()
    lens = torch.tensor(T._lens(B, S)).cuda()
    valid = (torch.arange(S, device="cuda")[None, :] < lens[:, None])[:, :, None]
    got = ops.fft_block(m32, _layer(config), x, lens)
    assert bool((got.masked_select(~valid.expand_as(got)) == 0).all())
    assert bool(torch.isfinite(got).all()) and bool((got.masked_select(valid.expand_as(got)) != 0).any())
