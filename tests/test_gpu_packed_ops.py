"""Every launch that runs on PACKED rows (csrc/kernels.h RowMap: the default layout of the synchronous forwards) ALONE on the
MI355X, against the float64 / numpy restatements of tests/packed_cpu.py.  tests/test_packed_ops_host.py holds the case tables,
proves on the CPU which launch form each case takes (ns_plan_attention_packed, ns_plan_gemm_launches) and that each restatement
rejects the wrong versions that matter; here the kernels are held to the same restatements:

  plan            every int of the device plan equals the numpy plan (the two unused ints keep the buffer's fill)
  GEMM            elementwise at FP32_REL through gemm_check over every packed row, guard rows included; the four rows before (then after) every
                  window edge are 1e3, so a tap leaking either way is >= 1e7 x the bound; a two-launch cut plan with the cut inside
                  the last window; the copy of utterance 0 (at a row offset
                  that is no multiple of 16 / 32 / 48) carries utterance 0's bits
  GEMM + LN       through the packed ffn / mha entries with the mask on: gemm_ln_check on the valid rows, exact zeros at
                  t >= lens[b]; the fft block is the bits of the two in sequence
  bf16 model      the same at the gates of tests/test_gpu_bf16_ops.py
  attention       the three packed forms x d_k 128 / 64 / 32 against float64 at 2e-5 (5e-5 with a spiked late key), NaN exactly on
                  the zero-length utterance's rows, split against single sweep within 1e-5, the copy's bits
  data movement   bit for bit against numpy on inputs of distinct values

Every figure is also reported next to torch's fp32 CPU evaluation of the same inputs (reported, not gated);
NS_PACKED_OPS_REPORT=<path> appends them to a JSON-lines file (profiles/packed_ops.md was written from one)."""
import numpy as np
import pytest
import torch

import tests.test_gpu_bf16_ops as BO
import tests.test_packed_ops_host as H
from tests import bf16_emu as E
from tests import packed_cpu as PC
from tests.test_gpu_rowops import duration_case
from tests.util import reporter, weights_for

pytestmark = pytest.mark.gpu

REL = E.FP32_REL
FILL = -7
METAS = dict(BO.METAS, tiny512=dict(config="tiny512", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25))
_MODELS, _SD = {}, {}


_report = reporter("NS_PACKED_OPS_REPORT")


def model(config, mode="fp32", row_epilogue="fused"):
    """(cfg, state dict as tensors, model) of a config in one precision / row_epilogue mode; one config's models at a time"""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    if config not in _SD:
        _SD.clear()
        _MODELS.clear()
        cfg, sd = weights_for(METAS[config])
        _SD[config] = (cfg, sd, {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    cfg, sd, sdt = _SD[config]
    if (mode, row_epilogue) not in _MODELS:
        m = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul=mode, row_epilogue=row_epilogue)).to("cuda").eval()
        m.load_state_dict(sd)
        _MODELS[(mode, row_epilogue)] = m
    return cfg, sdt, _MODELS[(mode, row_epilogue)]


def _by_config(cases, at=1):
    return sorted(cases, key=lambda c: ["tiny", "tiny512"].index(c[at]))


def plans(set_name, heads):
    """(the numpy plan, the device plan) of a length set"""
    from smart_nar_fast_tts_amd import ops

    S, lens, guard = H.SETS[set_name]
    return PC.plan_ref(lens, S, heads, guard), ops.pack_plan(lens, S, heads, guard, device="cuda", fill=FILL)


def _replica(got, p):
    return torch.equal(got[int(p.off[-2]):], got[:int(p.win[0])])


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("S,lens,guard,heads", H.PLAN_CASES, ids=lambda v: None if isinstance(v, list) else str(v))
def test_plan_every_int(S, lens, guard, heads):
    from smart_nar_fast_tts_amd import ops

    p = PC.plan_ref(lens, S, heads, guard)
    d = ops.pack_plan(lens, S, heads, guard, device="cuda", fill=FILL)
    assert (d.Mp, d.att_wgs) == (p.Mp, p.att_wgs)
    got = d.plan.cpu().numpy()
    assert got.shape == p.ints(FILL).shape and np.array_equal(got, p.ints(FILL)), np.nonzero(got != p.ints(FILL))[0][:8]
    for name in ("off", "win", "att_off", "att_order", "row_b", "row_t", "row_w"):
        assert np.array_equal(d.section(name).cpu().numpy(), getattr(p, name))


# ---------------------------------------------------------------------------------------------------- plain GEMM
def _gemm_case(config, mode, suffix, set_name, rel, round_fn):
    from smart_nar_fast_tts_amd import ops

    cfg, sd, m = model(config, mode)
    name = H.gemm_name(suffix, set_name)
    w, b, act = BO.contraction(cfg, sd, name)
    p, d = plans(set_name, 2)
    for side in ("tail", "head"):  # 1e3 in the four rows before / after every window edge: a leak in either direction reads it
        x = H.x_packed(p, w.shape[1], seed=p.Mp + w.shape[0], spike=1e3, side=side)
        got = ops.gemm_packed(m, name, x.cuda(), d).cpu()
        ref, unit = PC.gemm_packed_ref(x, w, b, p, act, round_fn), PC.gemm_packed_unit(x, w, b, p, round_fn)
        res = PC.gemm_packed_check(got, x, w, b, p, act, rel, round_fn, ref, unit)
        cpu = PC.gemm_packed_check(PC.gemm_packed_ref(x, w, b, p, act, round_fn, dtype=torch.float32), x, w, b, p, act, rel, round_fn, ref, unit)
        replica = _replica(got, p)
        _report(test="gemm", mode=mode, name=name, config=config, set=set_name, side=side, Mp=p.Mp, Cin=w.shape[1], N=w.shape[0], KW=w.shape[2],
                gpu_over_bound=res.worst, cpu_fp32_over_bound=cpu.worst, replica_bits=replica)
        assert bool(torch.isfinite(got).all())
        assert replica, f"{name} {set_name} {side}: the copy of utterance 0 differs in {int((got[int(p.off[-2]):] != got[:int(p.win[0])]).sum())} values"
        assert res.ok, f"{name} {config} {set_name} {side} ({mode}): {res.worst:.3g} x the bound (torch fp32 on the CPU: {cpu.worst:.3g} x)"


@pytest.mark.parametrize("suffix,config,set_name,forms", _by_config(H.GEMM_CASES), ids=lambda v: None if isinstance(v, list) else str(v))
def test_gemm_packed_elementwise_and_replica_bits(suffix, config, set_name, forms):
    import tests.test_fp32_ops_host as T

    assert [l[:7] for l in T.launches(H.plan_of(set_name).Mp, T.shape_of(H.gemm_name(suffix, set_name), config))] == forms
    _gemm_case(config, "fp32", suffix, set_name, REL, E.exact)


BF16_GEMM = [(s, "tiny", n) for n in ("dec256", "dec64") for s in (H._Q, H._FC, H._W1, H._W2, "mel_linear", "postnet.convolutions.1", "postnet.convolutions.0")] + [
    (H._W1, "tiny", "dec1300"), ("postnet.convolutions.4", "tiny", "dec1300x7")]


@pytest.mark.parametrize("suffix,config,set_name", BF16_GEMM)
def test_gemm_packed_bf16_model(suffix, config, set_name):
    """the bf16 GEMM has the same row_t / row_w lookup: the gate of tests/test_gpu_bf16_ops.py (GEMM_REL on rounded operands)"""
    _gemm_case(config, "bf16", suffix, set_name, E.GEMM_REL, E.bf)


# ---------------------------------------------------------------------------------------------------- GEMM + LayerNorm
def _ln_case(op, config, set_name, mode, row_epilogue, rel, round_fn):
    from smart_nar_fast_tts_amd import ops

    cfg, sd, m = model(config, mode, row_epilogue)
    enc = set_name == "pho33"
    d_model = cfg["transformer"]["encoder_hidden" if enc else "decoder_hidden"]
    heads = cfg["transformer"]["encoder_head" if enc else "decoder_head"]
    p, d = plans(set_name, heads)
    lens = torch.tensor(p.lens)
    x = H.x_packed(p, d_model, seed=p.Mp + d_model)
    L = H.layer(set_name)
    if op == "ffn":
        a = ops.gemm_packed(m, L + ".pos_ffn.w_1", x.cuda(), d).cpu()
        sub = L + ".pos_ffn"
        w, b, _ = BO.contraction(cfg, sd, sub + ".w_2")
    else:
        qkv = ops.gemm_packed(m, L + ".slf_attn.qkv", x.cuda(), d)
        a = ops.attention_core_packed(qkv, lens.cuda(), d, split="block", bf16=(mode == "bf16" and not enc)).cpu()
        sub = L + ".slf_attn"
        w, b, _ = BO.contraction(cfg, sd, sub + ".fc")
    got = ops.block_packed(m, op, L, x.cuda(), lens.cuda(), d, mask_rows=True).cpu()
    g, beta = sd[sub + ".layer_norm.weight"], sd[sub + ".layer_norm.bias"]
    valid = PC.valid_rows(p)
    assert bool(torch.isfinite(a[valid]).all())
    a0 = torch.where(valid[:, None], a, torch.zeros(()))  # (attention rows of a zero-length utterance are NaN; they are masked rows)
    res = PC.gemm_ln_packed_check(got, a0, w, b, x, g, beta, p, rel, round_fn, rows=valid)
    cpu = PC.gemm_ln_packed_check(PC.ln_packed_ref(round_fn(a0), round_fn(w), b, x, g, beta, p, dtype=torch.float32), a0, w, b, x, g, beta, p, rel, round_fn, rows=valid)
    _report(test=op + "_ln", mode=mode, row_epilogue=row_epilogue, config=config, set=set_name, Mp=p.Mp, Cin=w.shape[1], N=d_model,
            gpu_over_bound=res.worst, cpu_fp32_over_bound=cpu.worst)
    assert bool((got[~valid] == 0).all()), "rows at t >= lens[b] must be exactly zero"
    assert bool((got[valid] != 0).any())
    assert res.ok, f"{op} {config} {set_name} {mode} {row_epilogue}: {res} (torch fp32 on the CPU: {cpu.worst:.3g})"
    assert _replica(got, p)


@pytest.mark.parametrize("op,config,set_name,row_epilogue,form", _by_config(H.LN_CASES), ids=str)
def test_layernorm_packed_elementwise_and_masked_rows(op, config, set_name, row_epilogue, form):
    _ln_case(op, config, set_name, "fp32", row_epilogue, REL, E.exact)


@pytest.mark.parametrize("op,set_name,full_row", H.BF16_LN_CASES)
def test_layernorm_packed_bf16_model(op, set_name, full_row):
    """plain bf16 GEMM + k_layernorm on the row maps below the full-row threshold, the 64 x 256 LayerNorm tile at 13 057 rows"""
    from smart_nar_fast_tts_amd import ops

    assert ops.plan_gemm_bf16_ln(H.plan_of(set_name).Mp, 256, 1024 if op == "ffn" else 256) == full_row
    _ln_case(op, "tiny", set_name, "bf16", "fused", E.GEMM_REL, E.bf)


@pytest.mark.parametrize("config,set_name,row_epilogue", _by_config(H.MASKED_CASES, 0))
def test_fft_block_packed_masks_rows_and_is_its_two_halves(config, set_name, row_epilogue):
    from smart_nar_fast_tts_amd import ops

    cfg, sd, m = model(config, "fp32", row_epilogue)
    enc = set_name == "pho33"
    d_model = cfg["transformer"]["encoder_hidden" if enc else "decoder_hidden"]
    p, d = plans(set_name, cfg["transformer"]["encoder_head" if enc else "decoder_head"])
    lens = torch.tensor(p.lens).cuda()
    x = H.x_packed(p, d_model, seed=p.Mp + 3).cuda()
    valid = PC.valid_rows(p).cuda()
    got = ops.block_packed(m, "fft", H.layer(set_name), x, lens, d)
    assert bool((got[~valid] == 0).all()) and bool(torch.isfinite(got).all()) and bool((got[valid] != 0).any())
    x1 = ops.block_packed(m, "mha", H.layer(set_name), x, lens, d, mask_rows=True)
    want = ops.block_packed(m, "ffn", H.layer(set_name), x1, lens, d, mask_rows=True)
    assert torch.equal(got, want) and _replica(got.cpu(), p)


# ---------------------------------------------------------------------------------------------------- attention
def _qkv(p, heads, dk, seed, scale=1.0):
    torch.manual_seed(seed)
    qkv = torch.randn(p.Mp, 3 * heads * dk) * scale
    qkv[int(p.off[-2]):] = qkv[:int(p.win[0])]
    return qkv


def _attention(qkv, p, d, split, tickets, tol, label, dk):
    from smart_nar_fast_tts_amd import ops

    got = ops.attention_core_packed(qkv.cuda(), torch.tensor(p.lens).cuda(), d, split=split, tickets=tickets).cpu()
    ref = PC.attention_packed_ref(qkv, p, H.ATT_H)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan) and bool(torch.isfinite(got[~nan]).all()) and bool(nan.any())
    err = float((got.double() - ref).abs()[~nan].max())
    cpu = float((PC.attention_packed_ref(qkv, p, H.ATT_H, dtype=torch.float32).double() - ref).abs()[~nan].max())
    replica = _replica(torch.nan_to_num(got), p)
    _report(test="attention", label=label, dk=dk, Mp=p.Mp, split=bool(split), tickets=bool(tickets), gpu_max_abs_err=err, cpu_fp32_max_abs_err=cpu,
            tol=tol, replica_bits=replica)
    assert err < tol, (label, err, cpu)
    assert replica, "the copy of utterance 0 must carry its bits (same window, same key tiles, same split, merges in key order)"
    return got


@pytest.mark.parametrize("dk", H.ATT_DK)
@pytest.mark.parametrize("name,split,tickets,form,ranges,merge", H.ATT_CASES)
def test_attention_packed_vs_float64(name, split, tickets, form, ranges, merge, dk):
    f, nsplit, mg, _ = H.att_plan(name, dk, split, tickets)
    assert (H.STRIPS if f == 0 else (H.LIST_SPLIT if nsplit > 1 else H.LIST), nsplit > 1, mg) == (form, ranges, merge)
    p, d = plans(name, H.ATT_H)
    _attention(_qkv(p, H.ATT_H, dk, seed=p.Mp + dk), p, d, split, tickets, 2e-5, f"{name} {form}", dk)


@pytest.mark.parametrize("dk", H.ATT_DK)
@pytest.mark.parametrize("name", ["dec256", "dec1300"])
def test_attention_packed_split_equals_single_sweep_and_spiked_key(name, dk):
    """key ranges + merge (last arriver, merge launch) against the single sweep on the same input within 1e-5; then one key of the
    longest utterance far above the rest in a LATE range (the reference point of the online softmax must move there), at 5e-5"""
    p, d = plans(name, H.ATT_H)
    qkv = _qkv(p, H.ATT_H, dk, seed=dk + 1)
    outs = [_attention(qkv, p, d, s, t, 2e-5, f"{name} split={s} tickets={t}", dk) for s, t in ((True, True), (True, False), (False, False))]
    for o in outs[:2]:
        assert float((torch.nan_to_num(o) - torch.nan_to_num(outs[2])).abs().max()) < 1e-5
    u = int(np.argmax(p.keys()))                       # the longest utterance; its copy is spiked with it
    key = int(p.keys()[u]) - 40                        # in its last key range but one tile
    dm = H.ATT_H * dk
    qkv = _qkv(p, H.ATT_H, dk, seed=dk + 2, scale=0.5)
    for v in {u, p.B - 1 if u == 0 else u}:
        o = int(p.off[v])
        qkv[o + key, dm:dm + dk] = 6.0   # head 0's key: its score stands far above every other key's
        qkv[o:o + int(p.win[v]), :dk] += 1.0
    for s, t in ((True, True), (False, False)):
        _attention(qkv, p, d, s, t, 5e-5, f"{name} spiked split={s}", dk)


@pytest.mark.parametrize("name,split", [("dec256", True), ("dec64", True), ("dec1300", True), ("dec1300", False)])
def test_attention_packed_bf16_mode(name, split):
    """the BF = true kernels on packed rows at the gate of tests/test_gpu_bf16_ops.py (attention_check: the fp32 tier plus budgeted
    flips of the rounded P)"""
    from smart_nar_fast_tts_amd import ops

    dk = 128
    p, d = plans(name, H.ATT_H)
    qkv = _qkv(p, H.ATT_H, dk, seed=p.Mp)
    got = ops.attention_core_packed(qkv.cuda(), torch.tensor(p.lens).cuda(), d, split=split, bf16=True).cpu()
    live, parts = [], []
    for u, xw in enumerate(PC.windows(qkv, p)):
        n = int(p.keys()[u])
        gw = PC.windows(got, p)[u]
        if n == 0:
            assert bool(torch.isnan(gw).all())
            continue
        assert bool(torch.isfinite(gw).all())
        live.append(gw)
        parts.append(E.attention_emu(xw[None], torch.tensor([n]), H.ATT_H))
    ref, unit, flip = (torch.cat([t[i] for t in parts], dim=1) for i in range(3))
    res = E.attention_check(torch.cat(live)[None], ref, unit, flip, H.ATT_H)
    _report(test="attention_bf16", label=name, split=split, worst_flips=res.worst_flips, worst_over_fp32_tier=res.worst_fp32, pair_share=res.pair_share)
    assert res.ok, str(res)
    assert _replica(torch.nan_to_num(got), p)


# ---------------------------------------------------------------------------------------------------- data movement
def _distinct(shape, seed, lo=1.0):
    n = int(np.prod(shape))
    return torch.from_numpy((np.random.RandomState(seed).permutation(n).astype(np.float32) + lo).reshape(shape))


@pytest.mark.parametrize("L,D,T_len,heads", [(9, 4, 40, 2), (300, 256, 900, 2), (33, 260, 120, 8)])
def test_length_regulate_packed_bits_row_maps_and_status(L, D, T_len, heads):
    """durations of tests/test_gpu_rowops.py duration_case: utterance 1 has a total of 0, utterance 0 a total above T (cut, status
    bit 0); mel_lens is the total, with one utterance reported as -1 (a bad token: status bit 1, window = the guard)"""
    from smart_nar_fast_tts_amd import ops

    B = 4
    dur = duration_case(B, L, seed=L + D)
    dur[0] = dur[0].abs() + (T_len / L + 1)
    cnt = np.maximum(dur.numpy().astype(np.int64), 0)
    cum = torch.from_numpy(np.cumsum(cnt, axis=1).astype(np.int32))
    mel_lens = [int(v) for v in cnt.sum(axis=1)]
    assert mel_lens[0] > T_len and mel_lens[1] == 0 and 0 < mel_lens[2] < T_len - 20
    mel_lens[3] = -1
    x = _distinct((B, L, D), seed=D)
    out, status, d = ops.length_regulate_packed(x.cuda(), cum.cuda(), torch.tensor(mel_lens).cuda(), T_len, heads, fill=FILL)
    p = PC.plan_ref(mel_lens, T_len, heads, 20)
    want, want_status = PC.length_regulate_packed_ref(x, cum, mel_lens, T_len, p)
    assert np.array_equal(d.plan.cpu().numpy(), p.ints(FILL))
    assert torch.equal(status.cpu(), want_status) and want_status.tolist()[:2] == [1, 0] and want_status[3] & 2
    assert torch.equal(_bits(out.cpu()), _bits(want)) and bool((want != 0).any())


@pytest.mark.parametrize("D", [4, 256, 260])
def test_embed_pos_add_pos_pack_vector_bits(D):
    from smart_nar_fast_tts_amd import ops

    S, lens, guard = H.SETS["pho33"]
    p = PC.plan_ref(lens, S, 2, guard)
    n_vocab = 50
    rs = np.random.RandomState(D)
    texts = torch.from_numpy(rs.randint(0, n_vocab, size=(p.B, S)).astype(np.int64))
    texts[0, 3], texts[1, 0], texts[2, 1] = n_vocab, -1, n_vocab + 1000  # out of the vocabulary: row 0 (inside windows)
    emb, pos = _distinct((n_vocab, D), 1), _distinct((S + 3, D), 2, lo=-5000.0)
    d = ops.pack_plan(lens, S, 2, guard, device="cuda", fill=FILL)
    d.plan[4 * p.B + 4:] = FILL  # the row maps are this kernel's to write (the forward runs it behind launch_pack_plan_only)
    got = ops.embed_pos_packed(texts.cuda(), emb.cuda(), pos.cuda(), d)
    assert np.array_equal(d.plan.cpu().numpy(), p.ints(FILL))
    assert torch.equal(_bits(got.cpu()), _bits(PC.embed_pos_packed_ref(texts, emb, pos, p)))
    for set_name in ("pho33", "dec256"):
        S, lens, guard = H.SETS[set_name]
        p, d = plans(set_name, 2)
        x, pos = _distinct((p.Mp, D), 3), _distinct((S, D), 4, lo=0.5)
        assert torch.equal(_bits(ops.add_pos_packed(x.cuda(), pos.cuda(), d).cpu()), _bits(PC.add_pos_ref(x, pos, p)))
        src = _distinct((p.B, S), 5)
        assert torch.equal(_bits(ops.pack_vector(src.cuda(), d).cpu()), _bits(PC.pack_vector_ref(src, p)))


@pytest.mark.parametrize("D", [1, 6, 8, 256, 260])
@pytest.mark.parametrize("set_name", ["pho33", "dec64"])
def test_unpack_rows_and_phase1_bits(set_name, D):
    from smart_nar_fast_tts_amd import ops

    p, d = plans(set_name, 2)
    src = _distinct((p.Mp, D), D)
    lens = torch.tensor(p.lens)
    for ln in (None, lens):
        got = ops.unpack_rows(src.cuda(), None if ln is None else ln.cuda(), d).cpu()
        assert torch.equal(_bits(got), _bits(PC.unpack_rows_ref(src, ln, p)))
    if D % 4 == 0:
        vec = _distinct((p.Mp,), D + 1)
        rows, v = ops.unpack_phase1(src.cuda(), vec.cuda(), lens.cuda(), d)
        want_rows, want_v = PC.unpack_phase1_ref(src, vec, lens, p)
        assert torch.equal(_bits(rows.cpu()), _bits(want_rows)) and torch.equal(_bits(v.cpu()), _bits(want_v))


@pytest.mark.parametrize("with_pe", [True, False])
@pytest.mark.parametrize("T_len,n_mel", [(64, 80), (45, 4), (300, 80)])
def test_unpack_outputs_bits(T_len, n_mel, with_pe):
    """the case of tests/test_packed_ops_host.py outputs_case (w == T, w < T with frames in all three PostNet regions and both sides
    of each boundary, a zero and a negative length), at T = 64 as proven there and at two more axis lengths"""
    from smart_nar_fast_tts_amd import ops

    lens = (30, 44, 33, 0, 64, 45, -2, 30) if T_len == 64 else (T_len - 34, T_len - 20, T_len - 31, 0, T_len + 5, T_len - 19, -2, T_len - 34)
    p, ln, mel_p, post_p, p_p, e_p, bias, const = H.outputs_case(T_len, n_mel, lens)
    if not with_pe:
        p_p = e_p = None
    d = ops.pack_plan(list(lens), T_len, 2, 20, device="cuda")
    c = lambda t: None if t is None else t.cuda()  # noqa: E731
    got = ops.unpack_outputs(d, ln.cuda(), c(mel_p), c(post_p), c(p_p), c(e_p), c(bias), c(const), mask=with_pe)
    want = PC.unpack_outputs_ref(p, ln, mel_p, post_p, p_p, e_p, bias, const)
    b, ln0 = 0, lens[0]
    assert p.win[b] < T_len and ln0 + 10 < T_len - 10  # frames on both sides of t = len + 10 and t = T - 10 in utterance 0
    for g, w, what in zip(got[:4], want[:4], ("mel", "postnet", "p", "e")):
        assert (g is None) == (w is None), what
        if g is not None:
            assert torch.equal(_bits(g.cpu()), _bits(w)), (what, torch.nonzero((g.cpu() != w).reshape(p.B, T_len, -1).any(dim=2))[:6].tolist())
    if with_pe:
        assert torch.equal(got[4].cpu(), want[4])
    else:
        assert got[4] is None
