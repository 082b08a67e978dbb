"""The two launches of a VariancePredictor ALONE on the MI355X against float64, per row of tests/test_predictor_ops_host.py
PRED_CASES (that file proves the gates on the CPU and checks the table against the dispatch): every form the two contractions take
under their row epilogues — full-row heights 32 / 48 / 80 / 112, the four ticketed rungs, the two-launch form — at 256- and
512-wide models, with ragged lengths, a partial last row tile, utterances shorter than the kernel's reach and one of length 0.

Stage 1, ops.predictor_conv1 on inputs the test supplies: layer_norm_1(relu(conv1d_1(x))), elementwise at FP32_REL through
bf16_emu.gemm_ln_check(act="relu", resid=None).  Stage 2, ops.predictor_tail on the GPU's OWN h (one contraction plus its epilogue
under test): pred against float64 at PRED_TIGHT x the first-order bound, for control in {1, 0.5, 1.7}, with and without a target;
masked rows bitwise +0.0; x_out the BITS of fp32 (x_in + emb[bucketize(stored pred or target)]) + pos[t] on every row, with and
without the position add; outputs pre-filled with NaN; the last utterance a copy of the first and carrying its bits; below the
full-row threshold the two-launch model's outputs equal the fused model's bit for bit.

Every case reports the GPU's and torch's fp32 CPU share of the gate (NS_FP32_OPS_REPORT=<path> appends them to a JSON-lines file;
profiles/predictor_ops.md was written from one)."""
import pytest
import torch

import tests.test_fp32_ops_host as T
import tests.test_predictor_ops_host as P
from tests import bf16_emu as E
from tests.test_gpu_fp32_ops import _form_str
from tests.util import report as _report
from tests.util import weights_for

pytestmark = pytest.mark.gpu

_MODELS = {}
NAN = float("nan")


def model(config, row_epilogue="fused"):
    """the fp32 model of a config in one row_epilogue mode; one config's models at a time"""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    if (config, row_epilogue) not in _MODELS:
        if not any(k[0] == config for k in _MODELS):
            _MODELS.clear()
        cfg, sd = weights_for(P.METAS[config])
        m = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul="fp32", row_epilogue=row_epilogue)).to("cuda").eval()
        m.load_state_dict(sd)
        _MODELS[(config, row_epilogue)] = m
    return _MODELS[(config, row_epilogue)]


def _prefix(which):
    return f"variance_adaptor.{which}_predictor"


def _pos_rows(w, S, d):
    """the decoder position rows the forward adds for S frames: the cached parameter up to max_seq_len, the regenerated table beyond"""
    from smart_nar_fast_tts_amd import ops

    if S <= w["max_seq_len"]:
        return w["pos"][:S]
    return ops.sinusoid_table(S, d).cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tail(m, which, h, lens, B, S, d, control=1.0, target=None, x_in=None, add_pos=False):
    """ops.predictor_tail into NaN-filled outputs, back on the CPU"""
    from smart_nar_fast_tts_amd import ops

    pred = torch.full((B, S), NAN, device="cuda")
    x_out = None if x_in is None else torch.full((B, S, d), NAN, device="cuda")
    ops.predictor_tail(m, _prefix(which), h, lens, control=control, target=target, x_in=x_in, add_pos=add_pos, pred=pred, x_out=x_out)
    return pred.cpu(), (None if x_out is None else x_out.cpu())


@pytest.mark.parametrize("which", ["pitch", "energy", "duration"])
@pytest.mark.parametrize("case", P.by_config(P.PRED_CASES), ids=P.case_id)
def test_predictor_launches_alone_vs_float64(case, which):
    from smart_nar_fast_tts_amd import ops

    config, B, S, _, mode, forms1, forms2 = case
    M, d = B * S, T.D_MODEL[config]
    epi = 0 if mode == "two_launch" else T.ln_epi(M)
    assert [l[:7] for l in T.launches(M, (d, P.F, 3), epi)] == forms1 and [l[:7] for l in T.launches(M, (P.F, P.F, 3), epi)] == forms2
    m = model(config, mode)
    other = model(config, "two_launch") if mode == "fused" and M < 6369 else None
    w = P.pred_weights(config, which)
    lens_l = P.lens_of(case)
    lens = torch.tensor(lens_l)
    x = P.x_of(B, S, d, seed=M + d + len(which))
    xd, ld = x.cuda(), lens.cuda()
    what = f"{P.case_id(case)} {which} {_form_str(forms2)}"

    # ---- stage 1 on the test's x
    hd = ops.predictor_conv1(m, _prefix(which), xd)
    h = hd.cpu()
    s1 = P.stage1_check(h, x, w)
    s1_cpu = P.stage1_check(P.stage1(x, w, torch.float32), x, w)
    replica1 = torch.equal(_bits(h[B - 1]), _bits(h[0]))
    print(f"{what}: stage 1 gpu {s1.worst:.3g} x bound (torch fp32 on the CPU {s1_cpu.worst:.3g}), replica bits {replica1}")
    if other is not None:
        assert torch.equal(_bits(ops.predictor_conv1(other, _prefix(which), xd).cpu()), _bits(h)), f"{what}: stage 1 two-launch != fused bits"

    # ---- stage 2 on the GPU's own h
    reff, boundf = P.tail_ref(h, w, [S] * B)  # every row valid, control 1; pred and its bound scale with the control
    dead = ~(torch.arange(S)[None, :] < lens[:, None])
    ref, bound = reff.masked_fill(dead, 0.0), boundf.masked_fill(dead, 0.0)
    cpu = E.pred_check(P.tail_fp32(h, w, lens_l), ref, bound, P.PRED_TIGHT)
    emb = which != "duration"
    if emb:
        pos = _pos_rows(w, S, d)
        target = P.targets_of(w["bins"], B, S, seed=M)
        runs = [(1.0, None, False), (0.5, None, True), (1.7, target, True), (1.7, target, False), (0.5, target, False), (1.7, None, False)]
    else:
        runs = [(1.0, None, False), (0.5, None, False), (1.7, None, False)]
    worst = 0.0
    fails = []
    for control, tgt, add_pos in runs:
        c = 1.0 if tgt is not None else control
        kw = dict(control=control, target=None if tgt is None else tgt.cuda(), x_in=xd if emb else None, add_pos=add_pos)
        pred, x_out = _tail(m, which, hd, ld, B, S, d, **kw)
        tag = f"control {control} target {tgt is not None} add_pos {add_pos}"
        res = E.pred_check(pred, ref * c, bound * c, P.PRED_TIGHT)
        worst = max(worst, res.worst)
        print(f"{what} {tag}: pred gpu {res.worst:.3g} x gate")
        if not res.ok:
            fails.append(f"{tag}: pred {res.worst:.3g} x gate (torch fp32 on the CPU {cpu.worst:.3g})")
        if not bool((_bits(pred)[dead] == 0).all()):
            fails.append(f"{tag}: a masked pred is not +0.0")
        if emb:
            want = P.embed_ref(x, pred if tgt is None else tgt, w["bins"], w["emb"], pos if add_pos else None)
            if not torch.equal(_bits(x_out), _bits(want)):
                bad = (_bits(x_out) != _bits(want)).any(dim=-1)
                fails.append(f"{tag}: x_out differs from (x_in + emb[idx]) + pos on {int(bad.sum())} rows, first (b, t) = {bad.nonzero()[0].tolist()}, "
                             f"columns {(_bits(x_out) != _bits(want))[bad][0].nonzero().flatten().tolist()[:4]}")
        if other is not None:
            p2, x2 = _tail(other, which, hd, ld, B, S, d, **kw)
            if not torch.equal(_bits(p2), _bits(pred)) or (emb and not torch.equal(_bits(x2), _bits(x_out))):
                fails.append(f"{tag}: two-launch != fused bits")

    # ---- the copy of utterance 0 carries its bits (every row valid, so that every row of the two is compared)
    full = torch.full((B,), S, dtype=torch.long)
    predf, xf = _tail(m, which, hd, full.cuda(), B, S, d, x_in=xd if emb else None, add_pos=emb)
    replica2 = torch.equal(_bits(predf[B - 1]), _bits(predf[0])) and (not emb or torch.equal(_bits(xf[B - 1]), _bits(xf[0])))
    resf = E.pred_check(predf, reff, boundf, P.PRED_TIGHT)
    worst = max(worst, resf.worst)
    if emb and not torch.equal(_bits(xf), _bits(P.embed_ref(x, predf, w["bins"], w["emb"], pos))):
        fails.append("every row valid: x_out differs from (x_in + emb[idx]) + pos")
    buckets = int(torch.bucketize(predf, w["bins"]).unique().numel()) if emb else 0

    _report(test="predictor", which=which, case=P.case_id(case), config=config, B=B, S=S, mode=mode, form1=_form_str(forms1), form2=_form_str(forms2),
            stage1_gpu_over_bound=s1.worst, stage1_cpu_fp32_over_bound=s1_cpu.worst, pred_gpu_share=worst * P.PRED_TIGHT,
            pred_cpu_fp32_share=cpu.worst * P.PRED_TIGHT, pred_gpu_over_gate=worst, buckets=buckets, replica_bits=bool(replica1 and replica2),
            failures=len(fails))
    assert bool(torch.isfinite(h).all()) and s1.ok, f"{what}: stage 1 {s1} (torch fp32 on the CPU: {s1_cpu.worst:.3g})"
    assert replica1, f"{what}: stage 1, the copy of utterance 0 differs in {int((_bits(h[B - 1]) != _bits(h[0])).sum())} values"
    assert resf.ok, f"{what}: every row valid: pred {resf.worst:.3g} x gate"
    assert replica2, f"{what}: stage 2, the copy of utterance 0 differs"
    assert not fails, f"{what}: " + "; ".join(fails)
