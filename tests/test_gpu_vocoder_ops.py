"""Every launch form of the vocoder's implicit GEMM ALONE on the MI355X, past the first row tile, against a float64 evaluation of
the same launch, elementwise, for the fp32 kernel (csrc/vocoder.hip k_voc_gemm) and the bf16 one (csrc/vocoder_bf16.hip
k_voc_gemm_bf16, against the float64 evaluation of its emulation).  The launch, the gate |gpu - f64| <= REL * (conv(|a|, |W|) +
|bias|) + E and the table of cases are tests/vocoder_ops.py; the gate is proven on the CPU both ways, and the table's geometry (three
row tiles or more, a partial last one, a tile boundary inside an utterance, an utterance boundary inside a later tile) asserted, in
tests/test_vocoder_ops_host.py.

Asserted in every case: the gate at every element; the copy of utterance 0 in the last slot carries utterance 0's BITS (a row- or
tile-position-dependent error shows there below any tolerance); everything finite.  Reported in every case: the worst ratio to the
bound, and the same figure for torch's fp32 evaluation on the CPU (not gated here).  NS_VOC_OPS_REPORT=<path> appends every figure
to a JSON-lines file, from which profiles/vocoder_ops_r12.md is written."""
import pytest
import torch

from tests import vocoder_ops as V
from tests.util import reporter

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::FutureWarning")]

_GENS = {}


def gen(mode):
    if mode not in _GENS:
        from smart_nar_fast_tts_amd.vocoder import Generator

        h, sd, _ = V.model()
        g = Generator(h, matmul=mode).to("cuda").eval()
        g.load_state_dict(sd)
        _GENS[mode] = g
    return _GENS[mode]


_report = reporter("NS_VOC_OPS_REPORT")


def _judge(c, got, x, resid, acc):
    """the three assertions and the report of one case; got on the CPU"""
    h = V.model()[0]
    L = V.launch_of(c)
    ref = V.evaluate(L, x, resid, acc)
    assert got.shape == ref.out.shape, (got.shape, ref.out.shape)
    finite = bool(torch.isfinite(got).all())
    replica = torch.equal(got[c.B - 1], got[0])
    res = V.check(got, ref)
    cpu = V.check(V.evaluate(L, x, resid, acc, dtype=torch.float32).out, ref)
    Sg, N, K = V.grid(h, c)
    g = V.geometry(c.mode, N, c.B, Sg)
    _report(test=c.kind, form=c.form, stage=c.stage, mode=c.mode, B=c.B, S=c.S, N=N, K=K, tile=f"{g['BM']}x{g['BN']}", rows=g["M"],
            row_tiles=g["tiles"], gpu_over_bound=res.worst, cpu_fp32_over_bound=cpu.worst, replica_bits=replica, finite=finite)
    assert finite, f"{c.id}: {int((~torch.isfinite(got)).sum())} values are not finite"
    assert replica, f"{c.id}: the copy of utterance 0 differs in {int((got[c.B - 1] != got[0]).sum())} values"
    assert res.ok, f"{c.id}: {res} (torch fp32 on the CPU: {cpu.worst:.3g})"


@pytest.mark.parametrize("c", V.PLAIN_CASES, ids=lambda c: c.id)
def test_plain_form_past_one_tile(c):
    """ns_voc_op_conv (input lrelu, no output lrelu, no residual, no MRF) on one resblock conv per tile width (C = 256, 128, 64,
    32) and per (k, d) extreme"""
    x, _, _ = V.inputs(c)
    got = gen(c.mode).op_conv(V.FORMS[c.form].name(c.stage), x.cuda()).cpu()
    _judge(c, got, x, None, None)


@pytest.mark.parametrize("c", V.EPILOGUE_CASES, ids=lambda c: c.id)
def test_every_epilogue_form(c):
    """ns_voc_op_conv_form: c1, a middle c2, the last c2 with mrf 0 / 1 / 2 — what stage() launches — and lrelu + residual, at the
    widest tile (stage 0) and the narrowest (stage 3)"""
    f = V.FORMS[c.form]
    x, resid, acc = V.inputs(c)
    on = lambda t: None if t is None else t.cuda()  # noqa: E731
    acc_gpu = on(acc)
    got = gen(c.mode).op_conv_form(f.name(c.stage), x.cuda(), in_act=f.in_act, out_act=f.out_act, residual=on(resid), mrf=f.mrf,
                                   acc=acc_gpu).cpu()
    if acc is not None:
        assert torch.equal(acc_gpu.cpu(), acc), "the wrapper clones acc into the output: acc itself is not written"
    _judge(c, got, x, resid, acc)


@pytest.mark.parametrize("c", V.UP_CASES, ids=lambda c: c.id)
def test_upsampler_past_one_tile(c):
    """ns_voc_op_upsample into an output poisoned with NaN: the store shifted by -u/2 rows and clipped to the utterance writes
    every element of [B, S u, C / 2], past row 128 / 256 of the grid too"""
    h = V.model()[0]
    u, ch = h["upsample_rates"][c.stage], V.channels(h, c.stage)
    x, _, _ = V.inputs(c)
    out = torch.full((c.B, c.S * u, ch), float("nan"), device="cuda")
    got = gen(c.mode).op_upsample(c.stage, x.cuda(), out=out)
    assert got is out and got.shape == (c.B, c.S * u, ch)
    _judge(c, got.cpu(), x, None, None)
