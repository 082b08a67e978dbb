"""Driver-run evidence (-m gpu) for the parts of the path whose failure would be rare and silent:

* the TICKETED last-arriver epilogues (csrc/gemm_conv.hip TICKET, csrc/attention.hip k_attention_strip): LayerNorm /
  predictor tails / attention's key-range merge of small grids run inside the producing launch, published with
  write-through stores + one relaxed fetch_add and read back with sc1 loads, no fence.  A stale read would be a 1-in-N
  wrong LayerNorm row.  Checked here (a) against the two-launch form of the same arithmetic, bit for bit
  (``model_config["row_epilogue"] = "two_launch"`` never draws a ticket), and (b) under load: hundreds of forwards on four
  HIP streams, every output bit-identical to the first.
  What is protected: ``layer_norm(output + residual)`` (transformer/SubLayers.py:57,93), the predictor tail
  (model/modules.py:273-286), softmax(QK^T)V (transformer/Modules.py:14-25).
* random shapes: a fixed-seed slice of tests/fuzz_gpu.py (packed rows, both length regulators, d_k 32 / 64 / 128) against
  the oracle, so that the fuzz evidence is a driver-run test and not only a text record under profiles/.
"""
import types

import pytest
import torch

from tests.util import dev, load_golden, weights_for

pytestmark = pytest.mark.gpu

NAMES = ["mel", "postnet_mel", "p_pred", "e_pred", "log_d", "d_rounded", "src_masks", "mel_masks", "src_lens", "mel_lens"]


def build(cfg, sd, **extra):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    m = FastSpeech2Align(wl.preprocess_config(), dict(cfg, **extra)).to("cuda").eval()
    m.load_state_dict(sd)
    return m


def same(a, b, what):
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        assert a[i].shape == b[i].shape, (what, NAMES[i], a[i].shape, b[i].shape)
        x, y = a[i], b[i]
        if x.dtype.is_floating_point:  # NaN rows of an empty utterance: same place, same bits elsewhere
            assert torch.equal(torch.isnan(x), torch.isnan(y)), (what, NAMES[i])
            x, y = torch.nan_to_num(x), torch.nan_to_num(y)
        assert torch.equal(x, y), (what, NAMES[i], float((x.float() - y.float()).abs().max()))


def test_ticketed_epilogues_match_the_two_launch_form_bit_for_bit():
    import smart_nar_fast_tts_amd.workload as wl

    cases = []
    meta, z = load_golden("e2e_tiny_padded_src")
    cfg, sd = weights_for(meta)
    cases.append(("e2e_tiny_padded_src", cfg, sd, (z["speakers"], z["texts"], z["in_src_lens"], int(meta["L"]))))
    cfg1 = wl.model_config("ljspeech")
    sd1 = wl.synth_state_dict(cfg1, seed=0, frames_per_phoneme=8.0)
    cases.append(("cfg1_single", cfg1, sd1, wl.synth_inputs(1, 100, seed=0)))
    cases.append(("ragged batch of 5", cfg1, sd1, wl.synth_inputs(5, 64, seed=3, src_lens=[64, 9, 33, 50, 17])))
    cases.append(("ragged batch of 3, short", cfg1, sd1, wl.synth_inputs(3, 20, seed=4, src_lens=[20, 13, 7])))
    # the ladder's 48-row rungs (16-row family): 18 x 128 = 2304 encoder rows take the ticketed 48 x 64 K-split tile, 5 x ~1010 decoder
    # rows the ticketed 32 x 128 one while other launches of the same forwards run on the family's tiles
    cases.append(("uniform batch of 18", cfg1, sd1, wl.synth_inputs(18, 128, seed=6)))
    cases.append(("uniform batch of 5", cfg1, sd1, wl.synth_inputs(5, 128, seed=7)))
    # dense decoder attention with the planner's key split (B = 9: 3 ranges, B = 17: 4): the last range to arrive merges inside
    # k_attention (round 6) — against split-key k_attention + k_attention_merge, which the two-launch form still takes
    cases.append(("uniform batch of 9", cfg1, sd1, wl.synth_inputs(9, 128, seed=8)))
    cases.append(("uniform batch of 17", cfg1, sd1, wl.synth_inputs(17, 128, seed=9)))
    # a long single utterance: few workgroups, up to 16 key ranges through k_attention (the strip kernel declines > 4 tiles per wave)
    sd31 = wl.synth_state_dict(cfg1, seed=0, frames_per_phoneme=31.0)
    cases.append(("3 long utterances", cfg1, sd31, wl.synth_inputs(3, 100, seed=10)))
    built = {}
    for name, cfg, sd, inp in cases:
        key = id(sd)
        if key not in built:
            built.clear()
            built[key] = (build(cfg, sd), build(cfg, sd, row_epilogue="two_launch"))
        fused, two = built[key]
        a = [dev(x) for x in inp[:3]]
        with torch.no_grad():
            for packed in (True, False):
                fused.packed_rows = two.packed_rows = packed
                same(fused(a[0], a[1], a[2], inp[3]), two(a[0], a[1], a[2], inp[3]), f"{name} ({'packed' if packed else 'grid'})")


def test_500_forwards_on_four_streams_are_bit_identical_to_the_first():
    """Config 1 (one utterance, 55 launches, 22 of them ticketed) 500 times, round-robin on four HIP streams so that ticketed
    launches of different forwards overlap on the chip; plus a small ragged batch the same way."""
    import smart_nar_fast_tts_amd.workload as wl

    cfg = wl.model_config("ljspeech")
    m = build(cfg, wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=8.0))
    streams = [torch.cuda.Stream() for _ in range(4)]
    for what, inp, n in (("cfg1_single", wl.synth_inputs(1, 100, seed=0), 500),
                         ("ragged batch of 4", wl.synth_inputs(4, 48, seed=9, src_lens=[48, 11, 30, 22]), 200)):
        a = [dev(x) for x in inp[:3]]
        with torch.no_grad():
            ref = m(a[0], a[1], a[2], inp[3])
            torch.cuda.synchronize()
            bad = [torch.zeros((), dtype=torch.long, device="cuda") for _ in streams]
            for i in range(n):
                s = i % len(streams)
                with torch.cuda.stream(streams[s]):
                    o = m(a[0], a[1], a[2], inp[3])
                    for j in (0, 1, 2, 3, 4, 5):
                        bad[s] += (o[j] != ref[j]).sum()
                    bad[s] += (o[9] != ref[9]).sum()
            torch.cuda.synchronize()
        assert sum(int(b) for b in bad) == 0, (what, [int(b) for b in bad])


def test_fuzz_slice_vs_oracle():
    """38 random cases (~50 s): tiny / tiny512 / tiny_h4 models (d_k 128 / 64 / 32), both feature levels, both
    length regulators, control factors, ragged batches (most of them on packed rows), plus a few large batches that take the
    full-row tiles and the step-aware plan."""
    from tests import fuzz_gpu

    # (a fixed number of cases; the time limits are a safety net sized for a box whose host cores run the oracle at half the usual
    #  speed — round 5 met one: 23 of 44 cases in the old 55 s box — not what decides how many cases are compared)
    small = fuzz_gpu.run(types.SimpleNamespace(iters=32, seed=4, matmul="fp32", big=False), max_seconds=240)
    big = fuzz_gpu.run(types.SimpleNamespace(iters=6, seed=5, matmul="fp32", big=True), max_seconds=180)
    assert small["checked"] + small["skipped"] == 32 and small["checked"] >= 25 and small["packed"] >= 8, small
    assert big["checked"] + big["skipped"] == 6 and big["checked"] >= 4, big
    for r in (small, big):
        assert r["worst"]["mel"] < 1e-3 and r["worst"]["postnet"] < 1e-3, r


def test_two_host_threads_each_with_their_own_model():
    """include/nar_fs2.h THREADING: one ns_model serves one host thread at a time, DIFFERENT models are independent.  Two host
    threads (ctypes releases the GIL inside the native calls, so the launch sequences really interleave), each with its own
    model instance on its own HIP stream, 150 forwards each of different batches: every output bit-identical to what the same
    model gave single-threaded."""
    import threading

    import smart_nar_fast_tts_amd.workload as wl

    cfg = wl.model_config("ljspeech")
    sd = wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=8.0)
    jobs = [(build(cfg, sd), wl.synth_inputs(1, 100, seed=0)), (build(cfg, sd), wl.synth_inputs(3, 40, seed=8, src_lens=[40, 12, 27]))]
    refs = []
    for m, inp in jobs:
        a = [dev(x) for x in inp[:3]]
        with torch.no_grad():
            refs.append(m(a[0], a[1], a[2], inp[3]))
    torch.cuda.synchronize()
    errors, bad = [], [0, 0]

    def work(k):
        try:
            m, inp = jobs[k]
            st = torch.cuda.Stream()
            a = [dev(x) for x in inp[:3]]
            acc = torch.zeros((), dtype=torch.long, device="cuda")
            with torch.no_grad(), torch.cuda.stream(st):
                for _ in range(150):
                    o = m(a[0], a[1], a[2], inp[3])
                    for j in (0, 1, 2, 3, 4, 5, 9):
                        acc += (o[j] != refs[k][j]).sum()
            st.synchronize()
            bad[k] = int(acc)
        except Exception as e:  # surfaced below: an exception in a thread must fail the test
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    assert bad == [0, 0], bad
