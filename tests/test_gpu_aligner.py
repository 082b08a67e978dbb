"""Reference-mel aligner on the GPU: the cross-attention kernel alone against float64 under the elementwise gate that
tests/test_aligner_host.py proves both ways, ``model.align`` against the float64 evaluation of the imported reference (fixtures of
tests/golden/make_golden_aligner.py), the duration kernel — on the GPU's own maps and, alone, on maps crafted for its argmax, tie rule
and length handling —, the input kernel alone, and the forward's independence from it."""
import numpy as np
import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from smart_nar_fast_tts_amd import ops
from smart_nar_fast_tts_amd.model import FastSpeech2Align
from tests import aligner_cpu as ac
from tests.util import dev, load_golden

pytestmark = pytest.mark.gpu

QUERY_BLOCK = 64   # queries per workgroup of k_cross_attention (two waves of 32 rows)
KEY_STRIP = 32     # keys per strip
FIXTURES = ("aligner_tiny", "aligner_T_above_1000")

_CACHE = {}


def aligned(name):
    """(meta, z, cfg, model, AlignOutput on the fixture's inputs), computed once per fixture."""
    if name not in _CACHE:
        meta, z = load_golden(name)
        if "model" not in _CACHE:  # both fixtures share config and seeds
            cfg, sd = ac.fixture_weights(meta)
            m = FastSpeech2Align(wl.preprocess_config(), cfg).to("cuda").eval()
            m.load_state_dict(sd)
            _CACHE["model"] = (cfg, m, (meta["config"], meta["weight_seed"], meta["aligner_seed"]))
        cfg, m, key = _CACHE["model"]
        assert key == (meta["config"], meta["weight_seed"], meta["aligner_seed"])
        out = m.align(dev(z["texts"]), dev(z["src_lens"]), int(meta["L"]), dev(z["mels"]), dev(z["mel_lens"]))
        torch.cuda.synchronize()
        _CACHE[name] = (meta, z, cfg, m, out)
    return _CACHE[name]


@pytest.mark.parametrize("peak", [1.0, 8.0], ids=["flat", "peaky"])
@pytest.mark.parametrize("H,dk", [(2, 128), (4, 64)])
def test_cross_attention_against_float64(H, dk, peak):
    """ops.cross_attention alone (transformer/Modules.py:14-25 with the key-only mask) under tests/aligner_cpu.attention_gate:
    T = 1 and one query block + 5; L = 1, 7, one key strip, one strip + 1, two strips + 2; B = 3 ragged (src_len = L, 1 and L // 2)
    plus a replica of utterance 0 placed last, which must carry the same bits; masked columns exactly 0."""
    g = torch.Generator().manual_seed(11)
    d = H * dk
    for T in (1, QUERY_BLOCK + 5):
        for L in (1, 7, KEY_STRIP, KEY_STRIP + 1, 2 * KEY_STRIP + 2):
            lens = torch.tensor([L, 1, max(1, L // 2), L])
            q = torch.randn(3, T, d, generator=g) * peak
            kv = torch.randn(3, L, 2 * d, generator=g)
            q, kv = torch.cat([q, q[:1]]), torch.cat([kv, kv[:1]])
            ctx, attn = ops.cross_attention(q.cuda(), kv.cuda(), lens.cuda(), H)
            torch.cuda.synchronize()
            ctx, attn = ctx.cpu(), attn.cpu()
            assert ctx.shape == (4, T, d) and attn.shape == (4, H, T, L)
            rp, rc = ac.attention_gate(q, kv, lens, H, ctx, attn)
            print(f"H {H} dk {dk} T {T} L {L} peak {peak}: {rp:.3f} of the probability bound, {rc:.3f} of the output bound")
            assert rp <= 1.0 and rc <= 1.0, (T, L, rp, rc)
            assert torch.equal(attn[3], attn[0]) and torch.equal(ctx[3], ctx[0]), (T, L, "replica differs")
            for b in range(4):
                assert (attn[b, :, :, int(lens[b]):] == 0).all(), (T, L, b, "masked key is not exactly 0")
            assert float((attn.sum(-1) - 1).abs().max()) < 1e-5


def test_empty_source_is_nan_for_that_utterance_only():
    """src_len == 0: softmax over a row of -inf — NaN for that utterance, like the reference (transformer/Modules.py:20-23) and like
    k_attention; the neighbours stay finite and inside the gate."""
    g = torch.Generator().manual_seed(5)
    H, dk, T, L = 2, 128, 37, 40
    lens = torch.tensor([L, 0, 3])
    q, kv = torch.randn(3, T, H * dk, generator=g), torch.randn(3, L, 2 * H * dk, generator=g)
    ctx, attn = ops.cross_attention(q.cuda(), kv.cuda(), lens.cuda(), H)
    ctx, attn = ctx.cpu(), attn.cpu()
    assert torch.isnan(attn[1]).all() and torch.isnan(ctx[1]).all()
    assert torch.isfinite(attn[[0, 2]]).all() and torch.isfinite(ctx[[0, 2]]).all()
    rp, rc = ac.attention_gate(q, kv, lens, H, ctx, attn, skip=(1,))
    assert rp <= 1.0 and rc <= 1.0, (rp, rc)
    dur = ops.aligner_durations(attn.cuda(), lens.cuda(), torch.tensor([T, T, 20]).cuda()).cpu().numpy()
    assert dur.sum(axis=1).tolist() == [T, 0, 20]


def _stats(d):
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    return {"max": float(d.max()), "p999": float(np.quantile(d, 0.999))}


@pytest.mark.parametrize("name", FIXTURES)
def test_align_against_float64(name):
    """model.align on the fixture's inputs: every layer's alignment and tgt_output, every stored row — padded query rows included —
    against the imported reference cast to .double().  Rule of test_accuracy_against_float64 (tests/test_gpu_parity.py): maximum and
    p99.9 distance <= 1.5 x the fp32 reference's own distance from float64 (stored in the fixture), with that test's floors for
    quantities of order 1 where both sides sit at a few ulp (4e-7 for a probability, 1e-6 for the LayerNorm output)."""
    meta, z, cfg, m, out = aligned(name)
    assert len(out.tgt_alignment) == meta["n_layer"]
    assert out.durations.dtype == torch.long and tuple(out.durations.shape) == (meta["B"], meta["L"])
    rows = slice(None) if meta["rows"] is None else np.asarray(meta["rows"])
    got = out.tgt_output.cpu().numpy()
    assert got.shape == (meta["B"], meta["T"], 256)
    checks = [("tgt_output", _stats(np.abs(got[:, rows] - z["tgt_output_f64"])), meta["tgt_dist"], 1e-6)]
    for i, (a, a64) in enumerate(zip(out.tgt_alignment, ac.fixture_alignments(name, meta, z, "_f64"))):
        assert tuple(a.shape) == a64.shape
        checks.append((f"alignment {i}", _stats(np.abs(a.cpu().numpy() - a64)), meta["attn_dist"][i], 4e-7))
    worst = 0.0
    for what, hip, ref, floor in checks:
        for stat in ("p999", "max"):
            print(f"{name} {what:12s} {stat:5s} |HIP - f64| {hip[stat]:.3e}   |reference-fp32 - f64| {ref[stat]:.3e}   ratio {hip[stat] / ref[stat]:.2f}")
            worst = max(worst, hip[stat] / ref[stat])
            assert hip[stat] <= max(1.5 * ref[stat], floor), (name, what, stat, hip[stat], ref[stat])
    print(f"{name}: worst ratio {worst:.2f}")
    # padded keys hold exactly 0, padded frames of tgt_output are zero (transformer/Layers.py:65,68)
    sl, ml = z["src_lens"], z["mel_lens"]
    for b in range(meta["B"]):
        assert (out.tgt_alignment[-1][b, :, :, int(sl[b]):] == 0).all()
        assert (out.tgt_output[b, int(ml[b]):] == 0).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_durations(name):
    """The duration kernel: bit-exact against numpy applied to the GPU's own last-layer alignment; sums to mel_lens; against the
    durations of the fixture's float64 alignment a frame may differ only where the float64 top-two gap is below 1e-6, and at most
    1 % of the frames may."""
    meta, z, cfg, m, out = aligned(name)
    sl, ml = z["src_lens"], z["mel_lens"]
    last = out.tgt_alignment[-1].cpu().numpy()
    dur = out.durations.cpu().numpy()
    assert np.array_equal(dur, ac.durations(last, sl, ml))
    assert np.array_equal(dur.sum(axis=1), ml)
    a64 = ac.head_sum(ac.fixture_alignments(name, meta, z, "_f64")[-1])
    a32 = ac.head_sum(last)
    differ = frames = 0
    for b in range(meta["B"]):
        v64, v32 = a64[b, :ml[b], :sl[b]], a32[b, :ml[b], :sl[b]]
        i64, i32 = v64.argmax(axis=1), v32.argmax(axis=1)
        top2 = np.sort(v64, axis=1)[:, -2:] if sl[b] > 1 else np.stack([np.full(ml[b], -np.inf), v64[:, 0]], axis=1)
        gap = top2[:, 1] - top2[:, 0]
        bad = i64 != i32
        assert (gap[bad] < 1e-6).all(), (name, b, "an argmax differs from float64's where the float64 row has a clear peak")
        differ += int(bad.sum())
        frames += int(ml[b])
    print(f"{name}: {differ} of {frames} frames differ from the float64 argmax")
    assert differ <= 0.01 * frames


def test_forward_and_align_do_not_interfere():
    """A forward() before and after an align() on the same stream returns bit-identical tuples, and align() called twice is
    bit-identical: the aligner has its own arena and workspace."""
    meta, z, cfg, m, first = aligned("aligner_tiny")
    sp, tx, ln, L = wl.synth_inputs(3, 20, seed=2, src_lens=[20, 13, 7])

    def fwd():
        with torch.no_grad():
            o = m(dev(sp), dev(tx), dev(ln), L)
        torch.cuda.synchronize()
        return o

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)

    before = fwd()
    again = m.align(dev(z["texts"]), dev(z["src_lens"]), int(meta["L"]), dev(z["mels"]), dev(z["mel_lens"]), max_mel_len=int(meta["T"]))
    torch.cuda.synchronize()
    after = fwd()
    same(before, after)
    assert torch.equal(first.tgt_output, again.tgt_output) and torch.equal(first.durations, again.durations)
    same(first.tgt_alignment, again.tgt_alignment)
    with pytest.raises(ValueError, match="max_mel_len"):
        m.align(dev(z["texts"]), dev(z["src_lens"]), int(meta["L"]), dev(z["mels"]), dev(z["mel_lens"]), max_mel_len=int(meta["T"]) + 1)
    with pytest.raises(NotImplementedError):
        m(dev(sp), dev(tx), dev(ln), L, mels=dev(z["mels"]), mel_lens=dev(z["mel_lens"]))


# ---- k_aln_durations and k_aln_input alone, on inputs the test crafts ------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("H", [1, 2, 4])
def test_durations_on_crafted_maps(H, L):
    """ns_aln_op_durations alone, bit-exact against aligner_cpu.durations on maps built to hit the wave-level argmax where it can go
    wrong (``aligner_cpu.crafted_map``): ties between lanes, between l and l + 64 of one lane and ties only the head sum creates (lowest key wins),
    the maximum on the last valid key, all-equal and all -inf rows (key 0 wins), larger values, +inf and NaN behind src_len and past
    mel_len (none may count), src_len in {0, 1, L, L + 3, -2}, mel_len in {0, T, T + 4, -1}, B T = 1, 5 and 259 (a partial last
    workgroup of 4 waves), ``out`` pre-filled with garbage.  Valid entries are finite or -inf: a NaN inside the valid region is outside
    the kernel's contract (the aligner's softmax gives none where src_len > 0; where it is 0 nothing is counted)."""
    from smart_nar_fast_tts_amd import _lib

    lib = _lib.load()
    for BT, (B, T) in ac.GRIDS.items():
        a, sl, ml = ac.crafted_map(H, L, B, T, seed=1000 * H + 10 * L + B)
        with np.errstate(invalid="ignore"):
            want = ac.durations(a, sl, ml)
        ad, sd, md = dev(a), dev(sl), dev(ml)
        out = torch.full((B + 1, L), 0x5a5a5a5a5a5a5a5a, dtype=torch.long, device="cuda")
        _lib.check(lib.ns_aln_op_durations(_lib.ptr(ad), _lib.ptr(sd), _lib.ptr(md), B, H, T, L, _lib.ptr(out), _lib.stream_ptr(ad.device)),
                   "aligner_durations")
        got = out.cpu().numpy()
        assert np.array_equal(got[:B], want), (H, L, BT, np.argwhere(got[:B] != want)[:4].tolist())
        assert (got[B] == 0x5a5a5a5a5a5a5a5a).all(), "the row after the last utterance was written"
        frames_of = np.where(np.clip(sl, 0, L) > 0, np.clip(ml, 0, T), 0)
        assert np.array_equal(got[:B].sum(axis=1), frames_of), (H, L, BT)
        assert torch.equal(dev(a).view(torch.int32), ad.view(torch.int32)), "the map was written"
    # what the crafted rows are for, on the largest grid: the tie kinds resolve to the lower key whatever lane holds it
    B, T = ac.GRIDS[259]
    a, sl, ml = ac.crafted_map(H, L, B, T, seed=1000 * H + 10 * L + B)
    with np.errstate(invalid="ignore"):
        s = ac.head_sum(a)
    tied = sum(int((s[b, t, :n] == s[b, t, :n].max()).sum() > 1) for b in range(B) for t in range(int(min(max(ml[b], 0), T)))
               for n in [int(min(max(sl[b], 0), L))] if n > 1)
    assert L == 1 or tied >= 10, "the crafted maps hold tied maxima among the valid keys"


@pytest.mark.parametrize("B,T,C", [(1, 1, 80), (3, 7, 80), (2, 257, 80), (2, 5, 4)])
def test_aligner_input_replaces_frame_zero(B, T, C):
    """k_aln_input alone (ns_aln_op_input): frame 0 of every utterance is exactly +0.0 even where ``mels`` holds NaN or Inf there (a
    replacement, not a product), every other row carries the input's bits (NaN and Inf included), ``mels`` is unchanged and the floats
    after the last element are untouched; C % 4 != 0 and a misaligned pointer are refused."""
    g = torch.Generator().manual_seed(B * 1000 + T)
    mels = torch.randn(B, T, C, generator=g)
    mels[0, 0, 0], mels[B - 1, 0, C - 1], mels[0, 0, 1] = float("nan"), float("inf"), -0.0
    if T > 1:
        mels[0, 1, 0], mels[B - 1, T - 1, C - 1], mels[0, T - 1, 2] = float("nan"), float("-inf"), -0.0
    md = mels.cuda()
    buf = torch.full((B * T * C + 4,), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    x = buf[:B * T * C].view(B, T, C)
    ops.aligner_input(md, x)
    torch.cuda.synchronize()
    got, tail = x.cpu().view(torch.int32), buf[B * T * C:].cpu().view(torch.int32)
    assert (got[:, 0] == 0).all(), "frame 0 is not exactly +0.0"
    assert torch.equal(got[:, 1:], mels.view(torch.int32)[:, 1:]), "a later row does not carry the input's bits"
    assert torch.equal(md.cpu().view(torch.int32), mels.view(torch.int32)), "mels was written"
    assert (tail == -1).all(), "a float after the last element was written"
    with pytest.raises(RuntimeError):   # C % 4 != 0
        ops.aligner_input(md.view(-1)[:B * T * (C - 2)].view(B, T, C - 2), buf[:B * T * (C - 2)].view(B, T, C - 2))
    with pytest.raises(RuntimeError):   # x 4 bytes off a 16-byte boundary
        ops.aligner_input(md, buf[1:B * T * C + 1].view(B, T, C))
    assert (buf[B * T * C:].cpu().view(torch.int32) == -1).all() and torch.equal(x.cpu().view(torch.int32), got), "a refused call wrote"
