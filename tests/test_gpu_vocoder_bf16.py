"""Opt-in bf16 matmul mode of the HiFi-GAN vocoder (csrc/vocoder_bf16.hip, Generator(h, matmul="bf16")) on the MI355X against
an independent CPU emulation (tests/hifigan_bf16_emu.py, on top of tests/hifigan_cpu.py): every upsampler and resblock-conv weight
rounded with .to(torch.bfloat16), a forward pre-hook on the same modules that rounds the fp32 activation to bf16, evaluation in
float64.

Per layer the GPU differs from the emulation only by its fp32 summation order, so the bound is elementwise and tight.  Once
activations chain, a 1-ulp bf16 flip in an intermediate propagates, so stages and the whole generator are held to an SNR."""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402
from tests import hifigan_cpu  # noqa: E402
from tests.hifigan_bf16_emu import bf, emulation, snr_db  # noqa: E402
from tests.hifigan_bf16_emu import lrelu32 as _lrelu32  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::FutureWarning")]

B = 3
LENS = (1, 7, 33)  # a ragged batch: frames per utterance, padded to the longest
REL = 1.5e-5       # |gpu - emu| <= REL * (conv(|a_bf16|, |w_bf16|) + |bias|)
MIN_SNR_DB = 40.0


@pytest.fixture(scope="module")
def h():
    return wl.hifigan_config("v1")


@pytest.fixture(scope="module")
def sd(h):
    return wl.synth_vocoder_state_dict(h, seed=0)


@pytest.fixture(scope="module")
def refs(h, sd):
    """float64 reference, float64-intermediate emulation, folded fp32 weights"""
    return hifigan_cpu.folded(h, sd, torch.float64), emulation(h, sd), hifigan_cpu.folded(h, sd, torch.float32)


def _x(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def _ragged_mel(T=max(LENS), seed=5):
    mel = _x((B, 80, T), seed)
    for b, n in enumerate(LENS):  # padded frames hold values too (the forward's postnet output does), a different level
        mel[b, :, n:] = 0.3 * mel[b, :, n:] - 1.0
    return mel


@pytest.fixture(scope="module")
def fp32_before(h, sd):
    """the fp32 generator's output before any bf16 instance exists in this process (the bf16 fixtures depend on this one)"""
    from smart_nar_fast_tts_amd.vocoder import Generator

    g = Generator(h).to("cuda").eval()
    g.load_state_dict(sd)
    mel = _ragged_mel(seed=11).cuda()
    out = g(mel).cpu()
    del g
    return mel, out


@pytest.fixture(scope="module")
def gen(h, sd, fp32_before):
    from smart_nar_fast_tts_amd.vocoder import Generator

    g = Generator(h, matmul="bf16").to("cuda").eval()
    g.load_state_dict(sd)
    assert g.matmul == "bf16"
    return g


@pytest.fixture(scope="module")
def gen32(h, sd, fp32_before):
    from smart_nar_fast_tts_amd.vocoder import Generator

    g = Generator(h).to("cuda").eval()
    g.load_state_dict(sd)
    return g


def _check_layer(got, ref, unit):
    err = (got.double() - ref).abs()
    worst = float((err / unit.clamp_min(1e-30)).max()) / REL
    assert bool((err <= REL * unit).all()), f"worst |gpu - emu| / (REL * conv(|a|,|w|)) = {worst:.3g}"
    return worst


# ---------------------------------------------------------------------------------------------------- per layer, tight
@pytest.mark.parametrize("stage", range(4))
@pytest.mark.parametrize("j", range(3))
@pytest.mark.parametrize("which", (1, 2))
def test_resblock_convs_vs_emulation(gen, refs, h, stage, j, which):
    """every (C, k, d) of V1, both convs, at S = 1, 7, 33 rows per utterance (taps reaching past both ends of every utterance)"""
    emu = refs[1]
    rb = 3 * stage + j
    for n in range(3):
        conv = getattr(emu.resblocks[rb], f"convs{which}")[n]
        ch, d, pad = conv.in_channels, conv.dilation[0], conv.padding[0]
        w, bias = conv.weight.detach(), conv.bias.detach()  # float64 of the bf16-rounded / fp32 values
        for S in LENS:
            x = _x((B, S, ch), seed=100 * rb + 10 * n + S + 7 * which)
            got = gen.op_conv(f"resblocks.{rb}.convs{which}.{n}", x.cuda()).cpu()
            a = bf(_lrelu32(x)).double().transpose(1, 2)
            ref = F.conv1d(a, w, bias, padding=pad, dilation=d).transpose(1, 2)
            unit = F.conv1d(a.abs(), w.abs(), bias.abs(), padding=pad, dilation=d).transpose(1, 2)
            assert got.shape == (B, S, ch)
            _check_layer(got, ref, unit)


@pytest.mark.parametrize("i", range(4))
def test_upsample_vs_emulation(gen, refs, h, i):
    """both upsample shapes of V1 (u = 8, k = 16 and u = 2, k = 4) as the polyphase GEMM, edges of every utterance included"""
    up = refs[1].ups[i]
    u, k = h["upsample_rates"][i], h["upsample_kernel_sizes"][i]
    w, bias = up.weight.detach(), up.bias.detach()
    for S in LENS:
        x = _x((B, S, up.in_channels), seed=7 + 31 * i + S)
        got = gen.op_upsample(i, x.cuda()).cpu()
        a = bf(_lrelu32(x)).double().transpose(1, 2)
        ref = F.conv_transpose1d(a, w, bias, stride=u, padding=(k - u) // 2).transpose(1, 2)
        unit = F.conv_transpose1d(a.abs(), w.abs(), bias.abs(), stride=u, padding=(k - u) // 2).transpose(1, 2)
        assert got.shape == ref.shape == (B, S * u, up.out_channels)
        _check_layer(got, ref, unit)


def test_conv_pre_and_post_stay_fp32(gen, gen32):
    """conv_pre and conv_post are not GEMM-mode layers: the same kernels, the same bits as the fp32 generator"""
    for S in LENS:
        x = _x((B, S, 80), seed=900 + S).cuda()
        assert torch.equal(gen.op_conv("conv_pre", x), gen32.op_conv("conv_pre", x))
        x = _x((B, S * 256, 32), seed=950 + S).cuda()
        assert torch.equal(gen.op_conv("conv_post", x), gen32.op_conv("conv_post", x))


# ---------------------------------------------------------------------------------------------------- chained: SNR
def _stage(m, i, x):
    y = m.ups[i](F.leaky_relu(x.transpose(1, 2), 0.1))
    xs = None
    for jj in range(3):
        v = m.resblocks[3 * i + jj](y)
        xs = v if xs is None else xs + v
    return (xs / 3).transpose(1, 2)


@pytest.mark.parametrize("i", range(4))
def test_stage_snr(gen, refs, i):
    r64, emu, _ = refs
    x = _x((B, 33, r64.ups[i].in_channels), seed=40 + i) * 0.5
    got = gen.op_stage(i, x.cuda()).cpu()
    with torch.no_grad():
        ref = _stage(r64, i, x.double())
        e = _stage(emu, i, x.double())
    s_gpu, s_emu = snr_db(ref, got), snr_db(ref, e)
    assert s_gpu >= MIN_SNR_DB, (s_gpu, s_emu)
    assert abs(s_gpu - s_emu) <= 3.0, (s_gpu, s_emu)


def test_generator_snr(gen, refs):
    r64, emu, _ = refs
    mel = _ragged_mel()
    with torch.no_grad():
        ref = r64(mel.double())[:, 0]
        e = emu(mel.double())[:, 0]
    std = float(ref.std())
    assert 0.05 <= std <= 0.9, std  # a real waveform, not saturated
    got = gen(mel.cuda())
    assert got.shape == (B, 1, max(LENS) * 256) and got.dtype == torch.float32
    got = got[:, 0].cpu()
    s_gpu, s_emu = snr_db(ref, got), snr_db(ref, e)
    assert s_gpu >= MIN_SNR_DB, (s_gpu, s_emu)
    assert abs(s_gpu - s_emu) <= 3.0, (s_gpu, s_emu)  # as close as the bf16 roundings allow, and not an fp32 path (~130 dB)


def test_vocoder_infer_int16(gen, gen32):
    from smart_nar_fast_tts_amd.vocoder import vocoder_infer

    mel = _ragged_mel(seed=13).cuda()
    cfg = {"vocoder": {"model": "HiFi-GAN", "speaker": "LJSpeech"}}
    pc = {"preprocessing": {"audio": {"max_wav_value": 32768.0}}}
    lengths = [n * 256 for n in LENS]
    w16 = vocoder_infer(mel, gen, cfg, pc, lengths=lengths)
    w32 = vocoder_infer(mel, gen32, cfg, pc, lengths=lengths)
    assert [len(w) for w in w16] == [len(w) for w in w32] == lengths
    assert all(w.dtype == np.int16 for w in w16)
    a = torch.from_numpy(np.concatenate(w32).astype(np.float64))
    b = torch.from_numpy(np.concatenate(w16).astype(np.float64))
    assert snr_db(a, b) >= MIN_SNR_DB


# ---------------------------------------------------------------------------------------------------- bits
def test_determinism_and_layout(gen):
    mel = _ragged_mel(seed=9)
    mel[2] = mel[0]
    a = gen(mel.cuda())
    b = gen(mel.cuda())
    assert torch.equal(a, b)
    assert torch.equal(a[0], a[2])  # identical utterances inside one batch
    tm = mel.transpose(1, 2).contiguous().cuda()  # [B, T, 80], what the forward's postnet_output is
    view = tm.transpose(1, 2)
    assert not view.is_contiguous()
    assert torch.equal(gen(view), gen(view.contiguous()))
    assert torch.equal(gen(view), a)
    # a bf16 layer's bits do not depend on the batch: utterance 0 alone == utterance 0 of the batch of 3
    x = _x((B, 33, 256), seed=17).cuda()
    assert torch.equal(gen.op_conv("resblocks.1.convs1.2", x)[:1], gen.op_conv("resblocks.1.convs1.2", x[:1]))
    x = _x((B, 33, 512), seed=18).cuda()
    assert torch.equal(gen.op_upsample(0, x)[:1], gen.op_upsample(0, x[:1]))


def _bf16_bits_to_f32(bits):
    return torch.from_numpy((np.asarray(bits, np.uint32) << 16).view(np.float32))


def _tie_values(n, seed):
    """float32 values on or around bf16 rounding boundaries: exact ties of both parities, just above / below a tie, and ties that
    round up into the next binade (mantissa all ones)"""
    rs = np.random.RandomState(seed)
    hi = rs.randint(0x3C00, 0x3F80, size=n).astype(np.uint32)  # |v| in [2^-7, 1)
    hi[: n // 4] |= 1  # odd: a tie rounds up
    hi[n // 4: n // 2] &= ~np.uint32(1)  # even: a tie rounds down
    hi[n // 2: n // 2 + 8] = (hi[n // 2: n // 2 + 8] & ~np.uint32(0x7F)) | 0x7F  # x.1111111 + tie -> next binade
    lo = np.full(n, 0x8000, np.uint32)
    lo[n - n // 8:] = rs.choice([0x7FFF, 0x8001, 0x0001, 0xFFFF], size=n // 8)
    sign = (rs.rand(n) < 0.5).astype(np.uint32) << 31
    return torch.from_numpy(((hi << 16) | lo | sign).view(np.float32))


def test_weight_rounding_is_rne_ties_included(h, sd):
    """a resblock conv whose weights sit on bf16 rounding boundaries, zero bias, one-hot input (1.0 at channel c0, tap t0):
    output row t0 + 1 - j, column o, is exactly the RNE-rounded W[o, c0, j]"""
    from smart_nar_fast_tts_amd.vocoder import Generator

    plain = {k: v.clone() for k, v in hifigan_cpu.folded(h, sd).state_dict().items()}
    name, c0, t0, S = "resblocks.0.convs1.0", 17, 5, 12  # C = 256, k = 3, d = 1
    W = plain[name + ".weight"]
    W[:, c0, :] = _tie_values(W.shape[0] * 3, seed=3).reshape(W.shape[0], 3)
    plain[name + ".bias"] = torch.zeros_like(plain[name + ".bias"])
    g = Generator(h, matmul="bf16").to("cuda")
    g.load_state_dict(plain)
    x = torch.zeros(1, S, W.shape[1])
    x[0, t0, c0] = 1.0
    out = g.op_conv(name, x.cuda()).cpu()[0]
    exp = bf(W[:, c0, :])  # [256, 3]
    trunc = _bf16_bits_to_f32(W[:, c0, :].contiguous().view(torch.int32).numpy().astype(np.uint32) >> 16).reshape(exp.shape)
    assert not torch.equal(exp, trunc)  # the values do tell RNE from truncation
    for j in range(3):
        assert torch.equal(out[t0 + 1 - j], exp[:, j]), j
    others = [t for t in range(S) if t not in (t0 - 1, t0, t0 + 1)]
    assert bool((out[others] == 0).all())


def test_activation_rounding_is_rne_ties_included(h, sd):
    """one-hot weights (W[o, o, 1] = 1: the centre tap copies channel o), zero bias, activations on bf16 rounding boundaries:
    out == RNE(lrelu(x)) exactly, lrelu in fp32"""
    from smart_nar_fast_tts_amd.vocoder import Generator

    plain = {k: v.clone() for k, v in hifigan_cpu.folded(h, sd).state_dict().items()}
    name = "resblocks.3.convs2.1"  # C = 128, k = 3
    W = torch.zeros_like(plain[name + ".weight"])
    C = W.shape[0]
    W[torch.arange(C), torch.arange(C), 1] = 1.0
    plain[name + ".weight"] = W
    plain[name + ".bias"] = torch.zeros(C)
    g = Generator(h, matmul="bf16").to("cuda")
    g.load_state_dict(plain)
    S = 9
    x = _tie_values(2 * S * C, seed=4)[: 2 * S * C].reshape(2, S, C).contiguous()
    out = g.op_conv(name, x.cuda()).cpu()
    pos = x > 0
    exp = bf(_lrelu32(x))
    trunc = _bf16_bits_to_f32(x.view(torch.int32).numpy().astype(np.uint32) >> 16).reshape(x.shape)
    assert not torch.equal(exp[pos], trunc[pos])
    assert torch.equal(out, exp)


# ---------------------------------------------------------------------------------------------------- mode plumbing
def test_set_matmul_fails_after_bind_arena(h, sd):
    from smart_nar_fast_tts_amd.vocoder import Generator

    g = Generator(h, matmul="bf16").to("cuda")
    g.load_state_dict(sd)  # binds the arena
    assert g._lib.ns_voc_set_matmul(g._h, 0) != 0
    assert b"ns_voc_bind_arena" in g._lib.ns_last_error()
    g32 = Generator(h)
    assert g._arena.numel() > g32._lib.ns_voc_arena_bytes(g32._h)


def _files(tmp_path, h, sd):
    cfg_path, ckpt_path = tmp_path / "config.json", tmp_path / "generator.pth.tar"
    cfg_path.write_text(json.dumps(h))
    torch.save({"generator": {k: torch.from_numpy(v) for k, v in sd.items()}}, str(ckpt_path))
    return str(cfg_path), str(ckpt_path)


def test_get_vocoder_mode(tmp_path, h, sd):
    from smart_nar_fast_tts_amd.vocoder import get_vocoder

    cp, kp = _files(tmp_path, h, sd)
    dev = torch.device("cuda:0")
    voc = {"model": "HiFi-GAN", "speaker": "LJSpeech"}
    assert get_vocoder({"vocoder": dict(voc)}, dev, config_path=cp, ckpt_path=kp).matmul == "fp32"
    assert get_vocoder({"vocoder": dict(voc, matmul="bf16")}, dev, config_path=cp, ckpt_path=kp).matmul == "bf16"
    assert get_vocoder({"vocoder": dict(voc)}, dev, config_path=cp, ckpt_path=kp, matmul="bf16").matmul == "bf16"
    assert get_vocoder({"vocoder": dict(voc, matmul="bf16")}, dev, config_path=cp, ckpt_path=kp, matmul="fp32").matmul == "fp32"
    with pytest.raises(ValueError, match="matmul"):
        get_vocoder({"vocoder": dict(voc, matmul="fp8")}, dev, config_path=cp, ckpt_path=kp)


def test_fp32_untouched_by_bf16_instances(h, sd, gen, fp32_before):
    """an fp32 generator built and run after bf16 ones reproduces the bits of one run before any bf16 instance existed"""
    from smart_nar_fast_tts_amd.vocoder import Generator

    mel, before = fp32_before
    assert gen(mel) is not None  # a bf16 instance exists and has run
    g = Generator(h).to("cuda").eval()
    g.load_state_dict(sd)
    assert torch.equal(g(mel).cpu(), before)
    assert not torch.equal(gen(mel).cpu(), before)


def test_end_to_end(tmp_path, h, sd):
    from smart_nar_fast_tts_amd import batching
    from smart_nar_fast_tts_amd.model import FastSpeech2Align
    from smart_nar_fast_tts_amd.vocoder import get_vocoder, vocoder_infer

    cfg = wl.model_config("tiny")
    cfg["vocoder"] = {"model": "HiFi-GAN", "speaker": "LJSpeech"}
    pc = wl.preprocess_config()
    pc["preprocessing"]["audio"] = {"max_wav_value": 32768.0}
    pc["preprocessing"]["stft"] = {"hop_length": 256}
    m = FastSpeech2Align(pc, cfg).to("cuda:0").eval()
    m.load_state_dict(wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=4.0))
    cp, kp = _files(tmp_path, h, sd)
    voc = get_vocoder(cfg, torch.device("cuda:0"), config_path=cp, ckpt_path=kp, matmul="bf16")
    assert voc.matmul == "bf16"
    sp, tx, ln, L = wl.synth_inputs(3, 20, seed=2, src_lens=[20, 13, 7])
    with torch.no_grad():
        out = m(torch.from_numpy(sp).cuda(), torch.from_numpy(tx).cuda(), torch.from_numpy(ln).cuda(), L)
    mel_lens = out[9].cpu().tolist()
    wavs = vocoder_infer(out[1].transpose(1, 2), voc, cfg, pc, lengths=out[9] * 256)
    assert [len(w) for w in wavs] == [n * 256 for n in mel_lens]
    assert all(w.dtype == np.int16 for w in wavs)
    items = batching.synthesize(m, [(["a", "b", "c"], ["", "", ""], sp, tx, ln, L)], pc, vocoder=voc)
    assert len(items) == 3
    for it, w in zip(items, wavs):
        assert np.array_equal(it["wav"], w)


# ---------------------------------------------------------------------------------------------------- speed guard
def test_bf16_is_at_least_twice_as_fast(gen, gen32):
    """loose: catches a silent fp32 path.  B = 8, T = 256: median of 5 timed forwards after warm-up, bf16 <= 0.5x fp32"""
    mel = _x((8, 80, 256), seed=21).cuda() * 0.56

    def med(g):
        for _ in range(2):
            g(mel)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            g(mel)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts))

    t32, t16 = med(gen32), med(gen)
    assert t16 <= 0.5 * t32, (t16, t32)
