"""HiFi-GAN vocoder on the MI355X (csrc/vocoder.hip, smart_nar_fast_tts_amd.vocoder) against the independent CPU restatement
tests/hifigan_cpu.py in float64: every layer shape of V1, the whole generator, the int16 output, determinism, and the end-to-end
path FastSpeech2Align -> get_vocoder -> vocoder_infer / batching.synthesize(vocoder=...)."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402
from tests import hifigan_cpu  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::FutureWarning")]

B = 3
LENS = (1, 7, 33)  # a ragged batch: frames per utterance, padded to the longest
REL = 4e-6         # rounding-level bound: |gpu - f64| <= REL * conv(|x|, |W|) (+ |bias|)


@pytest.fixture(scope="module")
def h():
    return wl.hifigan_config("v1")


@pytest.fixture(scope="module")
def sd(h):
    return wl.synth_vocoder_state_dict(h, seed=0)


@pytest.fixture(scope="module")
def refs(h, sd):
    return hifigan_cpu.folded(h, sd, torch.float64), hifigan_cpu.folded(h, sd, torch.float32)


@pytest.fixture(scope="module")
def gen(h, sd):
    from smart_nar_fast_tts_amd.vocoder import Generator

    g = Generator(h).to("cuda").eval()
    g.load_state_dict(sd)
    return g


def _x(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def _check_layer(got, ref, unit):
    """elementwise |got - ref| <= REL * unit; returns the worst ratio err / unit in units of REL"""
    ref, unit = ref.detach(), unit.detach()
    err = (got.double() - ref).abs()
    worst = float((err / unit.clamp_min(1e-30)).max()) / REL
    assert bool((err <= REL * unit).all()), f"worst |gpu - f64| / (REL * conv(|x|,|W|)) = {worst:.3g}"
    return worst


@pytest.mark.parametrize("stage", range(4))
@pytest.mark.parametrize("j", range(3))
@pytest.mark.parametrize("which", (1, 2))
def test_resblock_convs_vs_f64(gen, refs, h, stage, j, which):
    """every (C, k, d) of V1: c = resblocks[3 stage + j].convs{which}[n], out = conv(lrelu(x, 0.1)) + bias, at S = 1, 7, 33 rows
    per utterance (taps reaching past both ends of every utterance, the k = 11, d = 5 window covering S = 33 twice over)"""
    r64 = refs[0]
    rb = 3 * stage + j
    for n in range(3):
        conv = getattr(r64.resblocks[rb], f"convs{which}")[n]
        ch, k, d = conv.in_channels, conv.kernel_size[0], conv.dilation[0]
        for S in LENS:
            x = _x((B, S, ch), seed=100 * rb + 10 * n + S)
            got = gen.op_conv(f"resblocks.{rb}.convs{which}.{n}", x.cuda()).cpu()
            a = F.leaky_relu(x.double(), 0.1).transpose(1, 2)
            ref = F.conv1d(a, conv.weight, conv.bias, padding=conv.padding[0], dilation=d).transpose(1, 2)
            unit = (F.conv1d(a.abs(), conv.weight.abs(), conv.bias.abs(), padding=conv.padding[0], dilation=d)).transpose(1, 2)
            _check_layer(got, ref, unit)
            assert got.shape == (B, S, ch) and k == h["resblock_kernel_sizes"][j]


@pytest.mark.parametrize("i", range(4))
def test_upsample_vs_f64(gen, refs, h, i):
    """both upsample shapes of V1 (u = 8, k = 16 and u = 2, k = 4) as the polyphase GEMM, edges of every utterance included"""
    up = refs[0].ups[i]
    u, k = h["upsample_rates"][i], h["upsample_kernel_sizes"][i]
    for S in LENS:
        x = _x((B, S, up.in_channels), seed=7 + 31 * i + S)
        got = gen.op_upsample(i, x.cuda()).cpu()
        a = F.leaky_relu(x.double(), 0.1).transpose(1, 2)
        ref = F.conv_transpose1d(a, up.weight, up.bias, stride=u, padding=(k - u) // 2).transpose(1, 2)
        unit = F.conv_transpose1d(a.abs(), up.weight.abs(), up.bias.abs(), stride=u, padding=(k - u) // 2).transpose(1, 2)
        assert got.shape == ref.shape == (B, S * u, up.out_channels)
        _check_layer(got, ref, unit)


def test_conv_pre_and_post_vs_f64(gen, refs):
    r64 = refs[0]
    for S in LENS:
        x = _x((B, S, 80), seed=900 + S)
        got = gen.op_conv("conv_pre", x.cuda()).cpu()
        a = x.double().transpose(1, 2)
        ref = r64.conv_pre(a).transpose(1, 2)
        unit = F.conv1d(a.abs(), r64.conv_pre.weight.abs(), r64.conv_pre.bias.abs(), padding=3).transpose(1, 2)
        _check_layer(got, ref, unit)
        x = _x((B, S * 256, 32), seed=950 + S)
        got = gen.op_conv("conv_post", x.cuda()).cpu()
        a = F.leaky_relu(x.double(), 0.01).transpose(1, 2)
        pre = r64.conv_post(a)[:, 0]
        unit = F.conv1d(a.abs(), r64.conv_post.weight.abs(), r64.conv_post.bias.abs(), padding=3)[:, 0]
        _check_layer(got, torch.tanh(pre), unit)  # (tanh is 1-Lipschitz)


def test_stage_vs_f64(gen, refs, h):
    """upsample + multi-receptive-field fusion of every stage, against f64 and as close as the CPU's fp32 run"""
    r64, r32 = refs
    for i in range(4):
        x = _x((B, 33, r64.ups[i].in_channels), seed=40 + i) * 0.5
        got = gen.op_stage(i, x.cuda()).cpu().double()

        def run(m, xx):
            y = m.ups[i](F.leaky_relu(xx.transpose(1, 2), 0.1))
            xs = None
            for jj in range(3):
                v = m.resblocks[3 * i + jj](y)
                xs = v if xs is None else xs + v
            return (xs / 3).transpose(1, 2)

        with torch.no_grad():
            ref = run(r64, x.double())
            cpu = run(r32, x).double()
        e_gpu, e_cpu = float((got - ref).abs().max()), float((cpu - ref).abs().max())
        assert e_gpu <= max(2 * e_cpu, 1e-5), (i, e_gpu, e_cpu)


def _ragged_mel(T=max(LENS), seed=5):
    mel = _x((B, 80, T), seed)
    for b, n in enumerate(LENS):  # padded frames hold values too (the forward's postnet output does), a different level
        mel[b, :, n:] = 0.3 * mel[b, :, n:] - 1.0
    return mel


def test_generator_vs_f64_and_int16(gen, refs):
    r64, r32 = refs
    mel = _ragged_mel()
    with torch.no_grad():
        ref = r64(mel.double())[:, 0]
        cpu = r32(mel)[:, 0].double()
    std = float(ref.std())
    assert 0.05 <= std <= 0.9, std  # not a vacuous comparison: a real waveform, not saturated
    got = gen(mel.cuda())
    assert got.shape == (B, 1, max(LENS) * 256) and got.dtype == torch.float32
    got = got[:, 0].cpu().double()
    e_gpu, e_cpu = float((got - ref).abs().max()), float((cpu - ref).abs().max())
    assert e_gpu <= max(2 * e_cpu, 1e-5), (e_gpu, e_cpu)
    from smart_nar_fast_tts_amd.vocoder import wav_cast_trim

    pc = {"preprocessing": {"audio": {"max_wav_value": 32768.0}}}
    lengths = [n * 256 for n in LENS]
    gi = wav_cast_trim(got.float(), pc, lengths)
    ri = [np.trunc(ref[b, :lengths[b]].numpy() * 32768.0).astype(np.int64) for b in range(B)]
    for b in range(B):
        assert len(gi[b]) == lengths[b]
        assert int(np.abs(gi[b].astype(np.int64) - ri[b]).max()) <= 1


def test_determinism(gen):
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


def _e2e(tmp_path, h, sd):
    from smart_nar_fast_tts_amd.model import FastSpeech2Align
    from smart_nar_fast_tts_amd.vocoder import get_vocoder

    cfg = wl.model_config("tiny")
    cfg["vocoder"] = {"model": "HiFi-GAN", "speaker": "LJSpeech"}
    pc = wl.preprocess_config()
    pc["preprocessing"]["audio"] = {"max_wav_value": 32768.0}
    pc["preprocessing"]["stft"] = {"hop_length": 256}
    m = FastSpeech2Align(pc, cfg).to("cuda:0").eval()
    m.load_state_dict(wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=4.0))
    cfg_path, ckpt_path = tmp_path / "config.json", tmp_path / "generator.pth.tar"
    cfg_path.write_text(json.dumps(h))
    torch.save({"generator": {k: torch.from_numpy(v) for k, v in sd.items()}}, str(ckpt_path))
    voc = get_vocoder(cfg, torch.device("cuda:0"), config_path=str(cfg_path), ckpt_path=str(ckpt_path))
    return m, voc, cfg, pc


def _run_e2e(m, voc, cfg, pc):
    from smart_nar_fast_tts_amd import batching
    from smart_nar_fast_tts_amd.vocoder import vocoder_infer

    sp, tx, ln, L = wl.synth_inputs(3, 20, seed=2, src_lens=[20, 13, 7])
    with torch.no_grad():
        out = m(torch.from_numpy(sp).cuda(), torch.from_numpy(tx).cuda(), torch.from_numpy(ln).cuda(), L)
    mel_lens = out[9].cpu().tolist()
    wavs = vocoder_infer(out[1].transpose(1, 2), voc, cfg, pc, lengths=out[9] * 256)
    assert [len(w) for w in wavs] == [n * 256 for n in mel_lens]
    assert all(w.dtype == np.int16 for w in wavs)
    batch = (["a", "b", "c"], ["", "", ""], sp, tx, ln, L)
    items = batching.synthesize(m, [batch], pc, vocoder=voc)
    assert len(items) == 3
    for it, w in zip(items, wavs):
        assert np.array_equal(it["wav"], w)
    plain = batching.synthesize(m, [batch], pc)
    assert all("wav" not in it for it in plain)
    items2 = batching.synthesize(m, [batch, batch], pc, streams=2, vocoder=voc)
    for it, w in zip(items2, wavs + wavs):
        assert np.array_equal(it["wav"], w)
    return wavs


def test_end_to_end(tmp_path, h, sd):
    m, voc, cfg, pc = _e2e(tmp_path, h, sd)
    wavs = _run_e2e(m, voc, cfg, pc)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        wavs_s = _run_e2e(m, voc, cfg, pc)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(wavs, wavs_s))
