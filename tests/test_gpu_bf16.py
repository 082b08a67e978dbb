"""The opt-in "bf16" precision mode (model_config["matmul"] = "bf16", ns_config.matmul_bf16x3 == 2) on the MI355X.

Contract: every contraction from the decoder input through the PostNet output (decoder QKV, Q K^T, P V, fc, FFN w_1 / w_2,
mel_linear, the five PostNet convolutions) takes both operands rounded to bf16 (round to nearest even) and accumulates in
fp32; everything upstream — encoder, durations, length regulator, pitch / energy at either level — is the exact fp32 path,
so outputs 2-9 are bit-identical to the fp32 model's.  The bf16 reference is an emulation: the oracle's decoder, mel_linear
and (BatchNorm-folded, like the library) PostNet on the oracle's own decoder input, with F.linear / F.conv1d / torch.bmm
rounding both operands to bf16.
"""
import json
import time
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import dev, load_golden, weights_for

pytestmark = pytest.mark.gpu

MAX_ABS = 2.5e-2   # bf16 mel vs the fp32 oracle, every frame (emulated: 8.0e-3)
MEAN_ABS = 4e-3    # (emulated: 1.3e-3)
# The bf16 forward is chaotic at the fp32-noise level: a relative perturbation of 2e-7 of the decoder input alone moves the
# emulation's mel by ~0.9e-3 mean (every rounding flip feeds the next layer's roundings), about 2/3 of its whole distance from
# fp32.  So HIP (whose fp32 upstream sits ~1e-6 from the oracle's) cannot land closer to the emulation than that; the test
# holds it to the emulation's own spread under such noise, and below the emulation's distance from fp32:
#   mean |HIP - emu| <= NOISE_FRAC * mean |emu - emu(noisy input)|  and  <= EMU_FRAC * mean |emu - fp32 oracle|
# (an implementation rounding anything differently — another operand, another P — sits at ~1.4x the latter)
NOISE_FRAC = 1.25
EMU_FRAC = 0.75
NOISE_REL = 2e-7
LJ = dict(config="ljspeech", weight_seed=0, frames_per_phoneme=8.0, dur_weight_scale=0.25)
TINY = dict(config="tiny", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25)


_MODELS = {}


def models(meta, **extra):
    """(cfg, sd, fp32 model, bf16 model) on the same weights; one weight set cached at a time"""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    key = json.dumps([meta, extra], sort_keys=True, default=str)
    if key not in _MODELS:
        _MODELS.clear()
        cfg, sd = weights_for(meta)
        cfg = dict(cfg, length_regulator=meta.get("length_regulator", "hard"), **extra)
        pc = wl.preprocess_config(meta.get("pitch_level", "frame_level"), meta.get("energy_level", "frame_level"))
        out = []
        for mode in ("fp32", "bf16"):
            m = FastSpeech2Align(pc, dict(cfg, matmul=mode)).to("cuda").eval()
            m.load_state_dict(sd)
            out.append(m)
        _MODELS[key] = (cfg, sd, out[0], out[1])
    return _MODELS[key]


# ---------------------------------------------------------------------------------------------------- the bf16 emulation
def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)  # round to nearest even


class _Shim:
    """a module with some attributes replaced"""

    def __init__(self, base, **over):
        self._base = base
        self.__dict__.update(over)

    def __getattr__(self, k):
        return getattr(self._base, k)


def _postnet_folded(w, mel):
    """the PostNet as the library computes it: eval BatchNorm folded into the conv in float64, folded weights rounded"""
    x = mel.transpose(1, 2)
    n = 0
    while f"postnet.convolutions.{n}.0.conv.weight" in w:
        n += 1
    for i in range(n):
        p = f"postnet.convolutions.{i}"
        wt = w[p + ".0.conv.weight"]
        sc = w[p + ".1.weight"].double() / torch.sqrt(w[p + ".1.running_var"].double() + 1e-5)
        wf = (wt.double() * sc[:, None, None]).float()
        bf = ((w[p + ".0.conv.bias"].double() - w[p + ".1.running_mean"].double()) * sc + w[p + ".1.bias"].double()).float()
        x = F.conv1d(_bf(x), _bf(wf), bf, padding=(wt.shape[2] - 1) // 2)
        if i < n - 1:
            x = torch.tanh(x)
    return x.transpose(1, 2)


def _attention_bf16(q, k, v, mask, d_k):
    """the attention of the contract: scores from bf16 Q, K in fp32, scaled, masked; P V from the un-normalised exponentials
    p = 2^(s log2(e) - M), M an integer >= the row maximum, rounded to bf16, divided by the fp32 sum of p afterwards.  (Rounding
    commutes with powers of two, so any integer M gives the same P: the kernels' online softmax rounds exactly these.)"""
    s = torch.bmm(_bf(q), _bf(k).transpose(1, 2)) * np.float32(1.4426950408889634 / np.sqrt(d_k))
    s = s.masked_fill(mask, -np.inf)
    mx = torch.ceil(s.max(dim=2, keepdim=True).values)
    p = torch.exp2(s - mx)
    return torch.bmm(_bf(p), _bf(v)) / p.sum(dim=2, keepdim=True)


def emulate_bf16(w, cfg, va, mel_masks, normalised_p=False):
    """(mel, postnet mel) of the bf16 contract from the oracle's decoder input stages["va"].  normalised_p: round the
    normalised softmax instead (torch.bmm(attn, v) with both operands rounded) — a different P rounding, reported only."""
    from oracle import fs2_oracle as orc

    Fs = _Shim(F, linear=lambda x, wt, b=None: F.linear(_bf(x), _bf(wt), b),
               conv1d=lambda x, wt, b=None, **kw: F.conv1d(_bf(x), _bf(wt), b, **kw))
    Ts = _Shim(torch, bmm=lambda a, b: torch.bmm(_bf(a), _bf(b)))
    att = orc.scaled_dot_product_attention if normalised_p else _attention_bf16
    with torch.no_grad(), mock.patch.object(orc, "F", Fs), mock.patch.object(orc, "torch", Ts), \
            mock.patch.object(orc, "scaled_dot_product_attention", att):
        x = orc.mel_decoder(w, va, mel_masks, cfg["transformer"]["decoder_head"], cfg["max_seq_len"])
        mel = Fs.linear(x, w["mel_linear.weight"], w["mel_linear.bias"])
    with torch.no_grad():
        post = _postnet_folded(w, mel) + mel
    return mel, post


def _oracle(w, cfg, inp, **kw):
    from oracle import fs2_oracle as orc

    st = {}
    with torch.no_grad():
        ref = orc.forward(w, cfg, torch.from_numpy(inp[0]), torch.from_numpy(inp[1]), torch.from_numpy(inp[2]), inp[3], stages=st, **kw)
    return ref, st


def _mae(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.from_numpy(a).double()
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.from_numpy(b).double()
    d = (a - b).abs()
    return float(d.max()), float(d.mean())


def _emulations(w, cfg, va, mel_masks):
    """the emulation, and the emulation on the decoder input perturbed by relative fp32-sized noise (seeded)"""
    g = torch.Generator().manual_seed(0)
    noisy = va * (1 + NOISE_REL * torch.randn(va.shape, generator=g))
    return emulate_bf16(w, cfg, va, mel_masks), emulate_bf16(w, cfg, noisy, mel_masks)


def _check_against_oracle_and_emulation(out, ref, emu, what, emu_noise, emu_np=None):
    """out: the bf16 model's 12-tuple with the oracle's pitch / energy as targets.  Every frame."""
    res = {}
    if emu_np is not None:
        res["mel_vs_normalised_p_emulation"] = _mae(out[0], emu_np[0])
    for i, name in ((0, "mel"), (1, "postnet")):
        mx, mean = _mae(out[i], ref[i])
        emx, emean = _mae(emu[i], ref[i])
        vmx, vmean = _mae(out[i], emu[i])
        nmx, nmean = _mae(emu_noise[i], emu[i])
        res[name] = dict(vs_fp32_max=mx, vs_fp32_mean=mean, emu_vs_fp32_mean=emean, emu_vs_fp32_max=emx, vs_emu_mean=vmean, vs_emu_max=vmx,
                         emu_noise_spread_mean=nmean)
        assert mx <= MAX_ABS and mean <= MEAN_ABS, (what, name, res[name])
        assert vmean <= NOISE_FRAC * nmean and vmean <= EMU_FRAC * emean, (what, name, "not the defined bf16 contraction", res[name])
    print(what, res)
    return res


def _run(m, inp, ref=None, **kw):
    kw = dict(kw)
    lens = torch.from_numpy(inp[2].copy()) if kw.pop("host_lens", False) else dev(inp[2])
    with torch.no_grad():
        if ref is not None:
            kw = dict(kw, p_targets=ref[2].cuda(), e_targets=ref[3].cuda())
        out = m(dev(inp[0]), dev(inp[1]), lens, inp[3], **kw)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------- 1. upstream is exact
@pytest.mark.parametrize("name", ["e2e_tiny_single", "e2e_tiny_phoneme_level", "e2e_tiny_pitch_phoneme_energy_frame",
                                  "e2e_tiny_pitch_frame_energy_phoneme", "e2e_tiny_gaussian_wired", "e2e_tiny_padded_src",
                                  "e2e_tiny_T_above_1000", "e2e_tiny_T_below_1000"])
def test_upstream_outputs_are_bit_identical_to_fp32(name):
    meta, z = load_golden(name)
    cfg, sd, m32, mbf = models(meta)
    args = (dev(z["speakers"]), dev(z["texts"]), dev(z["in_src_lens"]), int(meta["L"]))
    kw = dict(p_control=meta.get("p_control", 1.0), e_control=meta.get("e_control", 1.0))
    with torch.no_grad():
        a = m32(*args, **kw)
        b = mbf(*args, **kw)
    torch.cuda.synchronize()
    for i in range(2, 10):
        assert torch.equal(a[i], b[i]), (name, i)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]), (name, "the bf16 mode did not run")
    mx, mean = _mae(b[1], a[1])
    assert mx <= MAX_ABS and mean <= MEAN_ABS, (name, mx, mean)
    print(name, "postnet mel vs the fp32 model: max", mx, "mean", mean)


# ---------------------------------------------------------------------------------------------------- 2. accuracy, config 2
_CFG2 = {}


def _cfg2():
    from oracle import fs2_oracle as orc
    from tests.test_gpu_parity import _screened_full_batch

    if not _CFG2:
        cfg, sd, m32, mbf = models(LJ)
        w = orc.to_torch_weights(sd)
        st = {}
        inp, ref = _screened_full_batch(w, cfg, 16, 128, seed=3, stages=st)
        emu, emu_noise = _emulations(w, cfg, st["va"], ref[7])
        emu_np = emulate_bf16(w, cfg, st["va"], ref[7], normalised_p=True)
        _CFG2.update(cfg=cfg, w=w, inp=inp, ref=ref, emu=emu, emu_noise=emu_noise, emu_np=emu_np)
    return _CFG2


def test_mel_accuracy_config2_full_size():
    c = _cfg2()
    cfg, sd, m32, mbf = models(LJ)
    out = _run(mbf, c["inp"], c["ref"])
    a = _run(m32, c["inp"], c["ref"])
    assert np.array_equal(out[9].cpu().numpy(), c["ref"][9].numpy())
    for i in range(2, 10):
        assert torch.equal(out[i], a[i]), i
    assert not torch.equal(out[0], a[0]) and not torch.equal(out[1], a[1])
    _check_against_oracle_and_emulation(out, c["ref"], c["emu"], "config 2 (B=16, L=128), every frame:", c["emu_noise"], c["emu_np"])


# ---------------------------------------------------------------------------------------------------- 3. no small-launch fallback
@pytest.mark.parametrize("B,L,seed", [(2, 20, 1), (1, 100, 0)])
def test_small_launches_run_bf16_too(B, L, seed):
    import smart_nar_fast_tts_amd.workload as wl
    from oracle import fs2_oracle as orc

    cfg, sd, m32, mbf = models(LJ)
    w = orc.to_torch_weights(sd)
    inp = wl.synth_inputs(B, L, seed=seed)
    ref, st = _oracle(w, cfg, inp)
    emu, emu_noise = _emulations(w, cfg, st["va"], ref[7])
    out = _run(mbf, inp, ref)
    a = _run(m32, inp, ref)
    assert not torch.equal(out[0], a[0]) and not torch.equal(out[1], a[1]), "fell back to fp32"
    for i in range(2, 10):
        assert torch.equal(out[i], a[i]), i
    _check_against_oracle_and_emulation(out, ref, emu, f"B={B} L={L}:", emu_noise)


# ---------------------------------------------------------------------------------------------------- 4. invariants
@pytest.mark.parametrize("R", [9, 17])
def test_replicas_inside_a_batch_are_bit_identical(R):
    import smart_nar_fast_tts_amd.workload as wl

    cfg, sd, m32, mbf = models(LJ)
    sp, tx, ln, L = wl.synth_inputs(1, 128, seed=5)
    with torch.no_grad():
        one = mbf(dev(sp), dev(tx), dev(ln), L)
        T1 = int(one[9][0])
        big = mbf(dev(np.tile(sp, R)), dev(np.tile(tx, (R, 1))), dev(np.tile(ln, R)), L,
                  p_targets=one[2].repeat(R, 1), e_targets=one[3].repeat(R, 1))
    torch.cuda.synchronize()
    assert big[0].shape[1] == T1
    for i in (0, 1, 2, 3, 4, 5, 9):
        assert all(torch.equal(big[i][r], big[i][0]) for r in range(1, R)), (i, R)


def test_two_launch_row_epilogue_gives_the_same_bits():
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    cfg, sd, m32, mbf = models(LJ)
    m2 = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul="bf16", row_epilogue="two_launch")).to("cuda").eval()
    m2.load_state_dict(sd)
    for B, L, seed in ((1, 100, 0), (3, 40, 2), (16, 128, 3)):
        inp = wl.synth_inputs(B, L, seed=seed)
        a, b = _run(mbf, inp), _run(m2, inp)
        for i in range(10):
            assert torch.equal(a[i], b[i]), (B, L, i)


def test_packed_rows_against_the_padded_grid():
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    cfg, sd, m32, mbf = models(LJ)
    lens = np.array([128, 10, 64, 1, 100, 33, 127, 17, 128, 5, 77, 2])
    inp = wl.synth_inputs(len(lens), 128, seed=9, src_lens=lens)
    ms = {}
    for mode in ("dense", "packed"):
        ms[mode] = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul="bf16", padded_rows=mode)).to("cuda").eval()
        ms[mode].load_state_dict(sd)
    grid = _run(ms["dense"], inp)
    pk = _run(ms["packed"], inp, host_lens=True, p_targets=grid[2], e_targets=grid[3])
    assert ms["packed"]._lib.ns_last_phase2_rows(ms["packed"]._h) < grid[0].shape[0] * grid[0].shape[1], "did not run on packed rows"
    for i in range(5, 10):  # integers and masks (log durations: phase 1 may pack too, fp32 noise)
        assert torch.equal(pk[i].cpu(), grid[i].cpu()), i  # (src_lens comes back where it was passed: host vs device)
    assert float((pk[4] - grid[4]).abs().max()) < 1e-4
    for i in (0, 1):
        mx, mean = _mae(pk[i], grid[i])
        assert mx <= MAX_ABS and mean <= MEAN_ABS, (i, mx, mean)
        print("packed vs grid", i, mx, mean)


def test_capacity_mode_matches_the_synchronous_call():
    meta, z = load_golden("e2e_tiny_padded_src")
    cfg, sd, m32, mbf = models(meta)
    mbf.packed_rows = False
    args = (dev(z["speakers"]), dev(z["texts"]), dev(z["in_src_lens"]), int(meta["L"]))
    with torch.no_grad():
        base = mbf(*args)
        T = base[0].shape[1]
        cap = mbf(*args, max_mel_len=T, async_status=True)
    assert cap.check() == [0] * len(z["in_src_lens"])
    for i in range(10):
        assert torch.equal(cap[i], base[i]), i


def test_zero_length_utterance_gives_nan_where_fp32_does():
    import smart_nar_fast_tts_amd.workload as wl

    cfg, sd, m32, mbf = models(TINY)
    lens = np.array([20, 0, 7, 13])
    inp = wl.synth_inputs(4, 20, seed=6, src_lens=np.maximum(lens, 1))
    texts = inp[1].copy()
    texts[1, :] = 0
    args = (dev(inp[0]), dev(texts), dev(lens), inp[3])
    with torch.no_grad():
        a, b = m32(*args), mbf(*args)
    torch.cuda.synchronize()
    for i in range(2, 10):
        assert torch.equal(torch.isnan(a[i]), torch.isnan(b[i])) if a[i].is_floating_point() else torch.equal(a[i], b[i]), i
    for i in (0, 1):
        assert torch.equal(torch.isnan(a[i]), torch.isnan(b[i])), i


# ---------------------------------------------------------------------------------------------------- 5. arena
def test_arena_refuses_fp32_bytes_and_state_dict_round_trips():
    cfg, sd, m32, mbf = models(TINY)
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    m = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul="bf16")).to("cuda").eval()
    m.load_state_dict(sd)
    src = m32.arena_tensor()
    dst = m.arena_tensor()
    n = min(src.numel(), dst.numel())
    dst[:n].copy_(src[:n])
    with pytest.raises(RuntimeError, match="ns_adopt_arena"):
        m.adopt_arena()
    # a bf16 model's own bytes are adopted
    m.load_state_dict(sd)
    m3 = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul="bf16")).to("cuda").eval()
    m3.arena_tensor().copy_(mbf.arena_tensor())
    m3.adopt_arena()
    inp = wl.synth_inputs(2, 20, seed=1)
    a, b = _run(mbf, inp), _run(m3, inp)
    assert all(torch.equal(a[i], b[i]) for i in range(10))
    back = mbf.state_dict()
    for k, v in sd.items():
        if k in back:
            got = back[k].detach().cpu().numpy() if torch.is_tensor(back[k]) else np.asarray(back[k])
            assert np.array_equal(got, v), k


# ---------------------------------------------------------------------------------------------------- 6. not a slow path
def test_bf16_forward_is_faster_than_fp32_at_config2():
    import smart_nar_fast_tts_amd.workload as wl

    cfg, sd, m32, mbf = models(LJ)
    sp, tx, ln, L = wl.synth_inputs(16, 128, seed=3)
    args = (dev(sp), dev(tx), dev(ln), L)
    med = {}
    for name, m in (("fp32", m32), ("bf16", mbf)):
        ts = []
        with torch.no_grad():
            for it in range(13):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m(*args)
                torch.cuda.synchronize()
                if it >= 3:
                    ts.append(time.perf_counter() - t0)
        med[name] = float(np.median(ts))
    print("config 2 median forward: fp32 %.3f ms, bf16 %.3f ms, ratio %.3f" % (med["fp32"] * 1e3, med["bf16"] * 1e3, med["bf16"] / med["fp32"]))
    assert med["bf16"] < 0.8 * med["fp32"], med
