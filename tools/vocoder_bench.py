#!/usr/bin/env python3
"""HiFi-GAN vocoder (smart_nar_fast_tts_amd.vocoder) on one MI355X: whole-generator time, per-stage kernel time, FLOP from the
shapes and each stage's share of the MFMA peak of its matmul mode (fp32, or the bf16 dense peak with --matmul bf16), the same
generator run by torch-ROCm's own conv1d as a comparison line, and (--accuracy) the per-layer distance from a float64 evaluation
relative to the CPU's own fp32 run — or, with --matmul bf16, the per-layer distance to the CPU bf16 emulation and the
whole-generator SNR against float64 and against the fp32 GPU run.

    python tools/vocoder_bench.py --workload cfg2_b16 --steps 5 --warmup 2 [--matmul bf16] [--torch] [--accuracy] [--json out.json]

The mel comes from the real FastSpeech2Align forward with the synthetic weights of the workload (bench.py's inputs), transposed
the way synth_samples hands it over: a [B, 80, T] view of the [B, T, 80] postnet output.  Nothing here runs without the GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X fp32 matrix peak (v_mfma_f32_32x32x2_f32)
BF16_MFMA_PEAK_TFLOPS = 16 * F32_MFMA_PEAK_TFLOPS  # dense bf16 matrix peak (~2.5 PF, 16x the fp32 MFMA rate)
HBM_PEAK_GBS = 8000.0


def mel_from_forward(workload):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    cfg_name, B, L, fpp = wl.WORKLOADS[workload]
    cfg = wl.model_config(cfg_name)
    m = FastSpeech2Align(wl.preprocess_config(), cfg).to("cuda").eval()
    m.load_state_dict(wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=fpp))
    sp, tx, ln, Lm = wl.synth_inputs(B, L, seed=0)
    with torch.no_grad():
        out = m(torch.from_numpy(sp).cuda(), torch.from_numpy(tx).cuda(), torch.from_numpy(ln).cuda(), Lm)
    torch.cuda.synchronize()
    return out[1].transpose(1, 2), out[9].cpu()


def events_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def stage_bytes(B, S, cin, u, ch):
    """HBM bytes one stage moves at the least (activations only; the weights are a few MB): the upsampler reads its input and
    writes one activation; each of the 3 x 3 (c1, c2) pairs reads its input, writes and reads the hidden tensor, reads the
    residual and writes its output (5 activations); the MRF sum reads the running sum twice"""
    act = B * S * u * ch * 4
    return B * S * cin * 4 + act + 9 * 5 * act + 2 * act


def bench(args):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.vocoder import Generator

    h = wl.hifigan_config("v1")
    sd = wl.synth_vocoder_state_dict(h, seed=0)
    gen = Generator(h, matmul=args.matmul).to("cuda").eval()
    gen.load_state_dict(sd)
    mel, mel_lens = mel_from_forward(args.workload)
    B, _, T = mel.shape
    peak, frac = (BF16_MFMA_PEAK_TFLOPS, "frac_bf16_mfma_peak") if args.matmul == "bf16" else (F32_MFMA_PEAK_TFLOPS, "frac_fp32_mfma_peak")
    res = {"workload": args.workload, "matmul": args.matmul, "B": int(B), "T_pad": int(T), "valid_frames": int(mel_lens.sum()),
           "mel_std": round(float(mel.std()), 4)}
    with torch.no_grad():
        med, lo, hi = events_ms(lambda: gen(mel), args.steps, args.warmup)
    fl = wl.vocoder_flops_per_frame(h)
    flops = sum(fl.values()) * B * T
    audio_s = float(mel_lens.sum()) * 256 / 22050.0
    res.update({"ms_per_batch": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                "audio_seconds_per_second": round(audio_s / (med / 1e3), 1),
                "gflop_per_batch": round(flops / 1e9, 1), "tflops": round(flops / (med / 1e3) / 1e12, 2),
                frac: round(flops / (med / 1e3) / 1e12 / peak, 3)})
    # per stage: the same kernels the forward runs, one entry point each, timed with device events
    x = mel.transpose(1, 2).contiguous()
    stages = {}
    with torch.no_grad():
        t, _, _ = events_ms(lambda: gen.op_conv("conv_pre", x), args.steps, 1)
        stages["conv_pre"] = {"ms": round(t, 3), "gflop": round(fl["conv_pre"] * B * T / 1e9, 2)}
        y = gen.op_conv("conv_pre", x)
        S = T
        for i, u in enumerate(h["upsample_rates"]):
            cin, ch = y.shape[2], y.shape[2] // 2
            t, _, _ = events_ms(lambda: gen.op_stage(i, y), args.steps, 1)
            f = fl[f"stage{i}"] * B * T
            by = stage_bytes(B, S, cin, u, ch)
            stages[f"stage{i}"] = {"ms": round(t, 3), "gflop": round(f / 1e9, 1), "tflops": round(f / (t / 1e3) / 1e12, 2),
                                   frac: round(f / (t / 1e3) / 1e12 / peak, 3),
                                   "min_hbm_gb": round(by / 1e9, 2), "frac_hbm_peak": round(by / (t / 1e3) / 1e9 / HBM_PEAK_GBS, 3)}
            y = gen.op_stage(i, y)
            S *= u
        t, _, _ = events_ms(lambda: gen.op_conv("conv_post", y), args.steps, 1)
        by = y.numel() * 4 + B * S * 4
        stages["conv_post"] = {"ms": round(t, 3), "gflop": round(fl["conv_post"] * B * T / 1e9, 2),
                               "frac_hbm_peak": round(by / (t / 1e3) / 1e9 / HBM_PEAK_GBS, 3)}
    res["stages"] = stages
    res["stages_sum_ms"] = round(sum(s["ms"] for s in stages.values()), 3)
    if args.torch:
        from tests import hifigan_cpu

        ref = hifigan_cpu.folded(h, sd).cuda()
        with torch.no_grad():
            tm, _, _ = events_ms(lambda: ref(mel), max(2, args.steps // 2), 1)
            d = float((ref(mel) - gen(mel)).abs().max())
        res["torch_conv1d"] = {"ms_per_batch": round(tm, 3), "speedup_of_hip": round(tm / med, 2), "max_abs_diff_vs_hip": d}
    return res


def accuracy(args):
    """per layer: worst |y - f64| / conv(|x|, |W|) of the GPU and of torch's CPU fp32, and their ratio (B = 3, 33 frames)"""
    if args.matmul == "bf16":
        return accuracy_bf16(args)
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.vocoder import Generator
    from tests import hifigan_cpu

    h = wl.hifigan_config("v1")
    sd = wl.synth_vocoder_state_dict(h, seed=0)
    gen = Generator(h).to("cuda").eval()
    gen.load_state_dict(sd)
    r64 = hifigan_cpu.folded(h, sd, torch.float64)
    r32 = hifigan_cpu.folded(h, sd, torch.float32)
    rs = np.random.RandomState(1)
    rows = []
    S = 33
    for i in range(4):
        S_i = S * int(np.prod(h["upsample_rates"][:i]))
        up, up32 = r64.ups[i], r32.ups[i]
        u, k = h["upsample_rates"][i], h["upsample_kernel_sizes"][i]
        x = torch.from_numpy(rs.standard_normal((3, S_i, up.in_channels)).astype(np.float32))
        a = F.leaky_relu(x.double(), 0.1).transpose(1, 2)
        ref = F.conv_transpose1d(a, up.weight, up.bias, stride=u, padding=(k - u) // 2).transpose(1, 2)
        unit = F.conv_transpose1d(a.abs(), up.weight.abs(), up.bias.abs(), stride=u, padding=(k - u) // 2).transpose(1, 2)
        with torch.no_grad():
            c32 = F.conv_transpose1d(F.leaky_relu(x, 0.1).transpose(1, 2), up32.weight, up32.bias, stride=u, padding=(k - u) // 2).transpose(1, 2)
        g = gen.op_upsample(i, x.cuda()).cpu()
        rows.append(_acc_row(f"ups.{i}", 2 * up.in_channels, g, c32, ref, unit))
        S_o = S_i * u
        for j in range(3):
            rb = 3 * i + j
            for n in range(3):
                for which in (1, 2):
                    conv, conv32 = getattr(r64.resblocks[rb], f"convs{which}")[n], getattr(r32.resblocks[rb], f"convs{which}")[n]
                    ch, kk = conv.in_channels, conv.kernel_size[0]
                    x = torch.from_numpy(rs.standard_normal((3, S_o, ch)).astype(np.float32))
                    a = F.leaky_relu(x.double(), 0.1).transpose(1, 2)
                    kw = dict(padding=conv.padding[0], dilation=conv.dilation[0])
                    ref = F.conv1d(a, conv.weight, conv.bias, **kw).transpose(1, 2)
                    unit = F.conv1d(a.abs(), conv.weight.abs(), conv.bias.abs(), **kw).transpose(1, 2)
                    with torch.no_grad():
                        c32 = F.conv1d(F.leaky_relu(x, 0.1).transpose(1, 2), conv32.weight, conv32.bias, **kw).transpose(1, 2)
                    g = gen.op_conv(f"resblocks.{rb}.convs{which}.{n}", x.cuda()).cpu()
                    rows.append(_acc_row(f"resblocks.{rb}.convs{which}.{n}", ch * kk, g, c32, ref, unit))
    mel = torch.from_numpy(rs.standard_normal((3, 80, S)).astype(np.float32))
    with torch.no_grad():
        ref = r64(mel.double())
        c32 = r32(mel).double()
    g = gen(mel.cuda()).cpu().double()
    whole = {"wav_std": float(ref.std()), "gpu_max_abs": float((g - ref).abs().max()), "cpu_fp32_max_abs": float((c32 - ref).abs().max())}
    whole["ratio"] = whole["gpu_max_abs"] / whole["cpu_fp32_max_abs"]
    return {"layers": rows, "generator": whole}


def accuracy_bf16(args):
    """bf16 mode.  Per layer (B = 3, 33 frames): worst |gpu - emu| / (conv(|a_bf16|, |w_bf16|) + |bias|), emu = the CPU bf16
    emulation of tests/hifigan_bf16_emu.py in float64 (only the fp32 summation order differs), next to the 2^-9 of one bf16
    rounding.  Whole generator: waveform SNR against float64 and against the fp32 GPU run, and the emulation's own SNR."""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.vocoder import Generator
    from tests import hifigan_cpu
    from tests.hifigan_bf16_emu import bf, emulation, snr_db
    from tests.hifigan_bf16_emu import lrelu32 as _lrelu32

    h = wl.hifigan_config("v1")
    sd = wl.synth_vocoder_state_dict(h, seed=0)
    gen = Generator(h, matmul="bf16").to("cuda").eval()
    gen.load_state_dict(sd)
    g32 = Generator(h).to("cuda").eval()
    g32.load_state_dict(sd)
    r64, emu = hifigan_cpu.folded(h, sd, torch.float64), emulation(h, sd)
    rs = np.random.RandomState(1)
    rows, S = [], 33

    def row(name, K, g, ref, unit):
        return {"layer": name, "K": K, "gpu_vs_emu": float(((g.double() - ref).abs() / unit.clamp_min(1e-30)).max())}

    for i in range(4):
        S_i = S * int(np.prod(h["upsample_rates"][:i]))
        up = emu.ups[i]
        u, k = h["upsample_rates"][i], h["upsample_kernel_sizes"][i]
        x = torch.from_numpy(rs.standard_normal((3, S_i, up.in_channels)).astype(np.float32))
        a = bf(_lrelu32(x)).double().transpose(1, 2)
        kw = dict(stride=u, padding=(k - u) // 2)
        ref = F.conv_transpose1d(a, up.weight.detach(), up.bias.detach(), **kw).transpose(1, 2)
        unit = F.conv_transpose1d(a.abs(), up.weight.detach().abs(), up.bias.detach().abs(), **kw).transpose(1, 2)
        rows.append(row(f"ups.{i}", 2 * up.in_channels, gen.op_upsample(i, x.cuda()).cpu(), ref, unit))
        for j in range(3):
            rb = 3 * i + j
            for n in range(3):
                for which in (1, 2):
                    conv = getattr(emu.resblocks[rb], f"convs{which}")[n]
                    ch, kk = conv.in_channels, conv.kernel_size[0]
                    x = torch.from_numpy(rs.standard_normal((3, S_i * u, ch)).astype(np.float32))
                    a = bf(_lrelu32(x)).double().transpose(1, 2)
                    kw = dict(padding=conv.padding[0], dilation=conv.dilation[0])
                    ref = F.conv1d(a, conv.weight.detach(), conv.bias.detach(), **kw).transpose(1, 2)
                    unit = F.conv1d(a.abs(), conv.weight.detach().abs(), conv.bias.detach().abs(), **kw).transpose(1, 2)
                    g = gen.op_conv(f"resblocks.{rb}.convs{which}.{n}", x.cuda()).cpu()
                    rows.append(row(f"resblocks.{rb}.convs{which}.{n}", ch * kk, g, ref, unit))
    whole = {}
    mels = {"ragged_N(0,1)_B3_T33": torch.from_numpy(rs.standard_normal((3, 80, S)).astype(np.float32)),
            "N(0,0.56^2)_B2_T48": torch.from_numpy((0.56 * np.random.RandomState(1).standard_normal((2, 80, 48))).astype(np.float32))}
    for name, mel in mels.items():
        with torch.no_grad():
            ref = r64(mel.double())[:, 0]
            e = emu(mel.double())[:, 0]
        g = gen(mel.cuda())[:, 0].cpu().double()
        f = g32(mel.cuda())[:, 0].cpu().double()
        whole[name] = {"wav_std": float(ref.std()), "snr_db_vs_f64": snr_db(ref, g), "snr_db_vs_fp32_gpu": snr_db(f, g),
                       "emu_snr_db_vs_f64": snr_db(ref, e), "max_abs_vs_f64": float((g - ref).abs().max())}
    return {"matmul": "bf16", "layers": rows, "generator": whole}


def _acc_row(name, K, g, c32, ref, unit):
    eg = float(((g.double() - ref).abs() / unit.clamp_min(1e-30)).max())
    ec = float(((c32.double() - ref).abs() / unit.clamp_min(1e-30)).max())
    return {"layer": name, "K": K, "gpu": eg, "cpu_fp32": ec, "ratio": eg / ec if ec > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2_b16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--matmul", choices=("fp32", "bf16"), default="fp32", help="the Generator's matmul mode")
    ap.add_argument("--torch", action="store_true", help="also time the same generator on torch-ROCm's conv1d (comparison line)")
    ap.add_argument("--accuracy", action="store_true", help="per-layer float64 distances instead of timing")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vocoder_bench needs the MI355X")
    t0 = time.time()
    res = accuracy(a) if a.accuracy else bench(a)
    res["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
