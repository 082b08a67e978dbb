#!/usr/bin/env python3
"""Measure the wave-to-mel front end (audio.TacotronSTFT) on the MI355X and write profiles/melfront_r11.md:

  * the shares of the derived gates (tests/melfront_cpu.py) the HIP values and the reference's stored fp32 values use, per case;
  * time per batch at the config-2 size — B = 16 waves of 256 000 samples, ~1000 frames each — from HIP events;
  * the three launches' own times from `rocprofv3 --kernel-trace --stats`, in a run of their own (a fresh child process, started
    before this process opens the GPU);
  * the same batch through torch-ROCm ops on the same card: F.pad(reflect) + F.conv1d(stride = hop) + matmul + log, i.e. the
    reference's arithmetic without its .cpu().

    python tools/melfront_bench.py [--out profiles/melfront_r11.md] [--no-rocprof]

A number that could not be measured is written as "not measured", never guessed."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

B2, N2 = 16, 256000  # the config-2 batch
KERNELS = ("k_mel_frame_rows", "k_conv_gemm", "k_mel_project")


def config2_batch(torch):
    g = torch.Generator(device="cpu").manual_seed(0)
    return (torch.randn(B2, N2, generator=g) * 0.3).clamp_(-1, 1).cuda()


def loop(iters):
    """what the rocprofv3 child runs: nothing but front-end calls on the config-2 batch"""
    import torch

    import melfront_cpu as mc
    from smart_nar_fast_tts_amd import audio as A

    c = mc.LJSPEECH
    st = A.TacotronSTFT(c["filter_length"], c["hop_length"], c["win_length"], c["n_mel_channels"], c["sampling_rate"], c["mel_fmin"], c["mel_fmax"]).to("cuda:0")
    y = config2_batch(torch)
    for _ in range(iters):
        st.mel_spectrogram(y)
    torch.cuda.synchronize()


def rocprof_stats(iters=12):
    """{kernel: (calls, mean us)} from a rocprofv3 run of --loop, or None with the reason"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="melfront_prof_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                            "--loop", str(iters)], capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            return None, f"rocprofv3 exited with {r.returncode}"
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "no kernel_stats.csv written"
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    calls, total = int(row["Calls"]), float(row["TotalDurationNs"])
                    c0, t0 = out.get(k, (0, 0.0))
                    out[k] = (c0 + calls, t0 + total)
        return {k: (c, t / c / 1e3) for k, (c, t) in out.items() if c}, ""
    except Exception as e:  # a profiler that cannot run is reported, not fatal
        return None, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(d, ignore_errors=True)


def timed(torch, fn, warmup=3, iters=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melfront_r11.md"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--loop", type=int, default=0)
    a = ap.parse_args()
    if a.loop:
        return loop(a.loop)
    prof, why = (None, "switched off (--no-rocprof)") if a.no_rocprof else rocprof_stats()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import melfront_cpu as mc
    from smart_nar_fast_tts_amd import audio as A

    lines = ["# Wave-to-mel front end (audio.TacotronSTFT, csrc/melfront.hip): gate shares and time per batch", "",
             f"Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}.  Written by tools/melfront_bench.py.", "",
             "## Shares of the derived gates (tests/melfront_cpu.py; 1.0 = the gate)", "",
             "| case | utterance | frames | HIP mel | HIP energy | reference fp32 mel | reference fp32 energy |", "|---|---|---|---|---|---|---|"]
    stfts = {}
    for name, cfg in (("tiny", mc.TINY), ("ljspeech", mc.LJSPEECH)):
        st = A.TacotronSTFT(cfg["filter_length"], cfg["hop_length"], cfg["win_length"], cfg["n_mel_channels"], cfg["sampling_rate"], cfg["mel_fmin"],
                            cfg["mel_fmax"]).to("cuda:0")
        stfts[name] = st
        z = np.load(os.path.join(ROOT, "tests", "golden", f"melfront_{name}.npz"))
        n_waves = json.loads(str(z["meta"]))["n_waves"]
        waves = [z[f"wave{i}"] for i in range(n_waves)]
        y = np.zeros((n_waves, max(len(w) for w in waves)), np.float32)
        for i, w in enumerate(waves):
            y[i, :len(w)] = w
        mel, energy = st.mel_spectrogram(torch.from_numpy(y).cuda(), [len(w) for w in waves])
        mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
        for i, w in enumerate(waves):
            r = mc.reference64(w, cfg)
            t = len(w) // cfg["hop_length"] + 1
            hip, ref = mc.shares(mel[i, :, :t], energy[i, :t], r), mc.shares(z[f"mel{i}"], z[f"energy{i}"], r)
            lines.append(f"| fixture {name} | {i} | {t} | {hip['mel']:.3f} | {hip['energy']:.3f} | {ref['mel']:.3f} | {ref['energy']:.3f} |")
    rs = np.random.RandomState(3)
    st, cfg = stfts["ljspeech"], mc.LJSPEECH
    for n in (5000, 513, 2047, 65536):
        w = np.clip(rs.standard_normal(n) * 0.3, -1, 1).astype(np.float32)
        mel, energy = st.mel_spectrogram(torch.from_numpy(w[None]).cuda())
        hip = mc.shares(mel[0].cpu().numpy(), energy[0].cpu().numpy(), mc.reference64(w, cfg))
        lines.append(f"| random ljspeech n = {n} | 0 | {n // 256 + 1} | {hip['mel']:.3f} | {hip['energy']:.3f} | not measured | not measured |")

    # ---- time per batch, config-2 size
    y = config2_batch(torch)
    hip_ms = timed(torch, lambda: st.mel_spectrogram(y))
    fb = st.forward_basis.cuda()
    mb = st.mel_basis.cuda()
    half = cfg["filter_length"] // 2

    def torch_ops():
        x = F.pad(y.clamp(-1, 1)[:, None, None, :], (half, half, 0, 0), mode="reflect")[:, 0]
        ft = F.conv1d(x, fb, stride=cfg["hop_length"])
        mag = torch.sqrt(ft[:, :half + 1] ** 2 + ft[:, half + 1:] ** 2)
        return torch.log(torch.clamp(torch.matmul(mb, mag), min=1e-5)), torch.norm(mag, dim=1)

    ops_ms = timed(torch, torch_ops)
    m_ops, e_ops = torch_ops()
    m_hip, e_hip = st.mel_spectrogram(y)
    dmel, de = float((m_ops - m_hip).abs().max()), float(((e_ops - e_hip).abs() / e_ops.abs().clamp(min=1e-30)).max())
    T = N2 // 256 + 1
    lines += ["", f"## Time per batch: B = {B2} waves of {N2} samples ({T} frames each), HIP events, median (min - max) of 10 after 3 warm-up calls", "",
              "| path | ms per batch |", "|---|---|",
              f"| HIP front end, three launches | {hip_ms[0]:.3f} ({hip_ms[1]:.3f} - {hip_ms[2]:.3f}) |",
              f"| torch-ROCm ops on the same card: clamp + F.pad(reflect) + F.conv1d(stride = hop) + sqrt + matmul + clamp + log + norm | {ops_ms[0]:.3f} ({ops_ms[1]:.3f} - {ops_ms[2]:.3f}) |",
              "", f"The two agree to max |mel difference| = {dmel:.3e} and max relative energy difference = {de:.3e} on this batch.",
              "", "## The three launches (rocprofv3 --kernel-trace --stats, a run of its own over the same batch)", ""]
    if prof:
        lines += ["| kernel | calls | mean us |", "|---|---|---|"]
        lines += [f"| {k} | {prof[k][0]} | {prof[k][1]:.1f} |" if k in prof else f"| {k} | not measured | not measured |" for k in KERNELS]
    else:
        lines.append(f"not measured ({why})")
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
