"""The opt-in precision modes side by side: fp32 (default), bf16x3 and bf16 (model_config["matmul"]) on the same weights and
inputs, BASELINE configs 1, 2, 4 and 5.  Per config and mode: p50 ms per forward (HIP events around the whole forward, 10 timed
after 3 warm-up), valid mel-frames/s, the achieved rate of the two heaviest GEMM groups (FFN w_1 and PostNet 512->512, the
library's dispatch-timed profile slots) as a fraction of the mode's matrix peak (fp32 157.3 TF, bf16 2.5 PF), and the mel /
PostNet mel deviation from the fp32 oracle with the oracle's pitch / energy as targets (every frame).

    python tools/bf16_forward.py [--configs cfg2_b16,...] [--modes fp32,bf16] [--no-oracle] [--json OUT] [--md OUT]

Kernel-level view of the same launches: run it under `rocprofv3 --kernel-trace --stats -- python tools/bf16_forward.py ...`.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {"fp32": 157.3e12, "bf16x3": 2.5e15, "bf16": 2.5e15}


def run_config(name, modes, oracle, steps=10, warmup=3):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    cfg_name, B, L, fpp = wl.WORKLOADS[name]
    cfg = wl.model_config(cfg_name)
    sd = wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=fpp)
    sp, tx, ln, Lm = wl.synth_inputs(B, L, seed=0)
    ref = None
    if oracle:
        from oracle import fs2_oracle as orc

        with torch.no_grad():
            ref = orc.forward(orc.to_torch_weights(sd), cfg, torch.from_numpy(sp), torch.from_numpy(tx), torch.from_numpy(ln), Lm)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    args = (d(sp), d(tx), d(ln), Lm)
    rows = {}
    for mode in modes:
        m = FastSpeech2Align(wl.preprocess_config(), dict(cfg, matmul=mode)).to("cuda").eval()
        m.load_state_dict(sd)
        with torch.no_grad():
            for _ in range(warmup):
                out = m(*args)
            torch.cuda.synchronize()
            ts = []
            for _ in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = m(*args)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            frames = int(out[9].sum())
            p50 = float(np.median(ts))
            r = {"p50_ms": p50, "valid_frames": frames, "frames_per_s": frames / (p50 * 1e-3)}
            for slot, key in ((0, "ffn_w1"), (2, "postnet_mid")):
                m.profile_slots((slot,))
                for _ in range(3):
                    m(*args)
                torch.cuda.synchronize()
                ms, fl, n = m.read_profile(slot)
                m.profile_slots(())
                if n:
                    r[key] = {"us_per_launch": ms * 1e3 / n, "tflops": fl / (ms * 1e-3) / 1e12, "frac_peak": fl / (ms * 1e-3) / PEAK[mode]}
            if ref is not None:
                t = m(*args, p_targets=ref[2].cuda(), e_targets=ref[3].cuda())
                torch.cuda.synchronize()
                assert torch.equal(t[9].cpu(), ref[9]), (name, mode, "frame counts differ from the oracle")
                for i, key in ((0, "mel"), (1, "postnet")):
                    dd = (t[i].cpu().double() - ref[i].double()).abs()
                    r[key + "_vs_oracle"] = {"max_abs": float(dd.max()), "mean_abs": float(dd.mean())}
        rows[mode] = r
        del m
        torch.cuda.empty_cache()
    if "fp32" in rows:
        for mode, r in rows.items():
            r["speedup_vs_fp32"] = rows["fp32"]["p50_ms"] / r["p50_ms"]
    return {"config": name, "B": B, "L": L, "model": cfg_name, "modes": rows}


def to_md(res):
    lines = ["| config | mode | p50 ms | valid frames/s | vs fp32 | FFN w_1 TF (frac of peak) | PostNet 512 TF (frac) | mel max / mean vs oracle | PostNet max / mean |",
             "|---|---|---|---|---|---|---|---|---|"]
    for c in res:
        for mode, r in c["modes"].items():
            f = lambda k: f"{r[k]['tflops']:.1f} ({r[k]['frac_peak']:.3f})" if k in r else "-"  # noqa: E731
            g = lambda k: f"{r[k]['max_abs']:.2e} / {r[k]['mean_abs']:.2e}" if k in r else "-"  # noqa: E731
            lines.append(f"| {c['config']} | {mode} | {r['p50_ms']:.3f} | {r['frames_per_s'] / 1e6:.3f} M | {r.get('speedup_vs_fp32', 1.0):.2f}x | "
                         f"{f('ffn_w1')} | {f('postnet_mid')} | {g('mel_vs_oracle')} | {g('postnet_vs_oracle')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg1_single,cfg2_b16,cfg4_d512,cfg5_longform")
    ap.add_argument("--modes", default="fp32,bf16x3,bf16")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--md")
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    res = []
    for name in a.configs.split(","):
        res.append(run_config(name, a.modes.split(","), not a.no_oracle))
        print(json.dumps(res[-1]), flush=True)
    md = to_md(res)
    print(md)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "results": res}, fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(md)


if __name__ == "__main__":
    main()
