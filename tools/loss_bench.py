#!/usr/bin/env python3
"""Validation loss (loss.FastSpeech2Loss, csrc/loss.hip) on one MI355X at a workload's shape, behind the teacher-forced forward it
follows: mels = the model's own PostNet output, pitch / energy targets = its own predictions, T from the workload's mel_lens.  Per
workload: the median of --steps loss calls after --warmup (device events), the bytes the loss must read over that time as a share
of the HBM peak, the same arithmetic through the torch statement of tests/loss_cpu.py on the device (fp32; it ends in host reads, as
the reference's ``.item()`` logging does), and forward_teacher_forced() itself.  --md also records, from a CPU run of
tests/loss_cpu.py, how much of the tests' gate the fp32 evaluations use.

    python tools/loss_bench.py --workloads cfg2_b16 cfg5_longform --steps 30 --warmup 5 --md profiles/loss_r10.md

The timing part does not run without the GPU (--host-only: the gate shares alone)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s: data sheet; measured float4 copy


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
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def gate_shares():
    """fp32 evaluations on the CPU as shares of the gate: the reference's stored fp32 values and loss_cpu fp32 on the fixtures,
    loss_cpu fp32 on the seeded random cases."""
    from tests import loss_cpu as lc
    from tests.util import load_golden

    rows = []
    for name, source in (("loss_tiny", "teacher_tiny"), ("loss_tiny_phoneme_level", "teacher_tiny_phoneme_level")):
        _, z = load_golden(name)
        ms, zs = load_golden(source)
        i64, p64 = lc.fixture_case(zs, ms, "_f64")
        gate = lc.gates(i64, p64, ms["pitch"], ms["energy"])
        rows.append((name, "reference fp32", lc.shares(z["values"], z["values_f64"], gate)))
        i32, p32 = lc.fixture_case(zs, ms, "")
        rows.append((name, "loss_cpu fp32", lc.shares(lc.loss(i32, p32, ms["pitch"], ms["energy"], torch.float32), z["values_f64"], gate)))
    for name in lc.CASES:
        for level in lc.LEVELS:
            inputs, predictions, want, gate = lc.case(name, level)
            rows.append((f"{name} {level}", "loss_cpu fp32", lc.shares(lc.loss(inputs, predictions, level, level, torch.float32), want, gate)))
    return lc.NAMES, rows


def bench(workload, steps, warmup):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss
    from smart_nar_fast_tts_amd.model import FastSpeech2Align
    from tests import loss_cpu as lc

    cfg_name, B, L, fpp = wl.WORKLOADS[workload]
    cfg = wl.model_config(cfg_name)
    sd = wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=fpp)
    sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
    pc = wl.preprocess_config()
    m = FastSpeech2Align(pc, cfg).to("cuda").eval()
    m.load_state_dict(sd)
    sp, tx, ln, Lm = (torch.from_numpy(np.asarray(a)).cuda() if not isinstance(a, int) else a for a in wl.synth_inputs(B, L, seed=0))
    with torch.no_grad():
        free = m(sp, tx, ln, Lm)
    torch.cuda.synchronize()
    mels, mel_lens = free[1].contiguous(), free[9]
    T = int(mels.shape[1])
    batch = (None, None, sp, tx, ln, Lm, mels, mel_lens, T, free[2].contiguous(), free[3].contiguous())
    level = (pc["preprocessing"]["pitch"]["feature"], pc["preprocessing"]["energy"]["feature"])

    def teacher():
        return m.forward_teacher_forced(*batch[2:], async_status=True)

    out = teacher()
    out.check()
    loss = FastSpeech2Loss(pc, cfg)
    H = int(out[10][0].shape[1])
    frames = int((~out[7]).sum())
    cells = int((ln.clamp(0, L) * mel_lens.clamp(0, T)).sum())
    need = 3 * 4 * frames * int(mels.shape[2])
    need += 4 * 4 * cells + 2 * 4 * 2 * frames + 4 * 3 * int((~out[6]).sum())
    res = {"workload": workload, "B": B, "L": L, "T": T, "H": H, "unmasked_frames": frames, "attention_cells": cells, "bytes_needed": need,
           "bytes_dense": 3 * 4 * B * T * int(mels.shape[2]) + 4 * 4 * B * T * L}
    res["loss"] = events_ms(lambda: loss(batch, out), steps, warmup)
    s = res["loss"]["median_ms"] * 1e-3
    res["needed_bytes_per_s"] = need / s
    res["share_of_hbm_spec"] = need / s / HBM_SPEC
    res["share_of_hbm_copy_rate"] = need / s / HBM_COPY
    res["torch_statement_on_device"] = events_ms(lambda: lc.loss(batch, out, level[0], level[1], torch.float32), steps, warmup)
    res["teacher_forced_forward"] = events_ms(teacher, steps, warmup)
    res["loss_over_forward"] = res["loss"]["median_ms"] / res["teacher_forced_forward"]["median_ms"]
    got = torch.stack(loss(batch, out)).cpu().numpy()
    ref = lc.loss(batch, out, level[0], level[1], torch.float32)
    res["values"] = [float(v) for v in got]
    res["max_rel_vs_torch_statement"] = float(np.nanmax(np.abs(got - ref) / np.abs(ref)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["cfg2_b16", "cfg5_longform"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--md")
    ap.add_argument("--json")
    args = ap.parse_args()
    names, rows = gate_shares()
    results = [] if args.host_only else [bench(w, args.steps, args.warmup) for w in args.workloads]
    for r in results:
        print(json.dumps(r))
    lines = ["# Validation loss (csrc/loss.hip): measurements", "", "Written by `tools/loss_bench.py`.", ""]
    if results:
        lines += [f"## Time on one MI355X (device events, median of {args.steps} calls after {args.warmup} warm-up calls)", "",
                  "| workload | B, L, T, H | loss, ms (min - max) | bytes the loss must read | over time, TB/s | of 8.0 TB/s spec | of 6.29 TB/s copy rate | "
                  "torch statement on the device, ms | teacher-forced forward, ms | loss / forward |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in results:
            lo = r["loss"]
            lines.append(f"| {r['workload']} | {r['B']}, {r['L']}, {r['T']}, {r['H']} | {lo['median_ms']:.4f} ({lo['min_ms']:.4f} - {lo['max_ms']:.4f}) | "
                         f"{r['bytes_needed'] / 1e6:.2f} MB | {r['needed_bytes_per_s'] / 1e12:.3f} | {r['share_of_hbm_spec']:.3f} | {r['share_of_hbm_copy_rate']:.3f} | "
                         f"{r['torch_statement_on_device']['median_ms']:.3f} | {r['teacher_forced_forward']['median_ms']:.3f} | {r['loss_over_forward']:.4f} |")
        lines += ["", "Bytes the loss must read: three mel tensors on the unmasked frames, the four head-0 maps on the cells t < olen, l < ilen, the "
                  "per-frame and per-phoneme scalars.  The call time includes the host side of the call (argument checks, two launches); at these "
                  "sizes it is a whole-call rate, not a kernel's share of peak.  The torch statement ends in host reads.", ""]
    else:
        lines += ["## Time on one MI355X", "", "Not measured: this record was written with `--host-only`; no MI355X run of the loss has been "
                  "made yet.  Run the command in this tool's docstring on the GPU to fill in call time, bytes over time as a share of the HBM "
                  "peak, the torch statement on the device and the share of the teacher-forced forward.", ""]
    lines += ["## Share of the tests' gate used by fp32 evaluations on the CPU (`tests/loss_cpu.py`; the gate: `tests/test_loss_host.py`)", "",
              "| case | evaluation | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
    for case, who, share in rows:
        lines.append(f"| {case} | {who} | " + " | ".join(f"{v:.4f}" for v in share) + " |")
    worst = max(float(np.max(s)) for _, _, s in rows)
    lines += ["", f"Largest share: {worst:.4f} (the tests demand < 1/3)."]
    text = "\n".join(lines) + "\n"
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(text)
    else:
        print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
