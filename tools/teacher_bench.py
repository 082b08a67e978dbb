#!/usr/bin/env python3
"""Teacher-forced forward (FastSpeech2Align.forward_teacher_forced) on one MI355X at a workload's shape: mels = the model's own
PostNet output, T and mel_lens from the workload's free-running forward.  Per workload, the median of --steps calls after --warmup
(an event pair around each call, tools/aligner_bench.py's method, the legs alternating inside one loop) of

    teacher_forced            forward_teacher_forced(..., async_status=True): one encoder pass, no host read
    align_then_forward        align() followed by forward(max_mel_len=T, async_status=True) on the same inputs — what a caller could do
                              before this method existed (both calls are unchanged from the parent commit): two encoder passes, and
                              the decoder runs on the PREDICTED durations, so it is a cost comparison, not the same function
    align / forward_capacity  the two halves alone

and writes them, with the expectation they confirm or refute, as a markdown table.

    python tools/teacher_bench.py --workloads cfg2_b16 cfg1_single --steps 20 --warmup 5 --md profiles/teacher_forced_r08.md

Nothing here runs without the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402



def alternating_ms(legs, steps, warmup):
    """tools/aligner_bench.events_ms's event pair around each call, with the legs ALTERNATING inside one timed loop: whatever else
    shares the host or the card during the run falls on all of them alike."""
    for _ in range(warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _ in legs}
    for _ in range(steps):
        for k, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ts.items()}


def measure(name, steps, warmup):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    cfg_name, B, L, fpp = wl.WORKLOADS[name]
    cfg = wl.model_config(cfg_name)
    sd = wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=fpp)
    sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
    m = FastSpeech2Align(wl.preprocess_config(), cfg).to("cuda").eval()
    m.load_state_dict(sd)
    sp, tx, ln, Lm = (torch.from_numpy(np.asarray(a)).cuda() if not isinstance(a, int) else a for a in wl.synth_inputs(B, L, seed=0))
    with torch.no_grad():
        out = m(sp, tx, ln, Lm)
    torch.cuda.synchronize()
    mels, mel_lens = out[1].contiguous(), out[9].clone()
    T = int(mels.shape[1])
    res = {"workload": name, "B": B, "L": L, "T": T, "valid_frames": int(mel_lens.sum())}

    def teacher():
        return m.forward_teacher_forced(sp, tx, ln, Lm, mels, mel_lens, T, async_status=True)

    def align():
        return m.align(tx, ln, Lm, mels, mel_lens)

    def forward_capacity():
        return m(sp, tx, ln, Lm, max_mel_len=T, async_status=True)

    def both():
        align()
        return forward_capacity()

    res.update(alternating_ms((("teacher_forced", teacher), ("align_then_forward", both), ("align", align), ("forward_capacity", forward_capacity)),
                              steps, warmup))
    o = teacher()
    res["status_clean"] = o.check() == [0] * B
    res["durations_sum_equals_mel_lens"] = bool(torch.equal(o[11].sum(dim=1), mel_lens))
    res["same_durations_as_align"] = bool(torch.equal(o[11], align().durations))
    return res


def markdown(results, steps, warmup):
    lines = ["# Teacher-forced forward: measurement (recorded, not gated)", "",
             f"Produced by `tools/teacher_bench.py` (median of {steps} calls after {warmup} warm-up, an event pair around each call, the legs alternating in one loop, one MI355X;",
             "mels = the model's own PostNet output, T and mel_lens from the workload's free-running forward).  `align() + forward()` is",
             "`align()` followed by `forward(max_mel_len=T, async_status=True)` on the same inputs, both unchanged from the parent commit:",
             "the only way to approximate the branch before this method existed.  It runs the text encoder twice and decodes with the",
             "PREDICTED durations, so the comparison is one of cost, not of function.", "",
             "Hypothesis recorded before the run: one encoder pass fewer, and no device-to-host read anywhere on the enqueue path, so",
             "`forward_teacher_forced()` should cost no more than `align() + forward()` at either shape.  No test asserts a time.", "",
             "| workload | B | L | T | forward_teacher_forced ms | align() + forward() ms | ratio | align() ms | forward(capacity) ms |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        t, b = r["teacher_forced"]["median_ms"], r["align_then_forward"]["median_ms"]
        lines.append(f"| {r['workload']} | {r['B']} | {r['L']} | {r['T']} | {t:.3f} ({r['teacher_forced']['min_ms']:.3f}-{r['teacher_forced']['max_ms']:.3f}) | "
                     f"{b:.3f} ({r['align_then_forward']['min_ms']:.3f}-{r['align_then_forward']['max_ms']:.3f}) | {t / b:.2f} | "
                     f"{r['align']['median_ms']:.3f} | {r['forward_capacity']['median_ms']:.3f} |")
    lines += ["", "(median, min-max in brackets.)  Checks made beside the timing, per workload: " +
              "; ".join(f"{r['workload']}: status clean {r['status_clean']}, sum of durations == mel_lens {r['durations_sum_equals_mel_lens']}, "
                        f"durations == align()'s {r['same_durations_as_align']}" for r in results) + ".", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["cfg2_b16", "cfg1_single"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md")
    ap.add_argument("--json")
    args = ap.parse_args()
    results = [measure(w, args.steps, args.warmup) for w in args.workloads]
    print(json.dumps(results))
    for path, text in ((args.md, markdown(results, args.steps, args.warmup)), (args.json, json.dumps(results, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
