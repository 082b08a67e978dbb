#!/usr/bin/env python3
"""Reference-mel aligner (FastSpeech2Align.align) on one MI355X at a workload's shape: mels = the model's own PostNet output, T from
the workload's mel_lens.  Prints (and optionally writes as JSON) the median of --steps align() calls after --warmup, the same for
this repository's forward (phase 1 + phase 2) and for the torch restatement of the aligner (tests/aligner_cpu.py) moved to
torch-ROCm, all on the same card.

    python tools/aligner_bench.py --workload cfg2_b16 --steps 10 --warmup 3 [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/aligner_bench.py --workload cfg2_b16 --only-align     # kernel split, a run of its own

Nothing here runs without the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2_b16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-align", action="store_true", help="skip the comparison legs (profiler runs)")
    ap.add_argument("--json")
    args = ap.parse_args()

    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align
    from tests import aligner_cpu as ac

    cfg_name, B, L, fpp = wl.WORKLOADS[args.workload]
    cfg = wl.model_config(cfg_name)
    sd = wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=fpp)
    sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
    m = FastSpeech2Align(wl.preprocess_config(), cfg).to("cuda").eval()
    m.load_state_dict(sd)
    sp, tx, ln, Lm = (torch.from_numpy(np.asarray(a)).cuda() if not isinstance(a, int) else a for a in wl.synth_inputs(B, L, seed=0))

    def forward():
        with torch.no_grad():
            return m(sp, tx, ln, Lm)

    out = forward()
    torch.cuda.synchronize()
    mels, mel_lens = out[1].contiguous(), out[9]
    T = int(mels.shape[1])
    res = {"workload": args.workload, "B": B, "L": L, "T": T, "valid_frames": int(mel_lens.sum()), "n_layer": cfg["transformer"]["decoder_layer"]}

    def align():
        return m.align(tx, ln, Lm, mels, mel_lens)

    res["align"] = events_ms(align, args.steps, args.warmup)
    a = align()
    torch.cuda.synchronize()
    res["durations_sum_equals_mel_lens"] = bool(torch.equal(a.durations.sum(dim=1), mel_lens))
    if not args.only_align:
        res["forward"] = events_ms(forward, args.steps, args.warmup)
        w = {k: v.cuda() for k, v in ac.to_torch_weights(sd).items()}

        def torch_rocm():
            with torch.no_grad():
                return ac.align(w, cfg, tx, ln, mels, mel_lens)

        res["torch_rocm_restatement"] = events_ms(torch_rocm, args.steps, args.warmup)
        t_out, t_attn = torch_rocm()
        res["max_abs_vs_torch_rocm"] = {"tgt_output": float((t_out - a.tgt_output).abs().max()),
                                        "alignment_last": float((t_attn[-1] - a.tgt_alignment[-1]).abs().max())}
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
