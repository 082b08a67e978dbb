#!/usr/bin/env python3
"""The Gaussian length regulator's backward (csrc/gaussgrad.hip through ns_va_op_gu_bwd) on one MI355X, at config 2's training shape
(16 utterances of 128 phonemes, 1000 frames, d 256) and at config 5's long-form shape (8 x 128 phonemes at 31 frames each, 3968 frames).

Per shape, in one process, candidates alternating step by step, device events around the enqueue and wall clock to a synchronise,
medians over --steps after --warmup:
  * ns_va_op_gu_bwd: the denominators and the banded contraction (two launches; the entry point has no form with fewer)
  * ns_va_op_gu_bwd_unbanded: the same with every tile walking every live frame — what the 102-frame band saves
  * ns_va_op_gu_fwd, the three launches of the training forward, for scale
  * ns_va_op_lr_bwd, the hard regulator's backward at the same durations
  * torch-ROCm's autograd of the dense formulation (exp, sum, divide, matmul over [B, L, T]): forward + backward, which is what it takes
    to get d_x from it
Then one config-2 train_step (tools/train_bench.py's stages) with model_config["length_regulator"] absent and "gaussian".  --report adds
the shares of the bound tests/test_gpu_gaussian_grad.py appended to NS_FP32_OPS_REPORT.  Nothing about speed is asserted; every figure
is one run's, and a part that did not run is reported as such.

    python tools/gaussian_grad_bench.py --steps 20 --warmup 5 --md profiles/gaussian_grad.md
"""
import argparse
import json

import numpy as np
import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit

SHAPES = {"config 2: 16 x 128 phonemes, 1000 frames": (16, 128, 256, 1000, 7.8),
          "config 5 long-form: 8 x 128 phonemes, 3968 frames": (8, 128, 256, 3968, 31.0)}


def durations(rs, B, L, T, per_phoneme):
    """[B, L] int64: ragged utterances (the first one full) around ``per_phoneme`` frames each, totals at most T, the longest reaching it"""
    d = np.maximum(np.rint(rs.normal(per_phoneme, per_phoneme / 3.0, size=(B, L))), 0).astype(np.int64)
    src_lens = rs.randint(L // 2, L + 1, size=B)
    src_lens[0] = L
    d[np.arange(L)[None, :] >= src_lens[:, None]] = 0
    for b in range(B):
        while d[b].sum() > T:
            d[b, rs.randint(src_lens[b])] //= 2
    d[0, L // 2] += T - d[0].sum()
    return d


def dense(x, dur, mel_len, T):
    """the reference module's formulation in torch ops, frames at or past an utterance's total zeroed"""
    d = dur.to(x.dtype)
    c = (torch.cumsum(d, -1) - 0.5 * d).unsqueeze(-1)
    t = torch.arange(T, device=x.device, dtype=x.dtype)[None, None, :]
    e = torch.exp(-0.01 * (t - c) ** 2)
    w = e / (e.sum(1, keepdim=True) + 1e-20)
    out = torch.matmul(w.transpose(1, 2), x)
    return out.masked_fill((torch.arange(T, device=x.device)[None, :] >= mel_len[:, None]).unsqueeze(-1), 0.0)


def kernel_candidates(B, L, D, T, per_phoneme, seed):
    import smart_nar_fast_tts_amd._lib as Lb

    lib = Lb.load()
    P, S = Lb.ptr, Lb.stream_ptr
    rs = np.random.RandomState(seed)
    dur = torch.from_numpy(durations(rs, B, L, T, per_phoneme)).cuda()
    x, g = torch.randn(B, L, D, device="cuda"), torch.randn(B, T, D, device="cuda")
    out, dx = torch.empty(B, T, D, device="cuda"), torch.empty(B, L, D, device="cuda")
    saved, mel_len = torch.empty(B, L, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
    cum = torch.empty(B, L, dtype=torch.int32, device="cuda")
    n = lib.ns_va_gu_ws_bytes(B, L, T)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    Lb.check(lib.ns_va_op_gu_fwd(P(x), P(dur), B, L, D, T, P(out), P(saved), P(mel_len), P(ws), n, S()), "gu_fwd")
    Lb.check(lib.ns_va_op_lr_fwd(P(x), P(dur), B, L, D, T, P(out), P(cum), P(mel_len), S()), "lr_fwd")
    xg = x.clone().requires_grad_(True)

    def torch_dense():
        dense(xg, dur, mel_len, T).backward(g)

    calls = {
        "ns_va_op_gu_bwd (denominators + banded contraction)": lambda: Lb.check(lib.ns_va_op_gu_bwd(P(g), P(saved), P(mel_len), B, L, D, T, P(dx), None, P(ws), n, S()), "gu_bwd"),
        "ns_va_op_gu_bwd_unbanded (every live frame)": lambda: Lb.check(lib.ns_va_op_gu_bwd_unbanded(P(g), P(saved), P(mel_len), B, L, D, T, P(dx), None, P(ws), n, S()), "gu_bwd"),
        "ns_va_op_gu_fwd (prepare + centres + upsample)": lambda: Lb.check(lib.ns_va_op_gu_fwd(P(x), P(dur), B, L, D, T, P(out), P(saved), P(mel_len), P(ws), n, S()), "gu_fwd"),
        "ns_va_op_lr_bwd (the hard regulator's backward)": lambda: Lb.check(lib.ns_va_op_lr_bwd(P(g), P(cum), B, L, D, T, P(dx), S()), "lr_bwd"),
        "torch-ROCm autograd of the dense formulation, forward + backward": torch_dense,
    }
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    return [Candidate(k, f, [xg] if f is torch_dense else ()) for k, f in calls.items()]


def train_steps(steps, warmup):
    import smart_nar_fast_tts_amd.workload as wl
    from train_bench import bench_step, config2_batch

    cfg = wl.model_config("ljspeech")
    sd = wl.synth_state_dict(cfg, seed=0)
    sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
    batch = config2_batch(cfg)
    return [bench_step(f"config 2 train_step, length_regulator {name}", wl.preprocess_config(), c, sd, batch, steps, warmup)
            for name, c in (("absent (hard)", cfg), ("\"gaussian\"", dict(cfg, length_regulator="gaussian")))]


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, 20, 5)
    ap.add_argument("--report")
    ap.add_argument("--no-train-step", action="store_true", help="skip the two config-2 train steps")
    ap.add_argument("--note", help="one paragraph appended as it is (the inference benchmark against the parent's build)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = {"kernels": {}, "train_steps": None}
    lines = ["# The Gaussian length regulator's backward", "", "Written by `tools/gaussian_grad_bench.py`.  One MI355X, one run; device events around the enqueue "
             f"and wall clock to a synchronise, medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, ms; candidates alternate step by "
             "step in one process.  Nothing about speed is asserted.", ""]
    for i, (name, (B, L, D, T, per)) in enumerate(SHAPES.items()):
        cands = kernel_candidates(B, L, D, T, per, 40 + i)
        alternate(cands, args.steps, args.warmup)
        results["kernels"][name] = [c.result() for c in cands]
        lines += [f"## {name}, d {D}", ""] + candidate_table(results["kernels"][name]) + [""]
    if args.no_train_step:
        lines += ["## config-2 train_step", "", "Not run (--no-train-step).", ""]
    else:
        results["train_steps"] = train_steps(max(args.steps // 2, 3), 2)
        for r in results["train_steps"]:
            lines += [f"## {r['name']}", "", "| stage | p50 ms (min - max) | launches | host reads |", "|---|---|---|---|"]
            for s, v in r["stages"].items():
                lines.append(f"| {s} | {v['median_ms']:.3f} ({v['min_ms']:.3f} - {v['max_ms']:.3f}) | {v['launches']} | {v['host_reads']} |")
            lines.append("")
    if args.report:
        lines += ["## Shares of the bound (tests/test_gpu_gaussian_grad.py; tests/gaussian_grad_cpu.py states the bound)", ""]
        for r in (json.loads(x) for x in open(args.report) if x.strip()):
            if str(r.get("test", "")).startswith("gaussian_grad"):
                lines.append("* " + json.dumps(r))
        lines.append("")
    if args.note:
        lines += ["## The inference benchmark", "", args.note, ""]
    emit(args, lines, results)


if __name__ == "__main__":
    main()
