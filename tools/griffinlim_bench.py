#!/usr/bin/env python3
"""Time the HIP Griffin-Lim (audio.griffin_lim, ns_gl_*; audio/audio_processing.py:66-82, audio/stft.py:52-122) on the MI355X.

    python tools/griffinlim_bench.py [--iters 60] [--frames 1000] [--batch 16] [--repeats 5] [--json out.json]

Reports, per shape (the batch and one utterance): the time of ``--iters`` iterations (device events around the whole loop, median of
``--repeats`` after one warm-up run of the same shape), the two GEMMs' FLOP over that time, and the split of one iteration measured
operator by operator through the ns_gl_op_* entry points: hop rows, phase step, inverse (its GEMM and the overlap-add gather
together), and the forward STFT GEMM as the remainder of the step.  Every stage prints a line as it finishes.  HIP only: a torch-ROCm
``conv1d`` / ``conv_transpose1d`` baseline is not part of this tool (profiles/griffinlim_r12.md).  Needs the GPU; no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smart_nar_fast_tts_amd import _lib  # noqa: E402
from smart_nar_fast_tts_amd import audio as A  # noqa: E402

FL, HOP, WIN = 1024, 256, 1024


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("griffinlim_bench needs the MI355X: a CPU run gives no time")
    fn = A.STFT(FL, HOP, WIN).to("cuda:0")
    so, cut = _lib.load(), FL // 2 + 1
    results = []
    for B in (args.batch, 1):
        T = args.frames
        rs = np.random.RandomState(B)
        mag = torch.from_numpy(np.exp(rs.uniform(0, 4.6, (B, T, cut))).astype(np.float32)).cuda()
        ang = torch.from_numpy(rs.uniform(-np.pi, np.pi, (B, T, cut)).astype(np.float32)).cuda()
        lens = torch.full((B,), T, dtype=torch.long, device="cuda")
        print(f"B={B} T={T}: inputs on the device", flush=True)
        hip = timed(lambda: A.griffin_lim(mag.transpose(1, 2), fn, n_iters=args.iters, angles=ang.transpose(1, 2), lens=lens), args.repeats)
        print(f"B={B} T={T}: {args.iters} iterations {hip[0]:.3f} ms ({hip[1]:.3f} - {hip[2]:.3f})", flush=True)
        y_hip = A.griffin_lim(mag.transpose(1, 2), fn, n_iters=2, angles=ang.transpose(1, 2), lens=lens)
        assert bool(torch.isfinite(y_hip).all())
        # the split of one iteration, operator by operator (50 calls each inside one timed window)
        n_ws = int(so.ns_gl_ws_bytes(fn._h, B, T))
        ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
        S, n = T + FL // HOP - 1, HOP * (T - 1)
        wave, wl = y_hip.clone(), torch.empty(B, dtype=torch.long, device="cuda")
        X, rows, Y = torch.empty(B, T, FL, device="cuda"), torch.empty(B, S, HOP, device="cuda"), torch.randn(B, S, FL, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = _lib.ptr
        calls = {
            "step": lambda: so.ns_gl_op_step(fn._h, p(mag), p(lens), B, T, p(wave), n, p(wl), p(ws), n_ws, st),
            "inverse (GEMM + overlap-add)": lambda: so.ns_gl_op_inverse(fn._h, p(X), p(lens), B, T, p(wave), n, p(wl), p(ws), n_ws, st),
            "frame_rows": lambda: so.ns_gl_op_frame_rows(fn._h, p(wave), n, p(wl), B, n, S, p(rows), st),
            "rephase": lambda: so.ns_gl_op_rephase(fn._h, p(Y), p(mag), p(lens), B, T, S, p(X), st),
        }
        so.ns_gl_op_recombine(fn._h, p(mag), p(ang), p(lens), B, T, p(X), st)
        split = {}
        for k, f in calls.items():
            def many(f=f):
                for _ in range(50):
                    assert f() == 0
            split[k] = timed(many, 3)[0] / 50
            print(f"B={B} T={T}: {k} {split[k]:.4f} ms", flush=True)
        split["forward STFT GEMM (remainder)"] = split["step"] - sum(v for k, v in split.items() if k != "step")
        flop = 2 * 2.0 * B * T * FL * FL * args.iters
        r = dict(B=B, frames=T, iters=args.iters, hip_ms=dict(median=hip[0], min=hip[1], max=hip[2]),
                 gemm_tflops_over_whole_loop=flop / hip[0] / 1e9, split_ms_per_iteration=split)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
