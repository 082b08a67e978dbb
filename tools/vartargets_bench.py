#!/usr/bin/env python3
"""Times the variance targets on a config-2-shaped batch (B 16, L 128, T ~1000): the HIP path (process with fit, then
normalize) against two baselines on the same data, all in one run —
  (a) a torch-op version on the device, per utterance, with the host reads it needs (frame count, voiced indices, segment bounds);
  (b) the float64 numpy restatement on the host (tests/variance_targets_cpu.py), fed from and returning to the device.
Wall clock around a synchronised call for all three (the baselines contain host reads, which events do not see), device events for
the HIP path in addition; warm-up first, medians over --steps, min / max beside them.

    python tools/vartargets_bench.py --steps 30 --warmup 5 --md profiles/vartargets_r13.md
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def batch(B=16, L=128, T=1000, seed=0):
    rng = np.random.RandomState(seed)
    d = rng.randint(0, 16, size=(B, L)).astype(np.int64)
    src_lens = rng.randint(L // 2, L + 1, size=B).astype(np.int64)
    src_lens[0] = L
    t = np.arange(T)
    pitch = (180.0 + 60.0 * np.sin(t[None, :] / 17.0 + rng.uniform(0, 6, (B, 1))) + rng.normal(0, 6.0, (B, T))).astype(np.float32)
    pitch[rng.rand(B, T) < 0.35] = 0.0
    energy = (np.abs(rng.normal(30.0, 12.0, (B, T))) + 0.5).astype(np.float32)
    return pitch, energy, d, src_lens


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


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


def torch_per_utterance(pitch, energy, d, src_lens, p_frame, e_frame):
    """Baseline (a): torch ops on the device, one utterance at a time; raw targets only (no fit, no normalisation)."""
    B, T = pitch.shape
    L = d.shape[1]
    pt = torch.zeros((B, T if p_frame else L), device=pitch.device)
    et = torch.zeros((B, T if e_frame else L), device=pitch.device)
    for b in range(B):
        Ls = int(src_lens[b])                       # host read
        db = d[b, :Ls].clamp(min=0)
        c = torch.cumsum(db, 0)
        n = min(T, int(c[-1])) if Ls else 0         # host read
        p = pitch[b, :n].double()
        nz = torch.nonzero(p != 0).flatten()
        if nz.numel() <= 1:                         # host read
            continue
        lo, hi = (c - db).clamp(max=n), c.clamp(max=n)
        cnt = (hi - lo).clamp(min=1).double()

        def seg_mean(x):
            cs = torch.cat([x.new_zeros(1), torch.cumsum(x, 0)])
            return torch.where((db > 0) & (hi > lo), (cs[hi] - cs[lo]) / cnt, x.new_zeros(())).float()

        if p_frame:
            pt[b, :n] = pitch[b, :n]
        else:
            tt = torch.arange(n, device=p.device)
            k = torch.searchsorted(nz, tt, right=True) - 1
            x0, x1 = nz[k.clamp(min=0)], nz[(k + 1).clamp(max=nz.numel() - 1)]
            slope = (p[x1] - p[x0]) / (x1 - x0).clamp(min=1).double()
            y = torch.where(k < 0, p[nz[0]], torch.where(k + 1 >= nz.numel(), p[nz[-1]], slope * (tt - x0).double() + p[x0]))
            pt[b, :Ls] = seg_mean(y)
        if e_frame:
            et[b, :n] = energy[b, :n]
        else:
            et[b, :Ls] = seg_mean(energy[b, :n].double())
    return pt, et


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.targets import VarianceTargets
    from tests import variance_targets_cpu as vc

    assert torch.cuda.is_available(), "needs the MI355X"
    pitch, energy, d, sl = batch()
    dp, de, dd, dsl = (torch.from_numpy(a).cuda() for a in (pitch, energy, d, sl))
    rows = []
    for level in ("phoneme_level", "frame_level"):
        pc = wl.preprocess_config(level, level)
        vt = VarianceTargets(pc)
        frame = level == "frame_level"

        def hip():
            vt.reset()
            pt, et, fl, valid = vt.process(dp, de, dd, dsl)
            vt.normalize(pt, et, dsl, fl, valid)
            return pt, et

        def hip_targets_only():
            return vt.process(dp, de, dd, dsl, fit=False)

        def host_numpy():
            b = {"pitch": dp.cpu().numpy(), "energy": de.cpu().numpy(), "durations": dd.cpu().numpy(), "src_lens": dsl.cpu().numpy()}
            r = vc.pipeline(b, level, level)
            return torch.from_numpy(r["pitch"]["norm"].astype(np.float32)).cuda(), torch.from_numpy(r["energy"]["norm"].astype(np.float32)).cuda()

        res = {"level": level,
               "hip_process_fit_normalize_wall": wall_ms(hip, args.steps, args.warmup),
               "hip_process_fit_normalize_events": events_ms(hip, args.steps, args.warmup),
               "hip_targets_only_events": events_ms(hip_targets_only, args.steps, args.warmup),
               "torch_per_utterance_targets_only_wall": wall_ms(lambda: torch_per_utterance(dp, de, dd, dsl, frame, frame), max(3, args.steps // 5), 1),
               "numpy_host_wall": wall_ms(host_numpy, max(3, args.steps // 10), 1)}
        a = hip_targets_only()
        t = torch_per_utterance(dp, de, dd, dsl, frame, frame)
        res["max_abs_targets_hip_vs_torch"] = float(max((a[0] - t[0]).abs().max(), (a[1] - t[1]).abs().max()))
        rows.append(res)
        print(json.dumps(res))
    if args.md:
        with open(args.md, "w") as f:
            f.write("# Variance targets: HIP path against a torch-op and a numpy baseline (B 16, L 128, T 1000)\n\n")
            f.write(f"`python tools/vartargets_bench.py --steps {args.steps} --warmup {args.warmup}`; medians (min - max), ms.  The torch baseline computes raw targets "
                    "only (per utterance, with its host reads); the numpy baseline is the whole float64 restatement including both copies.\n\n")
            f.write("| level | HIP process + fit + normalize (wall) | same (device events) | HIP targets only (events) | torch per utterance, targets only (wall) | numpy on the host (wall) |\n|---|---|---|---|---|---|\n")
            for r in rows:
                c = lambda k: f"{r[k]['median_ms']:.3f} ({r[k]['min_ms']:.3f} - {r[k]['max_ms']:.3f})"  # noqa: E731
                f.write(f"| {r['level']} | {c('hip_process_fit_normalize_wall')} | {c('hip_process_fit_normalize_events')} | {c('hip_targets_only_events')} | "
                        f"{c('torch_per_utterance_targets_only_wall')} | {c('numpy_host_wall')} |\n")
            f.write("\nmax |HIP - torch| over the raw targets: " + ", ".join(f"{r['level']} {r['max_abs_targets_hip_vs_torch']:.3g}" for r in rows) + "\n")


if __name__ == "__main__":
    main()
