#!/usr/bin/env python3
"""Times one training-step tail on the full LJSpeech parameter set (workload.synth_state_dict: every float32 tensor,
seeded gradients): the HIP path — gradient norm + fused clip / Adam / zero_grad, three launches — against torch's own optimiser on
the same device in the same run: clip_grad_norm_ + Adam.step() + zero_grad(set_to_none=False) in its foreach form, and in its fused
form where that constructs.  The candidates alternate step by step; before every timed step the gradients are refilled outside the
timed window.  Per step: device events around the enqueue, and wall clock up to a device synchronise.  Warm-up first; medians with
min / max over --steps.  Achieved bytes/s of the HIP path = 9 floats per element (g read twice, p / m / v read and written, g written)
over the event time.  Launches per step are counted by torch.profiler in a pass of its own after the timing.

    python tools/optim_bench.py --steps 50 --warmup 10 --md profiles/optim_r14.md
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

COPY_RATE = 6.29e12  # float4 copy, bytes/s (MI355X_MICROARCH.md)
MAX_NORM = 1.0
HYPER = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.0)


def parameter_set(seed=0):
    import smart_nar_fast_tts_amd.workload as wl

    sd = wl.synth_state_dict(wl.model_config("ljspeech"), seed=seed)
    arrays = [np.ascontiguousarray(v) for v in sd.values() if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.size > 0]
    gen = torch.Generator().manual_seed(seed + 1)
    grads = [torch.randn(a.shape, generator=gen) * 0.05 for a in arrays]
    return arrays, grads


class Candidate:
    def __init__(self, name, arrays, grads, make):
        self.name = name
        self.params = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in arrays]
        self.g0 = [g.cuda() for g in grads]
        for p, g in zip(self.params, self.g0):
            p.grad = g.clone()
        self.step = make(self.params)
        self.events, self.wall = [], []

    def refill(self):
        torch._foreach_copy_([p.grad for p in self.params], self.g0)

    def timed(self, record):
        self.refill()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        self.step()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if record:
            self.events.append(a.elapsed_time(b))
            self.wall.append((t1 - t0) * 1e3)

    def launches(self):
        """Kernel launches of one step, by torch.profiler; None where the profiler gives nothing."""
        try:
            from torch.profiler import ProfilerActivity, profile

            self.refill()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                self.step()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
            return n or None
        except Exception as e:  # noqa: BLE001  (a profiler that is not there is not a benchmark failure)
            print("profiler:", type(e).__name__, e)
            return None


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--md", default=None)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    from smart_nar_fast_tts_amd import optim

    assert torch.cuda.is_available(), "needs the MI355X"
    arrays, grads = parameter_set()
    n_tensors, n_elems = len(arrays), int(sum(a.size for a in arrays))

    def make_hip(params):
        opt = optim.Adam(params, **HYPER)
        return lambda: opt.step(grad_clip_thresh=MAX_NORM, zero_grad=True)

    def make_torch(**kw):
        def make(params):
            opt = torch.optim.Adam(params, **HYPER, **kw)

            def step():
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
                opt.step()
                opt.zero_grad(set_to_none=False)
            return step
        return make

    cands = [Candidate("hip: norm + fused clip / Adam / zero", arrays, grads, make_hip),
             Candidate("torch foreach: clip_grad_norm_ + Adam.step + zero_grad", arrays, grads, make_torch(foreach=True))]
    try:
        cands.append(Candidate("torch fused: clip_grad_norm_ + Adam(fused=True).step + zero_grad", arrays, grads, make_torch(fused=True)))
    except Exception as e:  # noqa: BLE001
        print("torch fused Adam does not construct here:", type(e).__name__, e)
    for i in range(args.warmup + args.steps):
        for c in cands:  # alternate the candidates step by step
            c.timed(i >= args.warmup)
    # the same state after the same number of steps, against torch foreach
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(cands[0].params, cands[1].params))
    res = {"tensors": n_tensors, "elements": n_elems, "steps": args.steps, "warmup": args.warmup, "max_abs_param_diff_hip_vs_torch_foreach": diff, "candidates": []}
    for c in cands:
        r = {"name": c.name, "events": stats(c.events), "wall": stats(c.wall)}
        if c is cands[0]:
            r["bytes_per_step"] = 9 * 4 * n_elems
            r["achieved_bytes_per_s"] = r["bytes_per_step"] / (r["events"]["median_ms"] * 1e-3)
            r["share_of_float4_copy_rate"] = r["achieved_bytes_per_s"] / COPY_RATE
        res["candidates"].append(r)
    print(json.dumps(res), flush=True)
    for c, r in zip(cands, res["candidates"]):
        r["launches_per_step"] = None if args.no_launch_count else c.launches()
    res["candidates"][0]["launches_by_construction"] = 3
    print(json.dumps(res), flush=True)
    if args.md:
        with open(args.md, "a") as f:
            f.write(f"\n## Timing: one training-step tail on the LJSpeech parameter set ({n_tensors} tensors, {n_elems} elements)\n\n")
            f.write(f"`python tools/optim_bench.py --steps {args.steps} --warmup {args.warmup}`; candidates alternate step by step in one run; medians (min - max), ms.\n\n")
            f.write("| candidate | device events | wall clock to a synchronise | launches per step (torch.profiler) |\n|---|---|---|---|\n")
            for r in res["candidates"]:
                c = lambda k: f"{r[k]['median_ms']:.3f} ({r[k]['min_ms']:.3f} - {r[k]['max_ms']:.3f})"  # noqa: E731
                f.write(f"| {r['name']} | {c('events')} | {c('wall')} | {r['launches_per_step'] if r['launches_per_step'] is not None else 'not measured'} |\n")
            h = res["candidates"][0]
            f.write(f"\nThe HIP path issues 3 launches by construction.  It moves 9 floats per element = {h['bytes_per_step'] / 1e9:.3f} GB per step: "
                    f"{h['achieved_bytes_per_s'] / 1e12:.2f} TB/s over the median event time, {100 * h['share_of_float4_copy_rate']:.0f} % of the 6.29 TB/s float4-copy rate "
                    f"(a whole-step figure, launch gaps included, not a kernel's share of peak).\n")
            f.write(f"\nmax |HIP - torch foreach| over the parameters after {args.warmup + args.steps} equal steps: {diff:.3g}\n")


if __name__ == "__main__":
    main()
