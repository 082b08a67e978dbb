#!/usr/bin/env python3
"""VariancePredictor forward + backward (predictor.VariancePredictor; csrc/predgrad.hip) on one MI355X against torch.

Per shape (N(0, 1) rows, ragged lengths, the tiny config's pitch predictor, eval: no dropout), in one process, candidates alternating
step by step, device events around the enqueue and wall clock to a synchronise, medians over --steps after --warmup:
  (a) ``pred = module(x, mask); pred.backward(g)`` through predictor.VariancePredictor, x requiring grad (eleven gradients)
  (b) the same through an nn.Module restatement of the reference (Conv1d on transposed rows, ReLU, LayerNorm, Linear, masked_fill) and
      torch-ROCm autograd on the GPU
  (c) the weight gradient of conv1d_2 alone (ns_pg_op_wgrad without db: the GEMM and its fixed-order reduce), against its floor
      2 M F K Cin flop at the 157.3 TFLOP/s fp32 MFMA peak
Taken from the tool's own enqueue path: the launches of (a) as the C side counted them, and that (a) makes no host read (torch's sync
debug mode reports none).

    python tools/predictor_grad_bench.py --steps 30 --warmup 5 --md profiles/predictor_grad_timing.md
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK = 157.3e12  # fp32 MFMA flop/s (MI355X_MICROARCH.md)
SHAPES = {"cfg2_phoneme": dict(B=16, S=128), "cfg2_frame": dict(B=16, S=1000)}  # BASELINE config 2: phoneme level, frame level


class TorchPredictor(torch.nn.Module):
    """the reference's module restated (model/modules.py:233-286), dropout left out (eval)"""

    def __init__(self, cin, f, k):
        super().__init__()
        self.c1, self.c2 = torch.nn.Conv1d(cin, f, k, padding=(k - 1) // 2), torch.nn.Conv1d(f, f, k, padding=(k - 1) // 2)
        self.n1, self.n2 = torch.nn.LayerNorm(f), torch.nn.LayerNorm(f)
        self.lin = torch.nn.Linear(f, 1)

    def forward(self, x, mask):
        h = self.n1(torch.relu(self.c1(x.transpose(1, 2)).transpose(1, 2)))
        h = self.n2(torch.relu(self.c2(h.transpose(1, 2)).transpose(1, 2)))
        return self.lin(h).squeeze(-1).masked_fill(mask, 0.0)


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


class Candidate:
    def __init__(self, name, step, leaves):
        self.name, self.step, self.leaves = name, step, leaves
        self.events, self.wall = [], []

    def timed(self, record):
        for x in self.leaves:
            x.grad = None
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


def bench(shape, steps, warmup):
    import smart_nar_fast_tts_amd._lib as L
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import predictor

    B, S = SHAPES[shape]["B"], SHAPES[shape]["S"]
    M = B * S
    torch.manual_seed(16)
    ours = predictor.VariancePredictor(wl.model_config("tiny")).cuda().eval()
    cin, f, k = ours.input_size, ours.filter_size, ours.kernel
    ref = TorchPredictor(cin, f, k).cuda().eval()
    with torch.no_grad():
        for dst, src in zip((ref.c1.weight, ref.c1.bias, ref.n1.weight, ref.n1.bias, ref.c2.weight, ref.c2.bias, ref.n2.weight, ref.n2.bias, ref.lin.weight, ref.lin.bias),
                            ours.ordered_parameters()):
            dst.copy_(src)
    lens = torch.tensor([S - (37 * i) % (S // 2 + 1) for i in range(B)], device="cuda")
    mask = torch.arange(S, device="cuda")[None, :] >= lens[:, None]
    xa = torch.randn(B, S, cin, device="cuda").requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    g = torch.randn(B, S, device="cuda")

    def step_a():
        ours(xa, mask).backward(g)

    def step_b():
        ref(xb, mask).backward(g)

    step_a()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        step_a()
    torch.cuda.set_sync_debug_mode("default")
    launches = dict(ours.last_launches)
    host_reads = len([w for w in seen if "synchroniz" in str(w.message).lower()])
    assert host_reads == 0, [str(w.message) for w in seen]

    lib = L.load()
    dz, h1 = torch.randn(M, f, device="cuda"), torch.randn(M, f, device="cuda")
    dW = torch.empty(f, f, k, device="cuda")
    plan = (L.C.c_int32 * 8)()
    L.check(lib.ns_pg_plan_wgrad(M, f, f, k, plan), "ns_pg_plan_wgrad")
    ws = torch.empty(4 * plan[5] + (1 << 20) + 8 * 5 * f * ((M + 63) // 64), dtype=torch.uint8, device="cuda")

    def step_c():
        L.check(lib.ns_pg_op_wgrad(L.ptr(dz), L.ptr(h1), B, S, f, f, k, L.ptr(dW), None, L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pg_op_wgrad")

    leaves_a = [xa] + ours.ordered_parameters()
    leaves_b = [xb] + list(ref.parameters())
    cands = [Candidate("(a) predictor.VariancePredictor: forward + backward", step_a, leaves_a),
             Candidate("(b) torch nn.Module restatement + autograd on the GPU", step_b, leaves_b),
             Candidate("(c) the weight gradient of conv1d_2 alone (GEMM + reduce)", step_c, [])]
    for i in range(warmup + steps):
        for c in cands:
            c.timed(i >= warmup)
    diff = float((xa.grad - xb.grad).abs().max())
    flop = 2.0 * M * f * k * f
    res = {"shape": shape, "B": B, "S": S, "M": M, "launches": launches, "host_reads": host_reads, "wgrad_plan": list(plan), "wgrad_flop": flop,
           "wgrad_floor_us": flop / PEAK * 1e6, "max_abs_dx_diff_a_vs_b": diff, "candidates": []}
    for c in cands:
        res["candidates"].append({"name": c.name, "events": stats(c.events), "wall": stats(c.wall)})
    res["a_over_b_events"] = res["candidates"][0]["events"]["median_ms"] / res["candidates"][1]["events"]["median_ms"]
    res["wgrad_over_floor"] = res["candidates"][2]["events"]["median_ms"] * 1e3 / res["wgrad_floor_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = [bench(s, args.steps, args.warmup) for s in args.shapes]
    lines = ["# VariancePredictor forward + backward (DESIGN.md §20): timing on one MI355X", "", "Written by `tools/predictor_grad_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, "
             "ms; candidates alternate step by step in one process.", ""]
    for r in results:
        print(json.dumps(r), flush=True)
        lines += [f"## {r['shape']}: B = {r['B']}, S = {r['S']}, M = {r['M']}", "", "| candidate | device events | wall clock |", "|---|---|---|"]
        for c in r["candidates"]:
            f = lambda k: f"{c[k]['median_ms']:.3f} ({c[k]['min_ms']:.3f} - {c[k]['max_ms']:.3f})"  # noqa: E731
            lines.append(f"| {c['name']} | {f('events')} | {f('wall')} |")
        verdict = "faster than" if r["a_over_b_events"] < 1 else "SLOWER than"
        lines += ["", f"(a) is {verdict} (b): (a) / (b) = {r['a_over_b_events']:.3f} by device events.  (a) enqueued {r['launches'].get('forward')} launches forward and "
                  f"{r['launches'].get('backward')} backward and made {r['host_reads']} host reads (asserted).  The weight gradient (plan {r['wgrad_plan'][:5]}: "
                  f"{r['wgrad_plan'][3]} row ranges of {r['wgrad_plan'][2]} rows) is {r['wgrad_flop'] / 1e9:.2f} GFLOP: floor {r['wgrad_floor_us']:.1f} us at the fp32 MFMA "
                  f"peak, measured {r['candidates'][2]['events']['median_ms'] * 1e3:.1f} us for the whole call (two launches, the host side inside) = "
                  f"{r['wgrad_over_floor']:.1f} x the floor.  max |dx (a) - dx (b)|: {r['max_abs_dx_diff_a_vs_b']:.3g}.", ""]
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
