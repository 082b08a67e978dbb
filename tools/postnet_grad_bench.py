#!/usr/bin/env python3
"""PostNet forward + backward with train-mode BatchNorm (postnet.PostNet; csrc/postnetgrad.hip) on one MI355X against torch.

Per shape (N(0, 1) rows, the default PostNet(80, 512, 5, 5) in train() with dropout 0.5, both sides drawing their own masks), in one
process, candidates alternating step by step, device events around the enqueue and wall clock to a synchronise, medians over --steps
after --warmup:
  (a) ``y = module(x); y.backward(g)`` through postnet.PostNet, x requiring grad (21 gradients, 15 buffers updated)
  (b) the same through nn.Sequential(Conv1d, BatchNorm1d, Tanh, Dropout) x 5 on the transposed rows and torch-ROCm autograd on the GPU
  (c) each new kernel alone through its ns_pn_op_* entry at C = 512 and C = 80 with a keep-mask: the call's time (its one or two
      launches, the host side inside) and the bytes it must move — stats 4, apply 9, backward reduction 13, backward apply 17 bytes per
      element — as achieved bytes/s
The split of (a): new kernels = 4 x the C = 512 calls + 1 x the C = 80 calls of (c); the rest (the five layers' forward, weight-gradient
and data-gradient GEMMs, the packs, the mask draws) = (a) - that.  Reads nothing but its own tree.

    python tools/postnet_grad_bench.py --steps 20 --warmup 5 --md profiles/postnet_grad_timing.md
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

SHAPES = {"b16_t128": dict(B=16, T=128), "flagship_b16_t1010": dict(B=16, T=1010)}
BYTES = {"stats": 4, "apply": 9, "bwd_reduce": 13, "bwd_apply": 17}  # per element of [M, C], keep-mask included


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


class Candidate:
    def __init__(self, name, step, leaves=()):
        self.name, self.step, self.leaves = name, step, list(leaves)
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


def torch_postnet(n_mel, emb, k, n):
    chans = [n_mel] + [emb] * (n - 1) + [n_mel]
    layers = []
    for i in range(n):
        layers += [torch.nn.Conv1d(chans[i], chans[i + 1], k, padding=(k - 1) // 2), torch.nn.BatchNorm1d(chans[i + 1])]
        layers += ([torch.nn.Tanh()] if i < n - 1 else []) + [torch.nn.Dropout(0.5)]
    return torch.nn.Sequential(*layers)


def kernel_candidates(L, lib, M, Cw):
    u, dh, h = (torch.randn(M, Cw, device="cuda") for _ in range(3))
    h = torch.tanh(h) * 2.0
    keep = (torch.rand(M, Cw, device="cuda") >= 0.5).to(torch.uint8)
    h = h * keep
    gam, bet = torch.ones(Cw, device="cuda"), torch.zeros(Cw, device="cuda")
    rm, rv, nbt = torch.zeros(Cw, device="cuda"), torch.ones(Cw, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    st, means = torch.zeros(2, Cw, dtype=torch.float64, device="cuda"), torch.zeros(2, Cw, dtype=torch.float64, device="cuda")
    out, dz, dg, db = torch.empty(M, Cw, device="cuda"), torch.empty(M, Cw, device="cuda"), torch.empty(Cw, device="cuda"), torch.empty(Cw, device="cuda")
    ws = torch.empty(8 * 2 * Cw * ((M + 31) // 32) + 4096, dtype=torch.uint8, device="cuda")
    P, S = L.ptr, L.stream_ptr
    calls = {
        "stats": lambda: lib.ns_pn_op_stats(P(u), M, Cw, 1, P(rm), P(rv), P(nbt), P(st), P(ws), ws.numel(), S()),
        "apply": lambda: lib.ns_pn_op_apply(P(u), P(st), P(gam), P(bet), P(keep), 0.5, 0, M, Cw, P(out), S()),
        "bwd_reduce": lambda: lib.ns_pn_op_bwd_reduce(P(dh), P(u), P(h), P(st), P(keep), 0.5, 0, M, Cw, P(dg), P(db), P(means), P(ws), ws.numel(), S()),
        "bwd_apply": lambda: lib.ns_pn_op_bwd_apply(P(dh), P(u), P(h), P(st), P(means), P(gam), P(keep), 0.5, 0, M, Cw, Cw, P(dz), P(db), P(ws), ws.numel(), S()),
    }
    L.check(calls["stats"](), "ns_pn_op_stats")
    keepalive = (u, dh, h, keep, gam, bet, rm, rv, nbt, st, means, out, dz, dg, db, ws)
    return [Candidate(f"{k}@C={Cw}", (lambda f=f, k=k: L.check(f(), k))) for k, f in calls.items()], keepalive


def bench(shape, steps, warmup):
    import smart_nar_fast_tts_amd._lib as L
    from smart_nar_fast_tts_amd import postnet

    B, T = SHAPES[shape]["B"], SHAPES[shape]["T"]
    M = B * T
    torch.manual_seed(25)
    ours = postnet.PostNet().cuda().train()
    ref = torch_postnet(ours.n_mel, ours.emb, ours.kernel, ours.n).cuda().train()
    with torch.no_grad():
        for dst, src in zip(ref.parameters(), ours.ordered_parameters()):
            dst.copy_(src)
    xa = torch.randn(B, T, ours.n_mel, device="cuda").requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    g = torch.randn(B, T, ours.n_mel, device="cuda")

    def step_a():
        ours(xa).backward(g)

    def step_b():
        ref(xb.transpose(1, 2)).transpose(1, 2).backward(g)

    step_a()
    torch.cuda.synchronize()
    launches = dict(ours.last_launches)
    lib = L.load()
    cands = [Candidate("(a) postnet.PostNet: forward + backward", step_a, [xa] + ours.ordered_parameters()),
             Candidate("(b) torch nn.Sequential(Conv1d, BatchNorm1d, Tanh, Dropout) + autograd on the GPU", step_b, [xb] + list(ref.parameters()))]
    alive = []
    for Cw in (ours.emb, ours.n_mel):
        ks, keep = kernel_candidates(L, lib, M, Cw)
        cands += ks
        alive.append(keep)
    for i in range(warmup + steps):
        for c in cands:
            c.timed(i >= warmup)
    res = {"shape": shape, "B": B, "T": T, "M": M, "launches": launches, "candidates": [], "kernels": {}}
    for c in cands[:2]:
        res["candidates"].append({"name": c.name, "events": stats(c.events), "wall": stats(c.wall)})
    new_ms = 0.0
    for c in cands[2:]:
        kind, Cw = c.name.split("@C=")
        ms = float(np.median(c.events))
        moved = BYTES[kind] * M * int(Cw)
        res["kernels"][c.name] = {"median_ms": ms, "bytes": moved, "GBps": moved / (ms * 1e-3) / 1e9}
        new_ms += ms * ((ours.n - 1) if int(Cw) == ours.emb else 1)
    a = res["candidates"][0]["events"]["median_ms"]
    res["new_kernels_ms"], res["rest_ms"] = new_ms, a - new_ms
    res["a_over_b_events"] = a / res["candidates"][1]["events"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = [bench(s, args.steps, args.warmup) for s in args.shapes]
    lines = ["# PostNet forward + backward with train-mode BatchNorm: timing on one MI355X", "", "Written by `tools/postnet_grad_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, "
             "ms; candidates alternate step by step in one process.", ""]
    for r in results:
        print(json.dumps(r), flush=True)
        lines += [f"## {r['shape']}: B = {r['B']}, T = {r['T']}, M = {r['M']}", "", "| candidate | device events | wall clock |", "|---|---|---|"]
        for c in r["candidates"]:
            f = lambda k: f"{c[k]['median_ms']:.3f} ({c[k]['min_ms']:.3f} - {c[k]['max_ms']:.3f})"  # noqa: E731
            lines.append(f"| {c['name']} | {f('events')} | {f('wall')} |")
        verdict = "faster than" if r["a_over_b_events"] < 1 else "SLOWER than"
        lines += ["", f"(a) is {verdict} (b): (a) / (b) = {r['a_over_b_events']:.3f} by device events.  (a) enqueued {r['launches'].get('forward')} launches forward and "
                  f"{r['launches'].get('backward')} backward.  Of (a), the new kernels take {r['new_kernels_ms']:.3f} ms (4 x the C = 512 calls + 1 x the C = 80 "
                  f"calls below) and everything else — the five layers' GEMMs, packs and mask draws — {r['rest_ms']:.3f} ms.", "",
                  "| new kernel alone (whole call) | ms | bytes it must move | achieved GB/s |", "|---|---|---|---|"]
        for k, v in r["kernels"].items():
            lines.append(f"| {k} | {v['median_ms']:.4f} | {v['bytes']} | {v['GBps']:.0f} |")
        lines.append("")
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
