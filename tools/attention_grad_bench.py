#!/usr/bin/env python3
"""Self-attention sublayer forward + backward (sublayers.MultiHeadAttention; csrc/attngrad.hip) on one MI355X against torch.

Per shape (N(0, 1) rows, ragged lengths, d = 256, H = 2, eval: no dropout), in one process, candidates alternating step by step,
device events around the enqueue and wall clock to a synchronise, medians over --steps after --warmup:
  (a) ``y, _ = module(x, x, x, lens=lens); y.backward(g)`` through sublayers.MultiHeadAttention, x requiring grad (eleven gradients)
  (b) the same through an nn.Module restatement of the reference (three Linears, the head split, bmm, / sqrt(dk), masked_fill, softmax,
      bmm, fc, + x, LayerNorm) and torch-ROCm autograd on the GPU
  (c) the attention backward alone (ns_ag_op_attention_backward: the query-owning and the key-owning kernel), against its floor of
      10 B H S^2 dk flop (five S x S x dk products) at the 157.3 TFLOP/s fp32 MFMA peak
Taken from the tool's own enqueue path: the launches of (a) as the C side counted them, and that (a) makes no host read (torch's sync
debug mode reports none).

    python tools/attention_grad_bench.py --steps 30 --warmup 5 --md profiles/attention_grad_timing.md
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
SHAPES = {"cfg2_encoder": dict(B=16, S=128), "cfg2_decoder": dict(B=16, S=1000)}  # BASELINE config 2: phoneme level, frame level
D, H = 256, 2


class TorchAttention(torch.nn.Module):
    """the reference's module restated (transformer/SubLayers.py:8-59) for q = k = v, dropout left out (eval)"""

    def __init__(self, d, h):
        super().__init__()
        self.h = h
        self.w_qs, self.w_ks, self.w_vs, self.fc = (torch.nn.Linear(d, d) for _ in range(4))
        self.layer_norm = torch.nn.LayerNorm(d)

    def forward(self, x, mask):
        B, S, d = x.shape
        h, dk = self.h, d // self.h
        split = lambda t: t.view(B, S, h, dk).permute(2, 0, 1, 3).contiguous().view(-1, S, dk)  # noqa: E731
        q, k, v = split(self.w_qs(x)), split(self.w_ks(x)), split(self.w_vs(x))
        attn = torch.bmm(q, k.transpose(1, 2)) / dk ** 0.5
        attn = torch.softmax(attn.masked_fill(mask.repeat(h, 1, 1), float("-inf")), dim=2)
        out = torch.bmm(attn, v).view(h, B, S, dk).permute(1, 2, 0, 3).contiguous().view(B, S, d)
        return self.layer_norm(self.fc(out) + x)


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
    from smart_nar_fast_tts_amd import sublayers

    B, S = SHAPES[shape]["B"], SHAPES[shape]["S"]
    M, dk = B * S, D // H
    torch.manual_seed(22)
    ours = sublayers.MultiHeadAttention(H, D, dk, dk, dropout=0.1).cuda().eval()
    ref = TorchAttention(D, H).cuda().eval()
    ref.load_state_dict(ours.state_dict())
    lens = torch.tensor([S - (37 * i) % (S // 2 + 1) for i in range(B)], device="cuda")
    mask = (torch.arange(S, device="cuda")[None, None, :] >= lens[:, None, None]).expand(B, S, S)
    xa = torch.randn(B, S, D, device="cuda").requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    g = torch.randn(B, S, D, device="cuda")

    def step_a():
        ours(xa, xa, xa, lens=lens)[0].backward(g)

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
    call = ours._marshal(xa.detach(), None, lens, None)
    _, saved = ours._forward(call, save=True)
    md = M * D
    qkv, ctx, lse = saved[:3 * md], saved[3 * md:4 * md], saved[5 * md:]
    dctx, dqkv = torch.randn(M, D, device="cuda"), torch.empty(M, 3 * D, device="cuda")
    ws = torch.empty(4 * B * H * S + 256, dtype=torch.uint8, device="cuda")

    def step_c():
        L.check(lib.ns_ag_op_attention_backward(L.ptr(qkv), L.ptr(ctx), L.ptr(lse), L.ptr(dctx), L.ptr(call.lens), B, S, D, H, L.ptr(dqkv), L.ptr(ws),
                                                ws.numel(), L.stream_ptr()), "ns_ag_op_attention_backward")

    leaves_a = [xa] + ours.ordered_parameters()
    leaves_b = [xb] + list(ref.parameters())
    cands = [Candidate("(a) sublayers.MultiHeadAttention: forward + backward", step_a, leaves_a),
             Candidate("(b) torch nn.Module restatement + autograd on the GPU", step_b, leaves_b),
             Candidate("(c) the attention backward alone (two launches)", step_c, [])]
    for i in range(warmup + steps):
        for c in cands:
            c.timed(i >= warmup)
    diff = float((xa.grad - xb.grad).abs().max())
    flop = 10.0 * B * H * S * S * dk
    res = {"shape": shape, "B": B, "S": S, "M": M, "d": D, "H": H, "launches": launches, "host_reads": host_reads, "attention_backward_flop": flop,
           "attention_backward_floor_us": flop / PEAK * 1e6, "max_abs_dx_diff_a_vs_b": diff, "candidates": []}
    for c in cands:
        res["candidates"].append({"name": c.name, "events": stats(c.events), "wall": stats(c.wall)})
    res["a_over_b_events"] = res["candidates"][0]["events"]["median_ms"] / res["candidates"][1]["events"]["median_ms"]
    res["attention_backward_over_floor"] = res["candidates"][2]["events"]["median_ms"] * 1e3 / res["attention_backward_floor_us"]
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
    lines = ["# Self-attention sublayer forward + backward (DESIGN.md §22): timing on one MI355X", "", "Written by `tools/attention_grad_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, "
             "ms; candidates alternate step by step in one process.", ""]
    for r in results:
        print(json.dumps(r), flush=True)
        lines += [f"## {r['shape']}: B = {r['B']}, S = {r['S']}, d = {r['d']}, H = {r['H']}", "", "| candidate | device events | wall clock |", "|---|---|---|"]
        for c in r["candidates"]:
            f = lambda k: f"{c[k]['median_ms']:.3f} ({c[k]['min_ms']:.3f} - {c[k]['max_ms']:.3f})"  # noqa: E731
            lines.append(f"| {c['name']} | {f('events')} | {f('wall')} |")
        verdict = "faster than" if r["a_over_b_events"] < 1 else "SLOWER than"
        lines += ["", f"(a) is {verdict} (b): (a) / (b) = {r['a_over_b_events']:.3f} by device events.  (a) enqueued {r['launches'].get('forward')} launches forward and "
                  f"{r['launches'].get('backward')} backward and made {r['host_reads']} host reads (asserted).  The attention backward is "
                  f"{r['attention_backward_flop'] / 1e12:.4f} TFLOP: floor {r['attention_backward_floor_us']:.1f} us at the fp32 MFMA peak, measured "
                  f"{r['candidates'][2]['events']['median_ms'] * 1e3:.1f} us for the whole call (two launches, the host side inside) = "
                  f"{r['attention_backward_over_floor']:.1f} x the floor.  max |dx (a) - dx (b)|: {r['max_abs_dx_diff_a_vs_b']:.3g}.", ""]
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
