#!/usr/bin/env python3
"""Cross-attention sublayer forward + backward (sublayers.MultiHeadCrossAttention; csrc/xattngrad.hip) on one MI355X against torch.

Per shape (N(0, 1) rows, ragged source lengths, eval: no dropout; the upstream gradient of the map nonzero on head 0 only, as the
guided-attention loss gives it), in one process, candidates alternating step by step, device events around the enqueue and wall
clock to a synchronise, medians over --steps after --warmup:
  (a) ``y, attn = module(tgt, src, src, lens=src_lens); backward([y, attn], [g, dA])`` through sublayers.MultiHeadCrossAttention, tgt
      and src requiring grad (twelve gradients)
  (b) the same through an nn.Module restatement of the reference (three Linears, the head split, bmm, / sqrt(dk), masked_fill, softmax,
      bmm, fc, + tgt, LayerNorm, the map returned) and torch-ROCm autograd on the GPU
  (c) the attention backward alone (ns_xg_op_attention_backward) with the query parts of the key-owning kernel forced to 1 (two
      launches)
  (d) the same with the planned number of parts (ns_xg_kv_splits; three launches when it is above 1; not listed when it is 1)
against the floor of 10 B H T L dk flop (five T x L x dk products) at the 157.3 TFLOP/s fp32 MFMA peak.  Taken from the tool's own
enqueue path: the launches of (a) as the C side counted them, and that (a) makes no host read (torch's sync debug mode reports none).

``--parts 2 4 8`` times further forced numbers of parts (the sweep the split rule is judged by); ``--report FILE`` appends the worst
gate shares of one run of tests/test_gpu_cross_attention_grad.py (its NS_FP32_OPS_REPORT file).

    NS_FP32_OPS_REPORT=report.jsonl python -m pytest -m gpu tests/test_gpu_cross_attention_grad.py
    python tools/cross_attention_grad_bench.py --steps 30 --warmup 5 --parts 2 4 8 --report report.jsonl --md profiles/cross_attention_grad.md
"""
import argparse
import ctypes as C
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
SHAPES = {"aligner_h2": dict(B=16, T=1000, L=128, d=256, H=2), "aligner_h4": dict(B=16, T=1000, L=128, d=256, H=4),
          "small": dict(B=3, T=343, L=40, d=256, H=2)}


class TorchCrossAttention(torch.nn.Module):
    """the reference's module restated (transformer/SubLayers.py:8-59) for k = v, dropout left out (eval)"""

    def __init__(self, d, h):
        super().__init__()
        self.h = h
        self.w_qs, self.w_ks, self.w_vs, self.fc = (torch.nn.Linear(d, d) for _ in range(4))
        self.layer_norm = torch.nn.LayerNorm(d)

    def forward(self, tgt, src, mask):
        B, T, d = tgt.shape
        L = src.shape[1]
        h, dk = self.h, d // self.h
        split = lambda t, n: t.view(B, n, h, dk).permute(2, 0, 1, 3).contiguous().view(-1, n, dk)  # noqa: E731
        q, k, v = split(self.w_qs(tgt), T), split(self.w_ks(src), L), split(self.w_vs(src), L)
        attn = torch.bmm(q, k.transpose(1, 2)) / dk ** 0.5
        attn = torch.softmax(attn.masked_fill(mask.repeat(h, 1, 1), float("-inf")), dim=2)
        out = torch.bmm(attn, v).view(h, B, T, dk).permute(1, 2, 0, 3).contiguous().view(B, T, d)
        return self.layer_norm(self.fc(out) + tgt), attn.view(h, B, T, L).transpose(0, 1)


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


def bench(shape, steps, warmup, extra_parts=()):
    import smart_nar_fast_tts_amd._lib as L_
    from smart_nar_fast_tts_amd import sublayers

    B, T, L, D, H = (SHAPES[shape][k] for k in ("B", "T", "L", "d", "H"))
    dk = D // H
    torch.manual_seed(24)
    ours = sublayers.MultiHeadCrossAttention(H, D, dk, dk, dropout=0.1).cuda().eval()
    ref = TorchCrossAttention(D, H).cuda().eval()
    ref.load_state_dict(ours.state_dict())
    lens = torch.tensor([L - (37 * i) % (L // 2 + 1) for i in range(B)], device="cuda")
    mask = (torch.arange(L, device="cuda")[None, None, :] >= lens[:, None, None]).expand(B, T, L)
    ta = torch.randn(B, T, D, device="cuda").requires_grad_(True)
    sa = torch.randn(B, L, D, device="cuda").requires_grad_(True)
    tb, sb = ta.detach().clone().requires_grad_(True), sa.detach().clone().requires_grad_(True)
    g = torch.randn(B, T, D, device="cuda")
    dA = torch.zeros(B, H, T, L, device="cuda")
    dA[:, 0] = torch.randn(B, T, L, device="cuda") / T
    dA = dA.masked_fill(mask[:, None], 0.0)

    def step_a():
        y, attn = ours(ta, sa, sa, lens=lens)
        torch.autograd.backward([y, attn], [g, dA])

    def step_b():
        y, attn = ref(tb, sb, mask)
        torch.autograd.backward([y, attn], [g, dA])

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

    lib = L_.load()
    call = ours._marshal(ta.detach(), sa.detach(), None, lens, None)
    _, attn, saved = ours._forward(call, save=True)
    mt, ml = B * T * D, B * L * 2 * D
    q, kv, ctx = saved[:mt], saved[mt:mt + ml], saved[mt + ml:2 * mt + ml]
    dctx, dq, dkv = torch.randn(B * T, D, device="cuda"), torch.empty(B * T, D, device="cuda"), torch.empty(B * L, 2 * D, device="cuda")
    planned = lib.ns_xg_kv_splits(C.byref(call.shape))
    ws = torch.empty(4 * B * H * T + 256 + planned * 4 * ml + 256, dtype=torch.uint8, device="cuda")

    def alone(parts):
        def step():
            L_.check(lib.ns_xg_op_attention_backward(L_.ptr(q), L_.ptr(kv), L_.ptr(ctx), L_.ptr(attn), L_.ptr(dctx), L_.ptr(dA), L_.ptr(call.lens), B, T, L, D, H,
                                                     parts, L_.ptr(dq), L_.ptr(dkv), L_.ptr(ws), ws.numel(), L_.stream_ptr()), "ns_xg_op_attention_backward")
        return step

    cands = [Candidate("(a) sublayers.MultiHeadCrossAttention: forward + backward", step_a, [ta, sa] + ours.ordered_parameters()),
             Candidate("(b) torch nn.Module restatement + autograd on the GPU", step_b, [tb, sb] + list(ref.parameters())),
             Candidate("(c) the attention backward alone, nsplit = 1 (two launches)", alone(1), [])]
    if planned > 1:
        cands.append(Candidate(f"(d) the attention backward alone, nsplit = {planned} as planned (three launches)", alone(planned), []))
    for k in extra_parts:  # (--parts: a sweep for setting the rule; needs a workspace of its own size)
        if k not in (1, planned):
            cands.append(Candidate(f"(e) the attention backward alone, nsplit = {k} forced", alone(k), []))
    ws = torch.empty(4 * B * H * T + 256 + max((planned,) + tuple(extra_parts)) * 4 * ml + 256, dtype=torch.uint8, device="cuda")
    for i in range(warmup + steps):
        for c in cands:
            c.timed(i >= warmup)
    flop = 10.0 * B * H * T * L * dk
    res = {"shape": shape, "B": B, "T": T, "L": L, "d": D, "H": H, "launches": launches, "host_reads": host_reads, "planned_kv_splits": planned,
           "attention_backward_flop": flop, "attention_backward_floor_us": flop / PEAK * 1e6,
           "max_abs_dtgt_diff_a_vs_b": float((ta.grad - tb.grad).abs().max()), "max_abs_dsrc_diff_a_vs_b": float((sa.grad - sb.grad).abs().max()),
           "candidates": [{"name": c.name, "events": stats(c.events), "wall": stats(c.wall)} for c in cands]}
    res["a_over_b_events"] = res["candidates"][0]["events"]["median_ms"] / res["candidates"][1]["events"]["median_ms"]
    if planned > 1:
        res["planned_over_one_part"] = res["candidates"][3]["events"]["median_ms"] / res["candidates"][2]["events"]["median_ms"]
    return res


def shares_section(path):
    """The worst share of every gate in one run's report (the last run in the file), with the case it was measured at."""
    rows = [json.loads(line) for line in open(path) if line.strip()]
    rows = [r for r in rows if r.get("test", "").startswith("xg_")]
    first = max(i for i, r in enumerate(rows) if r["test"] == rows[0]["test"] and all(r.get(k) == rows[0].get(k) for k in ("cfg", "case", "dA", "kv_splits")))
    worst = {}
    for r in rows[first:]:
        where = " ".join(str(r[k]) for k in ("cfg", "case", "mode", "dA") if r.get(k) is not None)
        where += f" kv_splits {r['kv_splits']}" if r.get("kv_splits") else ""
        vals = r["shares"] if "shares" in r else {k: r[k] for k in ("q", "kv", "y", "attn", "ctx") if k in r} if r["test"] == "xg_forward" else {}
        for k, v in vals.items():
            if v >= worst.get((r["test"], k), (-1.0, ""))[0]:
                worst[(r["test"], k)] = (v, where)
    lines = ["## Shares of the gates (tests/test_gpu_cross_attention_grad.py, worst over the case table)", "",
             "| test | tensor | worst |error| / gate | at |", "|---|---|---|---|"]
    lines += [f"| {t} | {k} | {v:.3f} | {where} |" for (t, k), (v, where) in sorted(worst.items())]
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parts", nargs="*", type=int, default=[], help="further forced numbers of query parts to time, each in [1, 8]")
    ap.add_argument("--report", help="an NS_FP32_OPS_REPORT file of tests/test_gpu_cross_attention_grad.py: its worst shares are appended")
    ap.add_argument("--md")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = [bench(s, args.steps, args.warmup, tuple(args.parts)) for s in args.shapes]
    lines = ["# Cross-attention sublayer forward + backward (DESIGN.md §24): timing on one MI355X", "", "Written by `tools/cross_attention_grad_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, "
             "ms; candidates alternate step by step in one process.", ""]
    for r in results:
        print(json.dumps(r), flush=True)
        lines += [f"## {r['shape']}: B = {r['B']}, T = {r['T']}, L = {r['L']}, d = {r['d']}, H = {r['H']}", "", "| candidate | device events | wall clock |", "|---|---|---|"]
        for c in r["candidates"]:
            f = lambda k: f"{c[k]['median_ms']:.3f} ({c[k]['min_ms']:.3f} - {c[k]['max_ms']:.3f})"  # noqa: E731
            lines.append(f"| {c['name']} | {f('events')} | {f('wall')} |")
        verdict = "faster than" if r["a_over_b_events"] < 1 else "SLOWER than"
        lines += ["", f"(a) is {verdict} (b): (a) / (b) = {r['a_over_b_events']:.3f} by device events.  (a) enqueued {r['launches'].get('forward')} launches forward and "
                  f"{r['launches'].get('backward')} backward and made {r['host_reads']} host reads (asserted).  The attention backward is "
                  f"{r['attention_backward_flop'] / 1e9:.2f} GFLOP: floor {r['attention_backward_floor_us']:.1f} us at the fp32 MFMA peak, measured "
                  f"{r['candidates'][2]['events']['median_ms'] * 1e3:.1f} us for the whole call with one part (the host side inside).  "
                  f"max |dtgt (a) - dtgt (b)|: {r['max_abs_dtgt_diff_a_vs_b']:.3g}, max |dsrc (a) - dsrc (b)|: {r['max_abs_dsrc_diff_a_vs_b']:.3g}.", ""]
        if "planned_over_one_part" in r:
            earned = "earned its place" if r["planned_over_one_part"] < 1 else "did NOT earn its place"
            lines += [f"The planned query split (nsplit = {r['planned_kv_splits']}) {earned} here: (d) / (c) = {r['planned_over_one_part']:.3f} by device events.", ""]
        else:
            lines += ["The planned number of query parts is 1 at this shape: there is no (d).", ""]
    if args.report:
        lines += shares_section(args.report)
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
