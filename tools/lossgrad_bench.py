#!/usr/bin/env python3
"""Training loss (loss.FastSpeech2TrainingLoss; csrc/loss.hip + csrc/lossgrad.hip) on one MI355X: the shares of the tests' gate its
gradients use, and the time of value + backward against torch.

Shares (--shares): every case of tests/test_gpu_lossgrad.py — the two reference fixtures and loss_cpu.CASES at both feature levels
with their seeded grad_output — as max |HIP - float64| / gate per gradient tensor, with the worst element.

Timing, per shape (seeded tuples of tests/loss_cpu.random_case: ragged lengths, softmax maps), in one process, candidates alternating
step by step, device events around the enqueue and wall clock to a synchronise, medians over --steps after --warmup:
  (a) ``losses = Loss(batch, output); losses[0].backward()`` through FastSpeech2TrainingLoss
  (b) the same through the masked_select statement of the reference's loss (tests/lossgrad_cpu.statement: model/loss.py:164-250 with
      the four guided-attention grids built by one vectorised expression on the device — the reference builds them per utterance in a
      Python loop on the host, which this leaves out in torch's favour) and torch autograd on the GPU
  (c) the backward launch alone into preallocated buffers, and the bytes it must move (gradients written, unmasked predictions and
      targets read) over that time against the 6.29 TB/s float4-copy rate profiles/optim_r14.md uses.
Asserted from the tool's own enqueue path: (a) enqueues exactly three of our launches (the class counts them where it enqueues) and
makes no host read (torch's sync debug mode reports none).

    python tools/lossgrad_bench.py --shares --shapes cfg2_b16 cfg5_like --steps 30 --warmup 5 --md profiles/lossgrad_r15.md
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

COPY_RATE = 6.29e12  # float4 copy, bytes/s (MI355X_MICROARCH.md; profiles/optim_r14.md)
SHAPES = {"cfg2_b16": dict(B=16, L=128, T=1000, H=2), "cfg5_like": dict(B=8, L=128, T=4000, H=2)}  # BASELINE config 2; config 5's long form


def _cuda(x):
    if torch.is_tensor(x):
        return x.cuda()
    return [a.cuda() for a in x] if isinstance(x, (list, tuple)) else x


def _leaves(predictions):
    from tests import lossgrad_cpu as lg

    leaves = [t.detach().clone().requires_grad_(True) for t in lg.nine(predictions)]
    return tuple(leaves[:5]) + tuple(predictions[5:10]) + (leaves[5:], predictions[11]), leaves


def _loss(level):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    return FastSpeech2TrainingLoss(wl.preprocess_config(level, level), wl.model_config("tiny")).train()


def gate_shares():
    from tests import loss_cpu as lc
    from tests import lossgrad_cpu as lg
    from tests.util import load_golden

    rows = []

    def one(what, level, inputs, predictions, g, want, gates):
        gi = tuple(_cuda(x) for x in inputs)
        gp, leaves = _leaves(tuple(_cuda(x) for x in predictions))
        out = _loss(level)(gi, gp)
        gs = torch.as_tensor(np.asarray(g, dtype=np.float32)).cuda()
        grads = torch.autograd.grad(list(out), leaves, grad_outputs=[gs[i] for i in range(7)])
        got = [d.cpu().numpy() for d in grads]
        share, where = lg.shares(got, want, gates)
        worst = int(np.argmax(share))
        at = tuple(int(v) for v in np.unravel_index(where[worst], got[worst].shape)) if where[worst] >= 0 else ()
        rows.append((what, share, f"{lg.NAMES[worst]}{list(at)}"))

    for name, source in (("lossgrad_tiny", "teacher_tiny"), ("lossgrad_tiny_phoneme_level", "teacher_tiny_phoneme_level")):
        _, z = load_golden(name)
        ms, zs = load_golden(source)
        inputs, predictions = lc.fixture_case(zs, ms, "")
        ref32, ref64 = [z[n] for n in lg.NAMES], [z[n + "_f64"] for n in lg.NAMES]
        one(name, ms["pitch"], inputs, predictions, lg.G_TOTAL, ref64, lg.gate(ref32, ref64, lg.G_TOTAL, lg.n_attn_of(inputs, predictions)))
    for name in lc.CASES:
        for level in lc.LEVELS:
            inputs, predictions, g, want, gates, _, _, _ = lg.case(name, level)
            one(f"{name} {level}", level, inputs, predictions, g, want, gates)
    return lg.NAMES, rows


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
    from tests import loss_cpu as lc
    from tests import lossgrad_cpu as lg

    level = "frame_level"
    dims = SHAPES[shape]
    inputs, predictions = lc.random_case(pitch_level=level, energy_level=level, seed=15, **dims)
    gi = tuple(_cuda(x) for x in inputs)
    base = tuple(_cuda(x) for x in predictions)
    loss = _loss(level)
    gp_a, leaves_a = _leaves(base)
    gp_b, leaves_b = _leaves(base)

    def step_a():
        loss(gi, gp_a)[0].backward()

    def step_b():
        lg.statement(gi, gp_b, level, level)[0].backward()

    # launches and host reads of (a), from its own enqueue path
    step_a()
    torch.cuda.synchronize()
    for x in leaves_a:
        x.grad = None
    before = loss.launches
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        step_a()
    torch.cuda.set_sync_debug_mode("default")
    launches, host_reads = loss.launches - before, len([w for w in seen if "synchroniz" in str(w.message).lower()])
    assert launches == 3, f"value + backward enqueued {launches} launches, not 3"
    assert host_reads == 0, [str(w.message) for w in seen]

    # the backward launch alone
    call = loss._marshal(gi, base)
    _, record = loss._value_with_record(call)
    outs = [torch.empty_like(x) for x in call.nine]
    g = torch.tensor(lg.G_TOTAL).cuda()
    cands = [Candidate("(a) FastSpeech2TrainingLoss: value + total.backward()", step_a, leaves_a),
             Candidate("(b) torch masked_select statement + autograd on the GPU", step_b, leaves_b),
             Candidate("(c) the backward launch alone (ns_lossg_backward, nine outputs)", lambda: loss._backward(call, record, g, outs), [])]
    for i in range(warmup + steps):
        for c in cands:
            c.timed(i >= warmup)
    diff = max(float((a.grad - b.grad).abs().max()) for a, b in zip(leaves_a, leaves_b))
    frames, phonemes = int((~base[7]).sum()), int((~base[6]).sum())
    n_mel = int(base[0].shape[2])
    written = 4 * (2 * base[0].numel() + 2 * base[2].numel() + base[4].numel() + 4 * base[10][0].numel())
    read = 4 * (3 * frames * n_mel + 4 * frames + 2 * phonemes) + 8 * phonemes + base[6].numel() + base[7].numel()
    res = {"shape": shape, **dims, "unmasked_frames": frames, "unmasked_phonemes": phonemes, "launches": launches, "host_reads": host_reads,
           "bytes_written": written, "bytes_read": read, "max_abs_grad_diff_a_vs_b": diff, "candidates": []}
    for c in cands:
        res["candidates"].append({"name": c.name, "events": stats(c.events), "wall": stats(c.wall)})
    t = res["candidates"][2]["events"]["median_ms"] * 1e-3
    res["backward_bytes_per_s"] = (written + read) / t
    res["backward_share_of_float4_copy_rate"] = res["backward_bytes_per_s"] / COPY_RATE
    res["a_over_b_events"] = res["candidates"][0]["events"]["median_ms"] / res["candidates"][1]["events"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["cfg2_b16", "cfg5_like"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shares", action="store_true")
    ap.add_argument("--md")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = ["# Training loss backward (DESIGN.md §19): shares of the gate and timing on one MI355X", "", "Written by `tools/lossgrad_bench.py`.", ""]
    out = {}
    if args.shares:
        names, rows = gate_shares()
        out["shares"] = [{"case": c, "shares": [float(v) for v in s], "worst": w} for c, s, w in rows]
        lines += ["## Shares of the gate", "",
                  "The gate (`tests/lossgrad_cpu.py`), per gradient tensor and absolute: 2 x max |reference fp32 - reference float64| + one fp32 ulp of "
                  "max |reference float64|; the maps add 4 * 2^-24 * ALPHA * |g[0] + g[6]| / n_attn for the device's expf.  The reference is the imported "
                  "reference's own backward on the two fixtures and torch's CPU autograd of the masked_select statement on the seeded cases.  Below: "
                  "max |HIP - float64| / gate per tensor (<= 1 is inside), and the element of the largest share.", "",
                  "| case | " + " | ".join(names) + " | largest at |", "|---|" + "---|" * (len(names) + 1)]
        for case, share, worst in rows:
            lines.append(f"| {case} | " + " | ".join(f"{v:.4f}" for v in share) + f" | {worst} |")
        top = max(float(np.max(s)) for _, s, _ in rows)
        lines += ["", f"Largest share: {top:.4f}.", ""]
        print(json.dumps(out["shares"]), flush=True)
    results = [bench(s, args.steps, args.warmup) for s in args.shapes]
    out["timing"] = results
    for r in results:
        print(json.dumps(r), flush=True)
    if results:
        lines += [f"## Timing (device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after "
                  f"{args.warmup} warm-up steps, ms; candidates alternate step by step in one process)", ""]
        for r in results:
            lines += [f"### {r['shape']}: B = {r['B']}, L = {r['L']}, T = {r['T']}, H = {r['H']} ({r['unmasked_frames']} unmasked frames)", "",
                      "| candidate | device events | wall clock |", "|---|---|---|"]
            for c in r["candidates"]:
                f = lambda k: f"{c[k]['median_ms']:.3f} ({c[k]['min_ms']:.3f} - {c[k]['max_ms']:.3f})"  # noqa: E731
                lines.append(f"| {c['name']} | {f('events')} | {f('wall')} |")
            verdict = "faster than" if r["a_over_b_events"] < 1 else "NOT faster than"
            lines += ["", f"(a) is {verdict} (b): (a) / (b) = {r['a_over_b_events']:.3f} by device events.  (a) enqueued {r['launches']} launches of ours and made "
                      f"{r['host_reads']} host reads (asserted).  The backward launch writes {r['bytes_written'] / 1e6:.1f} MB and must read {r['bytes_read'] / 1e6:.1f} MB: "
                      f"{r['backward_bytes_per_s'] / 1e12:.2f} TB/s over (c)'s median, {100 * r['backward_share_of_float4_copy_rate']:.0f} % of the 6.29 TB/s float4-copy rate "
                      f"(a whole-call figure: the host side of the call and the launch gap are inside).  max |(a) - (b)| over the nine gradients: {r['max_abs_grad_diff_a_vs_b']:.3g}.", ""]
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
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
