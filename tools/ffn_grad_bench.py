#!/usr/bin/env python3
"""Position-wise feed-forward sublayer forward + backward (sublayers.PositionwiseFeedForward; csrc/ffngrad.hip) on one MI355X against
torch.

Per shape (N(0, 1) rows, d = 256, d_inner = 1024, kernel sizes (9, 1), eval: no dropout), in one process, candidates alternating step
by step, device events around the enqueue and wall clock to a synchronise, medians (p50) over --steps after --warmup:
  (a) ``y = module(x); y.backward(g)`` through sublayers.PositionwiseFeedForward, x requiring grad (seven gradients)
  (b) the same through an nn.Module restatement of the reference (nn.Conv1d, F.relu, nn.Conv1d, + x, nn.LayerNorm) and torch-ROCm
      autograd on the GPU
  (c) the backward alone with every output wanted, and with one output left out: the difference is what that output's launches take
      (dW1 and dW2: the weight gradient's GEMM and its reduce; dx: its data-gradient GEMM)
  (d) da = conv(du, w2^T) alone (ns_pg_op_dgrad: the pack kernel and the GEMM) and the ReLU gate alone (ns_fg_op_relu_gate with d_b1)
Each of the four GEMMs is 2 M d d_inner K flop; its share is that over its time over the 157.3 TFLOP/s fp32 MFMA peak.  Taken from the
tool's own enqueue path: the launches of (a) as the C side counted them, and that (a) makes no host read (torch's sync debug mode
reports none).  --report adds the accuracy shares tests/test_gpu_ffn_grad.py appended to NS_FP32_OPS_REPORT.

    python tools/ffn_grad_bench.py --steps 30 --warmup 5 --md profiles/ffn_grad.md
"""
import argparse
import json

import numpy as np
import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit, host_reads

PEAK = 157.3e12  # fp32 MFMA flop/s (MI355X_MICROARCH.md)
SHAPES = {"cfg2_encoder": dict(B=16, S=128), "cfg2_decoder": dict(B=16, S=1000)}  # BASELINE config 2: phoneme level, frame level
D, D_INNER, KS = 256, 1024, (9, 1)
NAMES = ("dx", "w1", "b1", "w2", "b2", "ln_g", "ln_b")  # order of the module's _backward


class TorchFFN(torch.nn.Module):
    """the reference's module restated (transformer/SubLayers.py:62-95), dropout left out (eval)"""

    def __init__(self, d, d_inner, ks):
        super().__init__()
        self.w_1 = torch.nn.Conv1d(d, d_inner, kernel_size=ks[0], padding=(ks[0] - 1) // 2)
        self.w_2 = torch.nn.Conv1d(d_inner, d, kernel_size=ks[1], padding=(ks[1] - 1) // 2)
        self.layer_norm = torch.nn.LayerNorm(d)

    def forward(self, x):
        out = self.w_2(torch.nn.functional.relu(self.w_1(x.transpose(1, 2)))).transpose(1, 2)
        return self.layer_norm(out + x)


def against_float64(ours, x, g, grads, h):
    """{name: max |grad - float64| / max |float64|} with the float64 gradients taken by torch's autograd on the GPU from the SAME gate:
    relu is replaced by a multiplication with the constant mask (h > 0) of the device's saved h, so a pre-activation that rounds to the
    other side of zero in float64 does not enter."""
    p = {n: t.detach().double().requires_grad_(True) for n, t in zip(NAMES[1:], ours.ordered_parameters())}
    x64 = x.detach().double().requires_grad_(True)
    conv = torch.nn.functional.conv1d
    pre = conv(x64.transpose(1, 2), p["w1"], p["b1"], padding=(KS[0] - 1) // 2)
    gated = pre * (h.reshape(x.shape[0], x.shape[1], -1) > 0).transpose(1, 2).double()
    u = conv(gated, p["w2"], p["b2"], padding=(KS[1] - 1) // 2).transpose(1, 2)
    y = torch.nn.functional.layer_norm(u + x64, (x.shape[-1],), p["ln_g"], p["ln_b"], 1e-5)
    want = torch.autograd.grad(y, [x64] + [p[n] for n in NAMES[1:]], grad_outputs=g.double())
    return {n: float((a.double() - w).abs().max() / w.abs().max()) for n, a, w in zip(NAMES, grads, want)}


def bench(shape, steps, warmup):
    import smart_nar_fast_tts_amd._lib as L
    from smart_nar_fast_tts_amd import sublayers

    B, S = SHAPES[shape]["B"], SHAPES[shape]["S"]
    M = B * S
    torch.manual_seed(28)
    ours = sublayers.PositionwiseFeedForward(D, D_INNER, KS, dropout=0.1).cuda().eval()
    ref = TorchFFN(D, D_INNER, KS).cuda().eval()
    ref.load_state_dict(ours.state_dict())
    xa = torch.randn(B, S, D, device="cuda").requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    g = torch.randn(B, S, D, device="cuda")

    def step_a():
        ours(xa).backward(g)

    def step_b():
        ref(xb).backward(g)

    step_a()
    torch.cuda.synchronize()
    n_reads, messages = host_reads(step_a)
    launches = dict(ours.last_launches)
    assert n_reads == 0, messages

    lib = L.load()
    call = ours._marshal(xa.detach(), None)
    _, saved = ours._forward(call, save=True)

    rel64 = against_float64(ours, xa, g, ours._backward(call, saved, g, [True] * 7), saved[:M * D_INNER])

    def backward(without=()):
        need = [n not in without for n in NAMES]
        return lambda: ours._backward(call, saved, g, need)

    du = torch.randn(M, D, device="cuda")
    da = torch.empty(M, D_INNER, device="cuda")
    h = saved[:M * D_INNER]
    d_b1 = torch.empty(D_INNER, device="cuda")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    w2 = ours.w_2.weight.detach()

    def step_da():
        L.check(lib.ns_pg_op_dgrad(L.ptr(du), L.ptr(w2), B, S, D, D_INNER, KS[1], L.ptr(da), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pg_op_dgrad")

    def step_gate():
        L.check(lib.ns_fg_op_relu_gate(L.ptr(da), L.ptr(h), M, D_INNER, L.ptr(da), L.ptr(d_b1), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_fg_op_relu_gate")

    leaves_a = [xa] + ours.ordered_parameters()
    leaves_b = [xb] + list(ref.parameters())
    cands = [Candidate("(a) sublayers.PositionwiseFeedForward: forward + backward", step_a, leaves_a),
             Candidate("(b) torch nn.Module restatement + autograd on the GPU", step_b, leaves_b),
             Candidate("(c) the backward alone, every output wanted", backward()),
             Candidate("(c) the backward without dW1", backward(("w1",))),
             Candidate("(c) the backward without dW2", backward(("w2",))),
             Candidate("(c) the backward without dx", backward(("dx",))),
             Candidate("(d) da = conv(du, w2^T) alone (pack + GEMM)", step_da),
             Candidate("(d) the ReLU gate alone, with d_b1 (two launches)", step_gate)]
    alternate(cands, steps, warmup)
    diff = float((xa.grad - xb.grad).abs().max())
    med = [float(np.median(c.events)) for c in cands]
    flop = {"dW1": 2.0 * M * D_INNER * KS[0] * D, "dW2": 2.0 * M * D * KS[1] * D_INNER, "da": 2.0 * M * D_INNER * KS[1] * D, "dx": 2.0 * M * D * KS[0] * D_INNER}
    ms = {"dW1": med[2] - med[3], "dW2": med[2] - med[4], "dx": med[2] - med[5], "da": med[6]}
    gemms = {k: {"flop": flop[k], "ms": ms[k], "floor_us": flop[k] / PEAK * 1e6, "share_of_peak": (flop[k] / (ms[k] * 1e-3) / PEAK) if ms[k] > 0 else None}
             for k in ("dW1", "dW2", "da", "dx")}
    gate_bytes = 3.0 * M * D_INNER * 4
    res = {"shape": shape, "B": B, "S": S, "M": M, "d": D, "d_inner": D_INNER, "kernel": list(KS), "launches": launches, "host_reads": n_reads,
           "max_abs_dx_diff_a_vs_b": diff, "rel_err_vs_float64_same_gate": rel64, "gemms": gemms, "gate_ms": med[7], "gate_bytes": gate_bytes, "gate_GBps": gate_bytes / (med[7] * 1e-3) / 1e9,
           "candidates": [c.result() for c in cands]}
    res["a_over_b_events"] = med[0] / med[1]
    return res


def accuracy_lines(path):
    """the largest share per test and tensor of an NS_FP32_OPS_REPORT file written by tests/test_gpu_ffn_grad.py"""
    worst = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            if not r.get("test", "").startswith("fg_"):
                continue
            flat = dict(r.get("shares", {}))
            flat.update({k: r[k] for k in ("h", "z", "y", "d_b1") if k in r})
            for k, v in flat.items():
                key = (r["test"] + (" " + r["mode"] if "mode" in r else ""), k)
                if v >= worst.get(key, (-1.0, ""))[0]:
                    worst[key] = (v, " ".join(str(r[f]) for f in ("cfg", "case", "shape") if f in r))
    lines = ["## Accuracy: the largest share of its bound per test and tensor (tests/test_gpu_ffn_grad.py, one run)", "",
             "h, z, y: of the fp32 bounds of tests/bf16_emu.py; d_b1 of the gate alone: of one fp32 rounding of the float64 column sum; the "
             "gradients: of the project gate, judged from the device's saved h and z; the native step: of optim_cpu.gate_of.", "",
             "| test | tensor | largest share | where |", "|---|---|---|---|"]
    for (test, k), (v, where) in sorted(worst.items()):
        lines.append(f"| {test} | {k} | {v:.3g} | {where} |")
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    common_args(ap, steps=30, warmup=5)
    ap.add_argument("--report", help="an NS_FP32_OPS_REPORT file of tests/test_gpu_ffn_grad.py to summarise")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = [bench(s, args.steps, args.warmup) for s in args.shapes]
    lines = ["# Position-wise feed-forward sublayer forward + backward (DESIGN.md §28): timing and accuracy on one MI355X", "",
             "Written by `tools/ffn_grad_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, "
             "ms; candidates alternate step by step in one process.  Nothing here is asserted.", ""]
    for r in results:
        print(json.dumps(r), flush=True)
        lines += [f"## {r['shape']}: B = {r['B']}, S = {r['S']}, d = {r['d']}, d_inner = {r['d_inner']}, kernel sizes {tuple(r['kernel'])}", ""]
        lines += candidate_table(r["candidates"])
        verdict = "faster than" if r["a_over_b_events"] < 1 else "SLOWER than"
        lines += ["", f"(a) is {verdict} (b): (a) / (b) = {r['a_over_b_events']:.3f} by device events.  (a) enqueued {r['launches'].get('forward')} launches forward and "
                  f"{r['launches'].get('backward')} backward and made {r['host_reads']} host reads (asserted).  max |dx (a) - dx (b)|: "
                  f"{r['max_abs_dx_diff_a_vs_b']:.3g} (torch's own fp32 forward, algorithms and gate; not a reference: the float64 comparison "
                  "follows).  Against float64 autograd on the GPU gated by the device's saved h, max |grad - float64| / max |float64|: "
                  + ", ".join(f"{k} {v:.2g}" for k, v in r["rel_err_vs_float64_same_gate"].items()) + ".", "",
                  "| GEMM of the backward | GFLOP | time, ms | floor at the fp32 MFMA peak, ms | achieved share of the peak | how timed |", "|---|---|---|---|---|---|"]
        how = {"dW1": "backward with everything - backward without dW1 (GEMM + reduce)", "dW2": "backward with everything - backward without dW2 (GEMM + reduce)",
               "da": "ns_pg_op_dgrad alone (pack + GEMM)", "dx": "backward with everything - backward without dx"}
        for k in ("dW1", "dW2", "da", "dx"):
            q = r["gemms"][k]
            share = "n/a" if q["share_of_peak"] is None else f"{q['share_of_peak']:.3f}"
            lines.append(f"| {k} | {q['flop'] / 1e9:.1f} | {q['ms']:.3f} | {q['floor_us'] / 1e3:.3f} | {share} | {how[k]} |")
        slow = max(("dW1", "dW2", "da", "dx"), key=lambda k: r["gemms"][k]["ms"])
        lines += ["", f"The slowest of the four is {slow}.  The ReLU gate with d_b1 (its own pass: {r['gate_bytes'] / 1e9:.3f} GB moved) takes {r['gate_ms']:.3f} ms "
                  f"= {r['gate_GBps']:.0f} GB/s for the whole call (two launches, the host side inside).", ""]
    if args.report:
        lines += accuracy_lines(args.report)
    emit(args, lines, results)


if __name__ == "__main__":
    main()
