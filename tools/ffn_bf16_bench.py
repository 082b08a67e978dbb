#!/usr/bin/env python3
"""The opt-in "bf16" matmul mode of the position-wise feed-forward sublayer (sublayers.PositionwiseFeedForward(matmul="bf16");
csrc/ffngrad_bf16.hip) against the exact-fp32 mode on one MI355X.

Per shape (N(0, 1) rows, d = 256, d_inner = 1024, kernel sizes (9, 1), eval: no dropout), in one process, the fp32 and the bf16
candidates alternating step by step, device events around the enqueue and wall clock to a synchronise, medians (p50) over --steps after
--warmup:
  (a) ``y = module(x); y.backward(g)`` in either mode, x requiring grad (seven gradients)
  (b) each weight gradient alone, GEMM + reduce: ns_pg_op_wgrad (k_pg_wgrad, fp32) and ns_fg_op_wgrad_bf16 (k_fg_wgrad_bf16), for dW1
      ([d_inner, d, 9]) and dW2 ([d, d_inner, 1]); 2 M N KW Cin flop each over the time of the two launches
  (c) da = conv(du, w2^T) alone, pack + GEMM: ns_pg_op_dgrad and ns_fg_op_conv_bf16 in transposed form
--report adds the shares of their gates tests/test_gpu_ffn_bf16.py appended to NS_FP32_OPS_REPORT.  Nothing here is asserted.

    python tools/ffn_bf16_bench.py --steps 30 --warmup 5 --md profiles/ffn_bf16.md
"""
import argparse
import ctypes
import json

import numpy as np
import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit

SHAPES = {"cfg2_encoder": dict(B=16, S=128), "cfg2_decoder": dict(B=16, S=1000)}  # BASELINE config 2: phoneme level, frame level
D, D_INNER, KS = 256, 1024, (9, 1)


def bench(shape, steps, warmup):
    import smart_nar_fast_tts_amd._lib as L
    from smart_nar_fast_tts_amd import sublayers

    B, S = SHAPES[shape]["B"], SHAPES[shape]["S"]
    M = B * S
    torch.manual_seed(36)
    mods = {"fp32": sublayers.PositionwiseFeedForward(D, D_INNER, KS, dropout=0.1).cuda().eval()}
    mods["bf16"] = sublayers.PositionwiseFeedForward(D, D_INNER, KS, dropout=0.1, matmul="bf16").cuda().eval()
    mods["bf16"].load_state_dict(mods["fp32"].state_dict())
    xs = {k: torch.randn(B, S, D, device="cuda", generator=torch.Generator("cuda").manual_seed(1)).requires_grad_(True) for k in mods}
    g = torch.randn(B, S, D, device="cuda")
    lib = L.load()
    ws = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    du, dh = torch.randn(M, D, device="cuda"), torch.randn(M, D_INNER, device="cuda")
    x2 = xs["fp32"].detach().reshape(M, D)
    h = torch.relu(torch.randn(M, D_INNER, device="cuda"))
    dW1, dW2 = torch.empty(D_INNER, D, KS[0], device="cuda"), torch.empty(D, D_INNER, KS[1], device="cuda")
    da = torch.empty(M, D_INNER, device="cuda")
    w2 = mods["fp32"].w_2.weight.detach()
    st = L.stream_ptr

    def module_step(k):
        return lambda: mods[k](xs[k]).backward(g)

    def wgrad32(dz, X, N, Cin, KW, dW):
        return lambda: L.check(lib.ns_pg_op_wgrad(L.ptr(dz), L.ptr(X), B, S, N, Cin, KW, L.ptr(dW), None, L.ptr(ws), ws.numel(), st()), "ns_pg_op_wgrad")

    def wgrad16(dz, X, N, Cin, KW, dW):
        return lambda: L.check(lib.ns_fg_op_wgrad_bf16(L.ptr(dz), L.ptr(X), B, S, N, Cin, KW, L.ptr(dW), L.ptr(ws), ws.numel(), st()), "ns_fg_op_wgrad_bf16")

    def da32():
        L.check(lib.ns_pg_op_dgrad(L.ptr(du), L.ptr(w2), B, S, D, D_INNER, KS[1], L.ptr(da), L.ptr(ws), ws.numel(), st()), "ns_pg_op_dgrad")

    def da16():
        L.check(lib.ns_fg_op_conv_bf16(L.ptr(du), L.ptr(w2), None, None, B, S, D, D_INNER, KS[1], 1, 0, L.ptr(da), L.ptr(ws), ws.numel(), st()), "ns_fg_op_conv_bf16")

    cands = [Candidate("(a) forward + backward, matmul = fp32", module_step("fp32"), [xs["fp32"]] + mods["fp32"].ordered_parameters()),
             Candidate("(a) forward + backward, matmul = bf16", module_step("bf16"), [xs["bf16"]] + mods["bf16"].ordered_parameters()),
             Candidate("(b) dW1 alone, fp32 (k_pg_wgrad + reduce)", wgrad32(dh, x2, D_INNER, D, KS[0], dW1)),
             Candidate("(b) dW1 alone, bf16 (k_fg_wgrad_bf16 + reduce)", wgrad16(dh, x2, D_INNER, D, KS[0], dW1)),
             Candidate("(b) dW2 alone, fp32 (k_pg_wgrad + reduce)", wgrad32(du, h, D, D_INNER, KS[1], dW2)),
             Candidate("(b) dW2 alone, bf16 (k_fg_wgrad_bf16 + reduce)", wgrad16(du, h, D, D_INNER, KS[1], dW2)),
             Candidate("(c) da alone, fp32 (pack + GEMM)", da32),
             Candidate("(c) da alone, bf16 (pack + GEMM)", da16)]
    alternate(cands, steps, warmup)
    med = [float(np.median(c.events)) for c in cands]
    flop = {"dW1": 2.0 * M * D_INNER * KS[0] * D, "dW2": 2.0 * M * D * KS[1] * D_INNER, "da": 2.0 * M * D_INNER * KS[1] * D}
    rates = {}
    for name, i in (("dW1", 2), ("dW2", 4), ("da", 6)):
        rates[name] = {"fp32_ms": med[i], "bf16_ms": med[i + 1], "fp32_TFLOPs": flop[name] / med[i] / 1e9, "bf16_TFLOPs": flop[name] / med[i + 1] / 1e9,
                       "speedup": med[i] / med[i + 1]}
    plan = (ctypes.c_int32 * 8)()
    lib.ns_fg_plan_wgrad_bf16(M, D_INNER, D, KS[0], plan)
    return {"shape": shape, "B": B, "S": S, "M": M, "launches": {k: dict(m.last_launches) for k, m in mods.items()}, "layer_speedup": med[0] / med[1],
            "gemms": rates, "dW1_plan": {"rows": plan[2], "ranges": plan[3], "tiles": plan[4]}, "candidates": [c.result() for c in cands],
            "max_rel_dx_distance": float((xs["bf16"].grad - xs["fp32"].grad).abs().max() / xs["fp32"].grad.abs().max())}


def accuracy_lines(path):
    """the largest share per test and quantity of an NS_FP32_OPS_REPORT file written by tests/test_gpu_ffn_bf16.py"""
    worst = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            if not r.get("test", "").startswith("fgb_") or r["test"] == "fgb_launches":  # (launch counts, not shares)
                continue
            for k in ("share", "forward", "transposed", "z", "y"):
                if k in r and r[k] >= worst.get((r["test"], k), (-1.0, ""))[0]:
                    worst[(r["test"], k)] = (r[k], " ".join(str(r[f]) for f in ("cfg", "weight", "case", "mode") if f in r))
    lines = ["## Accuracy: the largest share of its gate per test and quantity (tests/test_gpu_ffn_bf16.py, one run)", "",
             "share / forward / transposed: of GEMM_REL x the sum of |rounded products| (float64 with rounded operands); z: of the same plus the fp32 "
             "row arithmetic; y: of FP32_REL.", "", "| test | quantity | largest share | where |", "|---|---|---|---|"]
    for (test, k), (v, where) in sorted(worst.items()):
        lines.append(f"| {test} | {k} | {v:.3g} | {where} |")
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    common_args(ap, steps=30, warmup=5)
    ap.add_argument("--report", help="an NS_FP32_OPS_REPORT file of tests/test_gpu_ffn_bf16.py to summarise")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = [bench(s, args.steps, args.warmup) for s in args.shapes]
    lines = ["# Feed-forward sublayer in the opt-in bf16 matmul mode (DESIGN.md §36): timing against the fp32 mode on one MI355X", "",
             "Written by `tools/ffn_bf16_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, "
             "ms; the fp32 and bf16 candidates alternate step by step in one process.  Nothing here is asserted.", ""]
    for r in results:
        print(json.dumps(r), flush=True)
        lines += [f"## {r['shape']}: B = {r['B']}, S = {r['S']}, d = {D}, d_inner = {D_INNER}, kernel sizes {KS}", ""]
        lines += candidate_table(r["candidates"])
        lines += ["", f"One layer forward + backward: fp32 / bf16 = {r['layer_speedup']:.2f} by device events; launches {r['launches']}.  "
                  f"max |dx bf16 - dx fp32| / max |dx fp32| = {r['max_rel_dx_distance']:.2g} (the two modes compute different functions: not an error figure).  "
                  f"The bf16 dW1 split: {r['dW1_plan']}.", "",
                  "| contraction | fp32 ms | bf16 ms | fp32 TFLOP/s | bf16 TFLOP/s | fp32 / bf16 |", "|---|---|---|---|---|---|"]
        for k, q in r["gemms"].items():
            lines.append(f"| {k} | {q['fp32_ms']:.3f} | {q['bf16_ms']:.3f} | {q['fp32_TFLOPs']:.1f} | {q['bf16_TFLOPs']:.1f} | {q['speedup']:.2f} |")
        lines.append("")
    if args.report:
        lines += accuracy_lines(args.report)
    emit(args, lines, results)


if __name__ == "__main__":
    main()
