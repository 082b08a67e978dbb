#!/usr/bin/env python3
"""The trainable MelEncoder (stacks.MelEncoder, sublayers.Prenet; csrc/melencgrad.hip) on one MI355X, at config 2's aligner shape: 16
utterances of 1000 frames against 128 phonemes, the ljspeech model config (d 256, 2 heads, d_inner 1024, kernels (9, 1), 4 layers).

In one process, candidates alternating step by step, device events around the enqueue and wall clock to a synchronise, medians (p50)
over --steps after --warmup:
  (a) the Prenet alone, forward + backward in train() with a given keep-mask (p = 0.2): sublayers.Prenet against the same expression in
      torch-ROCm with the same weights, and the same without d_mels (no N = 80 data-gradient GEMM, no frame-0 select) and without d_w1
      (no weight gradient at Cin = 80).  At 17 short launches the call is bound by the enqueue, so those differences say little; the
      two launches that had never been timed are therefore also run alone, REPEAT times back to back between one pair of events:
      ns_pg_op_wgrad at N = 256, Cin = 80 (GEMM and reduce) and ns_pg_op_dgrad at N = 256, Cin = 80 (pack and the N = 80 GEMM)
  (b) the 4-layer stack, forward + backward in eval() (no dropout) with both length vectors given, the loss over y and every map:
      stacks.MelEncoder against an equivalent torch-ROCm composite with the same weights
--report adds the accuracy shares tests/test_gpu_mel_encoder.py appended to NS_FP32_OPS_REPORT; --bench-note adds one line about the
inference benchmark.  Nothing about speed is asserted; the stack is asserted to make no host read when both length vectors are given.

    python tools/mel_encoder_bench.py --steps 20 --warmup 3 --md profiles/mel_encoder_grad.md
"""
import argparse
import json

import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit, host_reads

B, T, L_SRC, D, N_MEL = 16, 1000, 128, 256, 80  # BASELINE config 2: frame level against phoneme level
REPEAT = 20


def torch_prenet(w1, b1, w2, b2, mels, pos, keep_scaled):
    lin = torch.nn.functional.linear
    x = torch.cat([torch.zeros_like(mels[:, :1]), mels[:, 1:]], dim=1)
    h = torch.relu(lin(torch.relu(lin(x, w1, b1)), w2, b2))
    return (h if keep_scaled is None else h * keep_scaled) + pos[None, :mels.shape[1]]


def torch_block(p, src, tgt, key_pad, row_pad, H):
    """FFTBlock2 (transformer/Layers.py:51-70) at dropout 0 from a dict of one layer's parameters"""
    lin = torch.nn.functional.linear
    Bc, Tc, d = tgt.shape
    Lc, dk = src.shape[1], d // H
    q = lin(tgt, p["crs_attn.w_qs.weight"], p["crs_attn.w_qs.bias"]).view(Bc, Tc, H, dk).transpose(1, 2)
    k = lin(src, p["crs_attn.w_ks.weight"], p["crs_attn.w_ks.bias"]).view(Bc, Lc, H, dk).transpose(1, 2)
    v = lin(src, p["crs_attn.w_vs.weight"], p["crs_attn.w_vs.bias"]).view(Bc, Lc, H, dk).transpose(1, 2)
    attn = torch.softmax((q @ k.transpose(-1, -2) / dk ** 0.5).masked_fill(key_pad[:, None, None, :], float("-inf")), dim=-1)
    ctx = (attn @ v).transpose(1, 2).reshape(Bc, Tc, d)
    x = torch.nn.functional.layer_norm(lin(ctx, p["crs_attn.fc.weight"], p["crs_attn.fc.bias"]) + tgt, (d,), p["crs_attn.layer_norm.weight"],
                                       p["crs_attn.layer_norm.bias"]).masked_fill(row_pad, 0)
    conv = torch.nn.functional.conv1d
    k1, k2 = p["pos_ffn.w_1.weight"].shape[2], p["pos_ffn.w_2.weight"].shape[2]
    h = torch.relu(conv(x.transpose(1, 2), p["pos_ffn.w_1.weight"], p["pos_ffn.w_1.bias"], padding=(k1 - 1) // 2))
    u = conv(h, p["pos_ffn.w_2.weight"], p["pos_ffn.w_2.bias"], padding=(k2 - 1) // 2).transpose(1, 2)
    y = torch.nn.functional.layer_norm(u + x, (d,), p["pos_ffn.layer_norm.weight"], p["pos_ffn.layer_norm.bias"])
    return y.masked_fill(row_pad, 0), attn


def bench_prenet(steps, warmup):
    from smart_nar_fast_tts_amd import ops, sublayers

    torch.manual_seed(40)
    m = sublayers.Prenet().cuda().train()
    params = m.ordered_parameters()
    mels = (torch.randn(B, T, N_MEL, device="cuda") * 2 - 3).requires_grad_(True)
    pos = ops.sinusoid_table(T + 1, D)
    keep = (torch.rand(B, T, D, device="cuda") >= m.p_drop).to(torch.uint8)
    keep_scaled = keep.float() / (1.0 - m.p_drop)
    g = torch.randn(B, T, D, device="cuda")

    def ours(x_grad=True, frozen=()):
        def step():
            for i, p in enumerate(params):
                p.requires_grad_(i not in frozen)
            mels.requires_grad_(x_grad)
            m(mels, pos, keep_mask=keep).backward(g)
        return step

    def composite():
        for p in params:
            p.requires_grad_(True)
        mels.requires_grad_(True)
        torch_prenet(*params, mels, pos, keep_scaled).backward(g)

    full = ours()
    full()
    launches = dict(m.last_launches)
    leaves = params + [mels]
    cands = [Candidate("sublayers.Prenet: forward + backward", full, leaves), Candidate("the same in torch-ROCm", composite, leaves),
             Candidate("sublayers.Prenet without d_mels", ours(x_grad=False), leaves), Candidate("sublayers.Prenet without d_w1", ours(frozen=(0,)), leaves)]
    alternate(cands, steps, warmup)
    for p in params:
        p.requires_grad_(True)
    res = {"B": B, "T": T, "launches": launches, "candidates": [c.result() for c in cands]}
    med = [c["events"]["median_ms"] for c in res["candidates"]]
    res["dmels_ms"], res["dw1_ms"] = med[0] - med[2], med[0] - med[3]
    return res


def bench_narrow_launches(steps, warmup):
    """the weight gradient at Cin = 80 and the data gradient into 80 columns alone, REPEAT calls between one pair of events"""
    import smart_nar_fast_tts_amd._lib as L

    lib = L.load()
    M = B * T
    dz, x, w = torch.randn(M, D, device="cuda"), torch.randn(M, N_MEL, device="cuda"), torch.randn(D, N_MEL, 1, device="cuda")
    dw, dx = torch.empty(D, N_MEL, 1, device="cuda"), torch.empty(M, N_MEL, device="cuda")
    ws = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")

    def wgrad():
        for _ in range(REPEAT):
            L.check(lib.ns_pg_op_wgrad(L.ptr(dz), L.ptr(x), B, T, D, N_MEL, 1, L.ptr(dw), None, L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pg_op_wgrad")

    def dgrad():
        for _ in range(REPEAT):
            L.check(lib.ns_pg_op_dgrad(L.ptr(dz), L.ptr(w), B, T, D, N_MEL, 1, L.ptr(dx), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_pg_op_dgrad")

    cands = [Candidate(f"weight gradient, N = 256, Cin = 80: {REPEAT} x (GEMM + reduce)", wgrad),
             Candidate(f"data gradient into 80 columns: {REPEAT} x (pack + GEMM)", dgrad)]
    alternate(cands, steps, warmup)
    res = {"M": M, "repeat": REPEAT, "candidates": [c.result() for c in cands]}
    flop = 2.0 * M * N_MEL * D
    res["per_call_ms"] = [c["events"]["median_ms"] / REPEAT for c in res["candidates"]]
    res["tflops"] = [flop / (t * 1e-3) / 1e12 for t in res["per_call_ms"]]
    return res


def bench_stack(steps, warmup):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import stacks

    cfg = wl.model_config("ljspeech")
    H = cfg["transformer"]["decoder_head"]
    torch.manual_seed(41)
    m = stacks.MelEncoder(cfg).cuda().eval()
    n_layers = len(m.layer_stack)
    _, _, src_lens_np, _ = wl.synth_inputs(B, L_SRC, seed=4)
    src_lens = torch.from_numpy(src_lens_np).cuda()
    mel_lens = torch.randint(T // 2, T + 1, (B,), device="cuda", dtype=torch.int64)
    src_mask = torch.arange(L_SRC, device="cuda")[None, :] >= src_lens[:, None]
    tgt_mask = torch.arange(T, device="cuda")[None, :] >= mel_lens[:, None]
    src = torch.randn(B, L_SRC, D, device="cuda").requires_grad_(True)
    mels = (torch.randn(B, T, N_MEL, device="cuda") * 2 - 3).requires_grad_(True)
    gs = [torch.randn(B, T, D, device="cuda")] + [torch.randn(B, H, T, L_SRC, device="cuda") / T for _ in range(n_layers)]
    named = dict(m.named_parameters())
    layers = [{k[len(f"layer_stack.{i}."):]: v for k, v in named.items() if k.startswith(f"layer_stack.{i}.")} for i in range(n_layers)]
    pos = m.position_enc.detach()[0]
    row_pad = tgt_mask.unsqueeze(-1)

    def whole():
        y, attns = m(src, mels, src_mask, tgt_mask, src_lens=src_lens, mel_lens=mel_lens)
        torch.autograd.backward([y] + attns, gs)

    def composite():
        x = torch_prenet(named["prenet.w_1.weight"], named["prenet.w_1.bias"], named["prenet.w_2.weight"], named["prenet.w_2.bias"], mels, pos, None)
        attns = []
        for p in layers:
            x, a = torch_block(p, src, x, src_mask, row_pad, H)
            attns.append(a)
        torch.autograd.backward([x] + attns, gs)

    whole()
    torch.cuda.synchronize()
    n_reads, messages = host_reads(whole)
    assert n_reads == 0, messages
    launches = m.last_launches
    with torch.no_grad():
        y_a = m(src, mels, src_mask, tgt_mask, src_lens=src_lens, mel_lens=mel_lens)[0]
        x = torch_prenet(named["prenet.w_1.weight"], named["prenet.w_1.bias"], named["prenet.w_2.weight"], named["prenet.w_2.bias"], mels, pos, None)
        for p in layers:
            x, _ = torch_block(p, src, x, src_mask, row_pad, H)
    leaves = [p for p in m.parameters() if p.requires_grad] + [src, mels]
    cands = [Candidate("stacks.MelEncoder: forward + backward", whole, leaves), Candidate("the same in torch-ROCm", composite, leaves)]
    alternate(cands, steps, warmup)
    return {"B": B, "T": T, "L": L_SRC, "layers": n_layers, "launches": launches, "host_reads": n_reads, "max_abs_y_vs_torch": float((y_a - x).abs().max()),
            "candidates": [c.result() for c in cands]}


def accuracy_lines(path):
    lines = ["## Accuracy (tests/test_gpu_mel_encoder.py, one run)", "",
             "Shares of util.gate_value(ref32, ref64) unless said otherwise.  The two kernels' outputs and the stack's gradients are held to "
             "bits by the tests (against the numpy statements and the hand chain); d_b2 is the share of its derived bound "
             "(0.5 ulp32 + M 2^-53 sum |dh|), the native step the largest share of optim_cpu.gate_of.", "", "| test | case | worst share |", "|---|---|---|"]
    worst_b2 = 0.0
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            t = r.get("test", "")
            if t == "me_kernels":
                worst_b2 = max(worst_b2, r["d_b2"])
            elif t == "me_prenet":
                lines.append(f"| me_prenet forward | {r['shape']} p {r['p']} | {max(r['forward'].values()):.3g} |")
                lines.append(f"| me_prenet gradients | {r['shape']} p {r['p']} | {max(r['shares'].values()):.3g} |")
            elif t in ("me_forward", "me_native_step"):
                lines.append(f"| {t} | {', '.join(r['shares'])} | {max(r['shares'].values()):.3g} |")
    lines.append(f"| me_kernels d_b2 (a share of 1 - 1e-6 is an exact tie of the one rounding) | 24 cases | {worst_b2:.7f} |")
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, steps=20, warmup=3)
    ap.add_argument("--report", help="an NS_FP32_OPS_REPORT file of tests/test_gpu_mel_encoder.py to summarise")
    ap.add_argument("--bench-note", help="one line about the inference benchmark before and after, copied into the markdown")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = {"prenet": bench_prenet(args.steps, args.warmup), "narrow": bench_narrow_launches(args.steps, args.warmup),
               "stack": bench_stack(args.steps, args.warmup)}
    print(json.dumps(results), flush=True)
    p, s, n = results["prenet"], results["stack"], results["narrow"]
    lines = ["# Trainable MelEncoder (DESIGN.md §31): timing and accuracy on one MI355X", "", "Written by `tools/mel_encoder_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up "
             "steps, ms; candidates alternate step by step in one process.  Nothing about speed is asserted.", "",
             f"## The Prenet: B = {p['B']}, T = {p['T']}, train() at p = 0.2 with a given keep-mask", ""]
    lines += candidate_table(p["candidates"])
    lines += ["", f"{p['launches']['forward']} launches forward, {p['launches']['backward']} backward.  By difference of the medians, leaving d_mels out saves "
              f"{p['dmels_ms']:.3f} ms and leaving d_w1 out {p['dw1_ms']:.3f} ms: at this many short launches the call is bound by the enqueue, not "
              "by the device, so the two launches are also timed alone.", "",
              f"## The two narrow launches alone: M = {n['M']} rows, {n['repeat']} calls back to back between one pair of events", ""]
    lines += candidate_table(n["candidates"])
    lines += ["", f"Per call: the weight gradient at Cin = 80 {n['per_call_ms'][0]:.4f} ms ({n['tflops'][0]:.1f} TFLOP/s of {2.0 * n['M'] * N_MEL * D / 1e9:.2f} "
              f"GFLOP), the data gradient into 80 columns {n['per_call_ms'][1]:.4f} ms ({n['tflops'][1]:.1f} TFLOP/s); the fp32 MFMA peak is 157.3.  "
              "Neither is tuned here.", "",
              f"## The stack: B = {s['B']}, T = {s['T']}, L = {s['L']}, {s['layers']} layers, eval(), both length vectors given", ""]
    lines += candidate_table(s["candidates"])
    lines += ["", f"{s['launches']['forward']} launches forward, {s['launches']['backward']} backward, {s['host_reads']} host reads (asserted).  "
              f"max |y - torch composite| = {s['max_abs_y_vs_torch']:.3g}.", ""]
    if args.report:
        lines += accuracy_lines(args.report)
    if args.bench_note:
        lines += ["## The inference benchmark", "", args.bench_note, ""]
    emit(args, lines, results)


if __name__ == "__main__":
    main()
