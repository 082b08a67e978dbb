#!/usr/bin/env python3
"""The pieces the trainable TxtEncoder / MelDecoder add to their FFT blocks (stacks.py; csrc/stackgrad.hip) on one MI355X.

In one process, candidates alternating step by step, device events around the enqueue and wall clock to a synchronise, medians (p50)
over --steps after --warmup:
  (a) the table gradient at the config-2 encoder shape (M = 16 x 128 rows, D = 256, n_vocab = 361): ns_st_op_embed_grad (one launch, no
      workspace), ns_va_op_embed_bwd (the variance embedding's: LDS table, partials, two launches) on the same indices as int32, and
      torch's own embedding_dense_backward (atomics or a sort, as torch chooses)
  (b) the row mask at the encoder and the decoder shape: ns_st_op_row_mask against torch's masked_fill (both out of place)
  (c) forward + backward of each stack (ljspeech config, eval: no dropout, lens given) against its FFT blocks alone, run from a ready
      input: the difference is what the stack adds (embedding + position add and the table gradient; the position add)
--report adds the accuracy shares tests/test_gpu_stacks.py appended to NS_FP32_OPS_REPORT.  Nothing here is asserted but that the
stacks make no host read when ``lens`` is given.

    python tools/stacks_bench.py --steps 30 --warmup 5 --md profiles/stacks_grad.md
"""
import argparse
import json

import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit, host_reads

SHAPES = {"cfg2_encoder": dict(B=16, S=128), "cfg2_decoder": dict(B=16, S=1000)}  # BASELINE config 2: phoneme level, frame level
D = 256


def bench_embed_grad(steps, warmup):
    import smart_nar_fast_tts_amd._lib as L
    import smart_nar_fast_tts_amd.workload as wl

    lib = L.load()
    B, S, V = SHAPES["cfg2_encoder"]["B"], SHAPES["cfg2_encoder"]["S"], wl.N_SYMBOLS + 1
    M = B * S
    _, texts, lens, _ = wl.synth_inputs(B, S, seed=3)
    texts = torch.from_numpy(texts).cuda()
    idx32 = texts.to(torch.int32).contiguous()
    g = torch.randn(M, D, device="cuda")
    out_a, out_b = torch.empty(V, D, device="cuda"), torch.empty(V, D, device="cuda")
    ws = torch.empty(lib.ns_va_embed_ws_bytes(M, D, V), dtype=torch.uint8, device="cuda")

    def ours():
        L.check(lib.ns_st_op_embed_grad(L.ptr(g), L.ptr(texts), M, D, V, L.ptr(out_a), L.stream_ptr()), "ns_st_op_embed_grad")

    def adaptor():
        L.check(lib.ns_va_op_embed_bwd(L.ptr(g), L.ptr(idx32), M, D, V, L.ptr(out_b), L.ptr(ws), ws.numel(), L.stream_ptr()), "ns_va_op_embed_bwd")

    def torch_own():
        torch.ops.aten.embedding_dense_backward(g, texts.reshape(-1), V, 0, False)

    cands = [Candidate("ns_st_op_embed_grad (k_st_embed_grad, 1 launch)", ours), Candidate("ns_va_op_embed_bwd (launch_va_embed_bwd, 2 launches)", adaptor),
             Candidate("torch embedding_dense_backward (padding_idx 0)", torch_own)]
    alternate(cands, steps, warmup)
    want = torch.ops.aten.embedding_dense_backward(g.double(), texts.reshape(-1), V, 0, False)
    return {"M": M, "D": D, "n_vocab": V, "ws_bytes_adaptor": int(ws.numel()), "max_abs_vs_torch_float64": float((out_a.double() - want).abs().max()),
            "candidates": [c.result() for c in cands]}


def bench_row_mask(shape, steps, warmup):
    import smart_nar_fast_tts_amd._lib as L

    lib = L.load()
    B, S = SHAPES[shape]["B"], SHAPES[shape]["S"]
    lens = torch.randint(S // 2, S + 1, (B,), device="cuda", dtype=torch.int64)
    mask = torch.arange(S, device="cuda")[None, :] >= lens[:, None]
    m8 = mask.view(torch.uint8)
    x, y = torch.randn(B, S, D, device="cuda"), torch.empty(B, S, D, device="cuda")
    pad = mask.unsqueeze(-1)

    def ours():
        L.check(lib.ns_st_op_row_mask(L.ptr(x), L.ptr(m8), None, B, S, D, L.ptr(y), L.stream_ptr()), "ns_st_op_row_mask")

    cands = [Candidate("ns_st_op_row_mask (k_st_row_mask)", ours), Candidate("torch masked_fill", lambda: x.masked_fill(pad, 0))]
    alternate(cands, steps, warmup)
    nbytes = 2.0 * B * S * D * 4
    res = {"shape": shape, "B": B, "S": S, "bytes": nbytes, "candidates": [c.result() for c in cands]}
    res["GBps"] = nbytes / (res["candidates"][0]["events"]["median_ms"] * 1e-3) / 1e9
    return res


def bench_stack(kind, steps, warmup):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import stacks

    shape = "cfg2_encoder" if kind == "encoder" else "cfg2_decoder"
    B, S = SHAPES[shape]["B"], SHAPES[shape]["S"]
    cfg = wl.model_config("ljspeech")
    torch.manual_seed(30)
    m = (stacks.TxtEncoder(cfg) if kind == "encoder" else stacks.MelDecoder(cfg)).cuda().eval()
    _, texts, lens_np, _ = wl.synth_inputs(B, S, seed=4)
    lens = torch.from_numpy(lens_np).cuda()
    mask = torch.arange(S, device="cuda")[None, :] >= lens[:, None]
    g = torch.randn(B, S, D, device="cuda")
    inp = torch.from_numpy(texts).cuda() if kind == "encoder" else torch.randn(B, S, D, device="cuda").requires_grad_(True)
    x0 = torch.randn(B, S, D, device="cuda").requires_grad_(True)

    def whole():
        y = m(inp, mask, lens=lens)
        (y if kind == "encoder" else y[0]).backward(g)

    def blocks():
        y = x0
        for layer in m.layer_stack:
            y, _ = layer(y, mask=mask, lens=lens)
        y.backward(g)

    whole()
    torch.cuda.synchronize()
    n_reads, messages = host_reads(whole)
    assert n_reads == 0, messages
    launches = m.last_launches
    leaves = list(m.parameters()) + [x0] + ([inp] if kind == "decoder" else [])
    cands = [Candidate(f"{type(m).__name__}: forward + backward", whole, leaves), Candidate("its FFT blocks alone, from a ready input", blocks, leaves)]
    alternate(cands, steps, warmup)
    res = {"kind": kind, "B": B, "S": S, "layers": len(m.layer_stack), "launches": launches, "host_reads": n_reads, "candidates": [c.result() for c in cands]}
    res["own_ms"] = res["candidates"][0]["events"]["median_ms"] - res["candidates"][1]["events"]["median_ms"]
    return res


def accuracy_lines(path):
    lines = ["## Accuracy (tests/test_gpu_stacks.py, one run)", "",
             "The eval() output of each stack against the float64 statement: the share of util.gate_value(ref32, ref64).  The native step: the largest "
             "share of optim_cpu.gate_of over the updated tensors.  The table gradient and the row mask are held to bits by the tests, as are "
             "the stacks' gradients (against the hand chain).", "", "| test | what | share |", "|---|---|---|"]
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            if r.get("test", "").startswith("st_"):
                for k, v in r.get("shares", {}).items():
                    lines.append(f"| {r['test']} | {r.get('kind', '')} {k} | {v:.3g} |")
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    common_args(ap, steps=30, warmup=5)
    ap.add_argument("--report", help="an NS_FP32_OPS_REPORT file of tests/test_gpu_stacks.py to summarise")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    results = {"embed_grad": bench_embed_grad(args.steps, args.warmup), "row_mask": [bench_row_mask(s, args.steps, args.warmup) for s in SHAPES],
               "stacks": [bench_stack(k, args.steps, args.warmup) for k in ("encoder", "decoder")]}
    print(json.dumps(results), flush=True)
    e = results["embed_grad"]
    lines = ["# TxtEncoder / MelDecoder training stacks (DESIGN.md §30): timing and accuracy on one MI355X", "", "Written by `tools/stacks_bench.py`.", "",
             f"Device events around the enqueue and wall clock to a synchronise; medians (min - max) of {args.steps} steps after {args.warmup} warm-up "
             "steps, ms; candidates alternate step by step in one process.  Nothing here is asserted.", "",
             f"## The table gradient: M = {e['M']} rows, D = {e['D']}, n_vocab = {e['n_vocab']}", ""]
    lines += candidate_table(e["candidates"])
    lines += ["", f"The variance embedding's kernel needs a {e['ws_bytes_adaptor'] / 1e6:.2f} MB workspace of partials; the new one needs none.  "
              f"max |ns_st_op_embed_grad - torch float64| = {e['max_abs_vs_torch_float64']:.3g}.", ""]
    for r in results["row_mask"]:
        lines += [f"## The row mask: {r['shape']}, B = {r['B']}, S = {r['S']}, D = {D} ({r['bytes'] / 1e6:.1f} MB moved)", ""]
        lines += candidate_table(r["candidates"])
        lines += ["", f"{r['GBps']:.0f} GB/s for the whole call, the host side inside.", ""]
    for r in results["stacks"]:
        lines += [f"## {r['kind']}: B = {r['B']}, S = {r['S']}, {r['layers']} layers, eval(), lens given", ""]
        lines += candidate_table(r["candidates"])
        lines += ["", f"The stack's own part: {r['own_ms']:.3f} ms by device events.  {r['launches']['forward']} launches forward, {r['launches']['backward']} backward, "
                  f"{r['host_reads']} host reads (asserted).", ""]
    if args.report:
        lines += accuracy_lines(args.report)
    emit(args, lines, results)


if __name__ == "__main__":
    main()
