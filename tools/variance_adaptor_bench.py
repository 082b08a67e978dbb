#!/usr/bin/env python3
"""VarianceAdaptor forward + backward (adaptor.VarianceAdaptor; csrc/adaptorgrad.hip) on one MI355X against torch.

At B = 16, L = 128, T_pad = 1010 (16160 frame rows), d = 256, n_bins = 256, teacher-forced, eval() (no dropout), for the mixes pp and ff,
in one process, candidates alternating step by step, device events around the enqueue and wall clock to a synchronise, medians over
--steps after --warmup:
  (a) adaptor.VarianceAdaptor: forward, then backward of the four outputs (x, the encoder output, requires grad)
  (b) the baseline: the SAME three predictor.VariancePredictor modules wired with torch.bucketize, F.embedding, repeat_interleave + pad
      and torch autograd — so (a) - (b) is the new kernels against torch's, nothing else
  (c) each new kernel alone through its ns_va_op_* entry (the whole call, host side inside) beside torch's own: embedding backward over
      16160 rows (ns_va_op_embed_bwd; torch.ops.aten.embedding_dense_backward; index_add_), the same with every row in one bin, the
      embedding forward, the length regulator forward and backward at 16 x 128 -> 1010, and a single phoneme of 1000 frames.
Reads nothing but its own tree.

    python tools/variance_adaptor_bench.py --steps 20 --warmup 5 --md profiles/variance_adaptor_timing.md
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

B, L, T, D, NB = 16, 128, 1010, 256, 256


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


def torch_regulate(x, duration, T):
    rows = []
    for b in range(x.shape[0]):
        e = torch.repeat_interleave(x[b], duration[b], dim=0)[:T]
        rows.append(torch.nn.functional.pad(e, (0, 0, 0, T - e.shape[0])))
    return torch.stack(rows)


def baseline_forward(m, x, src_mask, mel_mask, T, pitch_t, energy_t, duration):
    """the reference's wiring in torch ops around the same three HIP predictors"""
    emb = torch.nn.functional.embedding
    log_d = m.duration_predictor(x, src_mask)
    p = e = None
    if m.pitch_feature_level == "phoneme_level":
        p = m.pitch_predictor(x, src_mask)
        x = x + emb(torch.bucketize(pitch_t, m.pitch_bins), m.pitch_embedding.weight)
    if m.energy_feature_level == "phoneme_level":
        e = m.energy_predictor(x, src_mask)
        x = x + emb(torch.bucketize(energy_t, m.energy_bins), m.energy_embedding.weight)
    x = torch_regulate(x, duration, T)
    if m.pitch_feature_level == "frame_level":
        p = m.pitch_predictor(x, mel_mask)
        x = x + emb(torch.bucketize(pitch_t, m.pitch_bins), m.pitch_embedding.weight)
    if m.energy_feature_level == "frame_level":
        e = m.energy_predictor(x, mel_mask)
        x = x + emb(torch.bucketize(energy_t, m.energy_bins), m.energy_embedding.weight)
    return x, p, e, log_d


def durations(rs, total_max):
    """[B, L] int64: ragged utterances whose totals stay at or below total_max, the longest reaching it"""
    d = rs.randint(2, 14, size=(B, L)).astype(np.int64)
    src_lens = rs.randint(L // 2, L + 1, size=B)
    src_lens[0] = L
    d[np.arange(L)[None, :] >= src_lens[:, None]] = 0
    for b in range(B):
        while d[b].sum() > total_max:
            d[b, rs.randint(src_lens[b])] = 1
    d[0, 0] += total_max - d[0].sum()
    return d, src_lens


def module_candidates(mix):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import adaptor

    level = {"p": "phoneme_level", "f": "frame_level"}
    mc = wl.model_config("ljspeech")
    mc["variance_predictor"]["dropout"] = 0.0
    torch.manual_seed(26)
    m = adaptor.VarianceAdaptor(wl.preprocess_config(level[mix[0]], level[mix[1]]), mc).cuda().eval()
    rs = np.random.RandomState(27)
    d, src_lens = durations(rs, T)
    dur = torch.from_numpy(d).cuda()
    src_mask = torch.from_numpy(np.arange(L)[None, :] >= src_lens[:, None]).cuda()
    mel_mask = torch.from_numpy(np.arange(T)[None, :] >= d.sum(1)[:, None]).cuda()
    tgt = {}
    for s, c in zip(("pitch", "energy"), mix):
        bins = getattr(m, f"{s}_bins")
        lo, hi = float(bins[0]), float(bins[-1])
        n, mask = (L, src_mask) if c == "p" else (T, mel_mask)
        t = torch.from_numpy(rs.uniform(lo, hi, size=(B, n)).astype(np.float32)).cuda()
        tgt[s] = t.masked_fill(mask, 0.0)
    xa = torch.randn(B, L, D, device="cuda").requires_grad_(True)
    xb = xa.detach().clone().requires_grad_(True)
    g = [torch.randn(B, T, D, device="cuda"), torch.randn_like(tgt["pitch"]), torch.randn_like(tgt["energy"]), torch.randn(B, L, device="cuda")]
    params = [p for p in m.parameters() if p.requires_grad]

    def step_a():
        y, p, e, log_d, *_ = m(xa, src_mask, mel_mask, T, tgt["pitch"], tgt["energy"], dur)
        torch.autograd.backward([y, p, e, log_d], g)

    def step_b():
        torch.autograd.backward(list(baseline_forward(m, xb, src_mask, mel_mask, T, tgt["pitch"], tgt["energy"], dur)), g)

    n0 = m.launches()
    y, p, e, log_d, *_ = m(xa, src_mask, mel_mask, T, tgt["pitch"], tgt["energy"], dur)
    n1 = m.launches()
    torch.autograd.backward([y, p, e, log_d], g)
    n2 = m.launches()
    new = {k: dict(getattr(m, k).last_launches) for k in ("pitch_embedding", "energy_embedding", "length_regulator")}
    launches = {"forward": n1 - n0, "backward": n2 - n1, "new_kernels": new}
    return [Candidate(f"(a) {mix}: adaptor.VarianceAdaptor", step_a, [xa] + params),
            Candidate(f"(b) {mix}: the same predictors + torch bucketize / embedding / repeat_interleave + autograd", step_b, [xb] + params)], launches


def kernel_candidates():
    import smart_nar_fast_tts_amd._lib as Lb

    lib = Lb.load()
    P, S = Lb.ptr, Lb.stream_ptr
    M = B * T
    rs = np.random.RandomState(28)
    g = torch.randn(M, D, device="cuda")
    x = torch.randn(M, D, device="cuda")
    table = torch.randn(NB, D, device="cuda")
    bins = torch.linspace(-2, 2, NB - 1, device="cuda")
    target = torch.randn(M, device="cuda")
    idx = torch.bucketize(target, bins).to(torch.int32)
    idx64 = idx.long()
    one = torch.zeros(M, dtype=torch.int32, device="cuda")
    one64 = one.long()
    y, idx_out, dt = torch.empty(M, D, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(NB, D, device="cuda")
    ws = torch.empty(lib.ns_va_embed_ws_bytes(M, D, NB), dtype=torch.uint8, device="cuda")
    d, _ = durations(rs, T)
    dur = torch.from_numpy(d).cuda()
    xe, ge = torch.randn(B, L, D, device="cuda"), torch.randn(B, T, D, device="cuda")
    out, cum, mel_len, dx = torch.empty(B, T, D, device="cuda"), torch.empty(B, L, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda"), torch.empty(B, L, D, device="cuda")
    d1 = np.ones((1, 8), dtype=np.int64)
    d1[0, 3] = 1000
    dur1 = torch.from_numpy(d1).cuda()
    T1 = int(d1.sum())
    x1, g1 = torch.randn(1, 8, D, device="cuda"), torch.randn(1, T1, D, device="cuda")
    out1, cum1, len1, dx1 = torch.empty(1, T1, D, device="cuda"), torch.empty(1, 8, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(1, 8, D, device="cuda")
    acc = torch.zeros(NB, D, device="cuda")
    xg = xe.clone().requires_grad_(True)

    def torch_lr():
        torch_regulate(xg, dur, T).backward(ge)

    calls = {
        "embed_fwd: ns_va_op_embed_fwd": lambda: Lb.check(lib.ns_va_op_embed_fwd(P(x), P(target), P(bins), P(table), M, D, NB, P(y), P(idx_out), S()), "fwd"),
        "embed_fwd: torch x + F.embedding(bucketize)": lambda: x + torch.nn.functional.embedding(torch.bucketize(target, bins), table),
        "embed_bwd: ns_va_op_embed_bwd": lambda: Lb.check(lib.ns_va_op_embed_bwd(P(g), P(idx), M, D, NB, P(dt), P(ws), ws.numel(), S()), "bwd"),
        "embed_bwd: torch embedding_dense_backward": lambda: torch.ops.aten.embedding_dense_backward(g, idx64, NB, -1, False),
        "embed_bwd: torch zeros + index_add_": lambda: acc.zero_().index_add_(0, idx64, g),
        "embed_bwd, every row in one bin: ns_va_op_embed_bwd": lambda: Lb.check(lib.ns_va_op_embed_bwd(P(g), P(one), M, D, NB, P(dt), P(ws), ws.numel(), S()), "bwd"),
        "embed_bwd, every row in one bin: torch embedding_dense_backward": lambda: torch.ops.aten.embedding_dense_backward(g, one64, NB, -1, False),
        "embed_bwd, every row in one bin: torch zeros + index_add_": lambda: acc.zero_().index_add_(0, one64, g),
        "lr_fwd 16 x 128 -> 1010: ns_va_op_lr_fwd": lambda: Lb.check(lib.ns_va_op_lr_fwd(P(xe), P(dur), B, L, D, T, P(out), P(cum), P(mel_len), S()), "lr"),
        "lr_bwd 16 x 128 -> 1010: ns_va_op_lr_bwd": lambda: Lb.check(lib.ns_va_op_lr_bwd(P(ge), P(cum), B, L, D, T, P(dx), S()), "lr"),
        "lr fwd + bwd 16 x 128 -> 1010: torch repeat_interleave + pad + autograd": torch_lr,
        "lr_fwd, one phoneme of 1000 frames: ns_va_op_lr_fwd": lambda: Lb.check(lib.ns_va_op_lr_fwd(P(x1), P(dur1), 1, 8, D, T1, P(out1), P(cum1), P(len1), S()), "lr"),
        "lr_bwd, one phoneme of 1000 frames: ns_va_op_lr_bwd": lambda: Lb.check(lib.ns_va_op_lr_bwd(P(g1), P(cum1), 1, 8, D, T1, P(dx1), S()), "lr"),
    }
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    plan = (__import__("ctypes").c_int32 * 8)()
    lib.ns_va_plan_embed(M, D, NB, plan)
    return [Candidate(k, f, [xg] if f is torch_lr else ()) for k, f in calls.items()], list(plan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"B": B, "L": L, "T": T, "d": D, "n_bins": NB, "modules": {}, "kernels": {}}
    for mix in ("pp", "ff"):
        cands, launches = module_candidates(mix)
        for i in range(args.warmup + args.steps):
            for c in cands:
                c.timed(i >= args.warmup)
        a, b = (float(np.median(c.events)) for c in cands)
        res["modules"][mix] = {"launches": launches, "a_over_b_events": a / b,
                               "candidates": [{"name": c.name, "events": stats(c.events), "wall": stats(c.wall)} for c in cands]}
    cands, plan = kernel_candidates()
    for i in range(args.warmup + args.steps):
        for c in cands:
            c.timed(i >= args.warmup)
    res["plan_embed"] = plan
    for c in cands:
        res["kernels"][c.name] = stats(c.events)
    print(json.dumps(res), flush=True)
    lines = ["# VarianceAdaptor forward + backward: timing on one MI355X", "", "Written by `tools/variance_adaptor_bench.py`.", "",
             f"B = {B}, L = {L}, T_pad = {T} ({B * T} frame rows), d = {D}, n_bins = {NB}.  Device events around the enqueue and wall clock to a synchronise; "
             f"medians (min - max) of {args.steps} steps after {args.warmup} warm-up steps, ms; candidates alternate step by step in one process.", ""]
    for mix, r in res["modules"].items():
        lines += [f"## mix {mix}", "", "| candidate | device events | wall clock |", "|---|---|---|"]
        for c in r["candidates"]:
            f = lambda k: f"{c[k]['median_ms']:.3f} ({c[k]['min_ms']:.3f} - {c[k]['max_ms']:.3f})"  # noqa: E731
            lines.append(f"| {c['name']} | {f('events')} | {f('wall')} |")
        verdict = "faster than" if r["a_over_b_events"] < 1 else "SLOWER than"
        lines += ["", f"(a) is {verdict} (b): (a) / (b) = {r['a_over_b_events']:.3f} by device events.  (a) enqueued {r['launches']['forward']} launches forward and "
                  f"{r['launches']['backward']} backward; of those the new kernels: {json.dumps(r['launches']['new_kernels'])}.", ""]
    lines += ["## each new kernel alone (the whole call) beside torch's own", "",
              f"ns_va_plan_embed({B * T}, {D}, {NB}) = {plan}", "", "| call | ms: median (min - max) |", "|---|---|"]
    for k, v in res["kernels"].items():
        lines.append(f"| {k} | {v['median_ms']:.4f} ({v['min_ms']:.4f} - {v['max_ms']:.4f}) |")
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
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
