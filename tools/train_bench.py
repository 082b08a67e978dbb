#!/usr/bin/env python3
"""One training step of the trainable FastSpeech2Align (smart_nar_fast_tts_amd.training) on one MI355X, stage by stage, at two shapes:
config 2's training shape (16 utterances of 128 phonemes and 1000 frames, the ljspeech model config) and the test shape (the fixture
tests/golden/train_align_tiny.npz: B 2, L 7, T 20, 1 + 4 layers).

Per stage — forward, loss, backward, optimiser (clip + Adam + zero) — p50 over --steps after --warmup of device events around the
enqueue, the launches the C side counted and the device-to-host reads torch's sync debug mode reports (in the second step).  The stages run in their order
inside one step; each is timed between its own pair of events.  Then the mel head alone: sublayers.MelLinear forward + backward against
the same expression in torch-ROCm with the same weights, alternating step by step.  --report adds the accuracy shares
tests/test_gpu_train_align.py appended to NS_FP32_OPS_REPORT; --bench-note adds one line about the inference benchmark.  Nothing about
speed is asserted, and every figure is one run's.

    python tools/train_bench.py --steps 10 --warmup 2 --md profiles/train_step.md
"""
import argparse
import json

import numpy as np
import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit, host_reads, stats

STAGES = ("forward", "loss", "backward", "optimiser")


def config2_batch(cfg, B=16, L=128, T=1000, seed=0):
    import smart_nar_fast_tts_amd.workload as wl

    rs = np.random.RandomState(seed)
    _, texts, sl, _ = wl.synth_inputs(B, L, seed=seed)
    ml = np.full(B, T, dtype=np.int64)
    mels = (rs.standard_normal((B, T, wl.N_MEL)) * 2.0 - 3.0).astype(np.float32)
    pb, eb = wl.variance_bins(cfg)
    pt = rs.uniform(float(pb[0]), float(pb[-1]), (B, T)).astype(np.float32)
    et = rs.uniform(float(eb[0]), float(eb[-1]), (B, T)).astype(np.float32)
    return (None, None, np.zeros(B, dtype=np.int64), texts, sl, L, mels, ml, T, pt, et)


def to_device(batch):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a for a in batch)


def bench_step(name, pcfg, cfg, sd, batch, steps, warmup, rng="torch"):
    from smart_nar_fast_tts_amd import dropout, optim, training
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    m = training.FastSpeech2Align(pcfg, cfg)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.cuda().train()
    if rng == "philox":  # every mask of a step from one ns_km_draw (dropout.KeepMaskRNG); "torch": torch.bernoulli, mask by mask
        dropout.attach(m, dropout.KeepMaskRNG(1234))
    loss = FastSpeech2TrainingLoss(pcfg, cfg)
    ocfg = {"optimizer": dict(betas=[0.9, 0.98], eps=1e-9, weight_decay=0.0, warm_up_step=4000, anneal_steps=[], anneal_rate=1.0)}
    opt = optim.ScheduledOptim(m, ocfg, cfg, 0)
    batch = to_device(batch)
    times = {s: [] for s in STAGES}
    state = {}

    def fwd():
        state["out"] = m(*batch[2:])

    def lss():
        state["seven"] = loss(batch, state["out"])

    def bwd():
        state["seven"][0].backward()

    def step():
        opt.step_and_update_lr(1.0, zero_grad=True)

    stages = dict(zip(STAGES, (fwd, lss, bwd, step)))
    reads, launches = {}, {}
    for i in range(warmup + steps):
        for s in STAGES:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before = m.launches + loss.launches
            a.record()
            if i == 1:  # the second step: the first one uploads the optimiser's table, which a steady-state step does not
                reads[s] = host_reads(stages[s])[0]
            else:
                stages[s]()
            b.record()
            torch.cuda.synchronize()
            launches[s] = m.launches + loss.launches - before
            if i >= warmup:
                times[s].append(a.elapsed_time(b))
    # the optimiser's C ABI exposes no launch counter: its three launches (the norm in two, the fused clip / Adam / zero update) are
    # what DESIGN.md section 18 states, and the table says so in the cell
    launches["optimiser"] = "3 (by construction, DESIGN.md §18; not counted)"
    return {"name": name, "stages": {s: dict(stats(times[s]), launches=launches[s], host_reads=reads[s]) for s in STAGES},
            "parameters": int(sum(p.numel() for p in m.parameters() if p.requires_grad))}


def bench_mel_head(steps, warmup, B=16, T=1000, d=256):
    from smart_nar_fast_tts_amd import sublayers

    torch.manual_seed(41)
    m = sublayers.MelLinear(d).cuda()
    x = torch.randn(B, T, d, device="cuda").requires_grad_(True)
    g = torch.randn(B, T, 80, device="cuda")
    leaves = [m.weight, m.bias, x]
    ours = lambda: m(x).backward(g)  # noqa: E731
    theirs = lambda: torch.nn.functional.linear(x, m.weight, m.bias).backward(g)  # noqa: E731
    ours()
    counted = dict(m.last_launches)
    cands = [Candidate("sublayers.MelLinear: forward + backward", ours, leaves), Candidate("the same in torch-ROCm", theirs, leaves)]
    alternate(cands, steps, warmup)
    return {"B": B, "T": T, "d": d, "launches": counted, "candidates": [c.result() for c in cands]}


def main():
    import smart_nar_fast_tts_amd.workload as wl
    from tests import train_align_cpu as tc
    from tests.util import load_golden

    ap = argparse.ArgumentParser()
    common_args(ap, 10, 2)  # (at least two warm-up steps: the host reads are counted in the second)
    ap.add_argument("--report")
    ap.add_argument("--bench-note")
    ap.add_argument("--rng", choices=("torch", "philox"), default="torch",
                    help="who draws the dropout keep-masks: torch.bernoulli per mask (the default), or dropout.KeepMaskRNG, one HIP launch per step")
    args = ap.parse_args()
    cfg = wl.model_config("ljspeech")
    sd = wl.synth_state_dict(cfg, seed=0)
    sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
    meta, _ = load_golden("train_align_tiny")
    results = {"steps": [bench_step("config 2: 16 x 128 phonemes, 1000 frames, ljspeech config", wl.preprocess_config(), cfg, sd, config2_batch(cfg),
                                    args.steps, args.warmup, args.rng),
                         bench_step("test shape: 2 x 7 phonemes, 20 frames, 1 + 4 layers", *tc.fixture_config(meta), tc.fixture_state_dict(meta),
                                    tc.fixture_batch(meta), args.steps, args.warmup, args.rng)],
               "mel_head": bench_mel_head(args.steps, args.warmup)}
    lines = ["# One training step of the trainable FastSpeech2Align", "",
             f"One MI355X, one run, p50 of {args.steps} steps after {args.warmup} warm-up steps, device events around each stage's enqueue.",
             "Dropout as configured (masks drawn on the device" + (": one ns_km_draw per step, --rng philox" if args.rng == "philox" else "")
             + ").  Nothing about speed is asserted.", ""]
    for r in results["steps"]:
        lines += [f"## {r['name']} ({r['parameters'] / 1e6:.1f} M trainable parameters)", "", "| stage | p50 ms (min - max) | launches | host reads |", "|---|---|---|---|"]
        for s in STAGES:
            v = r["stages"][s]
            lines.append(f"| {s} | {v['median_ms']:.3f} ({v['min_ms']:.3f} - {v['max_ms']:.3f}) | {v['launches']} | {v['host_reads']} |")
        lines.append("")
    h = results["mel_head"]
    lines += [f"## The mel head alone: {h['B']} x {h['T']} rows, d {h['d']} -> 80 (launches {h['launches']})", ""] + candidate_table(h["candidates"]) + [""]
    if args.report:
        lines += ["## Accuracy (shares of the gate, from tests/test_gpu_train_align.py)", ""]
        rows = [json.loads(x) for x in open(args.report) if x.strip()]
        worst = max((r["d_bias"] for r in rows if r.get("test") == "mh_kernels"), default=None)
        if worst is not None:
            lines.append(f"* `k_mh_pad_colsum`: d_bias at most {worst:.3f} of `colsum_bound` over the 15 cases (and bit-equal to the replayed order)")
        for r in rows:
            if r.get("test") in ("ta_eval", "ta_train", "ta_native_step", "ta_round_trip"):
                lines.append(f"* `{r['test']}`: " + json.dumps({k: v for k, v in r.items() if k != "test"}))
        lin = [max(r["shares"].values()) for r in rows if r.get("test") == "mh_linear"]
        if lin:
            lines.append(f"* `MelLinear` through the two C calls: y and the three gradients at most {max(lin):.3f} of the gate over 6 cases")
        lines.append("")
    if args.bench_note:
        lines += ["## The inference benchmark", "", args.bench_note, ""]
    emit(args, lines, results)


if __name__ == "__main__":
    main()
