#!/usr/bin/env python3
"""What the dropout keep-masks of one training step cost on one MI355X, drawn two ways that alternate step by step in one session under
device events (tools/_bench.py): mask by mask with ``torch.bernoulli`` (the default path of every trainable layer: a ``torch.full``, a
``bernoulli`` and a cast per mask) against one ``ns_km_draw`` of the whole list (``dropout.KeepMaskRNG.prefetch``, csrc/keepmask.hip).

At two shapes — config 2's training shape (16 utterances of 128 phonemes and 1000 frames, the ljspeech model config) and the test shape
(B 2, L 7, T 20, 1 + 4 layers at the ljspeech dropout rates) — it records the draws alone (time, launches, bytes of temporaries), the
kernel's achieved store bandwidth against the 8 TB/s peak, and the forward of ``training.FastSpeech2Align`` with and without a
generator attached (two models on the same weights).  Nothing about speed is asserted, and every figure is one run's.

    python tools/keepmask_bench.py --steps 20 --warmup 3 --md profiles/keepmask.md
"""
import argparse

import numpy as np
import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit, stats
from train_bench import config2_batch, to_device

PEAK_TBS = 8.0
KERNEL_REPS = 10


def build(pcfg, cfg, sd):
    from smart_nar_fast_tts_amd import training

    m = training.FastSpeech2Align(pcfg, cfg)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.cuda().train()


def bench_shape(name, pcfg, cfg, sd, batch, steps, warmup):
    import smart_nar_fast_tts_amd._lib as nl
    from smart_nar_fast_tts_amd import dropout

    dev = torch.device("cuda", torch.cuda.current_device())
    m_torch, m_philox = build(pcfg, cfg, sd), build(pcfg, cfg, sd)
    rng = dropout.KeepMaskRNG(1234)
    dropout.attach(m_philox, rng)
    batch = to_device(batch)
    B, L, T = batch[3].shape[0], batch[3].shape[1], batch[6].shape[1]
    entries = m_torch._step_masks({}, B, L, T, int(batch[8]))
    elems = sum(int(np.prod(s)) for s, _ in entries)
    keep = {}

    def by_torch():  # _train.HipTrainModule._keep_masks' expression, mask by mask
        keep["t"] = [torch.bernoulli(torch.full(s, 1.0 - p, dtype=torch.float32, device=dev)).to(torch.uint8) for s, p in entries]

    def by_philox():
        rng.next_call()
        rng.prefetch(entries, dev)

    draws = [Candidate(f"{len(entries)} masks through torch.bernoulli", by_torch), Candidate("one ns_km_draw of the same list", by_philox)]
    alternate(draws, steps, warmup)
    before = rng.launches
    by_philox()
    counted = rng.launches - before
    arena_bytes = sum((int(np.prod(s)) + 15) // 16 * 16 for s, _ in entries)
    # the kernel alone: KERNEL_REPS draws of the list back to back into one arena between one pair of events, so that the host's share
    # of a single draw (the table lookup, the allocation, the views) is not in the figure
    table, need, _ = rng._table(tuple((tuple(s), float(p)) for s, p in entries), dev)[:3]
    arena = torch.empty(need, dtype=torch.uint8, device=dev)
    lib = nl.load()
    per_launch = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(KERNEL_REPS):
            nl.check(lib.ns_km_draw(nl.ptr(table), len(entries), 1234, i + 1, nl.ptr(arena), need, nl.stream_ptr(dev)), "ns_km_draw")
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            per_launch.append(a.elapsed_time(b) / KERNEL_REPS)
    fwd = [Candidate("forward, masks by torch.bernoulli (the parent's path)", lambda: m_torch(*batch[2:])),
           Candidate("forward, generator attached (one ns_km_draw)", lambda: m_philox(*batch[2:]))]
    alternate(fwd, steps, warmup)
    res = {"name": name, "masks": len(entries), "elements": elems, "arena_bytes": arena_bytes, "draws": [c.result() for c in draws],
           "launches": {"torch": f"{3 * len(entries)} (full, bernoulli, cast per mask; by construction, not counted)", "philox": counted},
           "temporaries_bytes": {"torch": 8 * elems, "philox": 0}, "forward": [c.result() for c in fwd],
           "forward_launches": {"torch": m_torch.last_launches["forward"], "philox": m_philox.last_launches["forward"]}}
    res["kernel_alone"] = stats(per_launch)
    ms = res["kernel_alone"]["median_ms"]
    res["store_tbs"] = arena_bytes / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")
    return res


def main():
    import smart_nar_fast_tts_amd.workload as wl
    from tests import train_align_cpu as tc
    from tests.util import load_golden

    ap = argparse.ArgumentParser()
    common_args(ap, 20, 3)
    ap.add_argument("--bench-note")
    args = ap.parse_args()
    cfg = wl.model_config("ljspeech")
    sd = wl.synth_state_dict(cfg, seed=0)
    sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
    meta, _ = load_golden("train_align_tiny")
    pcfg_t, cfg_t = tc.fixture_config(meta)
    cfg_t = dict(cfg_t, transformer=dict(cfg_t["transformer"], encoder_dropout=0.2, decoder_dropout=0.2),
                 variance_predictor=dict(cfg_t["variance_predictor"], dropout=0.5))
    results = {"shapes": [bench_shape("config 2: 16 x 128 phonemes, 1000 frames, ljspeech config", wl.preprocess_config(), cfg, sd, config2_batch(cfg),
                                      args.steps, args.warmup),
                          bench_shape("test shape: 2 x 7 phonemes, 20 frames, 1 + 4 layers", pcfg_t, cfg_t, tc.fixture_state_dict(meta), tc.fixture_batch(meta),
                                      args.steps, args.warmup)]}
    lines = ["# Dropout keep-masks: torch.bernoulli mask by mask against one ns_km_draw", "",
             f"One MI355X, one run, p50 of {args.steps} steps after {args.warmup} warm-up steps; the two candidates of a table alternate step by step.",
             "Device events span the enqueue and the kernels; wall clock runs to a synchronise.  Nothing about speed is asserted.", ""]
    for r in results["shapes"]:
        lines += [f"## {r['name']}", "", f"{r['masks']} masks, {r['elements'] / 1e6:.3f} M elements, arena {r['arena_bytes'] / 1e6:.3f} MB.", "",
                  "### The draws alone", ""] + candidate_table(r["draws"]) + [
                  "", f"* launches: torch {r['launches']['torch']}; ns_km_draw {r['launches']['philox']} (counted by the C side)",
                  f"* float32 temporaries written: torch {r['temporaries_bytes']['torch'] / 1e6:.3f} MB (the `full` and the `bernoulli` result, 4 bytes an "
                  f"element each, read back once each); ns_km_draw none",
                  f"* `k_km_draw` alone ({KERNEL_REPS} draws back to back between one pair of events, per draw): {r['kernel_alone']['median_ms']:.4f} ms "
                  f"({r['kernel_alone']['min_ms']:.4f} - {r['kernel_alone']['max_ms']:.4f}); achieved store bandwidth (arena bytes / that p50): "
                  f"{r['store_tbs']:.3f} TB/s = {100.0 * r['store_tbs'] / PEAK_TBS:.1f} % of the {PEAK_TBS:.0f} TB/s peak",
                  "", "### The forward of training.FastSpeech2Align", ""] + candidate_table(r["forward"]) + [
                  "", f"* launches the C side counted in the forward: {r['forward_launches']['torch']} without a generator (the torch draws are not among "
                  f"them), {r['forward_launches']['philox']} with one (the draw is)", ""]
    if args.bench_note:
        lines += ["## The inference benchmark", "", args.bench_note, ""]
    emit(args, lines, results)


if __name__ == "__main__":
    main()
