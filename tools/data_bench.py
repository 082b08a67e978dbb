#!/usr/bin/env python3
"""What a training batch costs on one MI355X, made two ways that alternate batch by batch in one session (tools/_bench.py): the host
route — the reference's collate restated in numpy (tests/dataset_cpu.py ``collate_statement``: ``np.pad`` per utterance, ``np.stack``)
followed by ``to_device`` to the GPU, seven pageable host-to-device copies — against one ``ns_ds_gather`` out of the device-resident
set (``data.DeviceDataset``, csrc/dataset.hip).

The set is synthetic and LJSpeech-sized: 13 100 utterances, L uniform in [40, 128] phonemes at the 8 frames per phoneme of workload
``cfg2_b16`` (T = min(8 L, 1000)), n_mel 80, frame-level pitch and energy; the batches are the first ones of a training epoch at config
2's batch size (16 utterances, sorted in groups of 64, so a batch is 16 x ~128 phonemes x ~1000 frames at the long end).  Recorded: the
pack + upload time and the uploaded bytes, both routes' p50 under device events and wall clock, the gather back to back, host reads per
batch, and each route beside one ``train_step`` at config 2 as tools/train_bench.py measures it in the same session.  Nothing about
speed is asserted, and every figure is one run's.

    python tools/data_bench.py --steps 20 --warmup 3 --md profiles/data_loader.md
"""
import argparse
import time

import numpy as np
import torch

from _bench import Candidate, alternate, candidate_table, common_args, emit, host_reads, stats
from train_bench import STAGES, bench_step, config2_batch

N_UTTERANCES, BATCH, GROUP = 13100, 16, 4
KERNEL_REPS = 10


def synthetic_set(n, seed=0):
    """lists of per-utterance arrays (views of four big ones) in the shape ``DeviceDataset.from_arrays`` takes"""
    import smart_nar_fast_tts_amd.workload as wl

    fpp = wl.WORKLOADS["cfg2_b16"][3]
    rs = np.random.default_rng(seed)
    L = rs.integers(40, 129, size=n)
    T = np.minimum((L * fpp).astype(np.int64), 1000)
    cut = lambda a, lens: np.split(a, np.cumsum(lens)[:-1])  # noqa: E731
    mel = rs.random((int(T.sum()), wl.N_MEL), dtype=np.float32)
    return dict(ids=[f"utt{i:05d}" for i in range(n)], raw_texts=[""] * n, speakers=[0] * n,
                texts=cut(rs.integers(1, wl.N_SYMBOLS, size=int(L.sum())), L), mels=cut(mel, T),
                pitches=cut(rs.random(int(T.sum()), dtype=np.float32), T), energies=cut(rs.random(int(T.sum()), dtype=np.float32), T))


def main():
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import data
    from tests import dataset_cpu as dc

    ap = argparse.ArgumentParser()
    common_args(ap, 20, 3)
    ap.add_argument("--utterances", type=int, default=N_UTTERANCES)
    ap.add_argument("--no-train-step", action="store_true", help="skip the train_step measurement (the shares are then left out)")
    ap.add_argument("--bench-note")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.init()
    u = synthetic_set(args.utterances)
    t0 = time.perf_counter()
    ds = data.DeviceDataset.from_arrays(u["ids"], u["raw_texts"], u["speakers"], u["texts"], u["mels"], u["pitches"], u["energies"], wl.preprocess_config(), dev)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0

    batches = data.plan_epoch(ds.text_lens, BATCH, GROUP, generator=torch.Generator().manual_seed(0))[:args.steps + args.warmup]
    order_dev, order_host, _pinned = ds.upload_order(batches)
    firsts = np.concatenate([[0], np.cumsum([len(b) for b in batches])])
    turn = {"host": 0, "gather": 0}
    keep = {}

    def host_route():
        k = turn["host"] % len(batches)
        turn["host"] += 1
        b = dc.collate_statement(u, batches[k].tolist())
        keep["host"] = tuple(torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in b)

    def gather_route():
        k = turn["gather"] % len(batches)
        turn["gather"] += 1
        keep["gather"] = ds.gather(order_dev, order_host, int(firsts[k]), len(batches[k]))

    cands = [Candidate("host route: collate_statement + to_device (7 pageable copies)", host_route),
             Candidate("one ns_ds_gather out of the device-resident set", gather_route)]
    alternate(cands, args.steps, args.warmup)
    # both routes give the same batch, bit for bit (the last one each made is the same index batch)
    same = all(torch.equal(a, b) for a, b in zip(keep["host"], keep["gather"]) if isinstance(a, torch.Tensor)) and \
        keep["host"][6].cpu().numpy().tobytes() == keep["gather"][6].cpu().numpy().tobytes()
    launches_before = ds.launches
    reads, msgs = host_reads(gather_route)
    counted = ds.launches - launches_before
    # the gather back to back: KERNEL_REPS gathers of one batch between one pair of events (allocation and enqueue included)
    k = int(np.argmax([int(ds.mel_lens[b].max()) for b in batches]))
    per = []
    for i in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(KERNEL_REPS):
            out = ds.gather(order_dev, order_host, int(firsts[k]), len(batches[k]))
        b.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            per.append(a.elapsed_time(b) / KERNEL_REPS)
    out_bytes = sum(t.numel() * t.element_size() for t in out if isinstance(t, torch.Tensor))
    back = stats(per)
    res = {"utterances": len(ds), "upload_bytes": ds.upload_bytes, "pack_and_upload_s": upload_s, "routes": [c.result() for c in cands],
           "same_bits": bool(same), "host_reads_per_batch": reads, "host_read_messages": msgs, "launches_per_batch": counted,
           "back_to_back": dict(back, batch_shape=[int(v) for v in out[6].shape], output_bytes=out_bytes,
                                tbs_moved=2.0 * out_bytes / (back["median_ms"] * 1e-3) / 1e12 if back["median_ms"] > 0 else float("nan"))}
    lines = ["# A training batch: the host collate + to_device against one gather out of the device-resident set", "",
             f"One MI355X, one run, p50 of {args.steps} batches after {args.warmup} warm-up batches; the two routes alternate batch by batch over the first "
             f"batches of one epoch (batch size {BATCH}, groups of {BATCH * GROUP}).  Device events span the enqueue and the device work; wall clock runs "
             "to a synchronise.  The stream is idle between batches, so the host time between a route's two events (numpy, allocation, enqueue) is in both clocks.  Nothing about speed is asserted.", "",
             f"The set: {len(ds)} synthetic utterances, {ds.upload_bytes / 1e9:.3f} GB on the device (mel, pitch, energy, text, speaker, four offset tables, "
             f"four length vectors); packing and uploading it took {upload_s:.2f} s of wall clock, once.", ""]
    lines += candidate_table(res["routes"])
    lines += ["", f"* both routes' last batch is the same bits: {res['same_bits']}",
              f"* launches per batch the C side counted: {counted}; host reads per batch torch's sync debug mode reported: {reads}",
              f"* the gather back to back ({KERNEL_REPS} gathers of the longest batch, mels {res['back_to_back']['batch_shape']}, between one pair of events; the "
              f"seven `torch.empty` and the enqueue included), per gather: {back['median_ms']:.4f} ms ({back['min_ms']:.4f} - {back['max_ms']:.4f}); "
              f"{out_bytes / 1e6:.3f} MB written and as much read: {res['back_to_back']['tbs_moved']:.3f} TB/s moved", ""]
    if not args.no_train_step:
        cfg = wl.model_config("ljspeech")
        sd = wl.synth_state_dict(cfg, seed=0)
        sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
        ts = bench_step("config 2", wl.preprocess_config(), cfg, sd, config2_batch(cfg), max(args.steps // 2, 5), 2)
        step_ms = sum(ts["stages"][s]["median_ms"] for s in STAGES)
        res["train_step_ms"] = step_ms
        lines += ["## Beside one training step", "",
                  f"One `train_step` at config 2 (16 x 128 phonemes, 1000 frames; forward + loss + backward + optimiser, p50 of each stage as "
                  f"tools/train_bench.py measures it, in this session): {step_ms:.2f} ms.", "",
                  "| route | device events, share of a step | wall clock, share of a step |", "|---|---|---|"]
        for c in res["routes"]:
            lines.append(f"| {c['name']} | {100.0 * c['events']['median_ms'] / step_ms:.2f} % | {100.0 * c['wall']['median_ms'] / step_ms:.2f} % |")
        lines.append("")
    if args.bench_note:
        lines += ["## The inference benchmark", "", args.bench_note, ""]
    emit(args, lines, res)


if __name__ == "__main__":
    main()
