"""What the tools/*_bench.py share: the repository on sys.path, the alternating two-clock timing of candidates, the host-read count, the
common command-line arguments and the markdown / JSON tail (DESIGN.md "Shared test and bench support").  What a tool measures — shapes,
the torch restatement, its candidates, derived figures, prose — stays in the tool.  Importing this module initialises no device."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def repo_root():
    return ROOT


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


class Candidate:
    """one timed step: device events around the enqueue and wall clock to a synchronise, the gradients of ``leaves`` cleared first"""

    def __init__(self, name, step, leaves=()):
        self.name, self.step, self.leaves = name, step, leaves
        self.events, self.wall = [], []

    def timed(self, record):
        import torch

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

    def result(self):
        return {"name": self.name, "events": stats(self.events), "wall": stats(self.wall)}


def alternate(cands, steps, warmup):
    """the candidates step by step in turn, ``warmup`` unrecorded rounds and then ``steps`` recorded ones"""
    for i in range(warmup + steps):
        for c in cands:
            c.timed(i >= warmup)


def host_reads(step):
    """(count, messages) of the host reads torch's sync debug mode reports during one ``step()``"""
    import torch

    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        step()
    torch.cuda.set_sync_debug_mode("default")
    return len([w for w in seen if "synchroniz" in str(w.message).lower()]), [str(w.message) for w in seen]


def common_args(ap, steps, warmup):
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--md")
    ap.add_argument("--json")


def candidate_table(candidates):
    """the markdown rows of ``Candidate.result()`` dicts: median (min - max) by device events and by wall clock"""
    lines = ["| candidate | device events | wall clock |", "|---|---|---|"]
    for c in candidates:
        f = lambda k: f"{c[k]['median_ms']:.3f} ({c[k]['min_ms']:.3f} - {c[k]['max_ms']:.3f})"  # noqa: E731
        lines.append(f"| {c['name']} | {f('events')} | {f('wall')} |")
    return lines


def emit(args, lines, results):
    """the markdown to --md (or stdout) and the results to --json"""
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
