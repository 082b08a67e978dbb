"""Build recipe for the C-ABI library: hipcc, gfx950 only, in-tree output
(``csrc/libnarfs2.so`` travels to the GPU box with the repo snapshot)."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libnarfs2.so")
SOURCES = ["gemm_conv.hip", "gemm_bf16x3.hip", "gemm_bf16.hip", "attention.hip", "rowops.hip", "api.hip", "vocoder.hip",
           "vocoder_bf16.hip", "vocoder_api.hip", "cross_attention.hip", "aligner_api.hip", "loss.hip", "loss_api.hip", "melfront.hip",
           "melfront_api.hip", "griffinlim.hip", "griffinlim_api.hip", "vartargets.hip", "vartargets_api.hip",
           "optim.hip", "optim_api.hip", "lossgrad.hip", "lossgrad_api.hip", "predgrad.hip", "predgrad_api.hip",
           "attngrad.hip", "attngrad_api.hip", "xattngrad.hip", "xattngrad_api.hip", "postnetgrad.hip", "postnetgrad_api.hip",
           "adaptorgrad.hip", "adaptorgrad_api.hip", "ffngrad.hip", "ffngrad_api.hip", "ffngrad_bf16.hip", "ffngrad_bf16_api.hip",
           "stackgrad.hip", "stackgrad_api.hip", "melencgrad.hip", "melencgrad_api.hip",
           "melheadgrad.hip", "melheadgrad_api.hip", "keepmask.hip", "keepmask_api.hip",
           "dataset.hip", "dataset_api.hip", "gaussgrad.hip", "gaussgrad_api.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result"]
# attention keeps its O^T / S^T accumulators in architectural VGPRs (gfx950 has one unified 512-entry file): the
# online softmax touches them with VALU ops, and in AGPR form hipcc shuttles all 64+16 registers through
# v_accvgpr_read/write every key tile.
EXTRA_FLAGS = {"attention.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]}


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = _hipcc()
    headers = sorted(os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "nar_fs2.h"))
    objs, jobs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + headers):
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(s, []) + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--no-undefined", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
