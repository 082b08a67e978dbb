"""CPU emulation of the vocoder's opt-in bf16 matmul mode, on top of tests/hifigan_cpu.py: every upsampler and resblock-conv
weight rounded with .to(torch.bfloat16), and a forward pre-hook on the same modules that rounds the fp32 activation (the leaky
ReLU output) to bf16 before the float64 (or fp32) evaluation.  Shared by tests/test_gpu_vocoder_bf16.py and
tools/vocoder_bench.py --accuracy --matmul bf16."""
from __future__ import annotations

import torch

from tests import hifigan_cpu


def bf(t):
    """round to bf16 (nearest even) and back, in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def lrelu32(x, slope=0.1):
    """the kernel's fp32 leaky ReLU: one fp32 multiply for x <= 0"""
    return torch.where(x > 0, x, x * torch.tensor(slope, dtype=torch.float32))


def gemm_modules(m):
    return list(m.ups) + [c for rb in m.resblocks for c in list(rb.convs1) + list(rb.convs2)]


def emulation(h, sd, dtype=torch.float64):
    """hifigan_cpu.Generator with the bf16 mode's roundings: weights rounded from the folded fp32 ones, and each GEMM layer's
    input rounded from fp32 to bf16 before the evaluation in dtype"""
    m = hifigan_cpu.folded(h, sd, torch.float32)
    with torch.no_grad():
        for mod in gemm_modules(m):
            mod.weight.copy_(bf(mod.weight))
    m = m.to(dtype)
    for mod in gemm_modules(m):
        mod.register_forward_pre_hook(lambda mod, inp: (inp[0].float().to(torch.bfloat16).to(inp[0].dtype),))
    return m


def snr_db(ref, x):
    ref, x = ref.double(), x.double()
    return 10.0 * float(torch.log10((ref ** 2).sum() / ((x - ref) ** 2).sum()))
