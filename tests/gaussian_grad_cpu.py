"""The yardstick of the Gaussian length regulator's backward (csrc/gaussgrad.hip k_gu_prepare / k_gu_denominators / k_gu_bwd), over the
forward's yardstick tests/gaussian_cpu.py.  No test lives here: tests/test_gaussian_grad_host.py proves it both ways on the CPU,
tests/test_gpu_gaussian_grad.py holds the kernels to it.

Reference, in float64: with w [B, L, T] of ``gaussian_cpu.Reference`` and lim_b = min(max(own_len_b, 0), T) (T where own_len is None)

    d_x[b, l] = sum_{t < lim_b} w_lt g[b, t]

The bound is the forward's, transposed, with the project's own figures and no new constant:

    |d_x' - d_x| <= sum_{t < lim_b} bound_w_lt |g_t| + FP32_REL sum_{t < lim_b} w_lt |g_t|

bound_w is the elementwise first-order bound of a generated weight (gaussian_cpu's docstring counts its roundings), FP32_REL the
project's figure for an fp32 contraction on a fmaf chain (tests/bf16_emu.py) — here the chain over t.  Where the bound is zero (an
utterance with lim_b = 0) d_x must be exactly +0.0.

``emulate`` is numpy fp32 in the kernel's order: the forward emulation's weights (the eight-stripe denominator tree, + 1e-20f, the
division), then per 32-phoneme tile acc = fmaf(w[t], g[t], acc) over the tile's frame band upwards.  The band is an identity: for
|t - c_l| >= 102 the argument is at least 104.03 and expf gives exactly +0.0, so a skipped frame would have added fmaf(+0.0, g, acc).
``MUTANTS`` are that emulation with one fault each; ``CASES`` are the forward's eleven plus the shapes the backward's tiling adds."""
import math

import numpy as np

from tests import gaussian_cpu as gc
from tests.bf16_emu import FP32_REL

PHONEME_TILE = 32     # phonemes per workgroup
CHANNEL_PASS = 128    # channels per workgroup: one 32-channel tile per wave
FRAME_CHUNK = 256     # GB_TC of csrc/gaussgrad.hip: frames staged per LDS chunk
REACH = 102           # GB_REACH: frames past which a weight is exactly +0.0

MUTANTS = ("row_limit_off_by_one", "own_len_ignored", "last_frame_chunk_dropped", "band_of_30_frames", "no_1e-20", "weights_untransposed",
           "last_channel_tile_zero", "centre_without_half")


def limits(own_len, B, T):
    return [T] * B if own_len is None else gc.row_limit(own_len, T)


def band(c_tile, lim, reach=REACH):
    """[t_lo, t_hi) of a tile whose (nondecreasing) fp32 centres are c_tile"""
    t_lo = max(0, int(math.floor(float(c_tile[0]))) - reach)
    t_hi = min(lim, int(math.ceil(float(c_tile[-1]))) + reach + 1)
    return t_lo, max(t_hi, t_lo)


class Reference:
    """d_x [B, L, D] in float64 with bound of the same shape; fwd is the gaussian_cpu.Reference it was made from"""

    def __init__(self, fwd, g, own_len=None):
        g = np.asarray(g)
        assert g.dtype == np.float32 and g.shape[1] == fwd.T and g.shape[0] == fwd.w.shape[0]
        self.fwd, self.T = fwd, fwd.T
        B = g.shape[0]
        self.lim = limits(own_len, B, fwd.T)
        live = (np.arange(fwd.T)[None, :] < np.asarray(self.lim)[:, None]).astype(np.float64)    # [B, T]
        g64 = g.astype(np.float64) * live[:, :, None]
        self.dx = np.einsum("blt,btd->bld", fwd.w, g64)
        self.bound = np.einsum("blt,btd->bld", fwd.bound_w, np.abs(g64)) + FP32_REL * np.einsum("blt,btd->bld", fwd.w, np.abs(g64))


def reference(x, d, g, own_len=None):
    return Reference(gc.Reference(x, d, None), g, own_len)


def share(got, ref):
    """worst |got - d_x| / bound; infinite for a NaN, an error where the bound is zero, or a -0.0 there"""
    got = np.asarray(got)
    zero = ref.bound == 0
    if np.signbit(got[zero]).any():
        return float("inf")
    return gc.share(got, ref.dx, ref.bound)


def emulate(d, g, own_len=None, banded=True, mutate=None, exp_ulp=0):
    """d_x [B, L, D] fp32 in the kernel's order and the weights [B, L, T] it used (+0.0 where it used none)"""
    assert mutate is None or mutate in MUTANTS, mutate
    d, g = np.asarray(d), np.asarray(g)
    B, L = d.shape
    D = g.shape[2]
    fwd_mut = mutate if mutate in ("no_1e-20", "centre_without_half") else None
    _, w, _ = gc.emulate(np.zeros((B, L, 1), np.float32), d, None, exp_ulp=exp_ulp, mutate=fwd_mut)
    c, _ = gc.centres(d)   # the band comes from the true centres: the mutants fault one thing each
    T = w.shape[2]
    lim = limits(None if mutate == "own_len_ignored" else own_len, B, T)
    if mutate == "row_limit_off_by_one":
        lim = [min(n + 1, T) for n in lim]
    if mutate == "weights_untransposed":
        n = min(L, T)
        sq = w[:, :n, :n].transpose(0, 2, 1).copy()
        w = np.zeros_like(w)
        w[:, :n, :n] = sq
    dx = np.zeros((B, L, D), dtype=np.float32)
    used = np.zeros_like(w)
    reach = 30 if mutate == "band_of_30_frames" else REACH
    for b in range(B):
        for l0 in range(0, L, PHONEME_TILE):
            l1 = min(l0 + PHONEME_TILE, L)
            t_lo, t_hi = band(c[b, l0:l1], lim[b], reach) if banded else (0, lim[b])
            if mutate == "last_frame_chunk_dropped" and t_hi > t_lo:
                t_hi = t_lo + (t_hi - t_lo - 1) // FRAME_CHUNK * FRAME_CHUNK
            acc = np.zeros((l1 - l0, D), dtype=np.float32)
            with np.errstate(invalid="ignore"):
                for t in range(t_lo, t_hi):
                    acc = gc._fma(w[b, l0:l1, t][:, None], g[b, t][None, :], acc)
            used[b, l0:l1, t_lo:t_hi] = w[b, l0:l1, t_lo:t_hi]
            dx[b, l0:l1] = acc
    if mutate == "last_channel_tile_zero":
        dx[:, :, (D - 1) // 32 * 32:] = 0.0
    return dx, used


# ---- the cases both tests run ---------------------------------------------------------------------------------------------------------
def _with_g(build, seed):
    def make():
        x, d, own_len = build()
        g = np.random.default_rng(1000 + seed).standard_normal((x.shape[0], gc.frames(d), x.shape[2])).astype(np.float32)
        return x, d, own_len, g
    return make


LONG_PAUSE_L = 40
LONG_PAUSE_ROW = [2, 1, 3, 0, 2] * 6 + [1, 250, 250] + [3, 2, 0, 1, 2, 4, 1]   # phonemes 31 and 32: the centres of tiles 0 and 1 lie 250 apart
assert len(LONG_PAUSE_ROW) == LONG_PAUSE_L

EXTRA = {
    "one_phoneme 2x1x8": gc._case(21, 2, 1, 8, top=9.0),
    "tile_less_one 1x31x36": gc._case(22, 1, 31, 36, top=3.0),
    "tile_plus_one 2x33x36": gc._case(23, 2, 33, 36, top=3.0),
    "four_channels 2x9x4": gc._case(24, 2, 9, 4),
    "two_channel_passes 1x9x132": gc._case(25, 1, 9, 132),
    "long_pause 2x40x8": gc._case(26, 2, LONG_PAUSE_L, 8, top=2.0, rows={0: LONG_PAUSE_ROW}, own_len=lambda T: [T - 5, 40]),
}
CASES = {name: _with_g(build, i) for i, (name, build) in enumerate({**gc.CASES, **EXTRA}.items())}
