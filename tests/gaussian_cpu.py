"""The yardstick of the Gaussian length regulator (csrc/rowops.hip k_gauss_centers / k_gauss_upsample; the reference's
GaussianUpsampling, model/modules.py:166-192): a float64 ``reference`` with an elementwise first-order bound, a numpy-fp32 ``emulate``
in the kernel's own order, ``MUTANTS`` of that emulation with one subtle fault each, and the ``CASES`` the host test
(tests/test_gaussian_host.py) and the GPU test (tests/test_gpu_gaussian_ops.py) share.

Reference, in float64 from the fp32 inputs x [B, L, D] and d [B, L]:

    c_l = cumsum(d)_l - d_l / 2      a_lt = 0.01 (t - c_l)^2      e_lt = exp(-a_lt)      S_t = sum_l e_lt + 1e-20
    w_lt = e_lt / S_t                out_t = sum_l w_lt x_l       t = 0 .. T - 1,  T = ceil(max_b sum_l d_bl)

With ``own_len`` (the form the forwards launch) rows at t >= own_len[b] are zeros; the weights are untouched.

Durations in every case are non-negative multiples of 0.5 with sums below 2^20 (``centres`` asserts it).  The kernel's sequential fp32
cumsum and c_l are then exact, and so is t - c_l (a multiple of 0.25 below 2^20 in magnitude: 22 bits).  What is left to round, with
u = 2^-24 (every fp32 rounding is at most u of its result):

  argument    a' = fl(0.01f * fl(df * df)): two roundings and 0.01f = 0.01 (1 - 0.37 u...): |a' - a| <= 2.4 u a <= Ka u a, Ka = 3.
              e' = expf(-a') = e (1 + eps_l),  |eps_l| <= Ka u a_l + x,  x the relative error of expf itself.
  denominator S' = sum_l e'_l summed as eight strided partial sums, a three-level tree and the + 1e-20f:
              S' = S (1 + sum_l w_l eps_l + sigma),  |sum_l w_l eps_l| <= Ka u abar + x,  abar_t = sum_l w_lt a_lt.
              sigma: a stripe of k terms rounds k - 1 times, each at most u of the stripe's partial sum, so the stripes together
              stay below u S max_k; only the n_sig_t terms above u S_t can round an addition by more than they are worth (a smaller
              one is lost whole, and those are a Gaussian tail far below u S), and consecutive phonemes alternate stripes, so
              max_k ~ n_sig / 8.  The tree adds 3 u, the + 1e-20f one more.
  division    one more u.

  |w' - w| <= w u (Ka (a_lt + abar_t) + Kc + n_sig_t / 8) + FLT_MIN / S_t

Kc = 12 = 2 x + 5 u leaves x = 3.5 u for expf: 1.75 ulp at the bottom of a binade (where an ulp is 2 u of the value), 3.5 ulp at
the top — a 1-ulp expf (OCML's documented accuracy) with room, a 2-ulp one over all but the lowest seventh of the binade.  The last term is one smallest
normal fp32 in e: an expf that flushes a denormal result to zero, or keeps it, is inside the bound either way.  Ka and Kc come from
this count of roundings, not from what a kernel gives; the emulation below stays at or below 0.44 of the weight bound and 0.21
of the output bound over CASES with expf pushed either way (printed by the host test), so neither needed a change.

  |out' - out| <= sum_l bound_w_lt |x_l| + FP32_REL sum_l w_lt |x_l|

the second term being the project's figure for an fp32 contraction (tests/bf16_emu.py) on the fmaf chain over l.
"""
import math

import numpy as np

from tests.bf16_emu import FP32_REL

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
KA, KC = 3.0, 12.0
LDS_CHUNK = 256      # GU_LC of csrc/rowops.hip: phonemes staged per LDS chunk
FRAME_TILE = 32      # frames per workgroup
CHANNEL_PASS = 512   # 16 channel tiles of 32 per pass over the phonemes
PACK_GUARD = 20      # guard rows of a packed window in phase 2

MUTANTS = ("centre_without_half", "centre_exclusive", "no_1e-20", "phoneme_256_dropped", "odd_tail_dropped", "stripe_7_not_in_denominator",
           "one_over_99", "frame_plus_half", "channel_tile_16_zero", "own_len_off_by_one", "no_own_len_zeroing")


def centres(d, mutate=None):
    """(c [B, L], s [B]) by the kernel's sequential fp32 cumsum; asserts the precondition under which both are exact."""
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.ndim == 2
    d64 = d.astype(np.float64)
    assert (d64 >= 0).all() and (d64 * 2 == np.round(d64 * 2)).all() and (d64.sum(axis=1) < 2 ** 20).all(), "durations: multiples of 0.5, sums < 2^20"
    half = np.float32(0.5)
    c = np.empty_like(d)
    acc = np.zeros(d.shape[0], dtype=np.float32)
    for l in range(d.shape[1]):
        before = acc
        acc = acc + d[:, l]
        c[:, l] = acc if mutate == "centre_without_half" else before if mutate == "centre_exclusive" else acc - half * d[:, l]
    if mutate is None:
        cum = np.cumsum(d64, axis=1)
        assert np.array_equal(c.astype(np.float64), cum - d64 / 2) and np.array_equal(acc.astype(np.float64), cum[:, -1]), "fp32 centres are not exact"
    return c, acc


def frames(d):
    return int(math.ceil(float(np.asarray(d, dtype=np.float64).sum(axis=1).max())))


def row_limit(own_len, T):
    """rows [0, limit[b]) of utterance b are live in the forwards' form"""
    return [int(min(max(int(n), 0), T)) for n in own_len]


class Reference:
    """out [B, T, D], w [B, L, T], s [B] in float64 with bound_out and bound_w of the same shapes"""

    def __init__(self, x, d, own_len=None):
        x, d = np.asarray(x), np.asarray(d)
        assert x.dtype == np.float32 and x.shape[:2] == d.shape
        c32, s32 = centres(d)
        B, L, D = x.shape
        self.T = T = frames(d)
        self.s = s32.astype(np.float64)
        c = c32.astype(np.float64)
        t = np.arange(T, dtype=np.float64)
        a = 0.01 * (t[None, None, :] - c[:, :, None]) ** 2
        e = np.exp(-a)
        S = e.sum(axis=1) + 1e-20
        self.w = w = e / S[:, None, :]
        abar = (w * a).sum(axis=1)
        n_sig = (e > U * S[:, None, :]).sum(axis=1)
        self.bound_w = w * U * (KA * (a + abar[:, None, :]) + KC + n_sig[:, None, :] / 8.0) + (FLT_MIN / S)[:, None, :]
        x64 = x.astype(np.float64)
        self.out = np.einsum("blt,bld->btd", w, x64)
        self.bound_out = np.einsum("blt,bld->btd", self.bound_w, np.abs(x64)) + FP32_REL * np.einsum("blt,bld->btd", w, np.abs(x64))
        if own_len is not None:
            for b, lim in enumerate(row_limit(own_len, T)):
                self.out[b, lim:] = 0.0
                self.bound_out[b, lim:] = 0.0


def reference(x, d, own_len=None):
    return Reference(x, d, own_len)


def share(got, ref, bound):
    """worst |got - ref| / bound; an error where the bound is 0, or a NaN, is infinite"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    if np.isnan(err).any():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def shares(out, w, ref):
    """(share of the weight bound, share of the output bound); w may be None (the forwards' form has no weight output)"""
    return (share(w, ref.w, ref.bound_w) if w is not None else 0.0), share(out, ref.out, ref.bound_out)


def _expf(arg, ulp):
    """a correctly rounded fp32 exp of fp32 arguments, pushed by ``ulp`` units in the last place"""
    e = np.exp(arg.astype(np.float64)).astype(np.float32)
    for _ in range(abs(ulp)):
        e = np.nextafter(e, np.float32(np.inf if ulp > 0 else 0.0))
    return e


def _fma(a, b, acc):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def emulate(x, d, own_len=None, exp_ulp=0, denominator="tree", mutate=None):
    """numpy fp32 in the kernel's own order: the eight strided partial sums of pass 1, the ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) tree,
    + 1e-20f, the division, then acc = fmaf(w_l, x_l, acc) over l upwards.  ``denominator="serial"`` sums pass 1 left to right instead;
    ``exp_ulp`` pushes every expf result; ``mutate`` names one deliberate fault (MUTANTS).  Returns (out [B, T, D], w [B, L, T], s [B])."""
    assert mutate is None or mutate in MUTANTS, mutate
    x, d = np.asarray(x), np.asarray(d)
    assert x.dtype == np.float32
    B, L, D = x.shape
    c, s = centres(d, mutate)
    T = frames(d)
    tf = np.arange(T, dtype=np.float32) + (np.float32(0.5) if mutate == "frame_plus_half" else np.float32(0.0))
    k = np.float32(1.0 / 99.0) if mutate == "one_over_99" else np.float32(0.01)
    out = np.zeros((B, T, D), dtype=np.float32)
    w = np.zeros((B, L, T), dtype=np.float32)
    for b in range(B):
        df = tf[None, :] - c[b][:, None]
        e = _expf(-(k * (df * df)), exp_ulp)
        in_den = e.copy()
        if mutate == "stripe_7_not_in_denominator":
            in_den[7::8] = 0.0
        if denominator == "tree":
            p = np.zeros((8, T), dtype=np.float32)
            for l0 in range(0, L, 8):
                n = min(8, L - l0)
                p[:n] = p[:n] + in_den[l0:l0 + n]
            S = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
        else:
            assert denominator == "serial", denominator
            S = np.zeros(T, dtype=np.float32)
            for l in range(L):
                S = S + in_den[l]
        if mutate != "no_1e-20":
            S = S + np.float32(1e-20)
        with np.errstate(divide="ignore", invalid="ignore"):
            wb = e / S[None, :]
        if mutate == "phoneme_256_dropped" and L > LDS_CHUNK:
            wb[LDS_CHUNK] = 0.0
        if mutate == "odd_tail_dropped" and L % 2 == 1:
            wb[L - 1] = 0.0
        w[b] = wb
        acc = np.zeros((T, D), dtype=np.float32)
        with np.errstate(invalid="ignore"):
            for l in range(L):
                acc = _fma(wb[l][:, None], x[b, l][None, :], acc)
        if mutate == "channel_tile_16_zero":
            acc[:, CHANNEL_PASS:CHANNEL_PASS + 32] = 0.0
        if own_len is not None and mutate != "no_own_len_zeroing":
            lim = row_limit(own_len, T)[b]
            acc[lim + (1 if mutate == "own_len_off_by_one" else 0):] = 0.0
        out[b] = acc
    return out, w, s


# ---- the cases both tests run ---------------------------------------------------------------------------------------------------------
LONG_ROW = (3, 140, 140, 2, 0, 0.5, 300, 1, 90, 90.5, 4)   # pauses of 100+ frames: weights above 1e-3 at exponent arguments up to 53


def _durations(rng, B, L, top, frames_of_longest=None):
    """multiples of 0.5 in [0, top]; utterance 0 is stretched through its last phoneme until the batch has ``frames_of_longest`` frames"""
    d = rng.integers(0, int(2 * top) + 1, size=(B, L)).astype(np.float32) * np.float32(0.5)
    if frames_of_longest is not None:
        d[0, -1] = 0
        assert frames(d) <= frames_of_longest, (frames(d), frames_of_longest)
        d[0, -1] = frames_of_longest - float(d[0].sum())
        assert frames(d) == frames_of_longest
    return d


def _case(seed, B, L, D, top=5.5, T=None, rows=None, own_len=None):
    """x ~ N(0, 1) [B, L, D] and d; ``rows`` replaces utterances' durations; ``own_len`` maps T to the forwards' lengths"""
    def build():
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((B, L, D)).astype(np.float32)
        d = _durations(rng, B, L, top, T)
        for b, row in (rows or {}).items():
            d[b] = np.asarray(row, dtype=np.float32)
        return x, d, (None if own_len is None else [int(n) for n in own_len(frames(d))])
    return build


# name -> builder of (x, d, own_len).  Plain form: own_len None.  The last two are the forms the forwards launch (dense grid / packed rows).
CASES = {
    "odd_L_partial_tile 2x7x24": _case(1, 2, 7, 24),
    "lds_chunk_edge 1x256x256": _case(2, 1, 256, 256, top=3.0),
    "padded_odd_tail 1x257x64": _case(3, 1, 257, 64, top=3.0),
    "three_chunks 2x513x32": _case(4, 2, 513, 32, top=3.0),
    "17_channel_tiles 1x9x520": _case(5, 1, 9, 520),
    "long_durations 1x11x32": _case(6, 1, len(LONG_ROW), 32, rows={0: LONG_ROW}),
    "zero_utterance T=128 2x12x24": _case(7, 2, 12, 24, T=128, rows={1: [0] * 12}),      # T a multiple of 32; 1e-20 takes over near t = 70
    "T=32k+1 3x10x40": _case(8, 3, 10, 40, T=97),
    "300_short 1x300x16": _case(9, 1, 300, 16, top=2.0),
    "forwards_dense 5x9x24": _case(10, 5, 9, 24, T=75, own_len=lambda T: [T, 0, T - 33, -1, T + 5]),
    "forwards_packed 5x9x24": _case(11, 5, 9, 24, T=70, own_len=lambda T: [0, 1, T - 7, T, T - 30]),
}
PLAIN = tuple(n for n in CASES if not n.startswith("forwards_"))
