"""The yardstick of the dropout keep-mask generator (csrc/keepmask.hip, ns_km_*), numpy only, written from the
definition in include/nar_fs2.h and not from the kernel:

    block j of a mask = Philox4x32-10 at counter (j, stream, call & 0xffffffff, call >> 32) under key (seed & 0xffffffff, seed >> 32)
    element e          = word e & 3 of block e >> 2;  keep = word < thr;  thr = floor((1.0 - p) * 2^32) in float64
    arena              = the slots back to back, each starting at a multiple of 16 bytes and ceil(n / 16) * 16 bytes long, the bytes
                         behind element n - 1 written as 0, nothing else written

``MUTANTS`` are the mistakes an implementation can make without failing to run; ``CATCHER`` names, for each, the case of ``CASES`` on
which it differs from the definition (tests/test_keepmask_host.py proves that on the CPU; the GPU test runs the same cases)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
CANARY = 0xA5
MUTANTS = ("rounds_9", "key_not_bumped", "le_not_lt", "words_reversed", "stream_ignored", "call_hi_ignored", "tail_unwritten")

# (counter, key, output) — the first and the third are the Random123 known answers
KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
         ((0, 0, 1, 0), (1234, 0), (0xd115a128, 0x52fc7c75, 0xc7f33f17, 0x0f1539db)))
THRESHOLDS = ((0.1, 3865470566), (0.2, 3435973836), (0.5, 2147483648))
FIRST_32 = (0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1)  # seed 1234, call 1, stream 0, p 0.2
PS = (0.1, 0.2, 0.5)
SINGLE_N = (1, 15, 16, 17, 4095, 4096, 4097, 2 * 7 * 256, 2 * 20 * 80)


def philox(c0, c1, c2, c3, k0, k1, rounds=10, bump=True):
    """Philox4x32 on arrays (or scalars) of 32-bit words: four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    for _ in range(rounds):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        if bump:
            k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """floor((1.0 - p) * 2^32) from the Python float p, in float64; raises where ns_km_threshold refuses"""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError("p must lie in (0, 1)")
    t = int(np.floor((1.0 - p) * 4294967296.0))
    if t < 1 or t > MASK32:
        raise ValueError("the threshold must lie in [1, 2^32)")
    return t


def words(seed, call, stream, n, mutate=None):
    """the n 32-bit words of a mask's elements, uint32 [n]"""
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    call_hi = 0 if mutate == "call_hi_ignored" else (call >> 32) & MASK32
    w = philox(j, 0 if mutate == "stream_ignored" else stream, call & MASK32, call_hi, seed & MASK32, (seed >> 32) & MASK32,
               rounds=9 if mutate == "rounds_9" else 10, bump=mutate != "key_not_bumped")
    if mutate == "words_reversed":
        w = w[::-1]
    return np.stack(w, axis=1).reshape(-1)[:n]


def mask(seed, call, stream, n, thr, mutate=None):
    """the keep-mask, uint8 [n]"""
    w = words(seed, call, stream, n, mutate)
    return (w <= np.uint32(thr) if mutate == "le_not_lt" else w < np.uint32(thr)).astype(np.uint8)


def layout(ns):
    """(byte offsets, arena bytes) of masks of ``ns`` elements in the order given"""
    offs, off = [], 0
    for n in ns:
        offs.append(off)
        off += (n + 15) // 16 * 16
    return offs, off


def arena(masks, seed, call, mutate=None, slack=0):
    """The arena of ``masks`` = [(n, stream, thr)] drawn into a buffer of CANARY bytes, ``slack`` bytes longer than the plan's: uint8"""
    offs, total = layout([m[0] for m in masks])
    a = np.full(total + slack, CANARY, dtype=np.uint8)
    for off, (n, stream, thr) in zip(offs, masks):
        a[off:off + n] = mask(seed, call, stream, n, thr, mutate)
        if mutate != "tail_unwritten":
            a[off + n:off + (n + 15) // 16 * 16] = 0
    return a


def word_of(seed, call, stream, e):
    return int(words(seed, call, stream, e + 1)[e])


def _cases():
    cases = {}
    for p in PS:
        for n in SINGLE_N:
            cases[f"single_n{n}_p{p}"] = dict(seed=1234, call=1, masks=[(n, 0, threshold(p))])
    cases["mixed"] = dict(seed=77, call=3, masks=[(n, 5 + i, threshold(PS[i % 3])) for i, n in enumerate((3584, 1, 4097, 16, 3200, 8200, 15))])
    cases["wide_state"] = dict(seed=(1 << 63) + 5, call=(1 << 32) + 7, masks=[(4099, MASK32 - 1, threshold(0.2)), (33, MASK32, threshold(0.5))])
    cases["call_2_pow_32"] = dict(seed=1234, call=1 << 32, masks=[(64, 0, threshold(0.5))])  # the low word of call is 0: only the high word tells it from call 0
    # a threshold that IS one of the mask's words: the only place where < and <= differ
    cases["thr_is_a_word"] = dict(seed=9, call=2, masks=[(40, 1, word_of(9, 2, 1, 21))])
    return cases


CASES = _cases()
CATCHER = {"rounds_9": "single_n16_p0.5", "key_not_bumped": "single_n16_p0.5", "le_not_lt": "thr_is_a_word", "words_reversed": "single_n16_p0.5",
           "stream_ignored": "mixed", "call_hi_ignored": "call_2_pow_32", "tail_unwritten": "single_n17_p0.2"}


def case_arena(name, mutate=None, slack=0):
    c = CASES[name]
    return arena(c["masks"], c["seed"], c["call"], mutate, slack)
