"""Float64 numpy restatement of the variance targets and dataset statistics (include/nar_fs2.h ns_vt_*): the tail of the
reference's ``Preprocessor.process_utterance`` and its ``build_from_path`` / ``remove_outlier`` / ``normalize``
(preprocessor/preprocessor.py:188-227, 61-133, 289-310), as a function of a padded batch.

Two forms of the per-phoneme average are carried: ``phoneme_mean`` (every mean over the ORIGINAL frames — what the package computes)
and ``phoneme_mean_inplace`` (the reference's loop, which writes phoneme i's mean into element i of the array it is still reading).
``alias_free`` is the condition under which they agree.  ``MUTANTS`` are deliberately wrong variants the gates must reject.
"""
import numpy as np

LEVELS = ("phoneme_level", "frame_level")
COMBOS = tuple((p, e) for p in LEVELS for e in LEVELS)
MUTANTS = ("segment_off_by_one", "zero_duration_nan", "no_interpolation", "nearest_interpolation", "zero_edge_fill", "no_trim",
           "nonstrict_outlier", "nearest_percentile", "ddof_1", "minmax_filtered", "divide_by_variance", "multiply_by_mask")
SORT_CAPACITY = 8192
U24 = 2.0 ** -24


def combo_key(p_level, e_level):
    return ("pp" if p_level == "phoneme_level" else "pf") + ("ep" if e_level == "phoneme_level" else "ef")


# ---- section 1: targets -------------------------------------------------------------------------------------------------------------
def frame_count(d, Ls, T, mutate=None):
    total = int(np.maximum(d[:Ls], 0).sum())
    return T if mutate == "no_trim" else min(T, total)


def interpolate(p, mutate=None):
    """The contour of preprocessor.py:199-206 on the trimmed float64 pitch ``p`` (at least two voiced frames)."""
    nz = np.where(p != 0)[0]
    if mutate == "no_interpolation":
        return p.copy()
    out = np.empty(len(p), dtype=np.float64)
    first, last = (0.0, 0.0) if mutate == "zero_edge_fill" else (p[nz[0]], p[nz[-1]])
    for t in range(len(p)):
        k = np.searchsorted(nz, t, side="right") - 1  # nz[k] <= t
        if k < 0:
            out[t] = first
        elif nz[k] == t:
            out[t] = p[t]
        elif k + 1 >= len(nz):
            out[t] = last
        else:
            x0, x1 = nz[k], nz[k + 1]
            if mutate == "nearest_interpolation":
                out[t] = p[x0] if t - x0 <= x1 - t else p[x1]
            else:
                slope = (p[x1] - p[x0]) / float(x1 - x0)
                out[t] = slope * float(t - x0) + p[x0]
    return out


def phoneme_mean(x, d, Ls, L, mutate=None):
    """Closed form: phoneme i = mean of x over [c_i - d_i, c_i) within [0, len(x)); 0 where d_i <= 0 or the intersection is empty."""
    out = np.zeros(L, dtype=np.float64)
    pos = 0
    shift = 1 if mutate == "segment_off_by_one" else 0
    for i in range(Ls):
        di = max(int(d[i]), 0)
        if di > 0:
            lo, hi = min(pos + shift, len(x)), min(pos + di + shift, len(x))
            if hi > lo:
                out[i] = np.mean(x[lo:hi])
        elif mutate == "zero_duration_nan":
            out[i] = np.nan
        pos += di
    return out


def phoneme_mean_inplace(x, d):
    """The reference's loop as written (preprocessor.py:208-216): in place, so a phoneme may read means already stored.  Raises
    IndexError once i >= len(x), as the reference does."""
    x = np.array(x, dtype=np.float64)
    pos = 0
    for i, di in enumerate(d):
        di = int(di)
        if di > 0:
            x[i] = np.mean(x[pos:pos + di])
        else:
            x[i] = 0
        pos += di
    return x[:len(d)]


def alias_free(d, Ls):
    """sum_{j<i} d_j >= i for every i with d_i > 0, and sum(d) >= Ls: the in-place loop then reads original frames only."""
    d = np.maximum(np.asarray(d[:Ls], dtype=np.int64), 0)
    before = np.concatenate([[0], np.cumsum(d)[:-1]]) if Ls else np.zeros(0, dtype=np.int64)
    return bool(np.all(before[d > 0] >= np.arange(Ls)[d > 0])) and int(d.sum()) >= Ls


def targets(pitch, energy, durations, src_lens, p_level, e_level, mutate=None):
    """-> dict(pitch [B, T or L] float64, energy, frame_lens [B] int64, valid [B] uint8); padding and invalid utterances are 0."""
    B, T = pitch.shape
    L = durations.shape[1]
    out = {"pitch": np.zeros((B, T if p_level == "frame_level" else L)), "energy": np.zeros((B, T if e_level == "frame_level" else L)),
           "frame_lens": np.zeros(B, dtype=np.int64), "valid": np.zeros(B, dtype=np.uint8)}
    for b in range(B):
        Ls = int(min(max(src_lens[b], 0), L))
        n = frame_count(durations[b], Ls, T, mutate)
        out["frame_lens"][b] = n
        if mutate == "multiply_by_mask":
            keep = (np.arange(T) < n).astype(np.float64)
            p, e = pitch[b].astype(np.float64) * keep, energy[b].astype(np.float64) * keep
        else:
            p, e = pitch[b, :n].astype(np.float64), energy[b, :n].astype(np.float64)
        if np.sum(p != 0) <= 1:
            continue
        out["valid"][b] = 1
        if p_level == "frame_level":
            out["pitch"][b, :len(p)] = p
        else:
            out["pitch"][b] = phoneme_mean(interpolate(p, mutate), durations[b], Ls, L, mutate)
        if e_level == "frame_level":
            out["energy"][b, :len(e)] = e
        else:
            out["energy"][b] = phoneme_mean(e, durations[b], Ls, L, mutate)
    return out


def counts(level, src_lens, frame_lens, valid, L, T):
    n = np.clip(frame_lens, 0, T) if level == "frame_level" else np.clip(src_lens, 0, L)
    return np.where(np.asarray(valid) != 0, n, 0).astype(np.int64)


# ---- section 2: fit -------------------------------------------------------------------------------------------------------------------
def percentile(s, q, mutate=None):
    """numpy's default (linear) percentile on sorted float64 ``s`` at q (n - 1), in numpy's _lerp form."""
    idx = (len(s) - 1) * q
    if mutate == "nearest_percentile":
        return s[int(np.round(idx))]
    lo = int(np.floor(idx))
    hi = min(lo + 1, len(s) - 1)
    g = idx - lo
    diff = s[hi] - s[lo]
    return s[hi] - diff * (1 - g) if g >= 0.5 else s[lo] + diff * g


def outlier_bounds(v, mutate=None):
    s = np.sort(np.asarray(v, dtype=np.float64))
    p25, p75 = percentile(s, 0.25, mutate), percentile(s, 0.75, mutate)
    return p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)


def remove_outlier(v, mutate=None):
    v = np.asarray(v, dtype=np.float64)
    if len(v) == 0:
        return v
    lower, upper = outlier_bounds(v, mutate)
    keep = (v >= lower) & (v <= upper) if mutate == "nonstrict_outlier" else (v > lower) & (v < upper)
    return v[keep]


def bound_margin(v):
    """Smallest relative distance of a value to an outlier bound (the discrete precondition: > 1e-5)."""
    v = np.asarray(v, dtype=np.float64)
    if len(v) < 2:
        return np.inf
    lower, upper = outlier_bounds(v)
    if lower == upper:  # p25 == p75: lower < v < upper keeps nothing whatever the rounding
        return np.inf
    scale = np.maximum(np.abs(v), 1e-30)
    return float(min(np.min(np.abs(v - lower) / scale), np.min(np.abs(v - upper) / scale)))


def check_preconditions(batch, full):
    """The discrete preconditions of one pipeline() result, asserted by the maker and restated by every test that gates on it:
    no value of a fitted utterance lies within relative 1e-5 of an outlier bound (100 x the 2^-24 rounding of a raw value), and no
    ``valid`` decision changes under such a perturbation — ``valid`` counts the frames with pitch != 0, and a relative change of 1e-5
    turns a nonzero fp32 into zero only if it is subnormal, so every nonzero f0 below n_b must be a normal, finite number."""
    for f in ("pitch", "energy"):
        for b in range(len(full["valid"])):
            n = int(full[f]["n"][b])
            m = bound_margin(full[f]["raw32"][b, :n])
            assert m > 1e-5, (f, b, m)
    for b in range(len(full["valid"])):
        p = np.asarray(batch["pitch"][b, :int(full["frame_lens"][b])], dtype=np.float64)
        nz = p[p != 0]
        assert np.all(np.isfinite(nz)) and np.all(np.abs(nz) >= 2.0 ** -126), b


class Running:
    """count / mean / M2 merged utterance by utterance with Chan's update — StandardScaler.partial_fit's arithmetic."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0.0, 0.0, 0.0

    def add(self, kept):
        nb = float(len(kept))
        if nb == 0:
            return
        mb = float(np.sum(kept) / nb)
        m2b = float(np.sum((kept - mb) ** 2))
        delta, tot = mb - self.mean, self.n + nb
        self.mean += delta * (nb / tot)
        self.m2 += m2b + delta * delta * (self.n * nb / tot)
        self.n = tot

    def std(self, mutate=None):
        if self.n == 0:
            return 1.0
        var = self.m2 / (self.n - 1 if mutate == "ddof_1" else self.n)
        s = float(np.sqrt(var))
        return s if s != 0 else 1.0


def fit(raw, n, run=None, mutate=None):
    """``raw`` [B, W] (the fp32 targets as float64, or the float64 ones), ``n`` [B] counts (0 = skipped) -> Running."""
    run = run if run is not None else Running()
    for b in range(raw.shape[0]):
        if n[b] > 0:
            run.add(remove_outlier(raw[b, :n[b]], mutate))
    return run


# ---- section 3: normalise -------------------------------------------------------------------------------------------------------------
def normalize(raw, n, mean, std, mutate=None):
    """-> (float64 normalised [B, W] with padding 0, min, max over ALL selected positions)."""
    y = np.zeros(raw.shape, dtype=np.float64)
    lo, hi = np.finfo(np.float64).max, np.finfo(np.float64).min
    div = std * std if mutate == "divide_by_variance" else std
    for b in range(raw.shape[0]):
        if n[b] <= 0:
            continue
        v = (np.asarray(raw[b, :n[b]], dtype=np.float64) - mean) / div
        y[b, :n[b]] = v
        sel = (remove_outlier(raw[b, :n[b]]) - mean) / div if mutate == "minmax_filtered" else v
        if len(sel):
            lo, hi = min(lo, float(np.min(sel))), max(hi, float(np.max(sel)))
    return y, lo, hi


def pipeline(batch, p_level, e_level, p_norm=True, e_norm=True, mutate=None, only=None):
    """Sections 1-3 over one batch.  The fit and the normalisation see the raw targets ROUNDED to fp32 (what the device holds);
    ``raw64`` keeps the unrounded values.  ``only``: utterance indices to keep (the others are treated as invalid)."""
    pitch, energy, d, sl = batch["pitch"], batch["energy"], batch["durations"], batch["src_lens"]
    T, L = pitch.shape[1], d.shape[1]
    t = targets(pitch, energy, d, sl, p_level, e_level, mutate)
    valid = t["valid"].copy()
    if only is not None:
        valid[[b for b in range(len(valid)) if b not in only]] = 0
    res = {"frame_lens": t["frame_lens"], "valid": t["valid"], "stats": {}}
    for name, level, norm in (("pitch", p_level, p_norm), ("energy", e_level, e_norm)):
        n = counts(level, sl, t["frame_lens"], valid, L, T)
        with np.errstate(invalid="ignore"):
            raw32 = t[name].astype(np.float32).astype(np.float64)
        run = fit(raw32, n, mutate=mutate)
        mean, std = (run.mean, run.std(mutate)) if norm else (0.0, 1.0)
        y, lo, hi = normalize(raw32, n, mean, std, mutate)
        res[name] = {"raw64": t[name], "raw32": raw32, "n": n, "norm": y, "count": run.n, "mean_raw": run.mean, "std_raw": run.std(mutate)}
        res["stats"][name] = [lo, hi, mean, std]
    return res


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"tiny": dict(B=6, L=12, T=40, pad=2), "edges": dict(B=4, L=300, T=1030, pad=3)}


def _durations(rng, Ls, total, zeros=()):
    """Ls non-negative integers summing to ``total``, zero at the indices in ``zeros``, every other one >= 1."""
    live = [i for i in range(Ls) if i not in set(zeros)]
    assert total >= len(live)
    cuts = np.sort(rng.choice(np.arange(1, total), size=len(live) - 1, replace=False)) if len(live) > 1 else np.zeros(0, dtype=np.int64)
    parts = np.diff(np.concatenate([[0], cuts, [total]]))
    d = np.zeros(Ls, dtype=np.int64)
    d[live] = parts
    return d


def _contour(rng, T, unvoiced):
    t = np.arange(T)
    f0 = 180.0 + 60.0 * np.sin(t / 17.0 + rng.uniform(0, 6)) + rng.normal(0, 6.0, T)
    spikes = rng.choice(T, size=max(1, T // 40), replace=False)
    f0[spikes] *= 2.6  # octave errors: the outliers remove_outlier exists for
    for lo, hi in unvoiced:
        f0[lo:hi] = 0.0
    return f0.astype(np.float32)


def _energy(rng, T):
    e = np.abs(rng.normal(30.0, 12.0, T)) + 0.5
    e[rng.choice(T, size=max(1, T // 50), replace=False)] *= 4.0
    return e.astype(np.float32)


def fixture_batch(cfg, seed):
    """Seeded batch of one of CONFIGS: dict(pitch [B, T] f32, energy [B, T] f32, durations [B, L + pad] int64 — read through
    ``[:, :L]`` so the row stride exceeds L —, src_lens [B] int64, replica = (i, j) or None).  Positions behind the masks hold
    ordinary finite numbers; tests overwrite them with NaN."""
    c = CONFIGS[cfg]
    B, L, T, pad = c["B"], c["L"], c["T"], c["pad"]
    rng = np.random.RandomState(seed)
    pitch, energy = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    dur = rng.randint(1, 9, size=(B, L + pad)).astype(np.int64)  # junk behind src_lens and behind L
    src_lens = np.zeros(B, np.int64)

    def put(b, d, unvoiced, voiced_only=None):
        src_lens[b] = len(d)
        dur[b, :len(d)] = d
        pitch[b] = _contour(rng, T, unvoiced)
        if voiced_only is not None:
            keep = np.zeros(T, bool)
            keep[list(voiced_only)] = True
            pitch[b, ~keep] = 0.0
        energy[b] = _energy(rng, T)

    replica = None
    if cfg == "tiny":
        put(0, _durations(rng, 12, 38), [(0, 4), (15, 21), (33, 40)])          # unvoiced runs at the start, in the middle, at the end
        put(1, _durations(rng, 9, 31), [(11, 14)])
        put(2, _durations(rng, 12, 40, zeros=(5, 9, 11)), [(0, 2), (20, 23)])  # zero durations once the prefix is ahead; sum(d) == T
        put(3, _durations(rng, 12, 36), [], voiced_only=(7, 22))               # exactly two voiced frames: still valid
        put(4, _durations(rng, 5, 17), [(8, 10)])
        put(5, _durations(rng, 12, 29), [(25, 29)])
    elif cfg == "edges":
        # 0: zero durations at the start (aliasing), in the middle and at the end; sum(d) == T; phoneme 60 straddles frame 256;
        #    the unvoiced run 500-530 straddles frame 512
        zeros = (0, 1, 2, 3, 150, 151, 152, 297, 298, 299)
        d = _durations(rng, 300, 1030, zeros=zeros)
        c0 = np.cumsum(d)
        i = int(np.searchsorted(c0, 256, side="right"))
        if 256 - (c0[i] - d[i]) < 4 or c0[i] - 256 < 4:  # make the phoneme that holds frame 256 reach well to both sides of it
            for k, side in ((6, range(i - 1, -1, -1)), (6, range(i + 1, 300))):
                j = next(j for j in side if d[j] > k + 1)
                d[j] -= k
                d[i] += k
        put(0, d, [(0, 6), (500, 530), (1010, 1030)])
        dur[1], pitch[1], energy[1], src_lens[1] = dur[0], pitch[0], energy[0], src_lens[0]  # 1: the replica of 0
        replica = (0, 1)
        put(2, _durations(rng, 211, 777, zeros=(100, 101, 210)), [(250, 262), (700, 777)])    # src_lens < L, sum(d) < T, alias-free
        put(3, _durations(rng, 257, 900), [], voiced_only=(400,))                             # one voiced frame: invalid
    else:
        raise KeyError(cfg)
    return {"pitch": pitch, "energy": energy, "durations_padded": dur, "durations": dur[:, :L], "src_lens": src_lens, "replica": replica}


def poison(batch, frame_lens):
    """NaN behind every mask of every input: frames >= n_b, durations at i >= src_lens (int64 has no NaN: a huge negative and a huge
    positive number alternate) and in the stride padding."""
    p, e, d = batch["pitch"].copy(), batch["energy"].copy(), batch["durations_padded"].copy()
    L = batch["durations"].shape[1]
    for b in range(p.shape[0]):
        p[b, frame_lens[b]:] = np.nan
        e[b, frame_lens[b]:] = np.nan
        junk = np.where(np.arange(d.shape[1]) % 2 == 0, -(1 << 62), (1 << 62))
        d[b, batch["src_lens"][b]:] = junk[batch["src_lens"][b]:]
    return dict(batch, pitch=p, energy=e, durations_padded=d, durations=d[:, :L])


# ---- gates (all derived) ----------------------------------------------------------------------------------------------------------------
def ulp32(y64):
    """The spacing of fp32 at |y64| (2^-149 at 0), per element of an array: not tests/util.py's ulp32, which takes one scalar."""
    a = np.abs(np.asarray(y64, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)).astype(np.float64) - a.astype(np.float64))


def raw_gate_ok(y32, y64):
    """|y - fl32(y64)| <= 1 ulp_fp32(y64): float64 accumulation, one rounding."""
    y64 = np.asarray(y64, dtype=np.float64)
    return np.abs(np.asarray(y32, dtype=np.float64) - y64.astype(np.float32).astype(np.float64)) <= ulp32(y64)


def norm_gate(x, mean, std):
    """2^-23 (|x| + |mean|) / std: the rounding of the quotient to fp32 plus a half-ulp difference of the raw value."""
    return 2.0 ** -23 * (np.abs(x) + abs(mean)) / std


def extrema_gates(c, mean, std):
    """The normalised-value gate at the two extrema: x is the raw fp32 value at the argmin / argmax of the float64 normalised values
    ``c["norm"]`` over the selected positions (``c`` = one feature of pipeline()).  -> (gate of the min, gate of the max)."""
    sel = np.arange(c["norm"].shape[1])[None, :] < c["n"][:, None]
    if not sel.any():
        return 0.0, 0.0
    y, x = c["norm"][sel], c["raw32"][sel]
    return float(norm_gate(x[np.argmin(y)], mean, std)), float(norm_gate(x[np.argmax(y)], mean, std))
