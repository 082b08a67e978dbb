"""The validation loss stated independently in torch on the CPU (model/loss.py:149-250): every part is a closed-form masked sum
over a count — ``where(mask, term, 0).sum() / mask.sum()`` — not a ``masked_select``; fp32 or float64.  Also: the gate of the
loss tests, seeded random tuples, the NaN poisoning of everything a mask hides, and the deliberately wrong variants the gate must
reject.

The guided-attention weights W are fp32 at every dtype, as in the reference (``.float()`` grids, model/loss.py:104-108); the
products W * p and all sums are in ``dtype``."""
import numpy as np
import torch

NAMES = ("total", "mel", "postnet", "pitch", "energy", "duration", "attn")
SIGMA, ALPHA = 0.2, 10.0  # model/loss.py:19
C_SUM, C_ATTN = 4e-6, 1e-5  # the gate's constants: the project's fp32-sum constant; 4 ulp on an exp argument that reaches -12.5

MUTANTS = ("mask_off_by_one", "log_without_plus_one", "head_1", "layer_3_four_times", "sigma_0.4", "alpha_dropped", "mean_over_BTL",
           "olen_is_T", "l2_for_l1", "multiply_by_mask")


def _clamped(lens, hi, device="cpu"):
    lens = lens if torch.is_tensor(lens) else torch.as_tensor(np.asarray(lens))
    return lens.to(device).long().clamp(0, hi)


def _parts(inputs, predictions, pitch_level, energy_level, dtype, mutate=None, olen_from_slot9=False):
    """Per part: (sum of the selected terms, count, sum of the selected term MAGNITUDES), all in ``dtype``."""
    src_lens, _, mel_targets, mel_lens, _, p_tgt, e_tgt = inputs[4:11]
    mel, post, p_pred, e_pred, log_d, _, src_masks, mel_masks, _, slot9, attn, d_tgt = predictions
    B, T, n_mel = mel.shape
    L = log_d.shape[1]
    dev = mel.device  # (the CPU in every test; tools/loss_bench.py times the same statement on the GPU)
    ar = lambda n: torch.arange(n, device=dev)  # noqa: E731
    f = lambda t: torch.as_tensor(t).to(dtype)  # noqa: E731
    keep_t, keep_l = ~torch.as_tensor(mel_masks), ~torch.as_tensor(src_masks)  # model/loss.py:188-189
    ilen = _clamped(src_lens, L, dev)
    olen = _clamped(slot9 if olen_from_slot9 else mel_lens, T, dev)
    if mutate == "olen_is_T":
        olen = torch.full_like(olen, T)
    if mutate == "mask_off_by_one":
        keep_t = ar(T)[None] <= (T - torch.as_tensor(mel_masks).sum(1))[:, None]
        keep_l = ar(L)[None] <= ilen[:, None]
        ilen, olen = (ilen + 1).clamp(max=L), (olen + 1).clamp(max=T)
    zero = torch.zeros((), dtype=dtype, device=dev)

    def masked(term, mag, keep):
        if mutate == "multiply_by_mask":
            return (term * keep).sum(), keep.sum() * (term.numel() // keep.numel()), (mag * keep).sum()
        k = keep.expand_as(term)
        return torch.where(k, term, zero).sum(), k.sum(), torch.where(k, mag, zero).sum()

    out = {}
    tgt = f(mel_targets)[:, :T]  # model/loss.py:191
    for name, x in (("mel", f(mel)), ("postnet", f(post))):
        err = (x - tgt) ** 2 if mutate == "l2_for_l1" else (x - tgt).abs()
        out[name] = masked(err, x.abs() + tgt.abs(), keep_t[:, :, None])
    for name, x, y, level in (("pitch", f(p_pred), f(p_tgt), pitch_level), ("energy", f(e_pred), f(e_tgt), energy_level)):
        out[name] = masked((x - y) ** 2, (x.abs() + y.abs()) ** 2, keep_t if level == "frame_level" else keep_l)
    d = torch.as_tensor(d_tgt)[:, :L].float()  # model/loss.py:190,214-216: .float() at every dtype
    log_t = torch.log(d if mutate == "log_without_plus_one" else d + 1).to(dtype)
    out["duration"] = masked((f(log_d) - log_t) ** 2, (f(log_d).abs() + log_t.abs()) ** 2, keep_l)
    # guided attention (model/loss.py:60-65,104-108,144-146,233-236)
    sigma = 0.4 if mutate == "sigma_0.4" else SIGMA
    gx = ar(T).float()[None, :, None] / olen.float()[:, None, None]
    gy = ar(L).float()[None, None, :] / ilen.float()[:, None, None]
    W = 1.0 - torch.exp(-((gy - gx) ** 2) / (2 * (sigma ** 2)))
    region = (ar(T)[None, :, None] < olen[:, None, None]) & (ar(L)[None, None, :] < ilen[:, None, None])
    s = m = zero
    for k in range(4):
        p = f(attn[3 if mutate == "layer_3_four_times" else k])[:, 1 if mutate == "head_1" else 0]
        if mutate == "multiply_by_mask":
            s, m = s + (W.to(dtype) * p * region).sum(), m + (p * region).sum()
        else:
            s, m = s + torch.where(region, W.to(dtype) * p, zero).sum(), m + torch.where(region, p, zero).sum()
    n = torch.tensor(B * T * L, device=dev) if mutate == "mean_over_BTL" else region.sum()
    alpha = 1.0 if mutate == "alpha_dropped" else ALPHA
    out["attn"] = (alpha * s, n, ALPHA * m)
    return out


def loss(inputs, predictions, pitch_level, energy_level, dtype=torch.float64, mutate=None, olen_from_slot9=False):
    """The seven values in the reference's order as a numpy array of ``dtype`` (NaN for an empty selection: 0 / 0)."""
    parts = _parts(inputs, predictions, pitch_level, energy_level, dtype, mutate, olen_from_slot9)
    v = {k: s / n.to(dtype) for k, (s, n, _) in parts.items()}
    total = v["mel"] + v["postnet"] + v["duration"] + v["pitch"] + v["energy"] + v["attn"]  # model/loss.py:238-240
    return np.array([float(x) for x in (total, v["mel"], v["postnet"], v["pitch"], v["energy"], v["duration"], v["attn"])],
                    dtype=np.float64 if dtype == torch.float64 else np.float32)


def gates(inputs, predictions, pitch_level, energy_level):
    """|x - x_f64| <= c * M per part, M the float64 mean over the part's selection of the term's magnitude: |a| + |b| for the two L1
    losses, (|a| + |b|)^2 for the three MSEs (b = log(d + 1) for the duration), alpha * sum_k p for the attention term; c = 4e-6,
    for attention 1e-5.  The total's gate is the sum of the six.  Returns the seven gates in the reference's order."""
    parts = _parts(inputs, predictions, pitch_level, energy_level, torch.float64)
    g = {k: float((C_ATTN if k == "attn" else C_SUM) * m / n.double()) for k, (_, n, m) in parts.items()}
    six = [g[k] for k in NAMES[1:]]
    return np.array([sum(six)] + six)


def shares(got, want, gate):
    """|got - want| / gate per value; a NaN on either side where the other is finite counts as infinitely far, NaN on both sides
    (an empty selection on both) as 0."""
    got, want, gate = (np.asarray(a, dtype=np.float64) for a in (got, want, gate))
    out = np.abs(got - want) / gate
    both = np.isnan(got) & np.isnan(want)
    out[both] = 0.0
    out[np.isnan(out) | np.isinf(got) | np.isinf(want)] = np.inf
    return out


def random_case(B, L, T, H, pitch_level="frame_level", energy_level="frame_level", seed=0, src_lens=None, mel_lens=None,
                extra_frames=0, extra_columns=0, n_mel=80):
    """A seeded tuple pair shaped like ``forward_teacher_forced()``'s: ragged lengths, softmax-normalised attention with exact zeros at
    padded keys and NaN rows for an utterance with src_lens == 0, slot 9 = the input mel_lens except 0 where src_lens == 0 (the
    durations' row sums), slot 7 built from slot 9.  ``mel_targets`` may carry ``extra_frames`` more frames and
    ``d_targets`` ``extra_columns`` more columns than the predictions (model/loss.py:191,214-216)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if src_lens is None:
        src_lens = [L] + [int(v) for v in torch.randint(1, L + 1, (B - 1,), generator=g)]
    if mel_lens is None:
        mel_lens = [T] + [int(v) for v in torch.randint(1, T + 1, (B - 1,), generator=g)]
    sl, ml = torch.tensor(src_lens, dtype=torch.long), torch.tensor(mel_lens, dtype=torch.long)
    slot9 = torch.where(sl > 0, ml, torch.zeros_like(ml))
    src_masks = torch.arange(L)[None] >= sl[:, None]
    mel_masks = torch.arange(T)[None] >= slot9[:, None]
    attn = []
    for _ in range(4):
        s = rnd(B, H, T, L) * 2.0
        attn.append(torch.softmax(s.masked_fill(src_masks[:, None, None, :], -np.inf), dim=-1))
    p_shape = (B, T) if pitch_level == "frame_level" else (B, L)
    e_shape = (B, T) if energy_level == "frame_level" else (B, L)
    d = torch.randint(0, 12, (B, L + extra_columns), generator=g) * (torch.arange(L + extra_columns)[None] < sl[:, None])
    mel_targets = rnd(B, T + extra_frames, n_mel) * 2.0 - 3.0
    predictions = (mel_targets[:, :T] + 0.3 * rnd(B, T, n_mel), mel_targets[:, :T] + 0.2 * rnd(B, T, n_mel), rnd(*p_shape), rnd(*e_shape),
                   rnd(B, L) + 1.5, d, src_masks, mel_masks, sl, slot9, attn, d)
    inputs = (None, None, None, None, sl, L, mel_targets, ml, T, rnd(*p_shape) * 1.5, rnd(*e_shape) * 1.5)
    return inputs, predictions


def poison(inputs, predictions, pitch_level, energy_level):
    """The same tuples with NaN in every position of every float tensor that a mask hides: padded frames and phonemes, t >= olen and
    l >= ilen of head 0, all of heads >= 1, the target frames and duration columns the reference slices away."""
    src_lens, _, mel_targets, mel_lens, _, p_tgt, e_tgt = inputs[4:11]
    mel, post, p_pred, e_pred, log_d, _, src_masks, mel_masks, _, slot9, attn, d_tgt = predictions
    B, T, _ = mel.shape
    L = log_d.shape[1]
    nan = float("nan")
    rows = lambda x, pad: x.masked_fill(pad[:, :, None] if x.dim() == 3 else pad, nan)  # noqa: E731
    tgt = mel_targets.clone()
    tgt[:, T:] = nan
    tgt[:, :T] = rows(tgt[:, :T], mel_masks)
    by = lambda level: mel_masks if level == "frame_level" else src_masks  # noqa: E731
    region = (torch.arange(T)[None, :, None] < _clamped(mel_lens, T)[:, None, None]) & (torch.arange(L)[None, None, :] < _clamped(src_lens, L)[:, None, None])
    maps = []
    for a in attn:
        a = a.clone()
        a[:, 1:] = nan
        a[:, 0] = a[:, 0].masked_fill(~region, nan)
        maps.append(a)
    predictions = (rows(mel, mel_masks), rows(post, mel_masks), rows(p_pred, by(pitch_level)), rows(e_pred, by(energy_level)),
                   rows(log_d, src_masks), d_tgt, src_masks, mel_masks, predictions[8], slot9, maps, d_tgt)
    inputs = tuple(inputs[:6]) + (tgt, mel_lens, inputs[8], rows(p_tgt, by(pitch_level)), rows(e_tgt, by(energy_level)))
    return inputs, predictions


def fixture_case(z, meta, suffix=""):
    """The stored tuple of a teacher_* fixture (tests/golden/make_golden_teacher.py) as the loss's two arguments; ``suffix`` "_f64"
    selects the float64 evaluation's arrays."""
    t = lambda k: torch.from_numpy(np.asarray(z[k]))  # noqa: E731
    dt = torch.float64 if suffix else torch.float32
    inputs = (None, None, None, None, t("src_lens"), meta["L"], t("mels").to(dt), t("mel_lens"), meta["T"], t("p_targets").to(dt), t("e_targets").to(dt))
    attn = [t(f"attn{i}{suffix}") for i in range(meta["n_layer"])]
    predictions = (t("output" + suffix), t("postnet_output" + suffix), t("p_predictions" + suffix), t("e_predictions" + suffix),
                   t("log_d_predictions" + suffix), t("d_targets"), t("src_masks"), t("mel_masks"), t("src_lens"), t("out_mel_lens"), attn,
                   t("d_targets"))
    return inputs, predictions


# (B, L, T, H) of the seeded random cases, each run at both feature levels (tests/test_loss_host.py, tests/test_gpu_loss.py)
CASES = {
    "smallest": dict(B=1, L=1, T=1, H=2),
    "unaligned_prime_T_empty_utterances": dict(B=3, L=37, T=131, H=2, src_lens=[37, 0, 20], mel_lens=[131, 90, 0]),
    "exact_tiles": dict(B=2, L=64, T=256, H=2),
    "L_past_two_strips_H4_longer_targets": dict(B=5, L=130, T=70, H=4, extra_frames=6, extra_columns=3),
    "many_slots": dict(B=4, L=96, T=1500, H=2),
}
LEVELS = ("frame_level", "phoneme_level")
_CASE_CACHE = {}


def case(name, level):
    """One of CASES at one feature level with its float64 values and gates, computed once and shared (never modified)."""
    key = (name, level)
    if key not in _CASE_CACHE:
        inputs, predictions = random_case(pitch_level=level, energy_level=level, seed=1 + 2 * list(CASES).index(name) + LEVELS.index(level), **CASES[name])
        _CASE_CACHE[key] = (inputs, predictions, loss(inputs, predictions, level, level), gates(inputs, predictions, level, level))
    return _CASE_CACHE[key]
