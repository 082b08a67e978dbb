"""float64 restatement of the reference's wave-to-mel function (audio/tools.py:8-15, audio/stft.py:52-81,159-178,
audio/audio_processing.py:85-91) for the tests of the HIP front end: clip, reflect pad, framing, the fp32 bases in float64
arithmetic, magnitude, mel, clamp + log, norm.  Also the hop-row route the GEMM takes, the error gates and the mutants.

GATES (derived here, not fitted): with c = 4e-6, the project's constant for an fp32 sum,
  spectrum   |y - y64| <= g_y = c * A,  A = sum_n |x_n| |w_n| per output (frame, basis row)
  magnitude  g_mag_k = g_re_k + g_im_k + eps32 * mag_k            (|d mag| <= |d re| + |d im|; one ulp for the fp32 square root)
  mel        g_mel_m = sum_k basis[m, k] g_mag_k + c * sum_k basis[m, k] mag_k        (basis >= 0; the band sum is an fp32 sum)
  log mel    g_log = g_mel / max(mel64 - g_mel, clip_val) + 4 eps32 |log64| + 1e-7    (|d log x| <= |dx| / min x on the clamped range;
             a few ulp for logf)
  energy     g_e = sqrt(sum_k g_mag_k^2) + c * e64     (d e = sum mag dmag / e <= ||dmag||_2 by Cauchy-Schwarz; the fp32 sum of squares)
An exactly silent frame has A = 0: its energy gate is 0 and its mel gate is the logf term alone.
"""
import numpy as np

from smart_nar_fast_tts_amd import audio as A

C_SUM = 4e-6
EPS32 = float(np.finfo(np.float32).eps)

LJSPEECH = dict(filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050, mel_fmin=0, mel_fmax=8000)
TINY = dict(filter_length=256, hop_length=32, win_length=192, n_mel_channels=16, sampling_rate=16000, mel_fmin=0, mel_fmax=8000)

MUTANTS = ("zero_pad", "edge_reflect", "symmetric_hann", "window_not_centred", "shift_one_hop", "power", "log10", "clip_1e-10",
           "energy_sum", "no_slaney_norm", "drop_nyquist", "no_clip")


def bases(cfg, mutant=None):
    """(forward_basis [fl + 2, fl] fp32, mel_basis [n_mel, fl / 2 + 1] fp32) of a configuration, or of one of its mutants."""
    fl, win = cfg["filter_length"], cfg["win_length"]
    fb = A.stft_forward_basis(fl, win)[:, 0, :]
    if mutant in ("symmetric_hann", "window_not_centred"):
        four = np.fft.fft(np.eye(fl))
        cut = fl // 2 + 1
        raw = np.vstack([np.real(four[:cut]), np.imag(four[:cut])]).astype(np.float32)
        if mutant == "symmetric_hann":
            w = A.pad_center(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / (win - 1)), fl)
        else:
            w = np.pad(A.hann_periodic(win), (0, fl - win))
        fb = raw * w.astype(np.float32)[None, :]
    mb = A.slaney_mel_basis(cfg["sampling_rate"], fl, cfg["n_mel_channels"], cfg["mel_fmin"], cfg["mel_fmax"], normalize=mutant != "no_slaney_norm")
    return fb, mb


def padded(wave, fl, mutant=None):
    x = np.asarray(wave, dtype=np.float32).astype(np.float64)
    if mutant != "no_clip":
        x = np.clip(x, -1.0, 1.0)
    mode = {"zero_pad": "constant", "edge_reflect": "symmetric"}.get(mutant, "reflect")
    return np.pad(x, (fl // 2, fl // 2), mode=mode)


def frames_of(xp, fl, hop, n, mutant=None):
    T = n // hop + 1
    if mutant == "shift_one_hop":
        xp = np.concatenate([xp[hop:], np.zeros(hop)])
    return np.stack([xp[t * hop:t * hop + fl] for t in range(T)])


def spectrum64(wave, cfg, fb=None, mutant=None):
    """(y64 [T, fl + 2], A [T, fl + 2]) by the framed product."""
    fl, hop = cfg["filter_length"], cfg["hop_length"]
    fb = bases(cfg, mutant)[0] if fb is None else fb
    fr = frames_of(padded(wave, fl, mutant), fl, hop, len(wave), mutant)
    b64 = fb.astype(np.float64)
    return fr @ b64.T, np.abs(fr) @ np.abs(b64).T


def spectrum64_hop_rows(wave, cfg, fb=None):
    """The same spectrum by the route the GEMM takes: the padded wave cut into rows of hop samples, frame t = rows t .. t + KW - 1,
    a Conv1d(Cin = hop, KW = fl / hop, pad 0) whose packed weight row is the basis row."""
    fl, hop = cfg["filter_length"], cfg["hop_length"]
    fb = bases(cfg)[0] if fb is None else fb
    kw, T = fl // hop, len(wave) // hop + 1
    xp = padded(wave, fl)
    rows = np.zeros((T + kw - 1) * hop)
    m = min(len(xp), len(rows))
    rows[:m] = xp[:m]
    R = rows.reshape(T + kw - 1, hop)
    W = fb.astype(np.float64).reshape(fb.shape[0], kw, hop)
    return sum(R[j:j + T] @ W[:, j, :].T for j in range(kw))


def hop_rows(wave, n, fl, hop, S):
    """What k_mel_frame_rows writes for one utterance: [S, hop] fp32 (pure data movement plus the clip)."""
    out = np.zeros(S * hop, np.float32)
    if n > fl // 2:
        xp = np.pad(np.clip(np.asarray(wave[:n], np.float32), -1.0, 1.0), (fl // 2, fl // 2), mode="reflect")
        m = min(len(xp), len(out))
        out[:m] = xp[:m]
    return out.reshape(S, hop)


def packed_columns(y, fl):
    """[T, fl + 2] (real rows over imaginary rows) -> the GEMM's packed [T, fl]: 0 = re_0, 1 = re_{fl/2}, 2k = re_k, 2k + 1 = im_k."""
    cut = fl // 2 + 1
    out = np.empty(y.shape[:-1] + (fl,), y.dtype)
    out[..., 0], out[..., 1] = y[..., 0], y[..., fl // 2]
    out[..., 2::2], out[..., 3::2] = y[..., 1:fl // 2], y[..., cut + 1:cut + fl // 2]
    return out


def project64(y, g_y, mb, clip_val=A.CLIP_VAL, mutant=None):
    """mel [n_mel, T], energy [T] and their gates from a spectrum [T, fl + 2] and its gate."""
    cut = y.shape[1] // 2
    re, im, g_re, g_im = y[:, :cut], y[:, cut:], g_y[:, :cut], g_y[:, cut:]
    mag = np.sqrt(re ** 2 + im ** 2)
    g_mag = g_re + g_im + EPS32 * mag
    if mutant == "power":
        mag = mag ** 2
    if mutant == "drop_nyquist":
        mag = mag.copy()
        mag[:, -1] = 0.0
    b = mb.astype(np.float64)
    mel_lin = mag @ b.T
    g_mel = g_mag @ b.T + C_SUM * mel_lin
    clip = 1e-10 if mutant == "clip_1e-10" else clip_val
    clamped = np.maximum(mel_lin, clip)
    mel = np.log10(clamped) if mutant == "log10" else np.log(clamped)
    g_log = g_mel / np.maximum(mel_lin - g_mel, clip_val) + 4 * EPS32 * np.abs(mel) + 1e-7
    energy = (mag ** 2).sum(1) if mutant == "energy_sum" else np.sqrt((mag ** 2).sum(1))
    g_e = np.sqrt((g_mag ** 2).sum(1)) + C_SUM * energy
    return mel.T, energy, g_log.T, g_e


def reference64(wave, cfg, mutant=None, mb=None):
    """float64 (mel [n_mel, T], energy [T], g_mel, g_energy) of one wave; ``mutant`` swaps in one deliberate mistake."""
    fb, mb0 = bases(cfg, mutant)
    y, Aabs = spectrum64(wave, cfg, fb, mutant)
    return project64(y, C_SUM * Aabs, mb0 if mb is None else mb, mutant=mutant)


def band_form(mb):
    """Per filter (first bin, weights from the first to the last non-zero bin), interior zeros kept: ns_mel_finalize_weights."""
    out = []
    for row in mb:
        nz = np.nonzero(row)[0]
        out.append((0, row[:0]) if len(nz) == 0 else (int(nz[0]), row[nz[0]:nz[-1] + 1]))
    return out


def share(x, x64, gate):
    """max |x - x64| / gate: <= 1 inside the gate.  0 / 0 counts as 0, anything beyond a zero gate as inf; a NaN as inf."""
    d = np.abs(np.asarray(x, np.float64) - x64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(d == 0, 0.0, d / gate)
    s = np.where(np.isnan(s), np.inf, s)
    return float(s.max()) if s.size else 0.0


def shares(mel, energy, ref):
    """{"mel": share, "energy": share} of fp32 results against ``ref = reference64(...)``."""
    mel64, e64, g_mel, g_e = ref
    return {"mel": share(mel, mel64, g_mel), "energy": share(energy, e64, g_e)}


def fixture_waves(cfg, seed):
    """Seeded synthetic waves that give every mutant something to get wrong: chirps plus noise, a stretch of exact silence longer
    than a frame, a stretch of Nyquist tone, and a few samples beyond +-1.  Lengths include one that is no multiple of hop."""
    fl, hop, sr = cfg["filter_length"], cfg["hop_length"], cfg["sampling_rate"]
    rs = np.random.RandomState(seed)
    waves = []
    for i, n in enumerate((7 * fl + 3 * hop, 6 * fl + hop // 2 + 7, 6 * fl + hop - 1)):
        t = np.arange(n) / sr
        f0, f1 = 100.0 * (i + 1), 0.45 * sr
        x = 0.5 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / t[-1] * t ** 2)) + 0.05 * rs.standard_normal(n)
        a = fl + hop * (i + 1)
        x[a:a + fl + 3 * hop] = 0.0                                  # exact silence covering whole frames
        c = a + fl + 4 * hop
        x[c:c + fl] = 0.4 * (-1.0) ** np.arange(fl)                  # Nyquist tone
        x[[3, n // 2, n - 5]] = [1.5, -1.25, 1.75]                    # beyond +-1: the clip matters
        x[:2] += [0.3, -0.2]                                         # the edges differ from their neighbours: reflect vs symmetric
        waves.append(x.astype(np.float32))
    return waves
