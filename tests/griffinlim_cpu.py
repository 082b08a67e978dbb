"""float64 restatement of the reference's mel-to-wave path (audio/tools.py:18-29, audio/audio_processing.py:7-82, audio/stft.py:52-122)
for the tests of the HIP Griffin-Lim: every operator, one iteration, the loop; the error gates; the mutants.  Spectra are held in the
reference's FULL layout [T, filter_length + 2] (real columns, then imaginary ones); melfront_cpu.packed_columns gives the device's.
Every function works per utterance on time-major arrays and takes ``dt`` (float64, or float32 for the numpy fp32 restatement whose
spectral convergence sets the 60-iteration allowance).

GATES (derived, not fitted; the linear-propagation convention of tests/melfront_cpu.py, c = 4e-6 per fp32 sum, eps32 per rounding):
  mel_to_mag g_mag = scaling * ((4 eps32 e) @ mel_basis) + (c + 2 eps32) mag      expf within a few ulp; the n_mel-term fp32 sum; the product
  recombine  g_X = 4 eps32 mag                                                    cosf / sinf within a few ulp on [-pi, pi], one product
  spectrum   g_Y = g_x-frames @ |fb| + c * sum |x| |fb|                           melfront_cpu's gate plus the input signal's own gate
  rephase    d = min(2, (g_re + g_im) / max(|Y| - g_re - g_im, tiny)) + 4 eps32;  g_X = mag d on both components
             (a unit vector moves by at most |dY| / (|Y| - |dY|), and never by more than 2; exact input: d = 4 eps32)
  inverse    g_frames = g_X @ |ib| + c * |X| @ |ib|;  g_y = scale * overlap-add(g_frames) / window_sum + 4 eps32 |y|
             (the overlap-add has at most filter_length / hop terms: its own rounding is inside the 4 eps32 |y| only where the terms do
             not cancel, so c * overlap-add(|frames|) is added as well)
A gate of one step feeds the next step's spectrum gate, so the loop's gate grows with every iteration; it is loose (the fp32 error
is about 1e-3 of it) but every O(1) mistake leaves it.
"""
import numpy as np

import melfront_cpu as mc
from smart_nar_fast_tts_amd import audio as A

C_SUM, EPS32 = mc.C_SUM, mc.EPS32
TINY32 = float(np.finfo(np.float32).tiny)
LJSPEECH, TINY = mc.LJSPEECH, mc.TINY
SCALING = 1000.0

MEL_MUTANTS = ("last_frame_kept", "scaling_1", "pinv_mel")
INVERSE_MUTANTS = ("no_wsum_div", "wsum_after_trim", "wsum_symmetric_hann", "no_scale", "ib_not_windowed", "dc_nyquist_2N", "sine_sign")
STEP_MUTANTS = ("zero_pad", "clip_in_loop")
REPHASE_MUTANTS = ("rephase_zero_at_zero",)
LOOP_MUTANTS = ("stale_phase",)
MUTANTS = MEL_MUTANTS + INVERSE_MUTANTS + STEP_MUTANTS + REPHASE_MUTANTS + LOOP_MUTANTS


def dims(cfg):
    return cfg["filter_length"], cfg["hop_length"], cfg["win_length"]


def bases(cfg, mutant=None):
    """(forward_basis [fl + 2, fl], inverse_basis [fl + 2, fl]) fp32"""
    fl, hop, win = dims(cfg)
    fb = A.stft_forward_basis(fl, win)[:, 0, :]
    ib = A.stft_inverse_basis(fl, hop, win)[:, 0, :]
    if mutant in ("ib_not_windowed", "dc_nyquist_2N", "sine_sign"):
        four = np.fft.fft(np.eye(fl))
        cut = fl // 2 + 1
        w = np.full(cut, 2.0 / fl)
        if mutant != "dc_nyquist_2N":
            w[0] = w[fl // 2] = 1.0 / fl
        sgn = -1.0 if mutant == "sine_sign" else 1.0
        raw = (np.vstack([four[:cut].real * w[:, None], sgn * four[:cut].imag * w[:, None]]) / (fl / hop)).astype(np.float32)
        window = np.ones(fl, np.float32) if mutant == "ib_not_windowed" else A.pad_center(A.hann_periodic(win), fl).astype(np.float32)
        ib = raw * window[None, :]
    return fb, ib


def mel_to_mag(mel, mb, mutant=None, dt=np.float64):
    """mel [T, n_mel] log-mel -> (mag [T - 1, bins], gate)"""
    e = np.exp(np.asarray(mel, np.float32).astype(dt))
    if mutant != "last_frame_kept":
        e = e[:-1]
    b = np.linalg.pinv(mb.astype(np.float64)).T.astype(dt) if mutant == "pinv_mel" else mb.astype(dt)
    s = dt(1.0 if mutant == "scaling_1" else SCALING)
    mag = (e @ b) * s
    gate = SCALING * ((4 * EPS32 * e) @ np.abs(b)) + (C_SUM + 2 * EPS32) * np.abs(mag)
    return mag, gate


def recombine(mag, ang, dt=np.float64):
    """(X [T, fl + 2] full layout, gate)"""
    mag, ang = np.asarray(mag).astype(dt), np.asarray(ang, np.float32).astype(dt)
    X = np.concatenate([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    g = 4 * EPS32 * np.abs(mag)
    return X, np.concatenate([g, g], axis=1)


def window_sum(T, cfg, mutant=None):
    fl, hop, win = dims(cfg)
    if mutant == "wsum_symmetric_hann":
        n = fl + hop * (T - 1)
        x = np.zeros(n, np.float32)
        wsq = A.pad_center((0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / (win - 1))) ** 2, fl)
        for i in range(T):
            x[i * hop:i * hop + fl] += wsq
        return x
    return A.window_sumsquare(T, hop, win, fl)


def overlap_add(frames, hop):
    T, fl = frames.shape
    out = np.zeros(fl + hop * (T - 1), frames.dtype)
    for t in range(T):
        out[t * hop:t * hop + fl] += frames[t]
    return out


def inverse(X, gX, cfg, mutant=None, dt=np.float64, ib=None):
    """X [T, fl + 2] -> (wave [hop (T - 1)], gate): stft.py:88-120"""
    fl, hop, win = dims(cfg)
    ib = (bases(cfg, mutant)[1] if ib is None else ib).astype(dt)
    X = X.astype(dt)
    T = X.shape[0]
    frames = X @ ib
    y = overlap_add(frames, hop)
    g = overlap_add(gX @ np.abs(ib) + C_SUM * (np.abs(X) @ np.abs(ib)), hop) + C_SUM * overlap_add(np.abs(frames), hop)
    ws = window_sum(T, cfg, mutant).astype(dt)
    if mutant == "wsum_after_trim":
        ws = np.concatenate([ws[fl // 2:], np.zeros(fl // 2, dt)])
    nz = ws > TINY32
    if mutant != "no_wsum_div":
        y[nz] = y[nz] / ws[nz]
    g[nz] = g[nz] / ws[nz]
    scale = dt(1.0 if mutant == "no_scale" else fl / hop)
    y = y * scale
    g = g * (fl / hop)
    y, g = y[fl // 2:-(fl // 2)], g[fl // 2:-(fl // 2)]
    return y, g + 4 * EPS32 * np.abs(y)


def frames_of(x, cfg, mutant=None):
    fl, hop, _ = dims(cfg)
    if mutant == "clip_in_loop":
        x = np.clip(x, -1.0, 1.0)
    xp = np.pad(x, (fl // 2, fl // 2), mode="constant" if mutant == "zero_pad" else "reflect")
    T = len(x) // hop + 1
    return np.stack([xp[t * hop:t * hop + fl] for t in range(T)])


def spectrum(x, gx, cfg, mutant=None, dt=np.float64, fb=None):
    """signal [n] -> (Y [T, fl + 2], gate) without the clip: stft.py:52-76"""
    fb = (bases(cfg)[0] if fb is None else fb).astype(dt)
    fr = frames_of(np.asarray(x).astype(dt), cfg, mutant)
    gfr = frames_of(np.asarray(gx, np.float64), cfg) if gx is not None else 0.0 * fr
    return fr @ fb.T, gfr @ np.abs(fb).T + C_SUM * (np.abs(fr) @ np.abs(fb).T)


def rephase(Y, gY, mag, mutant=None, dt=np.float64):
    """X = mag * Y / |Y| per bin, (mag, 0) where Y = 0: stft.py:79,84-86 without the angle.  (X [T, fl + 2], gate)"""
    cut = Y.shape[1] // 2
    re, im = Y[:, :cut].astype(dt), Y[:, cut:].astype(dt)
    mag = np.asarray(mag).astype(dt)
    r = np.hypot(re, im)
    zero = r == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ur, ui = np.where(zero, 0.0 if mutant == "rephase_zero_at_zero" else 1.0, re / r), np.where(zero, 0.0, im / r)
    X = np.concatenate([mag * ur, mag * ui], axis=1).astype(dt)
    gsum = (gY[:, :cut] + gY[:, cut:]) if gY is not None else np.zeros(r.shape)
    with np.errstate(invalid="ignore"):
        d = np.minimum(2.0, np.where(gsum == 0, 0.0, gsum / np.maximum(r - gsum, TINY32))) + 4 * EPS32
    g = np.abs(mag) * d
    return X, np.concatenate([g, g], axis=1)


def step(x, gx, mag, cfg, mutant=None, dt=np.float64):
    """one iteration (audio_processing.py:80-81): (signal, gate)"""
    Y, gY = spectrum(x, gx, cfg, mutant, dt)
    X, gX = rephase(Y, gY, mag, mutant, dt)
    return inverse(X, gX, cfg, None, dt)


def griffin_lim(mag, ang, n_iters, cfg, mutant=None, dt=np.float64, with_gate=True):
    """(signal, gate) after n_iters iterations from the given angles.  A mutant of one operator is applied wherever that operator runs."""
    inv_m = mutant if mutant in INVERSE_MUTANTS else None
    X, gX = recombine(mag, ang, dt)
    y, g = inverse(X, gX, cfg, inv_m, dt)
    fb, ib = (b.astype(dt) for b in bases(cfg, inv_m))
    Xprev = X
    for _ in range(n_iters):
        Y, gY = spectrum(y, g if with_gate else None, cfg, mutant, dt, fb=fb)
        X, gX = rephase(Y, gY if with_gate else None, mag, mutant, dt)
        if mutant == "stale_phase":
            X, Xprev = Xprev, X
        y, g = inverse(X, gX, cfg, inv_m, dt, ib=ib)
    return y, g


def spectral_convergence(y, mag, cfg):
    """|| |STFT64(y)| - mag || / ||mag|| (Frobenius), the STFT in float64"""
    Y, _ = spectrum(np.asarray(y, np.float64), None, cfg)
    cut = Y.shape[1] // 2
    m = np.hypot(Y[:, :cut], Y[:, cut:])
    mag = np.asarray(mag, np.float64)
    return float(np.linalg.norm(m - mag) / np.linalg.norm(mag))


def share(x, x64, gate):
    return mc.share(x, x64, gate)


def pad_rows(a, T):
    """zero rows up to T: what the device writes at and beyond an utterance's frames (gate 0 there)"""
    return np.concatenate([a, np.zeros((T - a.shape[0],) + a.shape[1:], a.dtype)]) if a.shape[0] < T else a


def fixture_mels(cfg, seed, frames=(24, 17, 9)):
    """Seeded log-mels [n_mel, T] of speech-like level: a few moving formant bumps over a floor near log(1e-5), so magnitudes after
    * 1000 are of order 1 .. 100 and some bins are almost silent.  Frame counts differ; all exceed KW / 2 + 3."""
    rs = np.random.RandomState(seed)
    n_mel = cfg["n_mel_channels"]
    out = []
    for T in frames:
        t, m = np.arange(T)[None, :], np.arange(n_mel)[:, None]
        mel = -9.0 + 0.3 * rs.standard_normal((n_mel, T))
        for _ in range(3):
            c, w = rs.uniform(0.1, 0.9) * n_mel, rs.uniform(1.0, 0.12 * n_mel)
            mel += 7.0 * np.exp(-0.5 * ((m - c - 0.1 * t) / w) ** 2) * (0.6 + 0.4 * np.sin(0.5 * t + rs.uniform(0, 6)))
        out.append(mel.astype(np.float32))
    return out
