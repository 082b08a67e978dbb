"""The Griffin-Lim mel-to-wave path on the MI355X (audio.STFT, griffin_lim, mel_to_wave, ns_gl_*) against the float64 restatement and
the gates of tests/griffinlim_cpu.py: each operator alone, one step, the loop as a chain of its steps, determinism, replicas, padding,
poison, the stored reference fixtures, spectral convergence after 60 iterations and the wave -> mel -> wave -> mel round trip."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import griffinlim_cpu as gc  # noqa: E402
import melfront_cpu as mc  # noqa: E402
from smart_nar_fast_tts_amd import _lib  # noqa: E402
from smart_nar_fast_tts_amd import audio as A  # noqa: E402

pytestmark = pytest.mark.gpu
CONFIGS = {"tiny": gc.TINY, "ljspeech": gc.LJSPEECH}
# frame counts per batch: three different utterances between KW / 2 + 3 and 24 frames; the same utterance twice; past one 256-row GEMM tile
BATCHES = {"tiny": {"three": [24, 7, 13], "twice": [11, 24, 11], "rows": [70, 70, 70, 70]},
           "ljspeech": {"three": [24, 5, 13], "twice": [9, 17, 9], "rows": [70, 70, 70, 70]}}


def taco(cfg):
    return A.TacotronSTFT(cfg["filter_length"], cfg["hop_length"], cfg["win_length"], cfg["n_mel_channels"], cfg["sampling_rate"],
                          cfg["mel_fmin"], cfg["mel_fmax"]).to("cuda:0")


@pytest.fixture(scope="module")
def tacos():
    return {name: taco(cfg) for name, cfg in CONFIGS.items()}


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in CONFIGS:
        z = np.load(os.path.join(HERE, "golden", f"griffinlim_{name}.npz"))
        out[name] = (json.loads(str(z["meta"])), z)
    return out


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


class Ops:
    """the ns_gl_op_* entry points of one STFT's handle; the workspace is poisoned with NaN before every call"""

    def __init__(self, fn):
        self.fn, self.so, self.h = fn, _lib.load(), fn._h
        self.fl, self.hop, self.bins, self.kw = fn.filter_length, fn.hop_length, fn.cutoff, fn.filter_length // fn.hop_length

    def ws(self, B, T):
        n = int(self.so.ns_gl_ws_bytes(self.h, B, T))
        w = torch.empty(n // 4 + 64, dtype=torch.float32, device="cuda")
        w.fill_(float("nan"))
        return w, n

    def st(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def mel_to_mag(self, mel_t, lens):
        B, T = mel_t.shape[:2]
        mag = nan_like(B, T - 1, self.bins)
        _lib.check(self.so.ns_gl_op_mel_to_mag(self.h, _lib.ptr(mel_t), _lib.ptr(lens), B, T, _lib.ptr(mag), self.st()), "mel_to_mag")
        return mag

    def recombine(self, mag, ang, lens):
        B, T = mag.shape[:2]
        X = nan_like(B, T, self.fl)
        _lib.check(self.so.ns_gl_op_recombine(self.h, _lib.ptr(mag), _lib.ptr(ang), _lib.ptr(lens), B, T, _lib.ptr(X), self.st()), "recombine")
        return X

    def rephase(self, Y, mag, lens):
        B, S = Y.shape[:2]
        T = mag.shape[1]
        X = nan_like(B, T, self.fl)
        _lib.check(self.so.ns_gl_op_rephase(self.h, _lib.ptr(Y), _lib.ptr(mag), _lib.ptr(lens), B, T, S, _lib.ptr(X), self.st()), "rephase")
        return X

    def inverse(self, X, lens, extra=0):
        B, T = X.shape[:2]
        ld = self.hop * (T - 1) + extra
        wave, wl = nan_like(B, ld), torch.full((B,), -7, dtype=torch.long, device="cuda")
        w, n = self.ws(B, T)
        _lib.check(self.so.ns_gl_op_inverse(self.h, _lib.ptr(X), _lib.ptr(lens), B, T, _lib.ptr(wave), ld, _lib.ptr(wl), _lib.ptr(w), n, self.st()), "inverse")
        return wave, wl

    def frame_rows(self, wav, lens, n_max, S):
        B = wav.shape[0]
        rows = nan_like(B, S, self.hop)
        _lib.check(self.so.ns_gl_op_frame_rows(self.h, _lib.ptr(wav), wav.shape[1], _lib.ptr(lens), B, n_max, S, _lib.ptr(rows), self.st()), "frame_rows")
        return rows

    def step(self, mag, lens, wave):
        B, T = mag.shape[:2]
        wave, wl = wave.clone(), torch.full((B,), -7, dtype=torch.long, device="cuda")
        w, n = self.ws(B, T)
        _lib.check(self.so.ns_gl_op_step(self.h, _lib.ptr(mag), _lib.ptr(lens), B, T, _lib.ptr(wave), wave.shape[1], _lib.ptr(wl), _lib.ptr(w), n, self.st()), "step")
        return wave, wl


@pytest.fixture(scope="module")
def ops(tacos):
    return {name: Ops(t.stft_fn) for name, t in tacos.items()}


def magnitudes(rs, T, bins):
    """positive magnitudes of order 1 .. 100 with non-zero bins 0 and N/2, a few exact zeros"""
    m = np.exp(rs.uniform(0.0, 4.6, (T, bins))).astype(np.float32)
    m[rs.rand(T, bins) < 0.02] = 0.0
    return m


def case(name, frames, seed):
    """a padded batch: per utterance magnitudes [T_b, bins] and angles, the padded device tensors, device lens"""
    cfg = CONFIGS[name]
    bins = cfg["filter_length"] // 2 + 1
    rs = np.random.RandomState(seed)
    mags, angs = [], []
    for b, t in enumerate(frames):
        same = next((i for i in range(b) if frames[i] == t), None) if len(set(frames)) < len(frames) and len(frames) == 3 else None
        mags.append(mags[same] if same is not None else magnitudes(rs, t, bins))
        angs.append(angs[same] if same is not None else rs.uniform(-np.pi, np.pi, (t, bins)).astype(np.float32))
    T = max(frames)
    pad = lambda a: np.stack([np.concatenate([x, rs.standard_normal((T - len(x), bins)).astype(np.float32)]) for x in a])  # noqa: E731  garbage beyond lens
    return cfg, mags, angs, dev(pad(mags)), dev(pad(angs)), dev(frames, np.int64), T


BATCH_IDS = [(n, k) for n in CONFIGS for k in ("three", "twice", "rows")]


def _utterances(frames, key):
    return range(len(frames)) if key != "rows" else (0, 3)  # the float64 work of the large batch is bounded: first and last utterance


# ---- each operator alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_op_mel_to_mag(ops, golden, name):
    meta, z = golden[name]
    cfg = CONFIGS[name]
    mels = [z[f"mel{i}"].T for i in range(meta["n_mels"])] + [z["mel1"].T]
    T = max(len(m) for m in mels)
    mel_t = np.full((len(mels), T, cfg["n_mel_channels"]), 3.0, np.float32)
    for b, m in enumerate(mels):
        mel_t[b, :len(m)] = m
    got = ops[name].mel_to_mag(dev(mel_t), dev([len(m) for m in mels], np.int64)).cpu().numpy()
    for b, m in enumerate(mels):
        want, g = gc.mel_to_mag(m, z["mel_basis"])
        sh = gc.share(got[b, :len(want)], want, g)
        print(f"{name} mel_to_mag utterance {b}: share of the gate {sh:.3g}; reference fp32 {gc.share(z[f'mag{min(b, 2) if b < 3 else 1}'], want, g):.3g}")
        assert sh <= 1.0
        assert not got[b, len(want):].any(), "the dropped last frame and the padding are zeros"
    assert got[3].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("name,key", BATCH_IDS)
def test_op_recombine_and_inverse(ops, name, key):
    frames = BATCHES[name][key]
    cfg, mags, angs, mag_d, ang_d, lens, T = case(name, frames, 31)
    o = ops[name]
    X = o.recombine(mag_d, ang_d, lens)
    wave, wl = o.inverse(X, lens)
    Xh, wh = X.cpu().numpy(), wave.cpu().numpy()
    assert wl.cpu().tolist() == [o.hop * (t - 1) for t in frames]
    for b in _utterances(frames, key):
        t = frames[b]
        X64, gX = gc.recombine(mags[b], angs[b])
        sh_x = gc.share(Xh[b, :t], mc.packed_columns(X64, o.fl), mc.packed_columns(gX, o.fl))
        # the inverse alone: float64 from the DEVICE's own X (exact input, zero input gate)
        Xfull = np.zeros((t, o.fl + 2))
        Xfull[:, 0], Xfull[:, o.fl // 2] = Xh[b, :t, 0], Xh[b, :t, 1]
        Xfull[:, 1:o.fl // 2], Xfull[:, o.bins + 1:o.bins + o.fl // 2] = Xh[b, :t, 2::2], Xh[b, :t, 3::2]
        y64, g = gc.inverse(Xfull, np.zeros_like(Xfull), cfg)
        n = o.hop * (t - 1)
        sh_y = gc.share(wh[b, :n], y64, g)
        edge = o.fl // 2
        sh_edge = max(gc.share(wh[b, :edge], y64[:edge], g[:edge]), gc.share(wh[b, n - edge:n], y64[n - edge:], g[n - edge:]))
        print(f"{name} {key} utterance {b} ({t} frames): recombine share {sh_x:.3g}, inverse share {sh_y:.3g} (ends, where window_sum is partial: {sh_edge:.3g})")
        assert sh_x <= 1.0 and sh_y <= 1.0
        assert not Xh[b, t:].any() and not wh[b, n:].any(), "rows beyond the frames and samples beyond wave_lens are zeros"
    if key == "twice":
        assert wh[0, :o.hop * (frames[0] - 1)].tobytes() == wh[2, :o.hop * (frames[2] - 1)].tobytes(), "replicas are bit-identical"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_op_inverse_partial_row_and_alone_equals_batch(ops, name):
    frames = BATCHES[name]["three"]
    cfg, mags, angs, mag_d, ang_d, lens, T = case(name, frames, 32)
    o = ops[name]
    X = o.recombine(mag_d, ang_d, lens)
    wave, _ = o.inverse(X, lens)
    wide, _ = o.inverse(X, lens, extra=12)  # ld_wave past the last hop row: the tail is a partial float4 row of zeros
    assert torch.equal(wide[:, :wave.shape[1]], wave) and not wide[:, wave.shape[1]:].any()
    for b, t in enumerate(frames):  # an utterance alone equals the same utterance inside the padded batch
        Xb = o.recombine(mag_d[b:b + 1, :t].contiguous(), ang_d[b:b + 1, :t].contiguous(), lens[b:b + 1])
        alone, _ = o.inverse(Xb, lens[b:b + 1])
        assert torch.equal(alone[0], wave[b, :o.hop * (t - 1)])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_op_frame_rows_without_the_clip_is_exact(ops, name):
    o = ops[name]
    rs = np.random.RandomState(33)
    lens = [o.hop * 9, o.fl // 2 + 1, o.hop * 5 + 7, o.fl // 2]
    n_max = max(lens)
    wav = (rs.standard_normal((len(lens), n_max + 4)) * 50).astype(np.float32)  # Griffin-Lim signals are far beyond +-1
    S = n_max // o.hop + o.kw
    rows = o.frame_rows(dev(wav), dev(lens, np.int64), n_max, S).cpu().numpy()
    for b, n in enumerate(lens):
        want = np.zeros(S * o.hop, np.float32)
        if n > o.fl // 2:
            xp = np.pad(wav[b, :n], (o.fl // 2, o.fl // 2), mode="reflect")
            want[:min(len(xp), len(want))] = xp[:len(want)]
        assert rows[b].reshape(-1).tobytes() == want.tobytes(), (name, b)
    assert np.abs(rows).max() > 100


@pytest.mark.parametrize("name", list(CONFIGS))
def test_op_rephase_crafted_rows(ops, name):
    o = ops[name]
    cfg = CONFIGS[name]
    rs = np.random.RandomState(34)
    T, S = 9, 9 + o.kw - 1
    Y = (rs.standard_normal((2, S, o.fl)) * 30).astype(np.float32)
    mag = np.stack([magnitudes(rs, T, o.bins) for _ in range(2)])
    Y[0, 1] = 0.0                       # an exactly silent frame
    Y[0, 2, [0, 1, 10, 11, 21]] = 0.0   # bins 0, N/2 and 5 exactly zero; bin 10 with a zero imaginary part
    Y[0, 3, 0], Y[0, 3, 1] = -3.0, -0.0  # negative real bins; a negative zero
    Y[0, 4] *= 1e-30                    # components whose squares underflow
    mag[0, 5] = 0.0                     # zero target magnitude
    Y[0, 6, 40] = np.nan
    Y[0, 7, [0, 50, 61]] = np.nan       # a NaN in bin 0 (whose imaginary part is forced to 0), the pair (NaN, 0) and the pair (0, NaN)
    Y[0, 7, [51, 60]] = 0.0
    nan_cols = {6: [40, 41], 7: [0, 50, 51, 60, 61]}  # packed columns that must come out NaN: every NaN's whole bin
    lens = [T, 7]
    X = o.rephase(dev(Y), dev(mag), dev(lens, np.int64)).cpu().numpy()
    for b, t in enumerate(lens):
        Yfull = np.zeros((t, o.fl + 2))
        Yfull[:, 0], Yfull[:, o.fl // 2] = Y[b, :t, 0], Y[b, :t, 1]
        Yfull[:, 1:o.fl // 2], Yfull[:, o.bins + 1:o.bins + o.fl // 2] = Y[b, :t, 2::2], Y[b, :t, 3::2]
        ok = ~np.isnan(Yfull)
        want, g = gc.rephase(np.nan_to_num(Yfull), None, mag[b, :t])
        wp, gp, okp = mc.packed_columns(want, o.fl), mc.packed_columns(g, o.fl), mc.packed_columns(ok, o.fl)
        if b == 0:
            for r, cols in nan_cols.items():
                okp[r, cols] = False  # the NaN's partner component in the same bin is NaN too
        sh = gc.share(X[b, :t][okp], wp[okp], gp[okp])
        print(f"{name} rephase utterance {b}: share of the gate {sh:.3g}")
        assert sh <= 1.0
        assert not X[b, t:].any()
    for r, cols in nan_cols.items():
        assert np.isnan(X[0, r, cols]).all() and np.isfinite(np.delete(X[0, r], cols)).all(), "a NaN makes its bin NaN and stays in its bin"
    assert np.array_equal(X[0, 1, 2::2], mag[0, 1, 1:o.fl // 2]) and not X[0, 1, 3::2].any(), "Y = 0 gives (mag, 0)"
    assert X[0, 3, 0] == -mag[0, 3, 0] and X[0, 3, 1] == mag[0, 3, o.fl // 2] and not X[0, 5].any()


@pytest.mark.parametrize("name,key", BATCH_IDS)
def test_op_step_from_the_devices_own_signal(ops, name, key):
    frames = BATCHES[name][key]
    cfg, mags, angs, mag_d, ang_d, lens, T = case(name, frames, 35)
    o = ops[name]
    wave0, _ = o.inverse(o.recombine(mag_d, ang_d, lens), lens)
    wave1, wl = o.step(mag_d, lens, wave0)
    w0, w1 = wave0.cpu().numpy(), wave1.cpu().numpy()
    assert wl.cpu().tolist() == [o.hop * (t - 1) for t in frames]
    for b in _utterances(frames, key):
        n = o.hop * (frames[b] - 1)
        want, g = gc.step(w0[b, :n], None, mags[b], cfg)
        sh = gc.share(w1[b, :n], want, g)
        print(f"{name} {key} step utterance {b}: share of the gate {sh:.3g}, amplitude {np.abs(want).max():.3g}")
        assert sh <= 1.0 and not w1[b, n:].any()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_transform_magnitude_and_circular_phase(tacos, name):
    cfg = CONFIGS[name]
    fn = tacos[name].stft_fn
    fl, hop = fn.filter_length, fn.hop_length
    rs = np.random.RandomState(36)
    lens = [hop * 12 + 5, fl // 2 + 1, hop * 7]
    x = (rs.standard_normal((3, max(lens))) * 20).astype(np.float32)
    mag, ph = fn.transform(dev(x), lens)
    T = max(lens) // hop + 1
    assert tuple(mag.shape) == tuple(ph.shape) == (3, fn.cutoff, T) and mag.transpose(1, 2).is_contiguous()
    mag, ph = mag.cpu().numpy(), ph.cpu().numpy()
    for b, n in enumerate(lens):
        Y, gY = gc.spectrum(x[b, :n], None, cfg)
        t, cut = len(Y), fn.cutoff
        re, im, gs = Y[:, :cut], Y[:, cut:], gY[:, :cut] + gY[:, cut:]
        m64 = np.hypot(re, im)
        sh_m = gc.share(mag[b, :, :t].T, m64, gs + gc.EPS32 * m64)
        d = np.abs(ph[b, :, :t].T - np.arctan2(im, re))
        d = np.minimum(d, 2 * np.pi - d)  # circular distance: a sign flip of a zero imaginary part moves the angle by 2 pi
        with np.errstate(divide="ignore"):
            bound = np.minimum(np.pi, gs / np.maximum(m64 - gs, gc.TINY32)) + 8 * gc.EPS32 * np.pi
        print(f"{name} transform utterance {b}: magnitude share {sh_m:.3g}, worst phase distance / bound {float((d / bound).max()):.3g}")
        assert sh_m <= 1.0 and (d <= bound).all()
        assert not mag[b, :, t:].any() and not ph[b, :, t:].any()


# ---- the loop -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_loop_is_its_steps_deterministic_and_replicated(tacos, ops, name):
    frames = BATCHES[name]["twice"]
    cfg, mags, angs, mag_d, ang_d, lens, T = case(name, frames, 37)
    o, fn = ops[name], tacos[name].stft_fn
    got = A.griffin_lim(mag_d.transpose(1, 2), fn, n_iters=3, angles=ang_d.transpose(1, 2), lens=lens)
    wave, _ = o.inverse(o.recombine(mag_d, ang_d, lens), lens)
    for _ in range(3):
        wave, _ = o.step(mag_d, lens, wave)
    assert torch.equal(got, wave), "griffin_lim(n_iters = 3) is recombine + inverse + three steps, bit for bit"
    again = A.griffin_lim(mag_d.transpose(1, 2), fn, n_iters=3, angles=ang_d.transpose(1, 2), lens=lens)
    assert torch.equal(got, again), "two runs give the same bits"
    n = o.hop * (frames[0] - 1)
    assert torch.equal(got[0, :n], got[2, :n]) and not got[0, n:].any(), "replicas are bit-identical; zeros beyond wave_lens"
    assert fn.wave_lens.cpu().tolist() == [o.hop * (t - 1) for t in frames]
    alone = A.griffin_lim(mag_d[1:2].transpose(1, 2), fn, n_iters=3, angles=ang_d[1:2].transpose(1, 2))
    assert torch.equal(alone[0], got[1]), "an utterance alone equals the same utterance inside the padded batch"
    # STFT.inverse is the n_iters = 0 loop in the reference's layouts
    inv = fn.inverse(mag_d.transpose(1, 2), ang_d.transpose(1, 2), lens)
    assert tuple(inv.shape) == (3, 1, o.hop * (T - 1)) and torch.equal(inv[:, 0], o.inverse(o.recombine(mag_d, ang_d, lens), lens)[0])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_mel_to_wave_is_mel_to_mag_then_griffin_lim_and_fixtures_inside_the_gate(tacos, ops, golden, name):
    meta, z = golden[name]
    cfg, t, o = CONFIGS[name], tacos[name], ops[name]
    mels = [z[f"mel{i}"] for i in range(meta["n_mels"])]
    T = max(m.shape[1] for m in mels)
    mel = np.full((len(mels), cfg["n_mel_channels"], T), 2.0, np.float32)
    ang = np.zeros((len(mels), o.bins, T - 1), np.float32)
    for b, m in enumerate(mels):
        mel[b, :, :m.shape[1]] = m
        ang[b, :, :m.shape[1] - 1] = z[f"angles{b}"].T
    mel_lens = [m.shape[1] for m in mels]
    mel_d, ang_d = dev(mel), dev(ang)
    for n_iters in (0, 2):
        wave, wl = A.mel_to_wave(mel_d, t, griffin_iters=n_iters, mel_lens=mel_lens, angles=ang_d)
        assert wl.cpu().tolist() == [o.hop * (n - 2) for n in mel_lens]
        mag = o.mel_to_mag(mel_d.transpose(1, 2).contiguous(), dev(mel_lens, np.int64))
        chain = A.griffin_lim(mag.transpose(1, 2), t.stft_fn, n_iters=n_iters, angles=ang_d, lens=[n - 1 for n in mel_lens])
        assert torch.equal(wave, chain)
        w = wave.cpu().numpy()
        for b, m in enumerate(mels):
            mag64, _ = gc.mel_to_mag(m.T, z["mel_basis"])
            y64, g = gc.griffin_lim(mag64, z[f"angles{b}"], n_iters, cfg)
            n = len(y64)
            sh, sh_ref = gc.share(w[b, :n], y64, g), gc.share(z[f"wave{b}_it{n_iters}"], y64, g)
            rel = np.abs(w[b, :n] - y64).max() / np.abs(y64).max()
            print(f"{name} fixture {b} n_iters {n_iters}: HIP share of the gate {sh:.3g} (reference fp32 {sh_ref:.3g}), relative distance {rel:.3g}")
            assert sh <= 1.0 and sh_ref <= 1.0 and not w[b, n:].any()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_sixty_iterations_spectral_convergence(tacos, golden, name):
    """Elementwise comparison means nothing after 60 iterations (fp32 and float64 trajectories drift apart), so the device's result is
    held to the float64 run's spectral convergence from the same angles: |SC_hip - SC_64| <= 8 |SC_np32 - SC_64|, the numpy fp32
    restatement's own distance (stored by the golden maker) times 8 for a different summation order; and not worse than the
    reference's own SC by more than the same allowance."""
    meta, z = golden[name]
    cfg, sc = CONFIGS[name], meta["sc"]
    mel = z["mel0"]
    wave, _ = A.mel_to_wave(dev(mel[None]), tacos[name], griffin_iters=sc["iters"], angles=dev(z["angles0"].T[None]))
    mag64, _ = gc.mel_to_mag(mel.T, z["mel_basis"])
    sc_hip = gc.spectral_convergence(wave[0].cpu().numpy(), mag64, cfg)
    allowance = 8 * abs(sc["sc_np32"] - sc["sc_f64"])
    print(f"{name}: SC_hip {sc_hip:.12g}, SC_64 {sc['sc_f64']:.12g}, SC_np32 {sc['sc_np32']:.12g}, SC_reference {sc['sc_reference']:.12g}, "
          f"|SC_hip - SC_64| {abs(sc_hip - sc['sc_f64']):.3g}, allowance {allowance:.3g}")
    assert abs(sc_hip - sc["sc_f64"]) <= allowance
    assert sc_hip <= sc["sc_reference"] + allowance


def test_too_short_device_lengths_and_zero_iterations(tacos, ops):
    o, t = ops["tiny"], tacos["tiny"]
    frames = [9, 5, 0, 6, 40]  # 32 * (5 - 1) = 128 = filter_length / 2: too short; 6 frames is the shortest legal; 40 is clamped to 9
    cfg, mags, angs, mag_d, ang_d, _, T = case("tiny", [9, 9, 9, 9, 9], 38)
    lens = dev(frames, np.int64)
    wave = A.griffin_lim(mag_d.transpose(1, 2), t.stft_fn, n_iters=2, angles=ang_d.transpose(1, 2), lens=lens)
    assert t.stft_fn.wave_lens.cpu().tolist() == [256, 0, 0, 160, 256]
    assert not wave[1].any() and not wave[2].any() and not wave[3, 160:].any() and torch.isfinite(wave).all()
    assert torch.equal(wave[4], wave[0]) is False and wave[0].abs().max() > 1
    with pytest.raises(ValueError, match="too short"):
        A.griffin_lim(mag_d.transpose(1, 2), t.stft_fn, n_iters=2, angles=ang_d.transpose(1, 2), lens=frames[:2] + [9, 9, 9])
    with pytest.raises(ValueError, match="too short"):
        A.mel_to_wave(torch.zeros(1, 16, 6, device="cuda"), t)
    x = A.griffin_lim(mag_d[:1].transpose(1, 2), t.stft_fn, n_iters=0, angles=ang_d[:1].transpose(1, 2))
    assert torch.equal(x[0], o.inverse(o.recombine(mag_d[:1], ang_d[:1], lens[:1]), lens[:1])[0][0])


def test_round_trip_on_the_device_and_inv_mel_spec(tacos, tmp_path):
    """wave -> mel -> wave -> mel without leaving the device; inv_mel_spec writes what mel_to_wave returns"""
    t = tacos["ljspeech"]
    sr, n = 22050, 256 * 40
    x = (0.4 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr) + 0.2 * np.sin(2 * np.pi * 1320.0 * np.arange(n) / sr)).astype(np.float32)
    mel, _ = t.mel_spectrogram(dev(x[None]))
    np.random.seed(3)
    wave, wl = A.mel_to_wave(mel, t, griffin_iters=30)
    assert wave.is_cuda and wl.cpu().tolist() == [256 * (mel.shape[2] - 2)] and torch.isfinite(wave).all()
    y = wave / wave.abs().max()
    mel2, _ = t.mel_spectrogram(y)
    a, b = mel[0, :, 2:-3], mel2[0, :, 2:-2]
    assert a.shape == b.shape
    # the level is lost (scaling 1000, then the normalisation above): compare the log-mels up to one offset, on the audible bands
    loud = a > a.max() - 6.0
    off = (a - b)[loud].mean()
    err = float(((a - b - off)[loud]).abs().mean())
    print(f"round trip: mean |log-mel difference| on the loud bands after removing the level offset {float(off):.3f}: {err:.3f}")
    # mel_basis^T is no inverse of mel_basis, so the round trip is lossy by construction: the float64 restatement of this very case
    # gives 0.64 (tests/griffinlim_cpu.py, same seed).  log(4): the resynthesised mel stays within a factor of four of the original on
    # the loud bands — a sanity level, not a precision gate; the gates are the tests above.
    assert err < float(np.log(4.0)), "the resynthesised wave carries the mel it was made from"
    from scipy.io import wavfile

    np.random.seed(3)
    path = str(tmp_path / "gl.wav")
    A.inv_mel_spec(mel[0], path, t, griffin_iters=30)
    rate, data = wavfile.read(path)
    assert rate == 22050 and data.dtype == np.float32 and data.tobytes() == wave[0].cpu().numpy().tobytes()
