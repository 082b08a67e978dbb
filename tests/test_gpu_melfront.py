"""The wave-to-mel front end on the MI355X (audio.TacotronSTFT, ns_mel_*) against the float64 restatement and the gates of
tests/melfront_cpu.py: the stored fixtures, random batches, each operator alone, poison, padding, determinism, layout, the chain
into forward_teacher_forced() and the loss, and the refusals."""
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

import melfront_cpu as mc  # noqa: E402
from smart_nar_fast_tts_amd import _lib  # noqa: E402
from smart_nar_fast_tts_amd import audio as A  # noqa: E402

pytestmark = pytest.mark.gpu
CONFIGS = {"tiny": mc.TINY, "ljspeech": mc.LJSPEECH}
LOG_CLIP = float(np.log(np.float64(np.float32(1e-5))))  # log(clip_val) of the fp32 clip_val, in float64


def make(cfg):
    return A.TacotronSTFT(cfg["filter_length"], cfg["hop_length"], cfg["win_length"], cfg["n_mel_channels"], cfg["sampling_rate"],
                          cfg["mel_fmin"], cfg["mel_fmax"]).to("cuda:0")


@pytest.fixture(scope="module")
def stfts():
    return {name: make(cfg) for name, cfg in CONFIGS.items()}


def batch_of(waves):
    n = max(len(w) for w in waves)
    y = np.zeros((len(waves), n), np.float32)
    for b, w in enumerate(waves):
        y[b, :len(w)] = w
    return y, [len(w) for w in waves]


def check_batch(st, cfg, waves, what, refs=None):
    """run the batch, compare every utterance with reference64 inside the gates, check lengths and zero padding; returns (mel, energy)"""
    y, lens = batch_of(waves)
    mel, energy = st.mel_spectrogram(torch.from_numpy(y).cuda(), lens)
    T = y.shape[1] // cfg["hop_length"] + 1
    assert tuple(mel.shape) == (len(waves), cfg["n_mel_channels"], T) and tuple(energy.shape) == (len(waves), T)
    assert st.mel_lens.cpu().tolist() == [n // cfg["hop_length"] + 1 for n in lens]
    mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
    for b, w in enumerate(waves):
        r = mc.reference64(w, cfg) if refs is None else refs[b]
        t = len(w) // cfg["hop_length"] + 1
        sh = mc.shares(mel[b, :, :t], energy[b, :t], r)
        print(f"{what} utterance {b} (n = {len(w)}, {t} frames): HIP shares of the gates {sh}")
        assert sh["mel"] <= 1.0 and sh["energy"] <= 1.0, (what, b, sh)
        assert not mel[b, :, t:].any() and not energy[b, t:].any(), "frames at and beyond mel_lens are exactly zero"
    return mel, energy


def random_wave(rs, n, scale=0.3):
    return np.clip(rs.standard_normal(n) * scale, -1.2, 1.2).astype(np.float32)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fixtures_inside_the_gates(stfts, name):
    z = np.load(os.path.join(HERE, "golden", f"melfront_{name}.npz"))
    meta = json.loads(str(z["meta"]))
    cfg = CONFIGS[name]
    waves = [z[f"wave{i}"] for i in range(meta["n_waves"])]
    refs = [mc.reference64(w, cfg) for w in waves]
    for i, r in enumerate(refs):
        assert np.array_equal(r[0], z[f"mel{i}_f64"]) and np.array_equal(r[1], z[f"energy{i}_f64"])
    mel, energy = check_batch(stfts[name], cfg, waves, f"fixture {name}", refs)
    # the reference's own fp32 values sit in the same gates, so the two differ by at most the sum of their distances
    for i in range(meta["n_waves"]):
        t = z[f"mel{i}"].shape[1]
        assert (np.abs(mel[i, :, :t].astype(np.float64) - z[f"mel{i}"]) <= 2 * refs[i][2]).all()
    # get_mel_from_wav: the single-wave surface gives the batch's bits (the reduction order depends on the shapes of a frame alone)
    m1, e1 = A.get_mel_from_wav(waves[1], stfts[name])
    t = len(waves[1]) // cfg["hop_length"] + 1
    assert m1.shape == (cfg["n_mel_channels"], t) and e1.shape == (t,)
    assert m1.tobytes() == np.ascontiguousarray(mel[1, :, :t]).tobytes() and e1.tobytes() == energy[1, :t].tobytes()


def test_random_batch_short_and_boundary_lengths(stfts):
    rs = np.random.RandomState(3)
    check_batch(stfts["ljspeech"], mc.LJSPEECH, [random_wave(rs, n) for n in (5000, 513, 2047)], "ljspeech B=3")  # M = 3 * 23 = 69 rows


def test_random_batch_beyond_the_small_grid(stfts):
    rs = np.random.RandomState(4)
    waves = [random_wave(rs, 65536) for _ in range(8)]  # M = 8 * 260 = 2080 rows
    y, lens = batch_of(waves)
    st = stfts["ljspeech"]
    mel, energy = st.mel_spectrogram(torch.from_numpy(y).cuda())
    mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
    for b in (0, 3, 7):  # three utterances bound the float64 work; every utterance goes through the same launches
        sh = mc.shares(mel[b], energy[b], mc.reference64(waves[b], mc.LJSPEECH))
        print(f"B=8 x 65536 utterance {b}: HIP shares of the gates {sh}")
        assert sh["mel"] <= 1.0 and sh["energy"] <= 1.0
    assert np.isfinite(mel).all() and np.isfinite(energy).all()


@pytest.mark.parametrize("hop", [32, 128])
def test_tiny_configuration_hops(hop):
    cfg = dict(mc.TINY, hop_length=hop)  # KW = 8 and 2
    rs = np.random.RandomState(5 + hop)
    check_batch(make(cfg), cfg, [random_wave(rs, n) for n in (1000, 129, 777, 2 * hop * 7)], f"tiny hop {hop}")


def test_silence_is_exact(stfts):
    rs = np.random.RandomState(6)
    waves = [random_wave(rs, 3000), np.zeros(3000, np.float32)]
    mel, energy = check_batch(stfts["ljspeech"], mc.LJSPEECH, waves, "silence")
    # every mel value of the silent utterance is the device's logf(clip_val): ONE value, within an fp32 ulp of the float64 logarithm
    assert len(np.unique(mel[1])) == 1 and abs(float(mel[1, 0, 0]) - LOG_CLIP) <= abs(float(np.spacing(np.float32(LOG_CLIP))))
    assert (energy[1] == 0).all()


# ---- each operator alone ------------------------------------------------------------------------------------------------------
def _ops_case(name, lens, seed):
    cfg = CONFIGS[name]
    fl, hop = cfg["filter_length"], cfg["hop_length"]
    rs = np.random.RandomState(seed)
    n_max = max(lens)
    y = (rs.standard_normal((len(lens), n_max + 5)) * 0.6).astype(np.float32)  # ld > n_max; values beyond +-1 occur
    Tc = n_max // hop + 1
    S = Tc + fl // hop - 1
    return cfg, fl, hop, y, n_max, Tc, S


@pytest.mark.parametrize("name,lens", [("ljspeech", [5000, 513, 2047, 512, 0]), ("tiny", [1000, 129, 128, 777])])
def test_op_frame_rows_bit_exact(stfts, name, lens):
    so = _lib.load()
    cfg, fl, hop, y, n_max, Tc, S = _ops_case(name, lens, 7)
    B = len(lens)
    rows = torch.full((B, S, hop), float("nan"), device="cuda")
    ml = torch.full((B,), -7, dtype=torch.long, device="cuda")
    yd, ld = torch.from_numpy(y).cuda(), torch.tensor(lens, dtype=torch.long).cuda()
    _lib.check(so.ns_mel_op_frame_rows(stfts[name]._h, _lib.ptr(yd), y.shape[1], _lib.ptr(ld), B, n_max, S, _lib.ptr(rows), _lib.ptr(ml), _lib.stream_ptr()), "frame_rows")
    want = np.stack([mc.hop_rows(y[b], lens[b], fl, hop, S) for b in range(B)])
    assert rows.cpu().numpy().tobytes() == want.tobytes()
    assert ml.cpu().tolist() == [n // hop + 1 if n > fl // 2 else 0 for n in lens]


@pytest.mark.parametrize("name,lens", [("ljspeech", [5000, 2047]), ("tiny", [1000, 777])])
def test_op_stft_elementwise(stfts, name, lens):
    so = _lib.load()
    cfg, fl, hop, y, n_max, Tc, S = _ops_case(name, lens, 8)
    B = len(lens)
    rows = np.stack([mc.hop_rows(y[b], lens[b], fl, hop, S) for b in range(B)])
    spec = torch.full((B * S, fl), float("nan"), device="cuda")
    rd = torch.from_numpy(rows).cuda()
    _lib.check(so.ns_mel_op_stft(stfts[name]._h, _lib.ptr(rd), B, S, _lib.ptr(spec), _lib.stream_ptr()), "stft")
    spec = spec.cpu().numpy().reshape(B, S, fl)
    for b in range(B):
        t = lens[b] // hop + 1
        y64, Aabs = mc.spectrum64(y[b, :lens[b]], cfg)
        sh = mc.share(spec[b, :t], mc.packed_columns(y64, fl), mc.packed_columns(mc.C_SUM * Aabs, fl))
        print(f"{name} stft utterance {b}: share of the spectrum gate {sh}")
        assert sh <= 1.0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_op_project_from_a_given_spectrum(stfts, name):
    so = _lib.load()
    cfg = CONFIGS[name]
    fl, hop, n_mel = cfg["filter_length"], cfg["hop_length"], cfg["n_mel_channels"]
    rs = np.random.RandomState(9)
    B, n = 2, 10 * hop + 3
    Tc = n // hop + 1
    S, T = Tc + fl // hop - 1, Tc + 2
    y = rs.standard_normal((B, S, fl + 2))
    y[:, :, fl // 2 + 1] = 0.0   # the two imaginary rows that do not exist
    y[:, :, fl + 1] = 0.0
    spec32 = mc.packed_columns(y, fl).astype(np.float32)
    y = y.astype(np.float32).astype(np.float64)
    lens = [n, n - hop]
    mel = torch.full((B, T, n_mel), float("nan"), device="cuda")
    energy = torch.full((B, T), float("nan"), device="cuda")
    sd, ld = torch.from_numpy(spec32).cuda(), torch.tensor(lens, dtype=torch.long).cuda()
    _lib.check(so.ns_mel_op_project(stfts[name]._h, _lib.ptr(sd), _lib.ptr(ld), B, S, n, T, _lib.ptr(mel), _lib.ptr(energy), _lib.stream_ptr()), "project")
    mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
    mb = stfts[name].mel_basis.numpy()
    for b in range(B):
        t = lens[b] // hop + 1
        r = mc.project64(y[b, :t], np.zeros_like(y[b, :t]), mb)  # an exact spectrum: only the magnitude / sum / log terms of the gates
        sh = mc.shares(mel[b, :t].T, energy[b, :t], r)
        print(f"{name} project utterance {b}: shares {sh}")
        assert sh["mel"] <= 1.0 and sh["energy"] <= 1.0
        assert not mel[b, t:].any() and not energy[b, t:].any()


# ---- poison, padding, determinism, layout -----------------------------------------------------------------------------------
def test_poison_beyond_the_lengths_and_in_the_workspace(stfts):
    st = stfts["ljspeech"]
    rs = np.random.RandomState(10)
    lens = [5000, 513, 2047]
    y, _ = batch_of([random_wave(rs, n) for n in lens])
    clean = st.mel_spectrogram(torch.from_numpy(y).cuda(), lens)
    clean = [t.cpu().numpy().tobytes() for t in clean]
    for poison in (float("nan"), 1e30):
        yp = y.copy()
        for b, n in enumerate(lens):
            yp[b, n:] = poison
        for w in st._ws.values():
            w.view(torch.float32).fill_(poison)
        got = st.mel_spectrogram(torch.from_numpy(yp).cuda(), torch.tensor(lens).cuda())  # device lengths: the same bits
        assert [t.cpu().numpy().tobytes() for t in got] == clean


def test_nan_reaches_exactly_the_frames_that_cover_it(stfts):
    st, cfg = stfts["ljspeech"], mc.LJSPEECH
    fl, hop = cfg["filter_length"], cfg["hop_length"]
    rs = np.random.RandomState(11)
    y = np.stack([random_wave(rs, 6000), random_wave(rs, 6000)])
    pos = 2500
    y[0, pos] = np.nan
    mel, energy = st.mel_spectrogram(torch.from_numpy(y).cuda())
    mel, energy = mel.cpu().numpy(), energy.cpu().numpy()
    frames = np.arange(6000 // hop + 1)
    covered = (frames * hop - fl // 2 <= pos) & (pos < frames * hop + fl // 2)  # away from both edges: no mirrored copy
    assert covered.sum() == fl // hop
    assert (np.isnan(mel[0]).all(0) == covered).all() and (np.isnan(mel[0]).any(0) == covered).all()
    assert (np.isnan(energy[0]) == covered).all()
    assert np.isfinite(mel[1]).all() and np.isfinite(energy[1]).all()


def test_max_mel_len_truncates_and_pads(stfts):
    st, cfg = stfts["ljspeech"], mc.LJSPEECH
    rs = np.random.RandomState(12)
    lens = [5000, 2047]
    y, _ = batch_of([random_wave(rs, n) for n in lens])
    yd = torch.from_numpy(y).cuda()
    full_mel, full_e = (t.cpu().numpy() for t in st.mel_spectrogram(yd, lens))
    assert full_mel.shape[2] == 20
    for T in (7, 20, 33):
        mel, e = st.mel_spectrogram(yd, lens, max_mel_len=T)
        assert tuple(mel.shape) == (2, 80, T) and tuple(e.shape) == (2, T)
        assert st.mel_lens.cpu().tolist() == [20, 8], "the lengths are not clamped to T"
        mel, e = mel.cpu().numpy(), e.cpu().numpy()
        k = min(T, 20)
        assert mel[:, :, :k].tobytes() == full_mel[:, :, :k].tobytes() and e[:, :k].tobytes() == full_e[:, :k].tobytes()
        assert not mel[:, :, k:].any() and not e[:, k:].any()


def test_determinism_and_replicas(stfts):
    st = stfts["ljspeech"]
    rs = np.random.RandomState(13)
    a, b = random_wave(rs, 40000), random_wave(rs, 31000)
    y, lens = batch_of([a, b, a, b, a])  # M = 5 * 160 rows
    yd = torch.from_numpy(y).cuda()
    m1, e1 = (t.cpu().numpy() for t in st.mel_spectrogram(yd, lens))
    m2, e2 = (t.cpu().numpy() for t in st.mel_spectrogram(yd, lens))
    assert m1.tobytes() == m2.tobytes() and e1.tobytes() == e2.tobytes()
    for i, j in ((0, 2), (0, 4), (1, 3)):
        assert m1[i].tobytes() == m1[j].tobytes() and e1[i].tobytes() == e1[j].tobytes()


def test_layout_is_a_view_of_time_major_storage(stfts):
    st = stfts["tiny"]
    mel, energy = st.mel_spectrogram(torch.zeros(2, 1000, device="cuda"))
    assert tuple(mel.shape) == (2, 16, 32) and not mel.is_contiguous()
    tm = mel.transpose(1, 2)
    assert tm.is_contiguous() and tm.data_ptr() == mel.data_ptr() and tm.untyped_storage().data_ptr() == mel.untyped_storage().data_ptr()
    assert st.mel_lens.dtype == torch.long and st.mel_lens.is_cuda


# ---- the chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["tiny", "ljspeech"])
def test_chain_into_teacher_forced_forward_and_loss(stfts, config):
    """wave -> mel_spectrogram -> forward_teacher_forced -> FastSpeech2Loss with no copy of the mel tensor.  The loss reads the alignment
    maps of decoder layers 0-3 (model/loss.py:233-236), which the one-layer `tiny` model does not have: there the chain runs up to the
    teacher-forced tuple and the loss's refusal is what is checked; the four-layer `ljspeech` model carries the finite-loss check."""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    st = stfts["ljspeech"]
    cfg = wl.model_config(config)
    sd = wl.synth_state_dict(cfg, seed=0, frames_per_phoneme=4.0)
    sd.update(wl.synth_aligner_state_dict(cfg, seed=0))
    m = FastSpeech2Align(wl.preprocess_config(), cfg).to("cuda:0").eval()
    m.load_state_dict(sd)
    _, tx, sl, L = wl.synth_inputs(2, 12, seed=2, src_lens=[12, 7])
    rs = np.random.RandomState(14)
    lens = [5000, 3000]
    y, _ = batch_of([random_wave(rs, n) for n in lens])
    mel, energy = st.mel_spectrogram(torch.from_numpy(y).cuda(), lens)
    mels = mel.transpose(1, 2)
    ptr, T = mels.data_ptr(), int(mels.shape[1])
    assert mels.is_contiguous() and ptr % 16 == 0
    texts, src_lens = torch.from_numpy(tx).cuda(), torch.from_numpy(sl).cuda()
    out = m.forward_teacher_forced(None, texts, src_lens, L, mels, st.mel_lens, T)
    assert mels.data_ptr() == ptr == mel.data_ptr()
    d = out[11].cpu().numpy()
    assert d.sum(1).tolist() == [min(n // 256 + 1, T) for n in lens]
    batch = (["a", "b"], ["", ""], None, texts, src_lens, L, mels, st.mel_lens, T, torch.zeros(2, T, device="cuda"), energy)
    loss = FastSpeech2Loss(m.preprocess_config, m.model_config)
    if cfg["transformer"]["decoder_layer"] < 4:
        with pytest.raises(ValueError, match="layers 0-3"):
            loss(batch, out)
        return
    vals = loss(batch, out)
    assert all(bool(torch.isfinite(v)) for v in vals), [float(v) for v in vals]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(stfts):
    st = stfts["ljspeech"]
    y = torch.zeros(2, 3000, device="cuda")
    with pytest.raises(ValueError, match="float32"):
        st.mel_spectrogram(y.double())
    with pytest.raises(ValueError, match="batch of waves"):
        st.mel_spectrogram(y[0])
    with pytest.raises(ValueError, match="batch of waves"):
        st.mel_spectrogram(y[None])
    with pytest.raises(ValueError, match=r"wav_lens\[1\] = 512: a wave must be longer than filter_length / 2 = 512"):
        st.mel_spectrogram(y, [3000, 512])
    with pytest.raises(ValueError, match=r"wav_lens\[0\] = 3001 exceeds"):
        st.mel_spectrogram(y, torch.tensor([3001, 3000]))
    with pytest.raises(ValueError, match="shape"):
        st.mel_spectrogram(y, [3000])
    with pytest.raises(ValueError, match="max_mel_len"):
        st.mel_spectrogram(y, max_mel_len=0)
    with pytest.raises(RuntimeError, match="cuda"):
        st.mel_spectrogram(y.cpu())
    with pytest.raises(ValueError, match="1-D"):
        A.get_mel_from_wav(np.zeros((2, 3000), np.float32), st)
    # device-side lengths cannot be validated without a read: too short -> zero frames, too long -> clamped to n
    mel, energy = st.mel_spectrogram(y + 0.25, torch.tensor([512, 9999]).cuda())
    assert st.mel_lens.cpu().tolist() == [0, 3000 // 256 + 1]
    assert not mel[0].any() and not energy[0].any() and bool(torch.isfinite(mel[1]).all()) and bool((energy[1] > 0).all())
    so, tm = _lib.load(), mel.transpose(1, 2)
    rc = so.ns_mel_forward(st._h, _lib.ptr(y), 3000, _lib.ptr(st.mel_lens), 2, 3000, 0, _lib.ptr(tm), _lib.ptr(energy), _lib.ptr(st.mel_lens), _lib.ptr(y), 16, None)
    assert rc != 0 and "T must be >= 1" in so.ns_last_error().decode()
    rc = so.ns_mel_forward(st._h, _lib.ptr(y), 3000, _lib.ptr(st.mel_lens), 2, 3000, 12, _lib.ptr(tm), _lib.ptr(energy), _lib.ptr(st.mel_lens), _lib.ptr(y), 16, None)
    assert rc != 0 and "workspace too small" in so.ns_last_error().decode()
