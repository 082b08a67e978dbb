#!/usr/bin/env python3
"""Golden vectors for the Griffin-Lim mel-to-wave path — runs ONLY where the reference lives read-only at /root/reference.  It imports
the reference's ``audio.stft.TacotronSTFT`` and ``audio.tools.inv_mel_spec`` with the stub recipe of make_golden_melfront.py (librosa
stubs, ``Tensor.cuda`` as the identity for the duration of the call), sets ``ref._stft_fn = ref.stft_fn`` on the instance (tools.py:28
reads an attribute that does not exist), captures the array ``inv_mel_spec`` hands to ``scipy.io.wavfile.write`` and seeds
``np.random`` before each call.

    python tests/golden/make_golden_griffinlim.py

griffinlim_tiny.npz       256 / 32 / 192, 16 mels: KW = 8, window shorter than the filter
griffinlim_ljspeech.npz   1024 / 256 / 1024, 80 mels: KW = 4
Each holds numbers only: the seeded mels (tests/griffinlim_cpu.fixture_mels), the angles the seed draws, the reference's fp32
magnitudes, window_sum and waves for n_iters 0 and 2, every 41st row of the reference's inverse_basis with float64 checksums, the
float64 waves, and the spectral convergence after 60 iterations of the reference, the float64 restatement and the numpy fp32
restatement.  Asserts max |closed-form inverse basis - reference buffer| <= 1e-16 and records the observed maximum.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))
sys.path.insert(3, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import griffinlim_cpu as gc  # noqa: E402
from make_golden_melfront import _stub_librosa, save  # noqa: E402
from smart_nar_fast_tts_amd import audio as A  # noqa: E402

SC_ITERS = 60


def make(name, cfg, seed):
    import audio.tools as ref_tools
    from audio.audio_processing import window_sumsquare
    from audio.stft import TacotronSTFT

    fl, hop, win = gc.dims(cfg)
    ref = TacotronSTFT(fl, hop, win, cfg["n_mel_channels"], cfg["sampling_rate"], cfg["mel_fmin"], cfg["mel_fmax"])
    ref._stft_fn = ref.stft_fn
    ib_ref = ref.stft_fn.inverse_basis.numpy()
    ib = A.stft_inverse_basis(fl, hop, win)
    assert ib_ref.shape == ib.shape and ib_ref.dtype == ib.dtype
    ib_diff = float(np.abs(ib.astype(np.float64) - ib_ref.astype(np.float64)).max())
    print(f"{name}: max |closed-form inverse basis - reference buffer| = {ib_diff:.3g}")
    assert ib_diff <= 1e-16
    mb = ref.mel_basis.numpy()
    captured = {}
    ref_tools.write = lambda path, sr, audio: captured.update(audio=np.array(audio, copy=True))
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    arrays, sc = {}, {}
    try:
        mels = gc.fixture_mels(cfg, seed)
        for i, mel in enumerate(mels):
            T = mel.shape[1] - 1
            waves = {}
            for n_iters in (0, 2) + ((SC_ITERS,) if i == 0 else ()):
                np.random.seed(seed + i)
                ref_tools.inv_mel_spec(torch.from_numpy(mel), None, ref, n_iters)
                waves[n_iters] = captured["audio"].astype(np.float32)
            np.random.seed(seed + i)
            ang = A.random_angles((1, fl // 2 + 1, T))[0].T.copy()      # time-major [T, bins]
            mag_ref = (torch.mm(ref.spectral_de_normalize(torch.from_numpy(mel)[None]).transpose(1, 2)[0], ref.mel_basis) * 1000).numpy()[:-1]
            mag64, g_mag = gc.mel_to_mag(mel.T, mb)
            print(f"{name} mel {i}: T = {T}, reference fp32 magnitude share of the gate {gc.share(mag_ref, mag64, g_mag):.3g}")
            for n_iters in (0, 2):
                y64, g = gc.griffin_lim(mag64, ang, n_iters, cfg)
                print(f"{name} mel {i}: n_iters {n_iters}: reference fp32 share of the gate {gc.share(waves[n_iters], y64, g):.3g}, "
                      f"relative distance {np.abs(waves[n_iters] - y64).max() / np.abs(y64).max():.3g}")
                arrays[f"wave{i}_it{n_iters}"] = waves[n_iters]
                arrays[f"wave{i}_it{n_iters}_f64"] = y64
            arrays.update({f"mel{i}": mel, f"angles{i}": ang, f"mag{i}": mag_ref})
            if i == 0:
                y64, _ = gc.griffin_lim(mag64, ang, SC_ITERS, cfg, with_gate=False)
                y32, _ = gc.griffin_lim(mag64.astype(np.float32), ang, SC_ITERS, cfg, dt=np.float32, with_gate=False)
                sc = dict(iters=SC_ITERS, sc_f64=gc.spectral_convergence(y64, mag64, cfg), sc_np32=gc.spectral_convergence(y32, mag64, cfg),
                          sc_reference=gc.spectral_convergence(waves[SC_ITERS], mag64, cfg),
                          drift_np32=float(np.abs(y32 - y64).max() / np.abs(y64).max()))
                print(f"{name}: {sc}")
                arrays["window_sum0"] = window_sumsquare("hann", T, hop_length=hop, win_length=win, n_fft=fl, dtype=np.float32)
    finally:
        torch.Tensor.cuda = cuda
    rows = np.arange(0, ib.shape[0], 41)
    arrays.update(basis_rows=rows, inverse_basis_rows=ib_ref[rows, 0, :], mel_basis=mb)
    meta = dict(config=cfg, seed=seed, n_mels=len(mels), sc=sc, inverse_basis_max_diff=ib_diff,
                inverse_basis_sum=float(ib_ref.astype(np.float64).sum()), inverse_basis_abs_sum=float(np.abs(ib_ref.astype(np.float64)).sum()))
    save(name, meta, **arrays)


if __name__ == "__main__":
    _stub_librosa()
    make("griffinlim_tiny", gc.TINY, 21)
    make("griffinlim_ljspeech", gc.LJSPEECH, 22)
