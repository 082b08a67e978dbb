#!/usr/bin/env python3
"""Golden vectors for the wave-to-mel front end — runs ONLY where the reference lives read-only at /root/reference.  It imports the
reference's ``audio.stft.TacotronSTFT`` and ``audio.tools.get_mel_from_wav`` with the stub-module recipe of make_golden_aligner.py:
``librosa`` is not installed, so ``librosa.util.pad_center`` / ``tiny`` / ``normalize`` are stubbed and ``librosa.filters.mel`` is the
package's Slaney restatement (audio.slaney_mel_basis — NOT librosa's own output); ``Tensor.cuda`` is the identity for the duration of
the call (stft.py:68-72 moves the convolution to a GPU and back).

    python tests/golden/make_golden_melfront.py

melfront_tiny.npz       256 / 32 / 192, 16 mels, 16 kHz: win_length < filter_length (the centre pad matters), KW = 8; the reference's
                        forward_basis buffer in full
melfront_ljspeech.npz   1024 / 256 / 1024, 80 mels, 22050 Hz, 0-8000 Hz; every 41st row of forward_basis plus a float64 checksum
                        (4 MB does not belong in git)
Each holds numbers only: the seeded waves (tests/melfront_cpu.fixture_waves), the reference's fp32 mel / energy and the float64
values and gates of tests/melfront_cpu.  Asserts that the package's basis equals the reference's buffer bit for bit.
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import melfront_cpu as mc  # noqa: E402
from smart_nar_fast_tts_amd import audio as A  # noqa: E402


def _stub_librosa():
    lib, util, filters = types.ModuleType("librosa"), types.ModuleType("librosa.util"), types.ModuleType("librosa.filters")
    util.pad_center = lambda data, size, **kw: A.pad_center(np.asarray(data), size)
    util.tiny = lambda x: np.finfo(np.asarray(x).dtype if np.issubdtype(np.asarray(x).dtype, np.floating) else np.float32).tiny
    util.normalize = lambda x, **kw: x
    filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: A.slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax)
    lib.util, lib.filters = util, filters
    sys.modules.update({"librosa": lib, "librosa.util": util, "librosa.filters": filters})


def save(name, meta, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}  {size / 1024:.0f} KiB")
    assert size < (1 << 20), "a committed file must stay below 1 MiB"


def make(name, cfg, seed, basis_rows):
    from audio.stft import TacotronSTFT  # the reference classes
    from audio.tools import get_mel_from_wav

    ref = TacotronSTFT(cfg["filter_length"], cfg["hop_length"], cfg["win_length"], cfg["n_mel_channels"], cfg["sampling_rate"],
                       cfg["mel_fmin"], cfg["mel_fmax"])
    fb_ref = ref.stft_fn.forward_basis.numpy()
    fb = A.stft_forward_basis(cfg["filter_length"], cfg["win_length"])
    assert fb_ref.shape == fb.shape and fb_ref.dtype == fb.dtype and np.array_equal(fb_ref.view(np.uint32), fb.view(np.uint32)), \
        "the package's forward_basis differs from the reference's buffer"
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    arrays, worst = {}, {"mel": 0.0, "energy": 0.0}
    try:
        waves = mc.fixture_waves(cfg, seed)
        for i, w in enumerate(waves):
            mel32, e32 = get_mel_from_wav(w, ref)
            r = mc.reference64(w, cfg)
            sh = mc.shares(mel32, e32, r)
            print(f"{name} wave {i}: n = {len(w)}, T = {mel32.shape[1]}, reference fp32 shares of the gates {sh}")
            worst = {k: max(worst[k], sh[k]) for k in worst}
            arrays.update({f"wave{i}": w, f"mel{i}": mel32, f"energy{i}": e32, f"mel{i}_f64": r[0], f"energy{i}_f64": r[1]})
    finally:
        torch.Tensor.cuda = cuda
    rows = np.arange(fb.shape[0]) if basis_rows is None else np.arange(0, fb.shape[0], basis_rows)
    arrays.update(basis_rows=rows, forward_basis_rows=fb_ref[rows, 0, :], mel_basis=ref.mel_basis.numpy())
    meta = dict(config=cfg, seed=seed, n_waves=len(waves), reference_shares=worst,
                forward_basis_sum=float(fb_ref.astype(np.float64).sum()), forward_basis_abs_sum=float(np.abs(fb_ref.astype(np.float64)).sum()))
    save(name, meta, **arrays)


if __name__ == "__main__":
    _stub_librosa()
    make("melfront_tiny", mc.TINY, 11, None)
    make("melfront_ljspeech", mc.LJSPEECH, 12, 41)
