"""Wave-to-mel front end: the reference's ``TacotronSTFT.mel_spectrogram`` and ``Audio.tools.get_mel_from_wav``
(audio/stft.py:52-81,159-178, audio/tools.py:8-15, audio/audio_processing.py:85-91) as three HIP launches on the caller's
stream (csrc/melfront.hip around one Conv1D-as-GEMM; ``ns_mel_*`` in include/nar_fs2.h).  It produces the ``mels`` that
``align()``, ``forward_teacher_forced()`` and ``FastSpeech2Loss`` consume, without a host round trip.

The other half of the reference's ``audio/`` package lives here too: ``STFT`` (``transform`` / ``inverse``, audio/stft.py:15-127),
``griffin_lim`` (audio/audio_processing.py:66-82), ``mel_to_wave`` / ``inv_mel_spec`` (audio/tools.py:18-34) over ``ns_gl_*``
(csrc/griffinlim.hip): a mel becomes a waveform without any trained weights.

DEVIATIONS from the reference, both documented in DESIGN.md §15:
  * the reference asserts ``min >= -1`` and ``max <= 1`` (a host read, stft.py:169-170); here the kernel clips, which is the
    identity on anything the assertion lets through and what ``get_mel_from_wav`` does ahead of the call (tools.py:9);
  * the mel filter bank restates the published Slaney formula (librosa's defaults ``htk=False, norm="slaney"``) — librosa is not a
    dependency, and the restatement has NOT been compared with librosa's output; ``mel_basis=`` / ``load_state_dict`` take
    librosa's own matrix."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._handle import DeviceModule, host_f32

CLIP_VAL = 1e-5  # dynamic_range_compression's default, the only value the reference uses (audio_processing.py:85)


# ---- the two bases, numpy only ---------------------------------------------------------------------------------------------
def hann_periodic(win_length: int) -> np.ndarray:
    """float64 periodic Hann window: ``scipy.signal.get_window("hann", win_length, fftbins=True)`` (stft.py:41)."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)


def pad_center(w: np.ndarray, size: int) -> np.ndarray:
    """``librosa.util.pad_center``: zeros on both sides, the extra one (odd difference) on the right (stft.py:42)."""
    lpad = (size - len(w)) // 2
    return np.pad(w, (lpad, size - len(w) - lpad))


def stft_forward_basis(filter_length: int, win_length: int) -> np.ndarray:
    """``STFT.forward_basis`` [filter_length + 2, 1, filter_length] exactly as stft.py:26-49 builds it: the DFT matrix in float64,
    real rows over imaginary rows, rounded to fp32, then multiplied IN fp32 by the fp32 window centre-padded to filter_length."""
    fourier = np.fft.fft(np.eye(filter_length))
    cutoff = filter_length // 2 + 1
    basis = np.vstack([np.real(fourier[:cutoff]), np.imag(fourier[:cutoff])]).astype(np.float32)
    window = pad_center(hann_periodic(win_length), filter_length).astype(np.float32)
    return np.ascontiguousarray((basis * window[None, :])[:, None, :], dtype=np.float32)


def stft_inverse_basis(filter_length: int, hop_length: int, win_length: int) -> np.ndarray:
    """``STFT.inverse_basis`` [filter_length + 2, 1, filter_length] (stft.py:25,34-36,47).  The reference takes
    ``pinv(scale * fourier_basis).T`` with ``scale = filter_length / hop_length`` through LAPACK, whose last bits depend on the
    machine; here it is the closed form.  The real-DFT matrix has two zero rows (im_0, im_{N/2}) and is invertible without them, so its
    pseudo-inverse is the inverse real DFT: row re_k = w_k cos(2 pi k n / N) / scale, row im_k = -w_k sin(2 pi k n / N) / scale,
    w_0 = w_{N/2} = 1 / N, otherwise 2 / N, and the rows im_0 and im_{N/2} exactly zero (the reference holds ~1e-18 there).  Rounded to
    fp32, then multiplied IN fp32 by the fp32 centre-padded window, as stft.py:43-47 does."""
    n = filter_length
    fourier = np.fft.fft(np.eye(n))
    cutoff = n // 2 + 1
    w = np.full(cutoff, 2.0 / n)
    w[0] = w[n // 2] = 1.0 / n
    scale = filter_length / hop_length
    basis = np.vstack([np.real(fourier[:cutoff]), np.imag(fourier[:cutoff])]) * np.concatenate([w, w])[:, None] / scale
    basis[cutoff] = 0.0
    basis[cutoff + n // 2] = 0.0
    window = pad_center(hann_periodic(win_length), n).astype(np.float32)
    return np.ascontiguousarray((basis.astype(np.float32) * window[None, :])[:, None, :], dtype=np.float32)


def window_sumsquare(n_frames: int, hop_length: int, win_length: int, n_fft: int) -> np.ndarray:
    """``window_sumsquare("hann", n_frames, hop_length, win_length, n_fft, dtype=np.float32)`` (audio_processing.py:7-63) including its
    arithmetic: an fp32 accumulator; every ``+=`` adds a float64 squared-window value and rounds once to fp32, frames ascending."""
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=np.float32)
    win_sq = pad_center(hann_periodic(win_length) ** 2, n_fft)
    for i in range(n_frames):
        sample = i * hop_length
        x[sample:min(n, sample + n_fft)] += win_sq[:max(0, min(n_fft, n - sample))]
    return x


def hz_to_mel(f):
    """Slaney's Auditory Toolbox scale (M. Slaney, "Auditory Toolbox, version 2", Interval Research Corp. TR 1998-010, mfcc.m):
    linear below 1 kHz at 200/3 Hz per mel, logarithmic above with 27 steps per factor 6.4."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_band_edges(n_mels: int, fmin: float, fmax: float) -> np.ndarray:
    """The n_mels + 2 band edges in Hz: equal steps on the Slaney mel scale between fmin and fmax."""
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))


def slaney_mel_basis(sampling_rate, filter_length, n_mel_channels, mel_fmin=0.0, mel_fmax=None, normalize=True) -> np.ndarray:
    """[n_mel, filter_length / 2 + 1] fp32 triangular filter bank, the arguments of ``librosa_mel_fn(sr, n_fft, n_mels, fmin, fmax)``
    (stft.py:145-147) with librosa's defaults ``htk=False, norm="slaney"``: triangle m rises from edge m to edge m + 1 and falls to
    edge m + 2 (Slaney 1998, mfcc.m), scaled by 2 / (f_{m+2} - f_m) so that every filter has unit area in Hz.  Computed in float64,
    rounded to fp32 once.  NOT compared with librosa's own output (it is not installed where this was written)."""
    fmax = float(sampling_rate) / 2.0 if mel_fmax is None else float(mel_fmax)
    freqs = np.linspace(0.0, float(sampling_rate) / 2.0, filter_length // 2 + 1)
    edges = mel_band_edges(n_mel_channels, float(mel_fmin or 0.0), fmax)
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    if normalize:
        weights = weights * (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return np.ascontiguousarray(weights, dtype=np.float32)


def config_struct(filter_length, hop_length, win_length, n_mel, clip_val=CLIP_VAL) -> _lib.NsMelConfig:
    c = _lib.NsMelConfig()
    c.filter_length, c.hop_length, c.win_length, c.n_mel = int(filter_length), int(hop_length), int(win_length), int(n_mel)
    c.clip_val = float(clip_val)
    return c


SPEC_FROM_MEL_SCALING = 1000.0  # the literal of tools.py:22


def gl_config_struct(filter_length, hop_length, win_length, n_mel, scaling=SPEC_FROM_MEL_SCALING) -> _lib.NsGlConfig:
    c = _lib.NsGlConfig()
    c.filter_length, c.hop_length, c.win_length, c.n_mel = int(filter_length), int(hop_length), int(win_length), int(n_mel)
    c.spec_from_mel_scaling = float(scaling)
    return c


def _device_lens(lens, B, dev, what, refuse, data="the data", one_message=False):
    """Per-utterance lengths as a device int64 [B].  A device tensor is checked for dtype, shape and device only: its values cannot
    be validated without a read and are clamped by the kernels.  Host values (a sequence, an array, a CPU tensor) are validated one
    by one: ``refuse(v)`` returns what follows ``"{what}[b] = v"`` in the ValueError, or None.  ``data`` names the tensor the lengths
    belong to; ``one_message``: ``STFT.transform``'s wording, one ValueError for dtype, shape and device together."""
    if torch.is_tensor(lens) and lens.is_cuda:
        shaped = lens.dtype == torch.long and tuple(lens.shape) == (B,)
        if one_message:
            if not shaped or lens.device != dev:
                raise ValueError(f"device {what} must be int64 [{B}] on {dev}, got {lens.dtype} {tuple(lens.shape)} on {lens.device}")
        elif lens.device != dev:
            raise RuntimeError(f"{what} is on {lens.device}, {data} on {dev}")
        elif not shaped:
            raise ValueError(f"device {what} must be int64 [{B}], got {lens.dtype} {tuple(lens.shape)}")
        return lens.contiguous()
    host = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens)
    if one_message:
        if host.dtype.kind not in "iu" or host.shape != (B,):
            raise ValueError(f"{what} must be {B} integers, got {host.dtype} {host.shape}")
    elif host.dtype.kind not in "iu":
        raise ValueError(f"{what} must hold integers, got {host.dtype}")
    elif host.shape != (B,):
        raise ValueError(f"{what} must have shape ({B},), got {host.shape}")
    for b, v in enumerate(host.tolist()):
        why = refuse(v)
        if why:
            raise ValueError(f"{what}[{b}] = {v}{why}")
    return torch.as_tensor(host.astype(np.int64)).to(dev)


class TacotronSTFT(DeviceModule):
    """Drop-in for the reference's ``TacotronSTFT(filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin,
    mel_fmax)`` on the MI355X.  ``mel_basis=`` hands in a filter bank (e.g. librosa's, from a saved ``state_dict()``) in place of the
    Slaney restatement.

    ``mel_spectrogram(y, wav_lens=None, max_mel_len=None)`` takes a BATCH of variable-length waves and nothing in it synchronises.
    Device-side ``wav_lens`` cannot be validated without a read; for them the kernels' rule holds: a length is clamped to
    ``[0, n]`` and an utterance of ``filter_length / 2`` samples or fewer (which the reference's reflect pad refuses) has zero
    frames — ``mel`` and ``energy`` all zeros, ``mel_lens`` 0.

    ``stft_fn`` is the reference's attribute of that name: an ``audio.STFT`` of the same configuration (and this mel basis), created
    on first use; ``mel_to_wave`` / ``inv_mel_spec`` run Griffin-Lim through it.

    Threading: one instance serves one host thread at a time; several HIP streams from that thread are fine (one workspace each)."""

    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax, mel_basis=None):
        self.filter_length, self.hop_length, self.win_length = int(filter_length), int(hop_length), int(win_length)
        self.n_mel_channels, self.sampling_rate = int(n_mel_channels), sampling_rate
        self.mel_fmin, self.mel_fmax = mel_fmin, mel_fmax
        self._open("ns_mel", config_struct(filter_length, hop_length, win_length, n_mel_channels), "TacotronSTFT")
        if mel_basis is None:
            mel_basis = slaney_mel_basis(sampling_rate, self.filter_length, self.n_mel_channels, mel_fmin, mel_fmax)
        self._stft_fn = None
        self.mel_lens = None
        self.load_state_dict({"stft_fn.forward_basis": stft_forward_basis(self.filter_length, self.win_length), "mel_basis": mel_basis})

    @classmethod
    def from_config(cls, preprocess_config: dict, mel_basis=None):
        """The arguments the reference's preprocessor passes (preprocessor/preprocessor.py:39-47)."""
        p = preprocess_config["preprocessing"]
        return cls(p["stft"]["filter_length"], p["stft"]["hop_length"], p["stft"]["win_length"], p["mel"]["n_mel_channels"],
                   p["audio"]["sampling_rate"], p["mel"]["mel_fmin"], p["mel"]["mel_fmax"], mel_basis=mel_basis)

    # ---- nn.Module-shaped surface (eval / train / to / cuda / state_dict: _handle.DeviceModule) ------
    @property
    def stft_fn(self) -> "STFT":
        """The reference's ``TacotronSTFT.stft_fn`` (stft.py:144), with this module's forward basis and mel basis."""
        if self._stft_fn is None:
            self._stft_fn = STFT(self.filter_length, self.hop_length, self.win_length, n_mel_channels=self.n_mel_channels,
                                 mel_basis=self._sd["mel_basis"], sampling_rate=self.sampling_rate)
            self._stft_fn.load_state_dict({"forward_basis": self._sd["stft_fn.forward_basis"]})
        if self._device is not None:
            self._stft_fn.to(self._device)
        return self._stft_fn

    @property
    def mel_basis(self) -> torch.Tensor:
        return torch.from_numpy(self._sd["mel_basis"].copy())

    @property
    def forward_basis(self) -> torch.Tensor:
        return torch.from_numpy(self._sd["stft_fn.forward_basis"].copy())

    def load_state_dict(self, state_dict, strict: bool = True):
        """Keys of the reference module: ``stft_fn.forward_basis``, ``mel_basis`` (either may be absent: the current one stays) and
        ``stft_fn.inverse_basis`` (accepted, ignored).  Unknown keys and shape mismatches raise before anything is replaced."""
        new, errors = dict(self._sd or {}), []
        for k, t in dict(state_dict).items():
            a = host_f32(t)
            err = self._h.check_weight(k, a)
            if err:
                errors.append(err)
            elif k != "stft_fn.inverse_basis":
                new[k] = a
        if errors:
            raise RuntimeError("load_state_dict: " + "; ".join(errors))
        self._stft_fn = None  # rebuilt from the new bases on next use
        return self._loaded(new)

    # ---- forward -------------------------------------------------------------------------------
    def frames(self, n: int) -> int:
        """Frames of a wave of ``n`` samples: ``n // hop_length + 1``."""
        return int(self._lib.ns_mel_frames(int(n), self.hop_length))

    def mel_spectrogram(self, y, wav_lens=None, max_mel_len=None):
        """``y`` [B, n] fp32 on the GPU; ``wav_lens`` a host sequence, a CPU tensor or a device int64 tensor (default: ``n`` for every
        row).  Returns ``(mel, energy)``: ``mel`` [B, n_mel, T] as in the reference — a ``transpose(1, 2)`` VIEW of time-major storage,
        so ``mel.transpose(1, 2)`` is the contiguous [B, T, n_mel] that ``align()`` / ``forward_teacher_forced()`` take — and ``energy``
        [B, T]; ``T = n // hop + 1`` unless ``max_mel_len`` is given (frames beyond it are dropped, frames up to it zero-filled).
        Frames at and beyond an utterance's own length are zeros.  ``self.mel_lens``: the device int64 lengths of this call."""
        if not torch.is_tensor(y):
            raise ValueError(f"y must be a tensor, got {type(y).__name__}")
        if y.dim() != 2:
            raise ValueError(f"y must be [B, n] (a batch of waves), got {tuple(y.shape)}")
        if y.dtype != torch.float32:
            raise ValueError(f"y must be float32, got {y.dtype}")
        if not y.is_cuda:
            raise RuntimeError("y must live on the MI355X (cuda) device; there is no CPU path")
        B, n = int(y.shape[0]), int(y.shape[1])
        T = self.frames(n) if max_mel_len is None else int(max_mel_len)
        if T < 1:
            raise ValueError(f"max_mel_len must be >= 1, got {max_mel_len}")
        dev = y.device
        half = self.filter_length // 2

        def refuse(v):
            if v <= half:
                return f": a wave must be longer than filter_length / 2 = {half} samples (the reflect pad, stft.py:60-64)"
            return f" exceeds the {n} samples of y" if v > n else None

        lens = _device_lens([n] * B if wav_lens is None else wav_lens, B, dev, "wav_lens", refuse, data="y")
        self.to(dev)
        y = y.contiguous()
        with torch.cuda.device(dev):
            mel = torch.empty(B, T, self.n_mel_channels, dtype=torch.float32, device=dev)
            energy = torch.empty(B, T, dtype=torch.float32, device=dev)
            mel_lens = torch.empty(B, dtype=torch.long, device=dev)
            if B > 0:
                stream = torch.cuda.current_stream(dev).cuda_stream
                nbytes = int(self._lib.ns_mel_ws_bytes(self._h, B, n))
                ws = self._ws.take(self._device, nbytes, stream)
                _lib.check(self._lib.ns_mel_forward(self._h, _lib.ptr(y), n, _lib.ptr(lens), B, n, T, _lib.ptr(mel), _lib.ptr(energy),
                                                    _lib.ptr(mel_lens), _lib.ptr(ws), ws.numel(), C.c_void_p(stream)), "ns_mel_forward")
        self.mel_lens = mel_lens
        return mel.transpose(1, 2), energy

    __call__ = mel_spectrogram


def get_mel_from_wav(audio, _stft: TacotronSTFT):
    """The ``audio/tools.py:8-15`` surface: a 1-D numpy / tensor wave -> numpy ``mel`` [n_mel, T] and ``energy`` [T]; one host read at
    the end.  (The clip of tools.py:9 happens in the kernel.)"""
    a = audio if torch.is_tensor(audio) else torch.as_tensor(np.asarray(audio, dtype=np.float32))
    if a.dim() != 1:
        raise ValueError(f"audio must be a 1-D wave, got shape {tuple(a.shape)}")
    dev = a.device if a.is_cuda else (_stft._device or torch.device("cuda", torch.cuda.current_device()))
    mel, energy = _stft.mel_spectrogram(a.to(device=dev, dtype=torch.float32).unsqueeze(0))
    return mel[0].cpu().numpy().astype(np.float32), energy[0].cpu().numpy().astype(np.float32)


# ---- Griffin-Lim: mel -> wave without trained weights (ns_gl_*) ------------------------------------------------------
def _as_long_lens(lens, B, T, dev, fl, hop, drop, what):
    """Per-utterance frame counts for Griffin-Lim.  Host values too short for the reflect pad of the loop's transform (stft.py:60-64)
    or beyond the T frames given are refused; on the device a too-short utterance gives a zero wave of length 0."""
    def refuse(v):
        if v > T:
            return f" exceeds the {T} frames given"
        if hop * (v - drop - 1) <= fl // 2:
            return (f": too short — Griffin-Lim's signal of hop_length * (frames - 1) samples must be longer than "
                    f"filter_length / 2 = {fl // 2} (the reflect pad, stft.py:60-64)")

    return _device_lens([T] * B if lens is None else lens, B, dev, what, refuse)


def _check_device_f32(t, what, ndim):
    if not torch.is_tensor(t):
        raise ValueError(f"{what} must be a tensor, got {type(t).__name__}")
    if t.dim() != ndim:
        raise ValueError(f"{what} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the MI355X (cuda) device; there is no CPU path")


class STFT(DeviceModule):
    """The reference's ``STFT(filter_length, hop_length, win_length, window="hann")`` (audio/stft.py:15-127) on the MI355X.
    ``transform`` and ``inverse`` take and return the reference's layouts, for batches of variable-length utterances (``lens``).
    ``n_mel_channels`` / ``mel_basis`` (not reference arguments) give the handle the mel basis ``mel_to_wave`` needs;
    ``TacotronSTFT.stft_fn`` passes its own.  ``state_dict()`` carries the reference module's two buffers.

    DEVIATION: ``inverse_basis`` is the closed form of ``stft_inverse_basis`` rather than LAPACK's ``pinv`` (they differ by ~1e-18)."""

    def __init__(self, filter_length, hop_length, win_length, window="hann", n_mel_channels=None, mel_basis=None, sampling_rate=None):
        if window != "hann":
            raise ValueError(f"only the reference's default window 'hann' is built, got {window!r}")
        self.filter_length, self.hop_length, self.win_length, self.window = int(filter_length), int(hop_length), int(win_length), window
        self.cutoff = self.filter_length // 2 + 1
        self.sampling_rate = sampling_rate
        if (n_mel_channels is None) != (mel_basis is None):
            raise ValueError("n_mel_channels and mel_basis come together")
        # a bare STFT has no mel stage: the smallest legal n_mel, and no mel_basis is ever loaded
        self._open("ns_gl", gl_config_struct(filter_length, hop_length, win_length, 4 if n_mel_channels is None else n_mel_channels), "STFT")
        self.n_mel_channels = None if n_mel_channels is None else int(n_mel_channels)
        self._mel_basis = None if mel_basis is None else np.ascontiguousarray(mel_basis, dtype=np.float32)
        if self._mel_basis is not None and (self._mel_basis.ndim != 2 or self._h.check_weight("mel_basis", self._mel_basis)):
            raise RuntimeError(f"STFT: mel_basis must be [{self.n_mel_channels}, {self.cutoff}], got {self._mel_basis.shape}")
        self.wave_lens = None
        self.frame_lens = None
        self.load_state_dict({"forward_basis": stft_forward_basis(self.filter_length, self.win_length),
                              "inverse_basis": stft_inverse_basis(self.filter_length, self.hop_length, self.win_length)})

    @property
    def forward_basis(self) -> torch.Tensor:
        return torch.from_numpy(self._sd["forward_basis"].copy())

    @property
    def inverse_basis(self) -> torch.Tensor:
        return torch.from_numpy(self._sd["inverse_basis"].copy())

    def load_state_dict(self, state_dict, strict: bool = True):
        """Keys of the reference module: ``forward_basis``, ``inverse_basis`` (either may be absent: the current one stays)."""
        new, errors = dict(self._sd or {}), []
        for k, t in dict(state_dict).items():
            a = host_f32(t)
            err = self._h.check_weight("stft_fn." + k, a) if k in ("forward_basis", "inverse_basis") else f"unexpected key '{k}'"
            if err:
                errors.append(err)
            else:
                new[k] = a
        if errors:
            raise RuntimeError("load_state_dict: " + "; ".join(errors))
        return self._loaded(new)

    def _weights(self):
        """The library's names: the two bases under ``stft_fn.``, and ``mel_basis`` when this STFT was given one."""
        weights = {"stft_fn." + k: a for k, a in self._sd.items()}
        if self._mel_basis is not None:
            weights["mel_basis"] = self._mel_basis
        return weights

    def _ws_for(self, B, T, dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        nbytes = int(self._lib.ns_gl_ws_bytes(self._h, B, T))
        return self._ws.take(self._device, nbytes, stream), stream

    # ---- the reference's three methods -------------------------------------------------------------
    def transform(self, input_data, lens=None):
        """``input_data`` [B, n] fp32 on the GPU, ``lens`` the utterances' sample counts (host or device; default ``n``).  Returns
        ``(magnitude, phase)`` [B, cutoff, T], ``T = n // hop + 1``, as transpose views of time-major storage; zeros at frames beyond an
        utterance's own.  No clip (stft.py:52-81)."""
        _check_device_f32(input_data, "input_data", 2)
        B, n = int(input_data.shape[0]), int(input_data.shape[1])
        dev, half = input_data.device, self.filter_length // 2
        T = n // self.hop_length + 1

        def refuse(v):
            if v <= half or v > n:
                return (f": a signal must be longer than filter_length / 2 = {half} samples (the reflect pad, "
                        f"stft.py:60-64) and within the {n} given")

        wl = _device_lens([n] * B if lens is None else lens, B, dev, "lens", refuse, one_message=True)
        self.to(dev)
        x = input_data.contiguous()
        with torch.cuda.device(dev):
            mag = torch.empty(B, T, self.cutoff, dtype=torch.float32, device=dev)
            ph = torch.empty(B, T, self.cutoff, dtype=torch.float32, device=dev)
            if B > 0:
                ws, stream = self._ws_for(B, T, dev)
                _lib.check(self._lib.ns_gl_transform(self._h, _lib.ptr(x), n, _lib.ptr(wl), B, n, T, _lib.ptr(mag), _lib.ptr(ph), _lib.ptr(ws),
                                                     ws.numel(), C.c_void_p(stream)), "ns_gl_transform")
        return mag.transpose(1, 2), ph.transpose(1, 2)

    def _griffin_lim(self, mag_t, ang_t, lens, n_iters, mel=False):
        """``mag_t`` time-major magnitudes [B, T, cutoff] (or, ``mel=True``, log-mel [B, T + 1, n_mel]); ``ang_t`` [B, T, cutoff]."""
        B, T = int(ang_t.shape[0]), int(ang_t.shape[1])
        dev = ang_t.device
        self.to(dev)
        n = self.hop_length * (T - 1)
        with torch.cuda.device(dev):
            wave = torch.empty(B, n, dtype=torch.float32, device=dev)
            wl = torch.empty(B, dtype=torch.long, device=dev)
            if B > 0:
                ws, stream = self._ws_for(B, T + 1, dev)
                fn, Tin = (self._lib.ns_gl_forward, T + 1) if mel else (self._lib.ns_gl_forward_mag, T)
                _lib.check(fn(self._h, _lib.ptr(mag_t), _lib.ptr(lens), B, Tin, _lib.ptr(ang_t), int(n_iters), _lib.ptr(wave), n, _lib.ptr(wl),
                              _lib.ptr(ws), ws.numel(), C.c_void_p(stream)), "ns_gl_forward")
        self.wave_lens = wl
        return wave

    def inverse(self, magnitude, phase, lens=None):
        """``magnitude``, ``phase`` [B, cutoff, T] fp32 on the GPU (a transpose view of time-major storage is taken as it is);
        ``lens`` the utterances' frame counts.  Returns [B, 1, hop * (T - 1)] (stft.py:83-122); ``self.wave_lens``: device lengths."""
        _check_device_f32(magnitude, "magnitude", 3)
        _check_device_f32(phase, "phase", 3)
        if tuple(magnitude.shape) != tuple(phase.shape) or magnitude.shape[1] != self.cutoff:
            raise ValueError(f"magnitude and phase must both be [B, {self.cutoff}, T], got {tuple(magnitude.shape)} and {tuple(phase.shape)}")
        B, T = int(magnitude.shape[0]), int(magnitude.shape[2])
        if T < 2:
            raise ValueError(f"at least 2 frames are needed, got {T}")
        fl_lens = _as_long_lens(lens, B, T, magnitude.device, self.filter_length, self.hop_length, 0, "lens")
        return self._griffin_lim(magnitude.transpose(1, 2).contiguous(), phase.transpose(1, 2).contiguous(), fl_lens, 0).unsqueeze(1)

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)

    __call__ = forward


def random_angles(shape) -> np.ndarray:
    """The start of audio_processing.py:74-75, drawn on the host exactly as the reference draws it (``np.random.seed`` reproduces it)."""
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def griffin_lim(magnitudes, stft_fn: STFT, n_iters=30, angles=None, lens=None):
    """``griffin_lim(magnitudes, stft_fn, n_iters)`` (audio_processing.py:66-82): ``magnitudes`` [B, cutoff, T] fp32 on the GPU ->
    ``signal`` [B, hop * (T - 1)].  ``angles`` (same shape, device) replaces the host-drawn random start; ``lens``: frame counts.
    Nothing is read back; the loop evaluates no angle."""
    _check_device_f32(magnitudes, "magnitudes", 3)
    if magnitudes.shape[1] != stft_fn.cutoff:
        raise ValueError(f"magnitudes must be [B, {stft_fn.cutoff}, T], got {tuple(magnitudes.shape)}")
    B, T = int(magnitudes.shape[0]), int(magnitudes.shape[2])
    if T < 2:
        raise ValueError(f"at least 2 frames are needed, got {T}")
    if n_iters < 0:
        raise ValueError(f"n_iters must be >= 0, got {n_iters}")
    dev = magnitudes.device
    fl_lens = _as_long_lens(lens, B, T, dev, stft_fn.filter_length, stft_fn.hop_length, 0, "lens")
    if angles is None:
        ang_t = torch.from_numpy(random_angles(tuple(magnitudes.shape))).transpose(1, 2).contiguous().to(dev)
    else:
        _check_device_f32(angles, "angles", 3)
        if tuple(angles.shape) != tuple(magnitudes.shape):
            raise ValueError(f"angles must have the shape of magnitudes {tuple(magnitudes.shape)}, got {tuple(angles.shape)}")
        ang_t = angles.transpose(1, 2).contiguous()
    return stft_fn._griffin_lim(magnitudes.transpose(1, 2).contiguous(), ang_t, fl_lens, n_iters)


def mel_to_wave(mel, _stft: TacotronSTFT, griffin_iters=60, mel_lens=None, angles=None):
    """The batched, file-less core of ``inv_mel_spec`` (tools.py:18-29): log-mel ``mel`` [B, n_mel, T] on the GPU (the transpose view
    ``mel_spectrogram`` returns is taken without a copy) -> ``(wave [B, hop * (T - 2)], wave_lens)``.  The last frame of every
    utterance is dropped, as tools.py:28 does; ``angles`` [B, cutoff, T - 1] (device) replaces the random start."""
    _check_device_f32(mel, "mel", 3)
    if mel.shape[1] != _stft.n_mel_channels:
        raise ValueError(f"mel must be [B, {_stft.n_mel_channels}, T], got {tuple(mel.shape)}")
    B, T = int(mel.shape[0]), int(mel.shape[2])
    if T < 3:
        raise ValueError(f"at least 3 mel frames are needed, got {T}")
    if griffin_iters < 0:
        raise ValueError(f"griffin_iters must be >= 0, got {griffin_iters}")
    dev = mel.device
    lens = _as_long_lens(mel_lens, B, T, dev, _stft.filter_length, _stft.hop_length, 1, "mel_lens")
    _stft.to(dev)
    fn = _stft.stft_fn
    shape = (B, fn.cutoff, T - 1)
    if angles is None:
        ang_t = torch.from_numpy(random_angles(shape)).transpose(1, 2).contiguous().to(dev)
    else:
        _check_device_f32(angles, "angles", 3)
        if tuple(angles.shape) != shape:
            raise ValueError(f"angles must be {shape}, got {tuple(angles.shape)}")
        ang_t = angles.transpose(1, 2).contiguous()
    wave = fn._griffin_lim(mel.transpose(1, 2).contiguous(), ang_t, lens, griffin_iters, mel=True)
    return wave, fn.wave_lens


def inv_mel_spec(mel, out_filename, _stft: TacotronSTFT, griffin_iters=60):
    """``inv_mel_spec(mel, out_filename, _stft, griffin_iters)`` (tools.py:18-34): one [n_mel, T] log-mel -> a float32 wav file.  One
    host read at the end.  (The reference reads ``_stft._stft_fn``, which does not exist; ``stft_fn`` is what it means.)"""
    from scipy.io.wavfile import write

    m = mel if torch.is_tensor(mel) else torch.as_tensor(np.asarray(mel, dtype=np.float32))
    if m.dim() != 2:
        raise ValueError(f"mel must be one [n_mel, T] spectrogram, got shape {tuple(m.shape)}")
    dev = m.device if m.is_cuda else (_stft._device or torch.device("cuda", torch.cuda.current_device()))
    wave, _ = mel_to_wave(m.to(device=dev, dtype=torch.float32).unsqueeze(0), _stft, griffin_iters)
    write(out_filename, _stft.sampling_rate, wave[0].cpu().numpy())
