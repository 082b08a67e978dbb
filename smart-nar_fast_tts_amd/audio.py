"""Wave-to-mel front end: the reference's ``TacotronSTFT.mel_spectrogram`` and ``Audio.tools.get_mel_from_wav``
(audio/stft.py:52-81,159-178, audio/tools.py:8-15, audio/audio_processing.py:85-91) as three HIP launches on the caller's
stream (csrc/melfront.hip around one Conv1D-as-GEMM; ``ns_mel_*`` in include/nar_fs2.h).  It produces the ``mels`` that
``align()``, ``forward_teacher_forced()`` and ``FastSpeech2Loss`` consume, without a host round trip.

DEVIATIONS from the reference, both documented in DESIGN.md §15:
  * the reference asserts ``min >= -1`` and ``max <= 1`` (a host read, stft.py:169-170); here the kernel clips, which is the
    identity on anything the assertion lets through and what ``get_mel_from_wav`` does ahead of the call (tools.py:9);
  * the mel filter bank restates the published Slaney formula (librosa's defaults ``htk=False, norm="slaney"``) — librosa is not a
    dependency, and the restatement has NOT been compared with librosa's output; ``mel_basis=`` / ``load_state_dict`` take
    librosa's own matrix."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

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


class TacotronSTFT:
    """Drop-in for the reference's ``TacotronSTFT(filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin,
    mel_fmax)`` on the MI355X.  ``mel_basis=`` hands in a filter bank (e.g. librosa's, from a saved ``state_dict()``) in place of the
    Slaney restatement.

    ``mel_spectrogram(y, wav_lens=None, max_mel_len=None)`` takes a BATCH of variable-length waves and nothing in it synchronises.
    Device-side ``wav_lens`` cannot be validated without a read; for them the kernels' rule holds: a length is clamped to
    ``[0, n]`` and an utterance of ``filter_length / 2`` samples or fewer (which the reference's reflect pad refuses) has zero
    frames — ``mel`` and ``energy`` all zeros, ``mel_lens`` 0.

    Threading: one instance serves one host thread at a time; several HIP streams from that thread are fine (one workspace each)."""

    MAX_WORKSPACE_STREAMS = 4

    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax, mel_basis=None):
        self.filter_length, self.hop_length, self.win_length = int(filter_length), int(hop_length), int(win_length)
        self.n_mel_channels, self.sampling_rate = int(n_mel_channels), sampling_rate
        self.mel_fmin, self.mel_fmax = mel_fmin, mel_fmax
        self._lib = _lib.load()
        hd = C.c_void_p()
        _lib.check(self._lib.ns_mel_create(C.byref(config_struct(filter_length, hop_length, win_length, n_mel_channels)), C.byref(hd)), "TacotronSTFT")
        self._h = hd
        if mel_basis is None:
            mel_basis = slaney_mel_basis(sampling_rate, self.filter_length, self.n_mel_channels, mel_fmin, mel_fmax)
        self._device = None
        self._arena = None
        self._ws = OrderedDict()
        self._sd = None
        self.mel_lens = None
        self.training = False
        self.load_state_dict({"stft_fn.forward_basis": stft_forward_basis(self.filter_length, self.win_length), "mel_basis": mel_basis})

    @classmethod
    def from_config(cls, preprocess_config: dict, mel_basis=None):
        """The arguments the reference's preprocessor passes (preprocessor/preprocessor.py:39-47)."""
        p = preprocess_config["preprocessing"]
        return cls(p["stft"]["filter_length"], p["stft"]["hop_length"], p["stft"]["win_length"], p["mel"]["n_mel_channels"],
                   p["audio"]["sampling_rate"], p["mel"]["mel_fmin"], p["mel"]["mel_fmax"], mel_basis=mel_basis)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.ns_mel_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- nn.Module-shaped surface --------------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("the front end has no trainable state")
        return self.eval()

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("this front end runs on an MI355X only (device must be 'cuda[:N]'); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._device != device:
            self._device = device
            self._ws = OrderedDict()
            self._arena = None
            self._upload()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    @property
    def mel_basis(self) -> torch.Tensor:
        return torch.from_numpy(self._sd["mel_basis"].copy())

    @property
    def forward_basis(self) -> torch.Tensor:
        return torch.from_numpy(self._sd["stft_fn.forward_basis"].copy())

    def state_dict(self):
        return OrderedDict((k, torch.from_numpy(v.copy())) for k, v in self._sd.items())

    def load_state_dict(self, state_dict, strict: bool = True):
        """Keys of the reference module: ``stft_fn.forward_basis``, ``mel_basis`` (either may be absent: the current one stays) and
        ``stft_fn.inverse_basis`` (accepted, ignored).  Unknown keys and shape mismatches raise before anything is replaced."""
        new, errors = dict(self._sd or {}), []
        for k, t in dict(state_dict).items():
            a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            if self._lib.ns_mel_check_weight(self._h, k.encode(), shape, a.ndim) != 0:
                errors.append(self._lib.ns_last_error().decode())
            elif k != "stft_fn.inverse_basis":
                new[k] = a
        if errors:
            raise RuntimeError("load_state_dict: " + "; ".join(errors))
        self._sd = new
        if self._device is not None:
            self._upload()
        return [], []

    def _upload(self):
        nbytes = self._lib.ns_mel_arena_bytes(self._h)
        with torch.cuda.device(self._device):
            arena = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
            _lib.check(self._lib.ns_mel_bind_arena(self._h, _lib.ptr(arena), nbytes), "ns_mel_bind_arena")
            for k, a in self._sd.items():
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(self._lib.ns_mel_set_weight(self._h, k.encode(), C.c_void_p(a.ctypes.data), shape, a.ndim), "load_state_dict")
            _lib.check(self._lib.ns_mel_finalize_weights(self._h, _lib.stream_ptr(self._device)), "load_state_dict")
            self._arena = arena

    def _workspace(self, nbytes: int, stream_handle: int) -> torch.Tensor:
        w = self._ws.get(stream_handle)
        if w is None or w.numel() < nbytes:
            self._ws.pop(stream_handle, None)
            w = torch.empty(int(nbytes), dtype=torch.uint8, device=self._device)
            self._ws[stream_handle] = w
        self._ws.move_to_end(stream_handle)
        while len(self._ws) > self.MAX_WORKSPACE_STREAMS:
            self._ws.popitem(last=False)
        return w

    def release_workspaces(self):
        self._ws = OrderedDict()

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
        if wav_lens is None:
            wav_lens = [n] * B
        if torch.is_tensor(wav_lens) and wav_lens.is_cuda:
            if wav_lens.device != dev:
                raise RuntimeError(f"wav_lens is on {wav_lens.device}, y on {dev}")
            if wav_lens.dtype != torch.long or tuple(wav_lens.shape) != (B,):
                raise ValueError(f"device wav_lens must be int64 [{B}], got {wav_lens.dtype} {tuple(wav_lens.shape)}")
            lens = wav_lens.contiguous()
        else:
            host = np.asarray(wav_lens.cpu() if torch.is_tensor(wav_lens) else wav_lens)
            if host.dtype.kind not in "iu":
                raise ValueError(f"wav_lens must hold integers, got {host.dtype}")
            if host.shape != (B,):
                raise ValueError(f"wav_lens must have shape ({B},), got {host.shape}")
            for b, v in enumerate(host.tolist()):
                if v <= half:
                    raise ValueError(f"wav_lens[{b}] = {v}: a wave must be longer than filter_length / 2 = {half} samples (the reflect pad, stft.py:60-64)")
                if v > n:
                    raise ValueError(f"wav_lens[{b}] = {v} exceeds the {n} samples of y")
            lens = torch.as_tensor(host.astype(np.int64)).to(dev)
        self.to(dev)
        y = y.contiguous()
        with torch.cuda.device(dev):
            mel = torch.empty(B, T, self.n_mel_channels, dtype=torch.float32, device=dev)
            energy = torch.empty(B, T, dtype=torch.float32, device=dev)
            mel_lens = torch.empty(B, dtype=torch.long, device=dev)
            if B > 0:
                stream = torch.cuda.current_stream(dev).cuda_stream
                nbytes = int(self._lib.ns_mel_ws_bytes(self._h, B, n))
                ws = self._workspace(nbytes, stream)
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
