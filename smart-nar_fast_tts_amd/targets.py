"""Pitch / energy variance targets and dataset statistics on the device: the tail of the reference's ``Preprocessor.process_utterance``
and its ``build_from_path`` / ``remove_outlier`` / ``normalize`` (preprocessor/preprocessor.py:188-227, 61-133, 289-310) as HIP launches
(csrc/vartargets.hip; ``ns_vt_*`` in include/nar_fs2.h).  Frame-level f0 is an input: pitch extraction, resampling, TextGrid parsing and
file I/O stay outside."""
from __future__ import annotations

import ctypes as C
import json
import os

import torch

from . import _lib
from ._handle import StreamWorkspaces
from ._train import guard

SORT_CAPACITY = _lib.NS["NS_VT_SORT_CAPACITY"]


class VarianceTargets:
    """``VarianceTargets(preprocess_config)`` turns frame-level pitch and energy plus the aligner's durations into the ``p_targets`` /
    ``e_targets`` that ``forward_teacher_forced`` and ``FastSpeech2Loss`` take, and keeps the running dataset statistics on the device.

    First pass over the dataset: ``process(..., fit=True)`` per batch (raw targets; the statistics absorb the outlier-filtered values).
    Second pass: ``normalize(...)`` per batch (in place), then ``stats()`` / ``write_stats(path)``.  Nothing synchronises except
    ``stats()``: every launch goes to the current stream of the tensors' device.

    DEVIATION: the reference averages in place and so reads values it has already overwritten when zero durations come early in an
    utterance (preprocessor.py:208-216); here every mean is over the original frames (include/nar_fs2.h, ns_vt_targets)."""

    MAX_WORKSPACE_STREAMS = 8

    def __init__(self, preprocess_config: dict):
        pre = preprocess_config["preprocessing"]
        self.pitch_feature_level = pre["pitch"]["feature"]
        self.energy_feature_level = pre["energy"]["feature"]
        for what, level in (("pitch", self.pitch_feature_level), ("energy", self.energy_feature_level)):
            if level not in ("phoneme_level", "frame_level"):
                raise ValueError(f"preprocessing.{what}.feature must be 'phoneme_level' or 'frame_level' (preprocessor.py:25-32), got {level!r}")
        self.pitch_normalization = bool(pre["pitch"]["normalization"])
        self.energy_normalization = bool(pre["energy"]["normalization"])
        self._lib = _lib.load()
        self._ws = StreamWorkspaces(self.MAX_WORKSPACE_STREAMS, per_device=True, slack=True)
        self._state = None        # device [10] float64 = ns_vt_state, created on the first batch's device

    # ---- plumbing ------------------------------------------------------------------------------
    def workspace(self, device, nbytes: int) -> torch.Tensor:
        return self._ws.take(device, nbytes)

    def _state_on(self, dev) -> torch.Tensor:
        if self._state is None:
            self._state = torch.empty(10, dtype=torch.float64, device=dev)
            _lib.check(self._lib.ns_vt_state_init(_lib.ptr(self._state, _lib.NsVtState), _lib.stream_ptr(dev)), "ns_vt_state_init")
        elif self._state.device != dev:
            raise RuntimeError(f"the running statistics live on {self._state.device}, this batch on {dev}")
        return self._state

    def reset(self):
        """Forget the running statistics (the next batch starts a new dataset)."""
        self._state = None
        return self

    def _levels(self):
        return self.pitch_feature_level == "frame_level", self.energy_feature_level == "frame_level"

    def _args(self, B, L, T):
        a = _lib.NsVtArgs()
        a.B, a.L, a.T = B, L, T
        a.pitch_frame_level, a.energy_frame_level = (int(v) for v in self._levels())
        a.pitch_normalization, a.energy_normalization = int(self.pitch_normalization), int(self.energy_normalization)
        a.durations_stride = L
        return a

    @staticmethod
    def _need(name, t, dtype, shape=None, ndim=None):
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
        if ndim is not None and t.dim() != ndim:
            raise ValueError(f"{name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")

    @staticmethod
    def _on_gpu(named):
        for name, t in named.items():
            if not t.is_cuda:
                raise RuntimeError(f"{name} must live on the MI355X (cuda) device; there is no CPU path")
        dev = next(iter(named.values())).device
        for name, t in named.items():
            if t.device != dev:
                raise RuntimeError(f"{name} is on {t.device}, {next(iter(named))} on {dev}")
        return dev

    # ---- pass 1 --------------------------------------------------------------------------------
    def process(self, pitch, energy, durations, src_lens, fit: bool = True):
        """``pitch``, ``energy`` [B, T] fp32 (f0 0 = unvoiced), ``durations`` [B, L] int64 (a column slice of a wider tensor is read
        through its row stride), ``src_lens`` [B] int64 -> ``(pitch_targets, energy_targets, frame_lens, valid)``: raw targets
        [B, L] or [B, T] fp32 per the configured level, frame counts [B] int64, the voiced flag [B] uint8.  ``fit=True`` also merges
        the batch into the running statistics."""
        self._need("pitch", pitch, torch.float32, ndim=2)
        B, T = (int(v) for v in pitch.shape)
        self._need("energy", energy, torch.float32, shape=(B, T))
        self._need("durations", durations, torch.int64, ndim=2)
        if int(durations.shape[0]) != B:
            raise ValueError(f"durations must have shape ({B}, L), got {tuple(durations.shape)}")
        L = int(durations.shape[1])
        self._need("src_lens", src_lens, torch.int64, shape=(B,))
        p_frame, e_frame = self._levels()
        if fit:
            for what, n in (("pitch", T if p_frame else L), ("energy", T if e_frame else L)):
                if n > SORT_CAPACITY:
                    raise ValueError(f"{what}: {n} values per utterance exceed the sort capacity of the fit ({SORT_CAPACITY})")
        dev = self._on_gpu(dict(pitch=pitch, energy=energy, durations=durations, src_lens=src_lens))
        with guard(dev):
            pitch, energy, src_lens = pitch.contiguous(), energy.contiguous(), src_lens.contiguous()
            if not (durations.stride(1) == 1 and durations.stride(0) >= L) and durations.numel() > 0:
                durations = durations.contiguous()
            a = self._args(B, L, T)
            a.durations_stride = int(durations.stride(0)) if B > 1 and L > 0 else L
            pt = torch.empty((B, T if p_frame else L), dtype=torch.float32, device=dev)
            et = torch.empty((B, T if e_frame else L), dtype=torch.float32, device=dev)
            frame_lens = torch.empty(B, dtype=torch.int64, device=dev)
            valid = torch.empty(B, dtype=torch.uint8, device=dev)
            a.pitch, a.energy, a.durations, a.src_lens = pitch.data_ptr(), energy.data_ptr(), durations.data_ptr(), src_lens.data_ptr()
            a.pitch_targets, a.energy_targets, a.frame_lens, a.valid = pt.data_ptr(), et.data_ptr(), frame_lens.data_ptr(), valid.data_ptr()
            ws = self.workspace(dev, self._lib.ns_vt_ws_bytes(B, L, T))
            st = _lib.stream_ptr(dev)
            _lib.check(self._lib.ns_vt_targets(C.byref(a), _lib.ptr(ws), ws.numel(), st), "ns_vt_targets")
            if fit:
                state = self._state_on(dev)
                _lib.check(self._lib.ns_vt_fit(C.byref(a), _lib.ptr(state, _lib.NsVtState), _lib.ptr(ws), ws.numel(), st), "ns_vt_fit")
        return pt, et, frame_lens, valid

    # ---- pass 2 --------------------------------------------------------------------------------
    def normalize(self, pitch_targets, energy_targets, src_lens, frame_lens, valid=None):
        """In place: ``(x - mean) / std`` on the selected positions of the raw targets of ``process`` (padding stays 0), and the
        min / max of the normalised values folded into the statistics.  ``valid`` (the flag ``process`` returned) keeps dropped
        utterances at 0 and out of the extrema.  Without it EVERY utterance is taken as valid: the zero rows of an utterance that
        ``process`` dropped become ``-mean / std`` below ``src_lens`` / ``frame_lens`` and that value enters min / max — leave the
        flag out only for a batch known to hold no dropped utterance.  Returns the two tensors."""
        self._need("pitch_targets", pitch_targets, torch.float32, ndim=2)
        self._need("energy_targets", energy_targets, torch.float32, ndim=2)
        B = int(pitch_targets.shape[0])
        self._need("src_lens", src_lens, torch.int64, shape=(B,))
        self._need("frame_lens", frame_lens, torch.int64, shape=(B,))
        if int(energy_targets.shape[0]) != B:
            raise ValueError(f"energy_targets must have {B} rows, got shape {tuple(energy_targets.shape)}")
        named = dict(pitch_targets=pitch_targets, energy_targets=energy_targets, src_lens=src_lens, frame_lens=frame_lens)
        if valid is not None:
            self._need("valid", valid, torch.uint8, shape=(B,))
            named["valid"] = valid
        dev = self._on_gpu(named)
        p_frame, e_frame = self._levels()
        wp, we = int(pitch_targets.shape[1]), int(energy_targets.shape[1])
        if p_frame == e_frame and wp != we:
            raise ValueError(f"pitch_targets and energy_targets share a feature level but not a width: {wp} and {we}")
        # the width of a frame-level tensor is T, of a phoneme-level one L; a dimension neither tensor has is 0 (never indexed)
        T = wp if p_frame else (we if e_frame else 0)
        L = wp if not p_frame else (we if not e_frame else 0)
        for name, t in (("pitch_targets", pitch_targets), ("energy_targets", energy_targets)):
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous (it is normalised in place)")
        with guard(dev):
            a = self._args(B, L, T)
            src_lens, frame_lens = src_lens.contiguous(), frame_lens.contiguous()
            a.src_lens, a.frame_lens = src_lens.data_ptr(), frame_lens.data_ptr()
            a.pitch_targets, a.energy_targets = pitch_targets.data_ptr(), energy_targets.data_ptr()
            if valid is not None:
                valid = valid.contiguous()  # a local, so that a copy outlives the launch's enqueue
            a.valid = valid.data_ptr() if valid is not None else None
            state = self._state_on(dev)
            ws = self.workspace(dev, self._lib.ns_vt_ws_bytes(B, L, T))
            _lib.check(self._lib.ns_vt_normalize(C.byref(a), _lib.ptr(state, _lib.NsVtState), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "ns_vt_normalize")
        return pitch_targets, energy_targets

    # ---- the statistics --------------------------------------------------------------------------
    def stats(self) -> dict:
        """``{"pitch": [min, max, mean, std], "energy": [...]}`` as the reference writes them (preprocessor.py:118-133): the extrema
        of the normalised values, and mean / std (0 / 1 when the feature's normalization flag is off).  The one host read."""
        if self._state is None:
            raise RuntimeError("stats(): nothing has been processed yet")
        s = self._state.cpu().tolist()  # count[2], mean[2], m2[2], min[2], max[2]
        out = {}
        for f, (name, norm) in enumerate((("pitch", self.pitch_normalization), ("energy", self.energy_normalization))):
            count, mean, m2, lo, hi = (s[2 * k + f] for k in range(5))
            std = 1.0
            if norm and count > 0:
                std = (m2 / count) ** 0.5 or 1.0
            out[name] = [lo, hi, mean if norm and count > 0 else 0.0, std]
        return out

    def write_stats(self, path: str) -> dict:
        """Writes ``stats.json`` in the reference's format; ``path`` is the file or the ``preprocessed_path`` directory."""
        if os.path.isdir(path):
            path = os.path.join(path, "stats.json")
        s = self.stats()
        with open(path, "w") as f:
            f.write(json.dumps(s))
        return s
