"""Validation loss of a teacher-forced batch: the reference's ``FastSpeech2Loss`` (model/loss.py:149-250) as two HIP launches
(csrc/loss.hip; ``ns_loss_*`` in include/nar_fs2.h), and the arithmetic of the ``evaluate`` module the reference imports but does
not ship (train.py:16).  The forward VALUE in ``eval()`` only: no backward, and no optimiser here — the optimiser half of the
training step (clip, Adam, the schedule) is ``optim.py``, which acts on gradients some other backward pass has produced."""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

_TRAINING = "training is out of scope for this path (SURVEY.md §2); only eval() is supported"
LOSS_NAMES = ("total", "mel", "postnet", "pitch", "energy", "duration", "attn")  # the reference's return order (model/loss.py:242-250)


class FastSpeech2Loss:
    """Drop-in for the reference's ``FastSpeech2Loss(preprocess_config, model_config)``; ``loss(inputs, predictions)`` returns the
    seven values ``(total, mel, postnet, pitch, energy, duration, attn)`` as 0-dim fp32 device tensors, views of one ``[7]`` tensor.

    ``inputs`` is the reference's batch tuple, read as ``inputs[4:]`` = ``src_lens, _, mel_targets, mel_lens, _, pitch_targets,
    energy_targets`` (model/loss.py:165-173); ``predictions`` is the 12-tuple of ``forward_teacher_forced()`` (a ``ForwardOutput`` or
    any tuple).  Nothing synchronises: both launches go to the current stream of the tensors' device.  Lengths given as host arrays
    are uploaded, device lengths are used as they are.  Non-contiguous tensors get ``.contiguous()``, except ``mel_targets`` with
    more than T frames and ``d_targets`` with more than L columns (model/loss.py:191,214-216), which are read through their strides.

    DEVIATION: the reference fails on a broadcast when ``T != max(mel_lens)`` or ``L != max(src_lens)`` (model/loss.py:60,69-71);
    here ``ilen`` is clamped to [0, L] and ``olen`` to [0, T], and the guided-attention region is what ``_make_masks`` would select
    if the shapes agreed."""

    MAX_WORKSPACE_STREAMS = 8

    def __init__(self, preprocess_config: dict, model_config: dict):
        self.pitch_feature_level = preprocess_config["preprocessing"]["pitch"]["feature"]
        self.energy_feature_level = preprocess_config["preprocessing"]["energy"]["feature"]
        for what, level in (("pitch", self.pitch_feature_level), ("energy", self.energy_feature_level)):
            if level not in ("phoneme_level", "frame_level"):
                raise ValueError(f"preprocessing.{what}.feature must be 'phoneme_level' or 'frame_level' (model/loss.py:199-211), got {level!r}")
        self._lib = _lib.load()
        self._ws = OrderedDict()  # (device index, stream handle) -> partial-slot workspace, least recently used first
        self.training = False

    # ---- nn.Module-shaped surface ------------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(_TRAINING)
        return self.eval()

    def to(self, device):  # (train.py:43 calls .to(device); the loss holds no tensors)
        return self

    def __call__(self, inputs, predictions):
        return self.forward(inputs, predictions)

    def workspace(self, device, nbytes: int) -> torch.Tensor:
        """The partial-slot workspace of the current stream of ``device`` (one per stream: calls on different streams may overlap)."""
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        w = self._ws.get(key)
        if w is None or w.numel() < nbytes:
            w = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
            self._ws[key] = w
        self._ws.move_to_end(key)
        while len(self._ws) > self.MAX_WORKSPACE_STREAMS:
            self._ws.popitem(last=False)
        return w

    # ---- forward -------------------------------------------------------------------------------
    def forward(self, inputs, predictions):
        if self.training:
            raise NotImplementedError(_TRAINING)
        if len(inputs) < 11:
            raise ValueError(f"inputs must be the reference's batch tuple of 11 entries (utils/tools.py:18-54), got {len(inputs)}")
        if len(predictions) != 12:
            raise ValueError(f"predictions must be the reference's 12-tuple (model/fastspeech2_align.py:87-100), got {len(predictions)} entries")
        src_lens, _, mel_targets, mel_lens, _, pitch_targets, energy_targets = inputs[4:11]
        mel, post, pitch, energy, log_d, _, src_masks, mel_masks, _, _, attn, d_targets = predictions
        if len(attn) < 4:
            raise ValueError(f"the guided-attention term reads the alignment maps of layers 0-3 (model/loss.py:233-236); got {len(attn)} map(s)")
        attn = list(attn[:4])
        named = dict(mel_predictions=mel, postnet_mel_predictions=post, pitch_predictions=pitch, energy_predictions=energy,
                     log_duration_predictions=log_d, src_masks=src_masks, mel_masks=mel_masks, duration_targets=d_targets,
                     mel_targets=mel_targets, pitch_targets=pitch_targets, energy_targets=energy_targets,
                     **{f"attn[{k}]": a for k, a in enumerate(attn)})
        for name, t in named.items():
            if not torch.is_tensor(t):
                raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
            if t.requires_grad:
                raise NotImplementedError(f"{name}.requires_grad: " + _TRAINING)
        for name, t in named.items():
            if not t.is_cuda:
                raise RuntimeError(f"{name} must live on the MI355X (cuda) device; there is no CPU path")
        dev = mel.device
        for name, t in named.items():
            if t.device != dev:
                raise RuntimeError(f"{name} is on {t.device}, mel_predictions on {dev}")
        for name, t in named.items():
            if name in ("src_masks", "mel_masks"):
                if t.dtype != torch.bool:
                    raise ValueError(f"{name} must be a bool tensor (model/loss.py:188-189 inverts it), got {t.dtype}")
            elif name == "duration_targets":
                if t.dtype.is_floating_point or t.dtype == torch.bool:
                    raise ValueError(f"duration_targets must be an integer tensor, got {t.dtype}")
            elif t.dtype != torch.float32:
                raise ValueError(f"{name} must be float32 (this path computes in fp32 only), got {t.dtype}")
        # shapes: what the reference's masked_select accepts
        if mel.dim() != 3 or attn[0].dim() != 4:
            raise ValueError(f"mel_predictions must be [B, T, n_mel] and attn[k] [B, H, T, L], got {tuple(mel.shape)} and {tuple(attn[0].shape)}")
        B, T, n_mel = (int(v) for v in mel.shape)
        H, L = int(attn[0].shape[1]), int(attn[0].shape[3])
        p_frame, e_frame = self.pitch_feature_level == "frame_level", self.energy_feature_level == "frame_level"

        def want(name, t, shape):
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")

        want("postnet_mel_predictions", post, (B, T, n_mel))
        want("mel_masks", mel_masks, (B, T))
        want("src_masks", src_masks, (B, L))
        want("log_duration_predictions", log_d, (B, L))
        for k in range(4):
            want(f"attn[{k}]", attn[k], (B, H, T, L))
        want("pitch_predictions", pitch, (B, T) if p_frame else (B, L))
        want("pitch_targets", pitch_targets, (B, T) if p_frame else (B, L))
        want("energy_predictions", energy, (B, T) if e_frame else (B, L))
        want("energy_targets", energy_targets, (B, T) if e_frame else (B, L))
        if mel_targets.dim() != 3 or mel_targets.shape[0] != B or mel_targets.shape[2] != n_mel or mel_targets.shape[1] < T:
            raise ValueError(f"mel_targets must have shape ({B}, >= {T}, {n_mel}) (mel_targets[:, :T], model/loss.py:191), got {tuple(mel_targets.shape)}")
        if d_targets.dim() != 2 or d_targets.shape[0] != B or d_targets.shape[1] < L:
            raise ValueError(f"duration_targets must have shape ({B}, >= {L}) (duration_targets[:, :L], model/loss.py:214-216), got {tuple(d_targets.shape)}")
        if n_mel % 4:
            raise ValueError(f"n_mel must be a multiple of 4 (rows are read as float4), got {n_mel}")
        if H < 1 and B * T * L > 0:
            raise ValueError("attn[k] has no head 0 (model/loss.py:233-236)")

        def lens(name, v):
            if torch.is_tensor(v) and v.is_cuda:
                if v.device != dev:
                    raise RuntimeError(f"{name} is on {v.device}, mel_predictions on {dev}")
            else:
                v = torch.as_tensor(np.asarray(v.cpu() if torch.is_tensor(v) else v))
            if v.dtype.is_floating_point or v.dtype == torch.bool:
                raise ValueError(f"{name} must hold integers, got {v.dtype}")
            if tuple(v.shape) != (B,):
                raise ValueError(f"{name} must have shape ({B},), got {tuple(v.shape)}")
            return v.to(device=dev, dtype=torch.long).contiguous()

        def dense(t):  # contiguous and 16-byte aligned
            t = t.contiguous()
            return t.clone() if t.data_ptr() % 16 else t

        with (contextlib.nullcontext() if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)):
            sl, ml = lens("src_lens", src_lens), lens("mel_lens", mel_lens)
            # the two slices the reference takes go through the strides
            if not (mel_targets.stride(2) == 1 and mel_targets.stride(1) == n_mel and mel_targets.stride(0) % 4 == 0
                    and mel_targets.stride(0) >= T * n_mel and mel_targets.data_ptr() % 16 == 0):
                mel_targets = dense(mel_targets)
            if d_targets.dtype != torch.long:
                d_targets = d_targets.long()
            if not (d_targets.stride(1) == 1 and d_targets.stride(0) >= L):
                d_targets = d_targets.contiguous()
            a = _lib.NsLossArgs()
            a.B, a.L, a.T, a.H, a.n_mel = B, L, T, H, n_mel
            a.pitch_frame_level, a.energy_frame_level = int(p_frame), int(e_frame)
            a.mel_targets_stride = int(mel_targets.stride(0)) if B > 1 else max(int(mel_targets.shape[1]), T) * n_mel
            a.d_targets_stride = int(d_targets.stride(0)) if B > 1 else max(int(d_targets.shape[1]), L)
            keep = [sl, ml, mel_targets, d_targets]

            def put(field, t, aligned=False):
                t = dense(t) if aligned else t.contiguous()
                keep.append(t)
                setattr(a, field, t.data_ptr())

            put("mel", mel, True)
            put("postnet", post, True)
            a.mel_targets, a.d_targets = mel_targets.data_ptr(), d_targets.data_ptr()
            put("mel_masks", mel_masks)
            put("src_masks", src_masks)
            put("pitch", pitch)
            put("pitch_targets", pitch_targets)
            put("energy", energy)
            put("energy_targets", energy_targets)
            put("log_d", log_d)
            a.src_lens, a.mel_lens = sl.data_ptr(), ml.data_ptr()
            for k in range(4):
                m = attn[k].contiguous()
                keep.append(m)
                a.attn[k] = m.data_ptr()
            ws = self.workspace(dev, self._lib.ns_loss_ws_bytes(B, L, T))
            out = torch.empty(7, dtype=torch.float32, device=dev)
            _lib.check(self._lib.ns_loss_forward(C.byref(a), _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.stream_ptr(dev)), "ns_loss_forward")
        return tuple(out[i] for i in range(7))


def evaluate(model, batches, loss=None):
    """EXTENSION: the ``evaluate`` module that train.py:16 imports and the reference does not ship, reduced to its arithmetic.  For
    every batch (the reference's 11-tuple, utils/tools.py:18-54, on the device) it runs ``model.forward_teacher_forced(*batch[2:],
    async_status=True)`` and the loss, and accumulates ``len(batch[0]) * losses`` in a device [7] float64 tensor; every status word
    is checked (a token id outside the vocabulary still raises ``IndexError``) and the host reads once, at the end.  Returns the seven
    dataset means ``(total, mel, postnet, pitch, energy, duration, attn)`` as floats."""
    loss = loss if loss is not None else FastSpeech2Loss(model.preprocess_config, model.model_config)
    acc, outs, n = None, [], 0
    for batch in batches:
        out = model.forward_teacher_forced(*batch[2:], async_status=True)
        vals = loss(batch, out)
        seven = vals[0]._base if vals[0]._base is not None else torch.stack(vals)  # the [7] tensor the seven views are cut from
        k = len(batch[0])
        acc = seven.double() * k if acc is None else acc + seven.double() * k
        outs.append(type(out)((), status=out.status, n_vocab=out._n_vocab))  # the status words only: the tuple's tensors may go
        n += k
    if acc is None:
        raise ValueError("evaluate(): no batches")
    for out in outs:
        out.check()
    return tuple(float(v) for v in (acc / n).cpu().tolist())
