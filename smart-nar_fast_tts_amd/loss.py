"""The loss of a teacher-forced batch: the reference's ``FastSpeech2Loss`` (model/loss.py:149-250) in HIP (csrc/loss.hip, csrc/lossgrad.hip;
``ns_loss_*`` and ``ns_lossg_*`` in include/nar_fs2.h), and the arithmetic of the ``evaluate`` module the reference imports but does
not ship (train.py:16).

``FastSpeech2Loss``           the forward VALUE in ``eval()`` only, two launches: no backward; it refuses ``train()`` and ``requires_grad``
``FastSpeech2TrainingLoss``   the same value plus ``total_loss.backward()`` (train.py:88) as a ``torch.autograd.Function``: one more
                              launch writes the gradients of the five predictions and the four alignment maps

No optimiser here — the optimiser half of the training step (clip, Adam, the schedule) is ``optim.py``, which consumes the gradients
that torch's backward of the model produces from these."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._handle import StreamWorkspaces
from ._train import guard

_TRAINING = "training is out of scope for this path (SURVEY.md §2); only eval() is supported"
_NINE_IN_KEEP = (4, 5, 8, 10, 12, 13, 14, 15, 16)  # mel, postnet, pitch, energy, log_d, attn[0..3] in _marshal's `keep` list
GRAD_NAMES = ("mel_predictions", "postnet_mel_predictions", "pitch_predictions", "energy_predictions", "log_duration_predictions",
              "attn[0]", "attn[1]", "attn[2]", "attn[3]")  # what FastSpeech2TrainingLoss differentiates (model/loss.py:175-179,185)
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
        self._ws = StreamWorkspaces(self.MAX_WORKSPACE_STREAMS, per_device=True, slack=True)
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
        return self._ws.take(device, nbytes)

    # ---- forward -------------------------------------------------------------------------------
    def forward(self, inputs, predictions):
        if self.training:
            raise NotImplementedError(_TRAINING)
        call = self._marshal(inputs, predictions)
        with guard(call.device):
            return self._value(call)

    def _value(self, call):
        """ns_loss_forward on the current stream of the call's device: the [7] tensor's seven views."""
        ws = self.workspace(call.device, self._lib.ns_loss_ws_bytes(call.B, call.L, call.T))
        out = torch.empty(7, dtype=torch.float32, device=call.device)
        _lib.check(self._lib.ns_loss_forward(C.byref(call.args), _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.stream_ptr(call.device)), "ns_loss_forward")
        return tuple(out[i] for i in range(7))

    def _refuse_grad(self, name, t):
        """A tensor with requires_grad: this class has no backward."""
        raise NotImplementedError(f"{name}.requires_grad: " + _TRAINING)

    def _marshal(self, inputs, predictions):
        """Checks the two tuples and lays them out for the C ABI: a ``_Call`` holding the filled ``ns_loss_args``, the tensors it points
        into, and the nine predictions as the dense tensors the kernels read (autograd-connected to the caller's where those require
        grad)."""
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
                self._refuse_grad(name, t)
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

        with guard(dev):
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
        call = _Call()
        call.args, call.keep, call.device, call.B, call.L, call.T = a, keep, dev, B, L, T
        call.nine = tuple(keep[i] for i in _NINE_IN_KEEP)
        return call


class _Call:
    """One marshalled loss call (``FastSpeech2Loss._marshal``)."""
    __slots__ = ("args", "keep", "device", "B", "L", "T", "nine")


class _LossFunction(torch.autograd.Function):
    """value = ns_lossg_forward (two launches, writes the record), backward = ns_lossg_backward (one launch).  The nine differentiable
    tensors are flat arguments; everything else rides on ``call``."""

    @staticmethod
    def forward(ctx, owner, call, *nine):
        out, record = owner._value_with_record(call)
        ctx.owner, ctx.call, ctx.record = owner, call, record
        ctx.save_for_backward(*nine)  # (autograd then refuses a backward after an in-place change of a prediction)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        nine = ctx.saved_tensors
        owner, call = ctx.owner, ctx.call
        need = ctx.needs_input_grad[2:]
        with guard(call.device):
            grads = owner._backward(call, ctx.record, g, [torch.empty_like(x, memory_format=torch.contiguous_format) if n else None
                                                          for x, n in zip(nine, need)])
        return (None, None) + tuple(grads)


class FastSpeech2TrainingLoss(FastSpeech2Loss):
    """``FastSpeech2Loss`` with a backward: the criterion of the reference's training step (train.py:43,83-88).

        Loss = FastSpeech2TrainingLoss(preprocess_config, model_config).to(device)          # train.py:43
        losses = Loss(batch, output)                                                        # train.py:83
        (losses[0] / grad_acc_step).backward()                                              # train.py:84-88

    ``train()`` and ``eval()`` both work and change nothing.  When no prediction requires grad, or under ``torch.no_grad()``, a call is
    the parent's: ``ns_loss_forward``, the same bits.  Otherwise the seven values are views of the ``[7]`` output of one
    ``torch.autograd.Function`` — the same bits again — and a backward of ``total``, of ``total / grad_acc_step`` or of any mix of the
    seven is ONE launch (csrc/lossgrad.hip) that reads autograd's ``grad_output`` and the forward's counts on the device: three
    launches for value and gradients, no host read.  Differentiated: the five predictions and the four alignment maps
    (``GRAD_NAMES``); a tensor of those that does not require grad gets no buffer and no write.  Targets, masks and lengths never get
    gradients, and a target that requires grad is refused (the reference switches it off in place, model/loss.py:194-197; we do not
    modify the caller's tensors).  Single backward only (``once_differentiable``).

    A masked-out position gets the gradient +0.0 and is never read, so NaN behind a mask stays there; a part whose selection is empty
    (value NaN) has an all-zero gradient, as ``masked_select``'s backward gives."""

    def __init__(self, preprocess_config: dict, model_config: dict):
        super().__init__(preprocess_config, model_config)
        self.launches = 0  # kernel launches enqueued by the differentiable path (tools/lossgrad_bench.py counts them)

    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    def _refuse_grad(self, name, t):
        if name not in GRAD_NAMES:
            raise ValueError(f"{name}.requires_grad: targets, masks and lengths get no gradient from the loss (model/loss.py:194-197); detach it first")

    def forward(self, inputs, predictions):
        call = self._marshal(inputs, predictions)
        if not (torch.is_grad_enabled() and any(t.requires_grad for t in call.nine)):
            with guard(call.device):
                return self._value(call)
        out = _LossFunction.apply(self, call, *call.nine)
        return tuple(out[i] for i in range(7))

    def _value_with_record(self, call):
        """ns_lossg_forward on the current stream of the call's device: ``(out [7], record)``.  The record is a fresh tensor per call:
        it carries the forward's counts to the backward and outlives the shared workspace."""
        dev = call.device
        with guard(dev):
            ws = self.workspace(dev, self._lib.ns_loss_ws_bytes(call.B, call.L, call.T))
            out = torch.empty(7, dtype=torch.float32, device=dev)
            record = torch.empty(self._lib.ns_lossg_record_bytes() // 8, dtype=torch.int64, device=dev)
            _lib.check(self._lib.ns_lossg_forward(C.byref(call.args), _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.ptr(record), _lib.stream_ptr(dev)),
                       "ns_lossg_forward")
        self.launches += 2
        return out, record

    def _backward(self, call, record, g, outs):
        """One launch on the current stream of the call's device: writes the gradient of ``(g * seven).sum()`` into every tensor of
        ``outs`` (the order of ``GRAD_NAMES``) that is not None, and returns ``outs``."""
        if tuple(g.shape) != (7,) or g.dtype != torch.float32 or g.device != call.device:
            raise ValueError(f"grad_output must be a float32 [7] tensor on {call.device}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = g.contiguous()
        d = _lib.NsLossgGrads()
        for i, (name, x, o) in enumerate(zip(GRAD_NAMES, call.nine, outs)):
            if o is None:
                continue
            if o.dtype != torch.float32 or o.device != call.device or tuple(o.shape) != tuple(x.shape) or not o.is_contiguous():
                raise ValueError(f"the gradient buffer of {name} must be a contiguous float32 tensor of shape {tuple(x.shape)} on {call.device}")
            if i < 5:
                setattr(d, ("mel", "postnet", "pitch", "energy", "log_d")[i], o.data_ptr())
            else:
                d.attn[i - 5] = o.data_ptr()
        _lib.check(self._lib.ns_lossg_backward(C.byref(call.args), _lib.ptr(record), _lib.ptr(g), C.byref(d), _lib.stream_ptr(call.device)),
                   "ns_lossg_backward")
        self.launches += 1
        return outs


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
