"""The reference's ``VarianceAdaptor`` (model/modules.py:17-159) as a trainable module, teacher-forced: the first composite of the
training side.  Three ``predictor.VariancePredictor`` (``ns_pg_*``) plus the two pieces that had no backward — the variance embedding
(``bucketize`` + ``nn.Embedding`` + add) and the length regulator (model/modules.py:195-230) — forward AND backward in HIP
(csrc/adaptorgrad.hip, ``ns_va_*`` in include/nar_fs2.h), under the reference's class and checkpoint names.

    va = VarianceAdaptor(preprocess_config, model_config).to(device)
    va.load_state_dict({k[len("variance_adaptor."):]: v for k, v in ckpt["model"].items() if k.startswith("variance_adaptor.")})   # strict
    x, p, e, log_d, d_rounded, mel_len, mel_mask = va(enc_out, src_mask, mel_mask, max_len, pitch_t, energy_t, duration_t)
    torch.autograd.backward([x, p, e, log_d], [d_out, d_pitch, d_energy, d_log_d])     # enc_out.grad and every parameter's .grad

The composite is wired through torch's autograd across five kinds of HIP Functions.  Where ``x`` fans out — into the duration
predictor, a variance predictor and the embedding add — autograd adds the branches' gradients with torch's own elementwise add: two or
three ``[B, S, d]`` additions per backward.  They are the only torch kernels between the input and the outputs or between the output
gradients and the parameter and input gradients (fusing them is a follow-up); everything else is the kernels of ``ns_pg_*`` and
``ns_va_*``.  No floating-point atomics anywhere: a backward run twice gives the same bits.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import json
import os

import torch

from . import _lib
from . import workload as wl
from ._train import CountedModule, aligned, guard, need_gpu
from .predictor import VariancePredictor

LEVELS = ("phoneme_level", "frame_level")


class _EmbedFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, x, target, bins, weight):
        y, idx = owner._forward(x, target, bins, weight)
        ctx.owner, ctx.idx = owner, idx  # the int32 bucket indices are all the backward keeps
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dx = g if ctx.needs_input_grad[1] else None  # the add passes the gradient through: the same tensor, no launch
        dw = ctx.owner._backward(g, ctx.idx) if ctx.needs_input_grad[4] else None
        return None, dx, None, None, dw


class VarianceEmbedding(CountedModule):
    """``x + weight[torch.bucketize(target, bins)]``: the reference's ``nn.Embedding(n_bins, d)`` (state-dict key ``weight``) together with
    the bucketize in front of it and the add behind it (model/modules.py:80-100, 121-149), one launch forward.

    ``x`` float32 ``[..., d]``, ``target`` float32 of ``x``'s leading shape, ``bins`` float32 ``[n_bins - 1]`` ascending edges.
    ``right=False``; a NaN target takes the last bin.  The add is unmasked, as in the reference: a padded row takes the embedding of its
    target too, and its gradient row is summed into the table.  One autograd Function; ``target`` and ``bins`` take no gradient, the
    gradient of ``x`` is ``grad_output`` itself, and the table's gradient is two launches (float64 sums in a fixed order, rounded once)
    that a frozen table (``weight.requires_grad == False``) does not make.  Refuses ``d % 4 != 0`` and ``n_bins`` outside [2, 2048]."""

    ABI = "ns_va"

    def __init__(self, n_bins, d):
        super().__init__()
        self.n_bins, self.d = int(n_bins), int(d)
        plan = (C.c_int32 * 8)()
        if self._lib.ns_va_plan_embed(1, self.d, self.n_bins, plan) != 0:
            raise ValueError(self._lib.ns_last_error().decode())
        self.weight = torch.nn.Parameter(torch.randn(self.n_bins, self.d))  # nn.Embedding's initialisation

    def forward(self, x, target, bins):
        need_gpu("VarianceEmbedding", "x", x)
        dev, lead = x.device, tuple(x.shape[:-1])
        if x.dtype != torch.float32 or x.dim() < 2 or x.shape[-1] != self.d or x.numel() == 0:
            raise ValueError(f"x must be a non-empty float32 [..., {self.d}] tensor, got {x.dtype} {tuple(x.shape)}")
        if tuple(target.shape) != lead or target.dtype != torch.float32 or target.device != dev:
            raise ValueError(f"target must be a float32 {lead} tensor on {dev}, got {target.dtype} {tuple(target.shape)} on {target.device}")
        if tuple(bins.shape) != (self.n_bins - 1,) or bins.dtype != torch.float32 or bins.device != dev:
            raise ValueError(f"bins must be a float32 [{self.n_bins - 1}] tensor on {dev}, got {bins.dtype} {tuple(bins.shape)} on {bins.device}")
        if self.weight.device != dev or self.weight.dtype != torch.float32:
            raise ValueError(f"weight must be a float32 tensor on {dev}, got {self.weight.dtype} on {self.weight.device}")
        if torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad):
            return _EmbedFunction.apply(self, x, target, bins, self.weight)
        return self._forward(x, target, bins, self.weight)[0]

    def _forward(self, x, target, bins, weight):
        dev = x.device
        xa, ta, ba, wa = aligned(x.detach()), target.detach().contiguous(), bins.detach().contiguous(), aligned(weight.detach())
        M = xa.numel() // self.d
        with guard(dev):
            y = torch.empty_like(xa)
            idx = torch.empty(tuple(x.shape[:-1]), dtype=torch.int32, device=dev)
            self._done(self._lib.ns_va_op_embed_fwd(_lib.ptr(xa), _lib.ptr(ta), _lib.ptr(ba), _lib.ptr(wa), M, self.d, self.n_bins, _lib.ptr(y),
                                                    _lib.ptr(idx), _lib.stream_ptr(dev)), "forward", "ns_va_op_embed_fwd")
        return y, idx

    def _backward(self, g, idx):
        dev = idx.device
        if tuple(g.shape) != tuple(idx.shape) + (self.d,) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {tuple(idx.shape) + (self.d,)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        M = idx.numel()
        with guard(dev):
            n = self._lib.ns_va_embed_ws_bytes(M, self.d, self.n_bins)
            if n == 0:
                _lib.check(1, "ns_va_embed_ws_bytes")
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            dw = torch.empty((self.n_bins, self.d), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_va_op_embed_bwd(_lib.ptr(g), _lib.ptr(idx), M, self.d, self.n_bins, _lib.ptr(dw), _lib.ptr(ws), ws.numel(),
                                                    _lib.stream_ptr(dev)), "backward", "ns_va_op_embed_bwd")
        return dw


class _RegulateFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, x, duration, T):
        out, mel_len, cum = owner._forward(x, duration, T)
        ctx.owner, ctx.cum, ctx.dims = owner, cum, tuple(x.shape)  # the int32 prefix sums are all the backward keeps
        ctx.mark_non_differentiable(mel_len)
        return out, mel_len

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        dx = ctx.owner._backward(g, ctx.cum, ctx.dims) if ctx.needs_input_grad[1] else None
        return None, dx, None, None


class LengthRegulator(CountedModule):
    """The reference's ``LengthRegulator`` (model/modules.py:195-230): ``forward(x [B, L, d], duration [B, L], max_len) -> (out [B, max_len, d],
    mel_len [B] int64)``.  Phoneme ``l`` of utterance ``b`` is repeated ``max(duration[b, l], 0)`` times; frames at or past an utterance's
    total are ``+0.0``; frames at or past ``max_len`` are dropped, while ``mel_len`` stays the uncropped total, as the reference returns it.
    Two launches (prefix sums, gather).  ``max_len=None`` pads to the batch maximum, which costs ONE device-to-host read of ``mel_len``
    between the two launches (the reference reads every duration with ``.item()``); pass ``max_len`` to stay asynchronous.

    The backward is one launch: ``d_x[b, l]`` is the sum of ``grad_output[b, t]`` over the phoneme's frames below ``max_len``, in ``t`` order,
    in float64, rounded once; a phoneme of duration 0 gets ``+0.0`` and frames past an utterance's total are never read.  ``duration``
    is an integer tensor (a floating one is truncated, as the reference's ``int()`` does) and takes no gradient."""

    ABI = "ns_va"

    def forward(self, x, duration, max_len=None):
        need_gpu("LengthRegulator", "x", x)
        if x.dtype != torch.float32 or x.dim() != 3 or x.numel() == 0 or x.shape[2] % 4 != 0:
            raise ValueError(f"x must be a non-empty float32 [B, L, d] tensor with d a multiple of 4, got {x.dtype} {tuple(x.shape)}")
        if tuple(duration.shape) != tuple(x.shape[:2]) or duration.device != x.device or duration.dtype == torch.bool:
            raise ValueError(f"duration must be a [B, L] = {tuple(x.shape[:2])} tensor on {x.device}, got {tuple(duration.shape)} on {duration.device}")
        if max_len is not None and int(max_len) <= 0:
            raise ValueError(f"max_len must be positive or None, got {max_len}")
        T = None if max_len is None else int(max_len)
        if torch.is_grad_enabled() and x.requires_grad:
            return _RegulateFunction.apply(self, x, duration, T)
        return self._forward(x, duration, T)[:2]

    def _forward(self, x, duration, T):
        dev = x.device
        B, L, D = x.shape
        xa, da = aligned(x.detach()), duration.detach().to(torch.int64).contiguous()
        with guard(dev):
            cum = torch.empty((B, L), dtype=torch.int32, device=dev)
            mel_len = torch.empty((B,), dtype=torch.int64, device=dev)
            st = _lib.stream_ptr(dev)
            first = _lib.ptr(da)
            if T is None:  # the scan alone, then the one read of the batch maximum
                self._done(self._lib.ns_va_op_lr_fwd(None, first, B, L, D, 0, None, _lib.ptr(cum), _lib.ptr(mel_len), st), "forward", "ns_va_op_lr_fwd")
                T = int(mel_len.max().item())
                if T <= 0:
                    raise ValueError("LengthRegulator: every duration is zero and max_len is None: there is no frame to pad to")
                first = None
            out = torch.empty((B, T, D), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_va_op_lr_fwd(_lib.ptr(xa), first, B, L, D, T, _lib.ptr(out), _lib.ptr(cum), _lib.ptr(mel_len), st),
                       "forward", "ns_va_op_lr_fwd", add=first is None)
        return out, mel_len, cum

    def _backward(self, g, cum, dims):
        dev = cum.device
        B, L, D = dims
        if g.dim() != 3 or g.shape[0] != B or g.shape[2] != D or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 [{B}, T, {D}] tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        with guard(dev):
            dx = torch.empty((B, L, D), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_va_op_lr_bwd(_lib.ptr(g), _lib.ptr(cum), B, L, D, g.shape[1], _lib.ptr(dx), _lib.stream_ptr(dev)),
                       "backward", "ns_va_op_lr_bwd")
        return dx


class _GaussianFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, x, duration, T):
        out, mel_len, centres = owner._forward(x, duration, T)
        ctx.owner, ctx.centres, ctx.mel_len, ctx.dims = owner, centres, mel_len, tuple(x.shape)  # the fp32 centres and the totals are all the backward keeps
        ctx.mark_non_differentiable(mel_len)
        return out, mel_len

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        dx = ctx.owner._backward(g, ctx.centres, ctx.mel_len, ctx.dims) if ctx.needs_input_grad[1] else None
        return None, dx, None, None


class GaussianUpsampling(CountedModule):
    """The reference's ``GaussianUpsampling`` (model/modules.py:162-192) in the ``LengthRegulator``'s place and with its signature:
    ``forward(x [B, L, d], duration [B, L], max_len=None) -> (out [B, max_len, d], mel_len [B] int64)``.  With
    ``c_l = cumsum(d)_l - d_l / 2`` (``d = max(duration, 0)``) frame ``t`` of an utterance is ``sum_l w_lt x_l``,
    ``w_lt = exp(-0.01 (t - c_l)^2) / (sum_l exp(-0.01 (t - c_l)^2) + 1e-20)``; frames at or past the utterance's total are ``+0.0``, frames at
    or past ``max_len`` are dropped, and ``mel_len`` stays the uncropped total — what ``model.FastSpeech2Align`` computes with
    ``model_config["length_regulator"] = "gaussian"`` (the same launch, so the same bits).  Three launches (prepare, centres, upsample).
    ``max_len=None`` pads to the batch maximum, which costs ONE device-to-host read of ``mel_len`` and one more prepare launch; pass
    ``max_len`` to stay asynchronous.

    The backward is two launches: the denominators, then ``d_x[b, l] = sum_t w_lt grad_output[b, t]`` over the live frames in ``t`` order
    on the fp32 matrix cores, with the forward's own weights bit for bit; a frame further than 102 frames from every centre of a
    32-phoneme tile has weight exactly ``+0.0`` for it and is not read.  A padded phoneme (duration 0) sits at the utterance's total and
    takes the gradient the transpose gives it, as it feeds the forward.  ``duration`` is an integer tensor (a floating one is
    truncated) and takes no gradient; the range is the reference's constant 10.  No parameters."""

    ABI = "ns_va"

    def forward(self, x, duration, max_len=None):
        need_gpu("GaussianUpsampling", "x", x)
        if x.dtype != torch.float32 or x.dim() != 3 or x.numel() == 0 or x.shape[2] % 4 != 0:
            raise ValueError(f"x must be a non-empty float32 [B, L, d] tensor with d a multiple of 4, got {x.dtype} {tuple(x.shape)}")
        if tuple(duration.shape) != tuple(x.shape[:2]) or duration.device != x.device or duration.dtype == torch.bool:
            raise ValueError(f"duration must be a [B, L] = {tuple(x.shape[:2])} tensor on {x.device}, got {tuple(duration.shape)} on {duration.device}")
        if max_len is not None and int(max_len) <= 0:
            raise ValueError(f"max_len must be positive or None, got {max_len}")
        T = None if max_len is None else int(max_len)
        if torch.is_grad_enabled() and x.requires_grad:
            return _GaussianFunction.apply(self, x, duration, T)
        return self._forward(x, duration, T)[:2]

    def _workspace(self, B, L, T, dev):
        n = self._lib.ns_va_gu_ws_bytes(B, L, T)
        if n == 0:
            _lib.check(1, "ns_va_gu_ws_bytes")
        return torch.empty(n, dtype=torch.uint8, device=dev)

    def _forward(self, x, duration, T):
        dev = x.device
        B, L, D = x.shape
        xa, da = aligned(x.detach()), duration.detach().to(torch.int64).contiguous()
        with guard(dev):
            centres = torch.empty((B, L), dtype=torch.float32, device=dev)
            mel_len = torch.empty((B,), dtype=torch.int64, device=dev)
            st = _lib.stream_ptr(dev)
            add = False
            if T is None:  # the prepare launch alone, then the one read of the batch maximum
                ws = self._workspace(B, L, 1, dev)
                self._done(self._lib.ns_va_op_gu_fwd(None, _lib.ptr(da), B, L, D, 0, None, _lib.ptr(centres), _lib.ptr(mel_len), _lib.ptr(ws), ws.numel(),
                                                     st), "forward", "ns_va_op_gu_fwd")
                T = int(mel_len.max().item())
                if T <= 0:
                    raise ValueError("GaussianUpsampling: every duration is zero and max_len is None: there is no frame to pad to")
                add = True
            ws = self._workspace(B, L, T, dev)
            out = torch.empty((B, T, D), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_va_op_gu_fwd(_lib.ptr(xa), _lib.ptr(da), B, L, D, T, _lib.ptr(out), _lib.ptr(centres), _lib.ptr(mel_len), _lib.ptr(ws),
                                                 ws.numel(), st), "forward", "ns_va_op_gu_fwd", add=add)
        return out, mel_len, centres

    def _backward(self, g, centres, mel_len, dims, w_out=None):
        dev = centres.device
        B, L, D = dims
        if g.dim() != 3 or g.shape[0] != B or g.shape[2] != D or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 [{B}, T, {D}] tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        T = g.shape[1]
        with guard(dev):
            ws = self._workspace(B, L, T, dev)
            dx = torch.empty((B, L, D), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_va_op_gu_bwd(_lib.ptr(g), _lib.ptr(centres), _lib.ptr(mel_len), B, L, D, T, _lib.ptr(dx), _lib.ptr(w_out), _lib.ptr(ws),
                                                 ws.numel(), _lib.stream_ptr(dev)), "backward", "ns_va_op_gu_bwd")
        return dx


REGULATORS = {"hard": LengthRegulator, "gaussian": GaussianUpsampling}


class VarianceAdaptor(torch.nn.Module):
    """Drop-in for ``VarianceAdaptor(preprocess_config, model_config)`` on its teacher-forced branch: the reference's state-dict keys
    (``pitch_bins``, ``energy_bins`` — Parameters with ``requires_grad=False`` — ``pitch_embedding.weight``, ``energy_embedding.weight``,
    ``duration_predictor.*``, ``pitch_predictor.*``, ``energy_predictor.*``), so a checkpoint's ``variance_adaptor.*`` slice loads with
    ``strict=True``; the reference's ``forward`` signature and its 7-tuple ``(x, pitch_prediction, energy_prediction,
    log_duration_prediction, duration_rounded, mel_len, mel_mask)``, where ``duration_rounded`` is ``duration_target`` itself and ``mel_mask``
    is passed through.  All four mixes of ``phoneme_level`` / ``frame_level`` for pitch and energy: a phoneme-level feature is predicted and
    embedded before the length regulator (mask ``src_mask``), a frame-level one after it (mask ``mel_mask``); energy reads ``x`` with the
    pitch embedding already added.  ``model_config["length_regulator"]`` (an extension key, absent = ``"hard"``) chooses what sits in
    ``self.length_regulator``: ``"hard"`` the ``LengthRegulator``, ``"gaussian"`` the ``GaussianUpsampling`` — neither has parameters, so
    the state-dict keys do not depend on it; any other value raises ``ValueError``.

    The bin edges come from ``<preprocessed_path>/stats.json`` through ``workload.variance_bins``, or from ``workload.SYNTH_STATS`` where
    that file is absent; a loaded checkpoint replaces them.  ``pitch_target``, ``energy_target`` and ``duration_target`` must all be
    given and the controls must be 1.0: without targets the reference predicts, rounds and regulates by its own predictions, which is the
    inference path — ``model.FastSpeech2Align``.  ``max_len=None`` costs one device-to-host read (LengthRegulator).  ``keep_masks`` (an
    extension) maps ``"duration"`` / ``"pitch"`` / ``"energy"`` to the predictor's ``(k1, k2)``; otherwise each predictor draws its own in
    ``train()``.

    Autograd connects the HIP Functions; the gradient additions at the fan-outs of ``x`` are torch's (see the module docstring).
    ``launches()`` sums the C side's launch counters of the six HIP submodules."""

    def __init__(self, preprocess_config, model_config):
        super().__init__()
        kind = model_config.get("length_regulator", "hard")  # the inference side's extension key (model.FastSpeech2Align)
        if kind not in REGULATORS:
            raise ValueError(f"model_config['length_regulator'] must be one of {tuple(REGULATORS)}, got {kind!r}")
        self.length_regulator = REGULATORS[kind]()
        self.duration_predictor = VariancePredictor(model_config)
        self.pitch_predictor = VariancePredictor(model_config)
        self.energy_predictor = VariancePredictor(model_config)
        self.pitch_feature_level = preprocess_config["preprocessing"]["pitch"]["feature"]
        self.energy_feature_level = preprocess_config["preprocessing"]["energy"]["feature"]
        for name, level in (("pitch", self.pitch_feature_level), ("energy", self.energy_feature_level)):
            if level not in LEVELS:
                raise ValueError(f"preprocessing.{name}.feature must be one of {LEVELS}, got {level!r}")
        for name in ("pitch", "energy"):
            q = model_config["variance_embedding"][f"{name}_quantization"]
            if q not in ("linear", "log"):
                raise ValueError(f"variance_embedding.{name}_quantization must be 'linear' or 'log', got {q!r}")
        stats = wl.SYNTH_STATS
        path = os.path.join(preprocess_config.get("path", {}).get("preprocessed_path", ""), "stats.json")
        if os.path.exists(path):
            with open(path) as f:
                stats = json.load(f)
        pb, eb = wl.variance_bins(model_config, stats)
        self.pitch_bins = torch.nn.Parameter(torch.from_numpy(pb.copy()), requires_grad=False)
        self.energy_bins = torch.nn.Parameter(torch.from_numpy(eb.copy()), requires_grad=False)
        n_bins, d = model_config["variance_embedding"]["n_bins"], model_config["transformer"]["encoder_hidden"]
        self.pitch_embedding = VarianceEmbedding(n_bins, d)
        self.energy_embedding = VarianceEmbedding(n_bins, d)

    def hip_modules(self):
        return (self.duration_predictor, self.pitch_predictor, self.energy_predictor, self.pitch_embedding, self.energy_embedding, self.length_regulator)

    def launches(self):
        """kernel launches enqueued so far by the six HIP submodules, as the C side counted them"""
        return sum(m.launches for m in self.hip_modules())

    def forward(self, x, src_mask, mel_mask=None, max_len=None, pitch_target=None, energy_target=None, duration_target=None,
                p_control=1.0, e_control=1.0, d_control=1.0, keep_masks=None):
        if pitch_target is None or energy_target is None or duration_target is None:
            raise NotImplementedError("VarianceAdaptor is the teacher-forced training branch: pitch_target, energy_target and duration_target must all "
                                      "be given.  Synthesis from the model's own predictions is model.FastSpeech2Align (the inference path).")
        if (p_control, e_control, d_control) != (1.0, 1.0, 1.0):
            raise NotImplementedError("the controls scale predictions on the inference path only (model.FastSpeech2Align); with targets given they must be 1.0")
        need_gpu("VarianceAdaptor", "x", x)
        km = keep_masks or {}
        log_duration_prediction = self.duration_predictor(x, src_mask, keep_masks=km.get("duration"))
        pitch_prediction = energy_prediction = None
        if self.pitch_feature_level == "phoneme_level":
            pitch_prediction = self.pitch_predictor(x, src_mask, keep_masks=km.get("pitch"))
            x = self.pitch_embedding(x, pitch_target, self.pitch_bins)
        if self.energy_feature_level == "phoneme_level":
            energy_prediction = self.energy_predictor(x, src_mask, keep_masks=km.get("energy"))
            x = self.energy_embedding(x, energy_target, self.energy_bins)
        x, mel_len = self.length_regulator(x, duration_target, max_len)
        if self.pitch_feature_level == "frame_level":
            pitch_prediction = self.pitch_predictor(x, mel_mask, keep_masks=km.get("pitch"))
            x = self.pitch_embedding(x, pitch_target, self.pitch_bins)
        if self.energy_feature_level == "frame_level":
            energy_prediction = self.energy_predictor(x, mel_mask, keep_masks=km.get("energy"))
            x = self.energy_embedding(x, energy_target, self.energy_bins)
        return x, pitch_prediction, energy_prediction, log_duration_prediction, duration_target, mel_len, mel_mask
