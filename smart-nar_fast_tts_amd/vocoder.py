"""HiFi-GAN vocoder on the MI355X: drop-in for the reference's ``hifigan`` package and utils/model.py:38-88
(``get_vocoder`` / ``vocoder_infer``), over the C-ABI of include/nar_fs2.h (``ns_voc_*``, csrc/vocoder.hip).

The reference's inference tail (synthesize.py -> utils/tools.py:189-199) hands ``postnet_output.transpose(1, 2)`` — [B, 80, T] on
the PADDED grid — to ``Generator.forward`` and trims utterance b to ``mel_lens[b] * hop_length`` samples afterwards; this module
computes on the same padded grid, so every kept sample has the reference's semantics.  A ``transpose(1, 2)`` view of a
contiguous [B, T, 80] tensor is consumed in place, with no copy.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import json
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._handle import DeviceModule, host_f32

DEFAULT_VOCODER = {"model": "HiFi-GAN", "speaker": "LJSpeech"}  # config/LJSpeech/model.yaml `vocoder`
MAX_WAV_VALUE = 32768.0  # config/LJSpeech/preprocess.yaml preprocessing.audio.max_wav_value
HOP_LENGTH = 256         # config/LJSpeech/preprocess.yaml preprocessing.stft.hop_length
MATMUL_MODES = {"fp32": 0, "bf16": 1}  # ns_voc_set_matmul


class AttrDict(dict):
    """hifigan's AttrDict: a dict whose keys are also attributes."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


NsVocConfig = _lib.STRUCTS["ns_voc_config"]


def config_struct(h) -> NsVocConfig:
    """ns_voc_config of a hifigan config.json; shapes the native side cannot hold raise ValueError (it validates the rest)."""
    c = NsVocConfig()
    ups, uks = list(h["upsample_rates"]), list(h["upsample_kernel_sizes"])
    rks, rds = list(h["resblock_kernel_sizes"]), [list(d) for d in h["resblock_dilation_sizes"]]
    if len(ups) != len(uks) or not 1 <= len(ups) <= 4:
        raise ValueError("upsample_rates / upsample_kernel_sizes: 1..4 entries of equal length")
    if len(rks) != len(rds) or not 1 <= len(rks) <= 4:
        raise ValueError("resblock_kernel_sizes / resblock_dilation_sizes: 1..4 entries of equal length")
    if any(len(d) != 3 for d in rds):
        raise ValueError("ResBlock1 takes exactly three dilations per resblock")
    c.n_mel = int(h.get("num_mels", 80))
    c.initial_channel = int(h["upsample_initial_channel"])
    c.n_up, c.n_rb = len(ups), len(rks)
    for i, (u, k) in enumerate(zip(ups, uks)):
        c.up_rates[i], c.up_kernels[i] = int(u), int(k)
    for j, (k, d) in enumerate(zip(rks, rds)):
        c.rb_kernels[j] = int(k)
        for n, dn in enumerate(d):
            c.rb_dilations[j][n] = int(dn)
    c.resblock = 1 if str(h["resblock"]) == "1" else 2
    return c


def fold_weight_norm(weight_g, weight_v) -> torch.Tensor:
    """remove_weight_norm's fold, on the host in float32: weight = g * v / ||v|| over every dim but 0 (torch._weight_norm)."""
    g = torch.as_tensor(weight_g, dtype=torch.float32).cpu()
    v = torch.as_tensor(weight_v, dtype=torch.float32).cpu()
    return torch._weight_norm(v, g, 0)


class Generator(DeviceModule):
    """hifigan.Generator (resblock "1") for inference.  ``load_state_dict`` takes the checkpoint's ``generator`` entry — weight-norm
    ``weight_g`` / ``weight_v`` pairs, folded here exactly like ``remove_weight_norm`` — or plain ``weight`` tensors; unknown keys and
    shape mismatches raise before anything loaded is replaced.  ``remove_weight_norm()`` is then a no-op.

    ``matmul="bf16"`` (opt-in) runs every upsampler and resblock convolution on the bf16 matrix cores: weights and the activated
    inputs rounded to bf16 (round to nearest even), products summed in fp32; everything else stays fp32 (include/nar_fs2.h
    ns_voc_set_matmul).  The default "fp32" path is the one the library runs without the call.

    eval / train / to / cuda / state_dict and the per-stream workspaces: ``_handle.DeviceModule``."""

    KIND = "vocoder"
    NO_TRAINING = "the vocoder is inference-only"
    PICKS_DEVICE_ON_LOAD = True

    def __init__(self, h, matmul: str = "fp32"):
        if matmul not in MATMUL_MODES:
            raise ValueError(f"matmul must be one of {sorted(MATMUL_MODES)}, got {matmul!r}")
        self.h = h if isinstance(h, AttrDict) else AttrDict(h)
        self._cfg = config_struct(self.h)
        self._open("ns_voc", self._cfg, "Generator")
        self.matmul = matmul
        if matmul != "fp32":
            _lib.check(self._lib.ns_voc_set_matmul(self._h, MATMUL_MODES[matmul]), "Generator")
        self.hop = int(np.prod(self.h["upsample_rates"]))
        self.n_mel = int(self._cfg.n_mel)

    def remove_weight_norm(self):
        """Weights are folded when they are loaded (see load_state_dict): nothing left to remove."""
        return None

    def load_state_dict(self, state_dict, strict: bool = True):
        folded, errors = OrderedDict(), []
        sd = dict(state_dict)
        for k in list(sd):
            if k.endswith(".weight_g"):
                p = k[: -len(".weight_g")]
                if p + ".weight_v" not in sd:
                    errors.append(f"'{k}' without '{p}.weight_v'")
                    continue
                g, v = sd.pop(k), sd.pop(p + ".weight_v")
                if torch.as_tensor(g).dim() != torch.as_tensor(v).dim() or torch.as_tensor(g).shape[0] != torch.as_tensor(v).shape[0]:
                    errors.append(f"size mismatch between '{k}' {tuple(torch.as_tensor(g).shape)} and '{p}.weight_v' "
                                  f"{tuple(torch.as_tensor(v).shape)}")
                    continue
                folded[p + ".weight"] = fold_weight_norm(g, v)
        for k in list(sd):
            if k.endswith(".weight_v"):
                errors.append(f"'{k}' without '{k[:-len('_v')]}_g'")
                sd.pop(k)
        folded.update(sd)
        new = OrderedDict()
        for k, t in folded.items():
            a = host_f32(t)
            err = self._h.check_weight(k, a)
            if err:
                errors.append(err)
                continue
            new[k] = a
        expected = self.expected_keys()
        missing = [k for k in expected if k not in new]
        if missing:
            errors.append("missing key(s): " + ", ".join(missing))
        if errors:
            raise RuntimeError("load_state_dict: " + "; ".join(errors))
        return self._loaded(new)

    def expected_keys(self):
        """Plain-weight key names of the native model, in load order."""
        h, keys = self.h, ["conv_pre.weight", "conv_pre.bias"]
        nk = len(h["resblock_kernel_sizes"])
        for i in range(len(h["upsample_rates"])):
            keys += [f"ups.{i}.weight", f"ups.{i}.bias"]
            for j in range(nk):
                for n in range(3):
                    for w in ("convs1", "convs2"):
                        keys += [f"resblocks.{i * nk + j}.{w}.{n}.weight", f"resblocks.{i * nk + j}.{w}.{n}.bias"]
        return keys + ["conv_post.weight", "conv_post.bias"]

    # ---- forward ---------------------------------------------------------------------------------
    def ws_bytes(self, B: int, T: int) -> int:
        return int(self._lib.ns_voc_ws_bytes(self._h, int(B), int(T)))

    def _ready(self, mels):
        if self._sd is None:
            raise RuntimeError("vocoder weights not loaded: call load_state_dict() first")
        if not torch.is_tensor(mels) or mels.device.type != "cuda":
            raise RuntimeError("mels must be a cuda tensor (there is no CPU path)")
        if self._device is None or mels.device != self._device:
            raise RuntimeError(f"mels are on {mels.device}, the vocoder on {self._device}: call .to(device) first")
        if mels.dtype != torch.float32:
            raise TypeError("mels must be float32")

    def __call__(self, mels: torch.Tensor) -> torch.Tensor:
        return self.forward(mels)

    def forward(self, mels: torch.Tensor) -> torch.Tensor:
        """mels [B, n_mel, T] -> waveform [B, 1, T * hop] in [-1, 1] (Generator.forward)."""
        self._ready(mels)
        if mels.dim() != 3 or mels.shape[1] != self.n_mel:
            raise ValueError(f"mels must be [B, {self.n_mel}, T], got {tuple(mels.shape)}")
        B, _, T = mels.shape
        wav = torch.empty(B, 1, T * self.hop, dtype=torch.float32, device=mels.device)
        if B == 0 or T == 0:
            return wav
        if mels.transpose(1, 2).is_contiguous() and mels.data_ptr() % 16 == 0:
            layout, src = _lib.NS["NS_VOC_MEL_TIME_MAJOR"], mels  # a transpose(1, 2) view of a [B, T, n_mel] tensor: read in place
        else:
            layout, src = _lib.NS["NS_VOC_MEL_CHANNEL_MAJOR"], mels.contiguous()
        stream = torch.cuda.current_stream(mels.device).cuda_stream
        nbytes = self.ws_bytes(B, T)
        ws = self._ws.take(self._device, nbytes, stream)
        with torch.cuda.device(mels.device):
            _lib.check(self._lib.ns_voc_forward(self._h, C.c_void_p(src.data_ptr()), layout, B, T, _lib.ptr(wav), _lib.ptr(ws),
                                                nbytes, C.c_void_p(stream)), "ns_voc_forward")
        return wav

    # ---- per-operator entry points (tests; time-major [B, S, C] activations) --------------------------
    def op_conv(self, name: str, x: torch.Tensor) -> torch.Tensor:
        self._ready(x)
        B, S, _ = x.shape
        if name == "conv_pre":
            out = torch.empty(B, S, int(self.h["upsample_initial_channel"]), device=x.device)
        elif name == "conv_post":
            out = torch.empty(B, S, device=x.device)
        else:
            out = torch.empty_like(x)
        x = x.contiguous()
        _lib.check(self._lib.ns_voc_op_conv(self._h, name.encode(), _lib.ptr(x), B, S, _lib.ptr(out), _lib.stream_ptr(x.device)),
                   "ns_voc_op_conv")
        return out

    def op_conv_form(self, name: str, x: torch.Tensor, *, in_act: bool = True, out_act: bool = False, residual=None, mrf: int = 0,
                     acc=None) -> torch.Tensor:
        """One resblock launch ("resblocks.{r}.convs{1,2}.{n}") in a form the stage gives it (ns_voc_op_conv_form):
        v = conv(lrelu(x) if in_act else x) + bias, lrelu(v) if out_act, + residual; mrf 0 returns v, 1 returns acc + v,
        2 returns (acc + v) / n_rb.  ``acc`` (the running multi-receptive-field sum) is required when mrf != 0 and refused
        otherwise; it is cloned into the output, never written."""
        self._ready(x)
        if mrf not in (0, 1, 2):
            raise ValueError(f"mrf must be 0, 1 or 2, got {mrf!r}")
        if (acc is None) != (mrf == 0):
            raise ValueError("acc (the running multi-receptive-field sum) is required when mrf != 0 and refused when mrf == 0")
        B, S, ch = x.shape
        w = self._sd.get(name + ".weight")
        if w is not None and w.shape[1] != ch:  # (an unknown name is the library's to refuse)
            raise ValueError(f"{name} takes [B, S, {w.shape[1]}] activations, got {tuple(x.shape)}")
        x = x.contiguous()
        for t, what in ((residual, "residual"), (acc, "acc")):
            if t is not None and (t.shape != x.shape or t.dtype != torch.float32 or t.device != x.device):
                raise ValueError(f"{what} must be a float32 tensor of x's shape {tuple(x.shape)} on x's device")
        residual = None if residual is None else residual.contiguous()
        out = torch.empty_like(x) if acc is None else acc.clone(memory_format=torch.contiguous_format)
        _lib.check(self._lib.ns_voc_op_conv_form(self._h, name.encode(), _lib.ptr(x), _lib.ptr(residual), _lib.ptr(out), B, S,
                                                 int(bool(in_act)), int(bool(out_act)), int(mrf), _lib.stream_ptr(x.device)),
                   "ns_voc_op_conv_form")
        return out

    def op_upsample(self, i: int, x: torch.Tensor, out=None) -> torch.Tensor:
        """``out``: a caller's [B, S u, C / 2] float32 tensor to write into (tests pre-fill it to see every element written)"""
        self._ready(x)
        B, S, cin = x.shape
        shape = (B, S * int(self.h["upsample_rates"][i]), cin // 2)
        if out is None:
            out = torch.empty(shape, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on x's device")
        x = x.contiguous()
        _lib.check(self._lib.ns_voc_op_upsample(self._h, int(i), _lib.ptr(x), B, S, _lib.ptr(out), _lib.stream_ptr(x.device)),
                   "ns_voc_op_upsample")
        return out

    def op_stage(self, i: int, x: torch.Tensor) -> torch.Tensor:
        self._ready(x)
        B, S, cin = x.shape
        out = torch.empty(B, S * int(self.h["upsample_rates"][i]), cin // 2, device=x.device)
        x = x.contiguous()
        nbytes = self._lib.ns_voc_op_stage_ws_bytes(self._h, int(i), B, S)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(self._lib.ns_voc_op_stage(self._h, int(i), _lib.ptr(x), B, S, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                             _lib.stream_ptr(x.device)), "ns_voc_op_stage")
        return out


def get_vocoder(model_config, device, config_path: str = "hifigan/config.json", ckpt_path=None, matmul=None):
    """utils/model.py:38-67 for "HiFi-GAN": Generator(AttrDict(config.json)), load ckpt["generator"], eval(), remove_weight_norm(),
    to(device).  ``ckpt_path`` defaults to the reference's hifigan/generator_{LJSpeech,universal}.pth.tar by speaker.
    ``matmul`` ("fp32" | "bf16") defaults to ``model_config["vocoder"].get("matmul", "fp32")``.
    "MelGAN" raises: the reference fetches it with torch.hub."""
    voc = model_config.get("vocoder", DEFAULT_VOCODER)
    name, speaker = voc["model"], voc.get("speaker", "LJSpeech")
    if name == "MelGAN":
        raise NotImplementedError("MelGAN is loaded through torch.hub by the reference; only HiFi-GAN has a native implementation")
    if name != "HiFi-GAN":
        raise ValueError(f"unknown vocoder {name!r}")
    if matmul is None:
        matmul = voc.get("matmul", "fp32")
    with open(config_path, "r") as f:
        config = AttrDict(json.load(f))
    vocoder = Generator(config, matmul=matmul)
    if ckpt_path is None:
        if speaker == "LJSpeech":
            ckpt_path = "hifigan/generator_LJSpeech.pth.tar"
        elif speaker == "universal":
            ckpt_path = "hifigan/generator_universal.pth.tar"
        else:
            raise ValueError(f"unknown vocoder speaker {speaker!r}")
    ckpt = torch.load(ckpt_path, map_location="cpu")
    vocoder.load_state_dict(ckpt["generator"])
    vocoder.eval()
    vocoder.remove_weight_norm()
    vocoder.to(device)
    return vocoder


def wav_cast_trim(wavs, preprocess_config, lengths=None):
    """The host half of vocoder_infer (utils/model.py:80-88): float waveforms [B, N] to a list of int16 numpy arrays — scaled by
    max_wav_value in float32, cast with numpy's truncation toward zero — utterance i cut to its first lengths[i] samples."""
    gain = preprocess_config.get("preprocessing", {}).get("audio", {}).get("max_wav_value", MAX_WAV_VALUE)
    pcm = (wavs.detach().cpu().numpy() * gain).astype(np.int16)
    out = list(pcm)
    if lengths is not None:
        out = [w[: lengths[i]] for i, w in enumerate(out)]
    return out


def vocoder_infer(mels, vocoder, model_config, preprocess_config, lengths=None):
    """utils/model.py:70-88 for HiFi-GAN: mels [B, n_mel, T] -> list of int16 numpy waveforms, utterance i cut to lengths[i]."""
    name = model_config.get("vocoder", DEFAULT_VOCODER)["model"]
    if name != "HiFi-GAN":
        raise NotImplementedError(f"vocoder {name!r}: only HiFi-GAN has a native implementation")
    with torch.no_grad():
        wavs = vocoder(mels).squeeze(1)
    return wav_cast_trim(wavs, preprocess_config, lengths)


def hop_length(preprocess_config) -> int:
    return int(preprocess_config.get("preprocessing", {}).get("stft", {}).get("hop_length", HOP_LENGTH))
