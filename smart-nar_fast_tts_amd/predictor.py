"""The reference's ``VariancePredictor`` (model/modules.py:233-286) as a trainable module whose forward AND backward are HIP
(csrc/predgrad.hip, ``ns_pg_*`` in include/nar_fs2.h): the duration, pitch and energy predictors behind the three loss gradients
``d_log_d``, ``d_pitch`` and ``d_energy`` of ``loss.FastSpeech2TrainingLoss``, in front of ``optim.ScheduledOptim``.

    p = VariancePredictor(model_config).to(device)
    p.load_state_dict({k[len(prefix):]: v for k, v in ckpt["model"].items() if k.startswith(prefix)})   # prefix = "variance_adaptor.pitch_predictor."
    pred = p(encoder_output, src_mask)          # [B, S]
    pred.backward(d_pitch)                      # parameter gradients (and encoder_output.grad when it requires grad)

The parameters are ordinary ``torch.nn.Parameter`` s under the reference's names; every call reads them afresh.  There is no CPU
path and no torch kernel between the input and ``pred`` or between ``grad_output`` and the gradients."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._train import HipTrainModule, WorkspaceCache, guard

PARAM_NAMES = ("conv_layer.conv1d_1.conv.weight", "conv_layer.conv1d_1.conv.bias", "conv_layer.layer_norm_1.weight",
               "conv_layer.layer_norm_1.bias", "conv_layer.conv1d_2.conv.weight", "conv_layer.conv1d_2.conv.bias",
               "conv_layer.layer_norm_2.weight", "conv_layer.layer_norm_2.bias", "linear_layer.weight", "linear_layer.bias")  # order of ns_pg_weights


class _Conv(torch.nn.Module):  # the reference's Conv wrapper (model/modules.py:289-332): a holder of `conv.weight` / `conv.bias`
    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = torch.nn.Conv1d(cin, cout, kernel_size=k, padding=(k - 1) // 2)


class VariancePredictor(HipTrainModule):
    """Drop-in for ``VariancePredictor(model_config)``: the same parameter names, the same ``forward(encoder_output, mask) -> [B, S]``.

    ``mask`` is a bool [B, S] tensor (True = padded) or None.  Under ``torch.no_grad()``, or when neither the input nor a parameter
    requires grad, a call is five launches and keeps nothing.  Otherwise it is one ``torch.autograd.Function`` (single backward) that
    keeps ``v1 = relu(conv1d_1(x))``, ``h1`` and ``v2`` (3 B S F floats) and whose backward honours ``needs_input_grad``: a tensor that
    needs no gradient gets no buffer, no write and no launch of its own, and comes back ``None``.  In ``train()`` with ``dropout > 0``
    the two keep-masks are drawn with ``torch.bernoulli`` on the device (``torch.manual_seed`` governs them); ``keep_masks=(k1, k2)``
    (bool or uint8 [B, S, F], nonzero = kept) supplies them instead.  ``eval()`` or ``dropout == 0`` uses none.

    Differs from the reference where it must: ``conv1d_2`` pads with ``(kernel_size - 1) // 2`` (the reference hard-codes 1, which is the
    same at its kernel size 3); filter_size must be 256 or 512, encoder_hidden a multiple of 16, the kernel size odd."""

    ABI, INPUT, PARAM_NAMES = "ns_pg", "encoder_output", PARAM_NAMES
    FIELDS, WEIGHTS, GRADS = _lib.PG_NAMES, _lib.NsPgWeights, _lib.NsPgGrads
    WORKSPACES = WorkspaceCache("ns_pg_ws_bytes", ("B", "S", "Cin", "F", "K"))

    def __init__(self, model_config: dict):
        super().__init__()
        self.input_size = model_config["transformer"]["encoder_hidden"]
        self.filter_size = model_config["variance_predictor"]["filter_size"]
        self.kernel = model_config["variance_predictor"]["kernel_size"]
        self.conv_output_size = self.filter_size
        self.dropout = float(model_config["variance_predictor"]["dropout"])
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"variance_predictor.dropout must lie in [0, 1), got {self.dropout}")
        layer = torch.nn.Module()
        layer.conv1d_1 = _Conv(self.input_size, self.filter_size, self.kernel)
        layer.layer_norm_1 = torch.nn.LayerNorm(self.filter_size)
        layer.conv1d_2 = _Conv(self.filter_size, self.filter_size, self.kernel)
        layer.layer_norm_2 = torch.nn.LayerNorm(self.filter_size)
        self.conv_layer = layer
        self.linear_layer = torch.nn.Linear(self.conv_output_size, 1)

    def _marshal(self, x, mask, keep_masks):
        call = self._begin(x, self.input_size)
        B, S, _ = x.shape
        dev = call.device
        s = _lib.NsPgShape()
        s.B, s.S, s.Cin, s.F, s.K = B, S, self.input_size, self.filter_size, self.kernel
        call.shape = s
        if mask is not None:
            if tuple(mask.shape) != (B, S) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
                raise ValueError(f"mask must be a bool [B, S] = {(B, S)} tensor on {dev}, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
            call.mask = (mask != 0).contiguous().view(torch.uint8)
        call.p = self.dropout if self.training else 0.0
        call.keep = self._keep_masks(keep_masks, [(B, S, self.filter_size)] * 2, dev, call.p, stacked=True)
        return call

    def forward(self, encoder_output, mask=None, keep_masks=None):
        return self._dispatch(self._marshal(encoder_output, mask, keep_masks), encoder_output)

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with guard(dev):
            ws, saved = self._workspace(call, save)
            pred = torch.empty((s.B, s.S), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_pg_forward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.mask), _lib.ptr(call.keep[0]),
                                               _lib.ptr(call.keep[1]), call.p, _lib.ptr(pred), _lib.ptr(saved), _lib.ptr(ws), ws.numel(),
                                               _lib.stream_ptr(dev)), "forward")
        return pred, saved

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * pred).sum()``: a list (dx, then the ten of PARAM_NAMES) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.S) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.S)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = g.contiguous()
        with guard(dev):
            outs, d = self._grad_block(call, need)
            ws, _ = self._workspace(call, save=False)
            self._done(self._lib.ns_pg_backward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.mask), _lib.ptr(call.keep[0]),
                                                _lib.ptr(call.keep[1]), call.p, _lib.ptr(saved), _lib.ptr(g), C.byref(d), _lib.ptr(ws),
                                                ws.numel(), _lib.stream_ptr(dev)), "backward")
        return outs
