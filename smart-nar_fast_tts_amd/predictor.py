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
from collections import OrderedDict

import torch

from . import _lib
from .loss import _guard

PARAM_NAMES = ("conv_layer.conv1d_1.conv.weight", "conv_layer.conv1d_1.conv.bias", "conv_layer.layer_norm_1.weight",
               "conv_layer.layer_norm_1.bias", "conv_layer.conv1d_2.conv.weight", "conv_layer.conv1d_2.conv.bias",
               "conv_layer.layer_norm_2.weight", "conv_layer.layer_norm_2.bias", "linear_layer.weight", "linear_layer.bias")  # order of ns_pg_weights
MAX_WORKSPACES = 8
_WS = OrderedDict()  # (device index, stream handle, B, S, Cin, F, K) -> workspace, least recently used first


def workspace(lib, shape, device) -> torch.Tensor:
    """The ``ns_pg_*`` workspace of this shape on the current stream of ``device`` (cached; at most ``MAX_WORKSPACES`` are kept)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, shape.B, shape.S, shape.Cin, shape.F, shape.K)
    w = _WS.get(key)
    if w is None:
        n = lib.ns_pg_ws_bytes(C.byref(shape))
        if n == 0:
            _lib.check(1, "ns_pg_ws_bytes")
        w = torch.empty(n, dtype=torch.uint8, device=device)
        _WS[key] = w
    _WS.move_to_end(key)
    while len(_WS) > MAX_WORKSPACES:
        _WS.popitem(last=False)
    return w


def _aligned(t):
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class _Call:
    """One marshalled call: the shape, the weight block and everything that must stay alive until the launches have run."""
    __slots__ = ("shape", "weights", "x", "mask", "keep", "p", "device", "params")


class _PredictorFunction(torch.autograd.Function):
    """forward = ns_pg_forward (keeps v1, h1, v2), backward = ns_pg_backward; the differentiable tensors are x and the ten parameters."""

    @staticmethod
    def forward(ctx, owner, call, x, *params):
        pred, saved = owner._forward(call, save=True)
        ctx.owner, ctx.call, ctx.saved = owner, call, saved
        ctx.save_for_backward(x, *params)  # (autograd then refuses a backward after an in-place change of a parameter)
        return pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ctx.saved_tensors  # noqa: B018  (the version check)
        grads = ctx.owner._backward(ctx.call, ctx.saved, g, ctx.needs_input_grad[2:])
        return (None, None) + tuple(grads)


class _Conv(torch.nn.Module):  # the reference's Conv wrapper (model/modules.py:289-332): a holder of `conv.weight` / `conv.bias`
    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = torch.nn.Conv1d(cin, cout, kernel_size=k, padding=(k - 1) // 2)


class VariancePredictor(torch.nn.Module):
    """Drop-in for ``VariancePredictor(model_config)``: the same parameter names, the same ``forward(encoder_output, mask) -> [B, S]``.

    ``mask`` is a bool [B, S] tensor (True = padded) or None.  Under ``torch.no_grad()``, or when neither the input nor a parameter
    requires grad, a call is five launches and keeps nothing.  Otherwise it is one ``torch.autograd.Function`` (single backward) that
    keeps ``v1 = relu(conv1d_1(x))``, ``h1`` and ``v2`` (3 B S F floats) and whose backward honours ``needs_input_grad``: a tensor that
    needs no gradient gets no buffer, no write and no launch of its own, and comes back ``None``.  In ``train()`` with ``dropout > 0``
    the two keep-masks are drawn with ``torch.bernoulli`` on the device (``torch.manual_seed`` governs them); ``keep_masks=(k1, k2)``
    (bool or uint8 [B, S, F], nonzero = kept) supplies them instead.  ``eval()`` or ``dropout == 0`` uses none.

    Differs from the reference where it must: ``conv1d_2`` pads with ``(kernel_size - 1) // 2`` (the reference hard-codes 1, which is the
    same at its kernel size 3); filter_size must be 256 or 512, encoder_hidden a multiple of 16, the kernel size odd."""

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
        self._lib = _lib.load()
        self.launches = 0          # kernel launches enqueued so far, as the C side counted them (ns_pg_last_launches)
        self.last_launches = {}    # {"forward": n, "backward": n} of the latest calls

    def ordered_parameters(self):
        named = dict(self.named_parameters())
        return [named[n] for n in PARAM_NAMES]

    # ---- marshalling ---------------------------------------------------------------------------
    def _marshal(self, x, mask, keep_masks):
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise RuntimeError("VariancePredictor: encoder_output must live on the MI355X (there is no CPU path)")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != self.input_size:
            raise ValueError(f"encoder_output must be float32 [B, S, {self.input_size}], got {x.dtype} {tuple(x.shape)}")
        B, S, _ = x.shape
        if B == 0 or S == 0:
            raise ValueError("encoder_output must not be empty")
        dev = x.device
        params = self.ordered_parameters()
        for n, p in zip(PARAM_NAMES, params):
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError(f"{n} must be a float32 tensor on {dev}, got {p.dtype} on {p.device}")
        call = _Call()
        call.device, call.x = dev, _aligned(x.detach())
        call.params = [_aligned(p.detach()) for p in params]
        s = _lib.NsPgShape()
        s.B, s.S, s.Cin, s.F, s.K = B, S, self.input_size, self.filter_size, self.kernel
        call.shape = s
        w = _lib.NsPgWeights()
        for f, p in zip(_lib.PG_NAMES, call.params):
            setattr(w, f, p.data_ptr())
        call.weights = w
        call.mask = None
        if mask is not None:
            if tuple(mask.shape) != (B, S) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
                raise ValueError(f"mask must be a bool [B, S] = {(B, S)} tensor on {dev}, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
            call.mask = (mask != 0).contiguous().view(torch.uint8)
        p = self.dropout if self.training else 0.0
        call.keep = (None, None)
        if keep_masks is not None:
            if p == 0.0:
                raise ValueError("keep_masks given although no dropout applies (eval() or dropout == 0)")
            ks = []
            for k in keep_masks:
                if tuple(k.shape) != (B, S, self.filter_size) or k.device != dev:
                    raise ValueError(f"a keep-mask must have shape {(B, S, self.filter_size)} on {dev}, got {tuple(k.shape)} on {k.device}")
                ks.append(_aligned((k != 0).contiguous().view(torch.uint8)))
            if len(ks) != 2:
                raise ValueError("keep_masks must be a pair (dropout_1, dropout_2)")
            call.keep = tuple(ks)
        elif p > 0.0:
            with _guard(dev):
                prob = torch.full((2, B, S, self.filter_size), 1.0 - p, dtype=torch.float32, device=dev)
                k = torch.bernoulli(prob).to(torch.uint8)
            call.keep = (k[0], k[1])
        call.p = p
        return call

    # ---- forward / backward ----------------------------------------------------------------------
    def forward(self, encoder_output, mask=None, keep_masks=None):
        call = self._marshal(encoder_output, mask, keep_masks)
        params = self.ordered_parameters()
        if not (torch.is_grad_enabled() and (encoder_output.requires_grad or any(p.requires_grad for p in params))):
            return self._forward(call, save=False)[0]
        return _PredictorFunction.apply(self, call, encoder_output, *params)

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with _guard(dev):
            ws = workspace(self._lib, s, dev)
            pred = torch.empty((s.B, s.S), dtype=torch.float32, device=dev)
            saved = torch.empty(self._lib.ns_pg_saved_bytes(C.byref(s)) // 4, dtype=torch.float32, device=dev) if save else None
            _lib.check(self._lib.ns_pg_forward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.mask), _lib.ptr(call.keep[0]),
                                               _lib.ptr(call.keep[1]), call.p, _lib.ptr(pred), _lib.ptr(saved), _lib.ptr(ws), ws.numel(),
                                               _lib.stream_ptr(dev)), "ns_pg_forward")
        n = self._lib.ns_pg_last_launches()
        self.launches += n
        self.last_launches["forward"] = n
        return pred, saved

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * pred).sum()``: a list (dx, then the ten of PARAM_NAMES) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.S) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.S)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = g.contiguous()
        with _guard(dev):
            outs = [torch.empty_like(t, memory_format=torch.contiguous_format) if n else None for t, n in zip([call.x] + call.params, need)]
            d = _lib.NsPgGrads()
            d.dx = outs[0].data_ptr() if outs[0] is not None else None
            for f, o in zip(_lib.PG_NAMES, outs[1:]):
                setattr(d, f, o.data_ptr() if o is not None else None)
            ws = workspace(self._lib, s, dev)
            _lib.check(self._lib.ns_pg_backward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.mask), _lib.ptr(call.keep[0]),
                                                _lib.ptr(call.keep[1]), call.p, _lib.ptr(saved), _lib.ptr(g), C.byref(d), _lib.ptr(ws),
                                                ws.numel(), _lib.stream_ptr(dev)), "ns_pg_backward")
        n = self._lib.ns_pg_last_launches()
        self.launches += n
        self.last_launches["backward"] = n
        return outs
