"""What the trainable HIP layers share on the Python side (predictor.VariancePredictor over ``ns_pg_*``, sublayers.MultiHeadAttention
over ``ns_ag_*``): the device guard, the workspace cache, the one ``torch.autograd.Function`` and the module base class that marshals
the input, the ten parameters, the keep-masks and the gradient block.  A layer keeps its constructor checks, its ``PARAM_NAMES``, its
shape struct, its mask handling and its two ctypes calls.  sublayers.MultiHeadCrossAttention (``ns_xg_*``) has two inputs and two
outputs and brings its own function, ``CrossTrainFunction``, and its own marshalling on the same base."""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import OrderedDict

import torch

from . import _lib


def guard(dev):
    return contextlib.nullcontext() if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def aligned(t):
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class WorkspaceCache:
    """The workspaces of one layer: (device index, stream handle, the shape's fields) -> tensor, least recently used first, at most
    ``MAX`` kept.  ``query`` is the layer's ``ns_*_ws_bytes``."""
    MAX = 8

    def __init__(self, query, fields):
        self.query, self.fields, self.kept = query, fields, OrderedDict()

    def get(self, lib, shape, device) -> torch.Tensor:
        """The workspace of this shape on the current stream of ``device``."""
        key = (device.index, torch.cuda.current_stream(device).cuda_stream) + tuple(getattr(shape, f) for f in self.fields)
        w = self.kept.get(key)
        if w is None:
            n = getattr(lib, self.query)(C.byref(shape))
            if n == 0:
                _lib.check(1, self.query)
            w = torch.empty(n, dtype=torch.uint8, device=device)
            self.kept[key] = w
        self.kept.move_to_end(key)
        while len(self.kept) > self.MAX:
            self.kept.popitem(last=False)
        return w


class Call:
    """One marshalled call: the shape, the weight block and everything that must stay alive until the launches have run."""
    __slots__ = ("shape", "weights", "x", "src", "mask", "lens", "keep", "p", "device", "params")


class TrainFunction(torch.autograd.Function):
    """forward = the owner's ``_forward`` (keeps its saved buffer), backward = its ``_backward``; the differentiable tensors are x and
    the ten parameters."""

    @staticmethod
    def forward(ctx, owner, call, x, *params):
        y, saved = owner._forward(call, save=True)
        ctx.owner, ctx.call, ctx.saved = owner, call, saved
        ctx.save_for_backward(x, *params)  # (autograd then refuses a backward after an in-place change of a parameter)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ctx.saved_tensors  # noqa: B018  (the version check)
        grads = ctx.owner._backward(ctx.call, ctx.saved, g, ctx.needs_input_grad[2:])
        return (None, None) + tuple(grads)


class CrossTrainFunction(torch.autograd.Function):
    """The same for a layer with two differentiable inputs and two outputs (sublayers.MultiHeadCrossAttention): forward = the owner's
    ``_forward`` -> (y, attn, saved buffer), backward = its ``_backward`` from the gradients of both outputs.  The attention map is the
    layer's own output and is saved as such, so autograd's version counter refuses a backward after an in-place change of it.  Absent
    output gradients arrive as ``None`` (``set_materialize_grads(False)``): an unused map costs no zero tensor and no read."""

    @staticmethod
    def forward(ctx, owner, call, tgt, src, *params):
        y, attn, saved = owner._forward(call, save=True)
        ctx.owner, ctx.call, ctx.saved = owner, call, saved
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(tgt, src, attn, *params)
        return y, attn

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, d_attn):
        attn = ctx.saved_tensors[2]  # (the version check of every saved tensor)
        grads = ctx.owner._backward(ctx.call, ctx.saved, attn, g, d_attn, ctx.needs_input_grad[2:])
        return (None, None) + tuple(grads)


class HipTrainModule(torch.nn.Module):
    """Base of a layer whose forward and backward are one handle-less C ABI.  It holds no parameter, buffer or submodule of its own.
    A subclass sets ``ABI`` ("ns_pg"), ``PARAM_NAMES`` (checkpoint names, ABI order), ``FIELDS`` (the same ten as struct fields),
    ``WEIGHTS`` / ``GRADS`` (the ctypes structs), ``WORKSPACES`` (its WorkspaceCache) and ``INPUT`` (what messages call ``x``), and
    defines ``_forward(call, save) -> (y, saved)`` and ``_backward(call, saved, g, need) -> [dx, ten gradients]``."""

    def __init__(self):
        super().__init__()
        self._lib = _lib.load()
        self.launches = 0          # kernel launches enqueued so far, as the C side counted them (ns_*_last_launches)
        self.last_launches = {}    # {"forward": n, "backward": n} of the latest calls

    def ordered_parameters(self):
        named = dict(self.named_parameters())
        return [named[n] for n in self.PARAM_NAMES]

    def _begin(self, x, width) -> Call:
        """Checks ``x`` (float32 [B, S, width] on the GPU) and the parameters; a Call with device, x, params and the weight block."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise RuntimeError(f"{type(self).__name__}: {self.INPUT} must live on the MI355X (there is no CPU path)")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != width:
            raise ValueError(f"{self.INPUT} must be float32 [B, S, {width}], got {x.dtype} {tuple(x.shape)}")
        if x.shape[0] == 0 or x.shape[1] == 0:
            raise ValueError(f"{self.INPUT} must not be empty")
        dev = x.device
        params = self.ordered_parameters()
        for n, p in zip(self.PARAM_NAMES, params):
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError(f"{n} must be a float32 tensor on {dev}, got {p.dtype} on {p.device}")
        call = Call()
        call.device, call.x = dev, aligned(x.detach())
        call.params = [aligned(p.detach()) for p in params]
        call.weights = self.WEIGHTS()
        for f, p in zip(self.FIELDS, call.params):
            setattr(call.weights, f, p.data_ptr())
        call.src = call.mask = call.lens = None
        return call

    def _keep_masks(self, given, n, shape, dev, p):
        """The ``n`` keep-masks (uint8 ``shape``) of a call at drop probability ``p``: the ``given`` ones validated, else one
        ``torch.bernoulli`` draw of all ``n``, else ``n`` Nones."""
        arg, one = ("keep_masks", "a keep-mask") if n > 1 else ("keep_mask", "keep_mask")
        if given is not None:
            if p == 0.0:
                raise ValueError(f"{arg} given although no dropout applies (eval() or dropout == 0)")
            ks = []
            for k in given:
                if tuple(k.shape) != shape or k.device != dev:
                    raise ValueError(f"{one} must have shape {shape} on {dev}, got {tuple(k.shape)} on {k.device}")
                ks.append(aligned((k != 0).contiguous().view(torch.uint8)))
            if len(ks) != n:
                raise ValueError("keep_masks must be a pair (dropout_1, dropout_2)")
            return tuple(ks)
        if p > 0.0:
            with guard(dev):
                k = torch.bernoulli(torch.full((n,) + shape if n > 1 else shape, 1.0 - p, dtype=torch.float32, device=dev)).to(torch.uint8)
            return tuple(k[i] for i in range(n)) if n > 1 else (k,)
        return (None,) * n

    def _dispatch(self, call, x):
        """The plain forward, or TrainFunction when autograd will want a backward."""
        params = self.ordered_parameters()
        if not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))):
            return self._forward(call, save=False)[0]
        return TrainFunction.apply(self, call, x, *params)

    def _workspace(self, call, save):
        """(workspace, saved buffer or None); under ``guard(call.device)``."""
        ws = self.WORKSPACES.get(self._lib, call.shape, call.device)
        if not save:
            return ws, None
        n = getattr(self._lib, self.ABI + "_saved_bytes")(C.byref(call.shape)) // 4
        return ws, torch.empty(n, dtype=torch.float32, device=call.device)

    def _grad_block(self, call, need):
        """(outs, GRADS struct): a fresh tensor for dx and each parameter that ``need`` asks for, None and a null pointer elsewhere."""
        outs = [torch.empty_like(t, memory_format=torch.contiguous_format) if n else None for t, n in zip([call.x] + call.params, need)]
        d = self.GRADS()
        for f, o in zip(("dx",) + tuple(self.FIELDS), outs):
            setattr(d, f, o.data_ptr() if o is not None else None)
        return outs, d

    def _done(self, rc, which):
        """Raises on a failed ``ns_*_forward`` / ``ns_*_backward``, else books its launches."""
        _lib.check(rc, f"{self.ABI}_{which}")
        n = getattr(self._lib, self.ABI + "_last_launches")()
        self.launches += n
        self.last_launches[which] = n
