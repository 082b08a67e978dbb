"""What the trainable HIP layers share on the Python side (predictor.VariancePredictor over ``ns_pg_*``, the two attentions of
sublayers.py over ``ns_ag_*`` / ``ns_xg_*``, its PositionwiseFeedForward over ``ns_fg_*`` and its Prenet over ``ns_me_*``, postnet.PostNet over ``ns_pn_*``, the
embedding and the length regulator of adaptor.py over ``ns_va_*``): the device guards, the launch bookkeeping (``CountedModule``), the workspace cache, the autograd Functions and the
module base class that marshals the inputs, the parameters, the keep-masks and the gradient block.  A layer keeps its constructor
checks, its ``PARAM_NAMES``, its shape struct, its mask handling and its two ctypes calls.  The cross-attention has two outputs, one of
them saved for the backward, and so brings ``CrossTrainFunction`` next to ``TrainFunction``; everything else it takes from the base."""
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


def need_gpu(who, name, t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{who}: {name} must live on the MI355X (there is no CPU path)")


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
    """One marshalled call: the shape, the weight block and everything that must stay alive until the launches have run.  ``inputs``
    are the differentiable inputs in the order of the layer's ``INPUT_GRADS`` (``x`` first; the cross-attention adds ``src``);
    ``training`` and ``buffers`` are the BatchNorm mode and the live running statistics of a layer that has them; ``pos`` is the
    position table of a Prenet call."""
    __slots__ = ("shape", "weights", "x", "src", "inputs", "mask", "lens", "keep", "p", "training", "buffers", "device", "params", "pos")


class TrainFunction(torch.autograd.Function):
    """forward = the owner's ``_forward`` (keeps its saved buffer), backward = its ``_backward``; the differentiable tensors are x and
    the parameters."""

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


class CountedModule(torch.nn.Module):
    """Launch bookkeeping of a module over one handle-less C ABI, named by the subclass's ``ABI`` ("ns_pg"): ``launches`` enqueued so
    far and ``last_launches`` per direction, as the C side counted them (``ns_*_last_launches``)."""

    def __init__(self):
        super().__init__()
        self._lib = _lib.load()
        self.launches = 0
        self.last_launches = {}    # {"forward": n, "backward": n} of the latest calls

    def _done(self, rc, which, entry=None, add=False):
        """Raises on a failed entry point (``ns_*_forward`` / ``ns_*_backward`` unless ``entry`` names another), else books its
        launches under ``which``; ``add``: on top of the call before, for a direction made of two calls."""
        _lib.check(rc, entry or f"{self.ABI}_{which}")
        n = getattr(self._lib, self.ABI + "_last_launches")()
        self.launches += n
        self.last_launches[which] = n + (self.last_launches.get(which, 0) if add else 0)


class HipTrainModule(CountedModule):
    """Base of a layer whose forward and backward are one handle-less C ABI.  It holds no parameter, buffer or submodule of its own.
    A subclass sets ``ABI`` ("ns_pg"), ``PARAM_NAMES`` (checkpoint names, ABI order), ``FIELDS`` (the same as struct fields),
    ``WEIGHTS`` / ``GRADS`` (the ctypes structs), ``WORKSPACES`` (its WorkspaceCache), ``INPUT`` (what messages call ``x``) and, where
    it has more differentiable inputs than ``x``, ``INPUT_GRADS`` (their fields in GRADS), and defines ``_forward(call, save) -> (y,
    saved)`` and ``_backward(call, saved, g, need) -> [input gradients, parameter gradients]``."""

    INPUT_GRADS = ("dx",)
    _keep_mask_rng = None  # a dropout.KeepMaskRNG once dropout.attach() set one; None: torch.bernoulli draws the masks

    def ordered_parameters(self):
        named = dict(self.named_parameters())
        return [named[n] for n in self.PARAM_NAMES]

    def _begin(self, x, width) -> Call:
        """Checks ``x`` (float32 [B, S, width] on the GPU) and the parameters; a Call with device, x, params and the weight block."""
        need_gpu(type(self).__name__, self.INPUT, x)
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
        call.inputs = [call.x]
        call.params = [aligned(p.detach()) for p in params]
        call.weights = self.WEIGHTS()
        for f, p in zip(self.FIELDS, call.params):
            setattr(call.weights, f, p.data_ptr())
        call.src = call.mask = call.lens = call.buffers = None
        call.training = False
        return call

    def _keep_masks(self, given, shapes, dev, p, stacked=False):
        """The keep-masks (uint8, one per entry of ``shapes``) of a call at drop probability ``p``: the ``given`` ones validated, else
        drawn with ``torch.bernoulli`` — one draw per mask in order, or, ``stacked`` (the shapes are equal), one draw of all of them —
        else Nones.  With a generator attached (``dropout.attach``) the draw is its ``take``: consecutive streams, one per mask."""
        n = len(shapes)
        arg, one = ("keep_masks", "a keep-mask") if n > 1 else ("keep_mask", "keep_mask")
        if given is not None:
            if p == 0.0:
                raise ValueError(f"{arg} given although no dropout applies (eval() or dropout == 0)")
            given = list(given)
            if len(given) != n:
                raise ValueError(f"keep_masks must hold {n} masks, got {len(given)}")
            for k, shape in zip(given, shapes):
                if tuple(k.shape) != shape or k.device != dev:
                    raise ValueError(f"{one} must have shape {shape} on {dev}, got {tuple(k.shape)} on {k.device}")
            return tuple(aligned((k != 0).contiguous().view(torch.uint8)) for k in given)
        if p > 0.0 and self._keep_mask_rng is not None:
            return self._keep_mask_rng.take(shapes, p, dev)
        if p > 0.0:
            draws =[(n,) + shapes[0]] if stacked else shapes
            with guard(dev):
                ks = [torch.bernoulli(torch.full(s, 1.0 - p, dtype=torch.float32, device=dev)).to(torch.uint8) for s in draws]
            return tuple(ks[0]) if stacked else tuple(ks)
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
        """(outs, GRADS struct): a fresh tensor for each input and each parameter that ``need`` asks for, None and a null pointer
        elsewhere."""
        outs = [torch.empty_like(t, memory_format=torch.contiguous_format) if n else None for t, n in zip(call.inputs + call.params, need)]
        d = self.GRADS()
        for f, o in zip(self.INPUT_GRADS + tuple(self.FIELDS), outs):
            setattr(d, f, o.data_ptr() if o is not None else None)
        return outs, d
