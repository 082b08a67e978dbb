"""The reference's ``MultiHeadAttention`` (transformer/SubLayers.py:8-59) as a trainable module whose forward AND backward are HIP
(csrc/attngrad.hip, ``ns_ag_*`` in include/nar_fs2.h), restricted to self-attention — what the ``slf_attn`` of every encoder and
decoder ``FFTBlock`` is.

    a = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout).to(device)
    a.load_state_dict({k[len(prefix):]: v for k, v in ckpt["model"].items() if k.startswith(prefix)})   # prefix = "txt_encoder.layer_stack.0.slf_attn."
    y, _ = a(x, x, x, mask=slf_attn_mask)       # or a(x, x, x, lens=src_lens): no mask tensor, no host read
    y.backward(dy)                              # parameter gradients (and x.grad when it requires grad)

The parameters are ordinary ``torch.nn.Parameter`` s under the reference's names; every call reads them afresh.  There is no CPU
path and no torch kernel between ``x`` and ``y`` or between ``grad_output`` and the gradients.

Deviation from the reference: the second return value is ``None``, not the attention map.  The [B, H, S, S] map is never written to
memory (128 MB per decoder layer at B 16, S 1000), and no caller in the reference's loss reads a SELF-attention map (the guided
attention loss reads the cross-attention maps of ``FFTBlock2.crs_attn``, which this module does not cover)."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch

from . import _lib
from .loss import _guard

PARAM_NAMES = ("w_qs.weight", "w_qs.bias", "w_ks.weight", "w_ks.bias", "w_vs.weight", "w_vs.bias", "fc.weight", "fc.bias",
               "layer_norm.weight", "layer_norm.bias")  # order of ns_ag_weights
MAX_WORKSPACES = 8
_WS = OrderedDict()  # (device index, stream handle, B, S, d, H) -> workspace, least recently used first


def workspace(lib, shape, device) -> torch.Tensor:
    """The ``ns_ag_*`` workspace of this shape on the current stream of ``device`` (cached; at most ``MAX_WORKSPACES`` are kept)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, shape.B, shape.S, shape.d, shape.H)
    w = _WS.get(key)
    if w is None:
        n = lib.ns_ag_ws_bytes(C.byref(shape))
        if n == 0:
            _lib.check(1, "ns_ag_ws_bytes")
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
    __slots__ = ("shape", "weights", "x", "lens", "keep", "p", "device", "params")


class _AttentionFunction(torch.autograd.Function):
    """forward = ns_ag_forward (keeps qkv, ctx, z, lse), backward = ns_ag_backward; the differentiable tensors are x and the ten parameters."""

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


class MultiHeadAttention(torch.nn.Module):
    """Drop-in for ``MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=0.1)`` as a self-attention sublayer: the same parameter
    names (``w_qs``, ``w_ks``, ``w_vs``, ``fc``, ``layer_norm``), ``forward(q, k, v, mask=None, lens=None, keep_mask=None) ->
    (output, None)`` with ``output = layer_norm(dropout(fc(attention)) + q)``, NOT masked (FFTBlock does that outside).

    ``q``, ``k`` and ``v`` must be the same float32 [B, S, d_model] tensor.  The key-padding mask is given either as ``lens`` (int
    [B] on the device: keys ``j >= lens[b]`` are masked) or as the reference's ``mask`` (bool [B, S, S] with ``mask[b, i, j] = j >=
    lens[b]`` for every ``i``); from a mask alone the lengths are derived on the device from ``mask[:, 0, :]`` and, while
    ``validate_mask`` is True, the whole mask is compared with the one those lengths give — one host read per call, which passing
    ``lens`` (with or without the mask) avoids.  With neither, every key is valid.  Padded query rows are computed like any other.

    Under ``torch.no_grad()``, or when neither the input nor a parameter requires grad, a call keeps nothing.  Otherwise it is one
    ``torch.autograd.Function`` (single backward) that keeps ``qkv``, ``ctx``, ``z = dropout(fc(ctx)) + x`` and the row log-sum-exp
    (5 B S d + B H S floats) and whose backward honours ``needs_input_grad``: a tensor that needs no gradient gets no buffer, no write
    and no launch of its own, and comes back ``None``.  In ``train()`` with ``dropout > 0`` the keep-mask is drawn with
    ``torch.bernoulli`` on the device; ``keep_mask`` (bool or uint8 [B, S, d_model], nonzero = kept) supplies it instead.

    Raises on what it cannot do: cross-attention (``q``, ``k``, ``v`` not one tensor), ``d_k != d_v``, ``n_head * d_k != d_model``,
    d_model not 256 or 512, d_k not 32, 64 or 128, a mask that is not a key-padding mask."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.1):
        super().__init__()
        if d_k != d_v:
            raise ValueError(f"MultiHeadAttention: d_k must equal d_v, got {d_k} and {d_v}")
        if n_head * d_k != d_model:
            raise ValueError(f"MultiHeadAttention: n_head * d_k must equal d_model, got {n_head} * {d_k} and {d_model}")
        if d_model not in (256, 512) or d_k not in (32, 64, 128):
            raise ValueError(f"MultiHeadAttention: d_model must be 256 or 512 and d_k 32, 64 or 128, got {d_model} and {d_k}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"MultiHeadAttention: dropout must lie in [0, 1), got {dropout}")
        self.n_head, self.d_k, self.d_v, self.d_model = n_head, d_k, d_v, d_model
        self.p_drop = float(dropout)
        self.w_qs = torch.nn.Linear(d_model, n_head * d_k)
        self.w_ks = torch.nn.Linear(d_model, n_head * d_k)
        self.w_vs = torch.nn.Linear(d_model, n_head * d_v)
        self.layer_norm = torch.nn.LayerNorm(d_model)
        self.fc = torch.nn.Linear(n_head * d_v, d_model)
        self.validate_mask = True
        self._lib = _lib.load()
        self.launches = 0          # kernel launches enqueued so far, as the C side counted them (ns_ag_last_launches)
        self.last_launches = {}    # {"forward": n, "backward": n} of the latest calls

    def ordered_parameters(self):
        named = dict(self.named_parameters())
        return [named[n] for n in PARAM_NAMES]

    # ---- marshalling ---------------------------------------------------------------------------
    def _marshal(self, x, mask, lens, keep_mask):
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise RuntimeError("MultiHeadAttention: the input must live on the MI355X (there is no CPU path)")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != self.d_model:
            raise ValueError(f"the input must be float32 [B, S, {self.d_model}], got {x.dtype} {tuple(x.shape)}")
        B, S, d = x.shape
        if B == 0 or S == 0:
            raise ValueError("the input must not be empty")
        dev = x.device
        params = self.ordered_parameters()
        for n, p in zip(PARAM_NAMES, params):
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError(f"{n} must be a float32 tensor on {dev}, got {p.dtype} on {p.device}")
        call = _Call()
        call.device, call.x = dev, _aligned(x.detach())
        call.params = [_aligned(p.detach()) for p in params]
        s = _lib.NsAgShape()
        s.B, s.S, s.d, s.H = B, S, d, self.n_head
        call.shape = s
        w = _lib.NsAgWeights()
        for f, p in zip(_lib.AG_NAMES, call.params):
            setattr(w, f, p.data_ptr())
        call.weights = w
        call.lens = None
        if lens is not None:
            if not isinstance(lens, torch.Tensor) or tuple(lens.shape) != (B,) or lens.device != dev or lens.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"lens must be an int64 [B] = {(B,)} tensor on {dev}")
            call.lens = lens.to(torch.int64).contiguous()
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, S, S) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
                raise ValueError(f"mask must be a bool [B, S, S] = {(B, S, S)} tensor on {dev}")
            if call.lens is None:
                with _guard(dev):
                    m = mask != 0
                    call.lens = (S - m[:, 0, :].sum(-1)).to(torch.int64)
                    if self.validate_mask:
                        want = torch.arange(S, device=dev)[None, None, :] >= call.lens[:, None, None]
                        if not bool((m == want).all()):
                            raise ValueError("mask is not a key-padding mask: mask[b, i, j] must equal j >= lens[b] for every i")
        p = self.p_drop if self.training else 0.0
        call.keep = None
        if keep_mask is not None:
            if p == 0.0:
                raise ValueError("keep_mask given although no dropout applies (eval() or dropout == 0)")
            if tuple(keep_mask.shape) != (B, S, d) or keep_mask.device != dev:
                raise ValueError(f"keep_mask must have shape {(B, S, d)} on {dev}, got {tuple(keep_mask.shape)} on {keep_mask.device}")
            call.keep = _aligned((keep_mask != 0).contiguous().view(torch.uint8))
        elif p > 0.0:
            with _guard(dev):
                call.keep = torch.bernoulli(torch.full((B, S, d), 1.0 - p, dtype=torch.float32, device=dev)).to(torch.uint8)
        call.p = p
        return call

    # ---- forward / backward ----------------------------------------------------------------------
    def forward(self, q, k, v, mask=None, lens=None, keep_mask=None):
        if k is not q or v is not q:
            raise NotImplementedError("MultiHeadAttention: self-attention only (q, k and v must be the same tensor); cross-attention is not covered")
        call = self._marshal(q, mask, lens, keep_mask)
        params = self.ordered_parameters()
        if not (torch.is_grad_enabled() and (q.requires_grad or any(p.requires_grad for p in params))):
            return self._forward(call, save=False)[0], None
        return _AttentionFunction.apply(self, call, q, *params), None

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with _guard(dev):
            ws = workspace(self._lib, s, dev)
            y = torch.empty((s.B, s.S, s.d), dtype=torch.float32, device=dev)
            saved = torch.empty(self._lib.ns_ag_saved_bytes(C.byref(s)) // 4, dtype=torch.float32, device=dev) if save else None
            _lib.check(self._lib.ns_ag_forward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.lens), _lib.ptr(call.keep), call.p,
                                               _lib.ptr(y), _lib.ptr(saved), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "ns_ag_forward")
        n = self._lib.ns_ag_last_launches()
        self.launches += n
        self.last_launches["forward"] = n
        return y, saved

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * y).sum()``: a list (dx, then the ten of PARAM_NAMES) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.S, s.d) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.S, s.d)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = _aligned(g)
        with _guard(dev):
            outs = [torch.empty_like(t, memory_format=torch.contiguous_format) if n else None for t, n in zip([call.x] + call.params, need)]
            d = _lib.NsAgGrads()
            d.dx = outs[0].data_ptr() if outs[0] is not None else None
            for f, o in zip(_lib.AG_NAMES, outs[1:]):
                setattr(d, f, o.data_ptr() if o is not None else None)
            ws = workspace(self._lib, s, dev)
            _lib.check(self._lib.ns_ag_backward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.lens), _lib.ptr(call.keep), call.p,
                                                _lib.ptr(saved), _lib.ptr(g), C.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
                       "ns_ag_backward")
        n = self._lib.ns_ag_last_launches()
        self.launches += n
        self.last_launches["backward"] = n
        return outs
