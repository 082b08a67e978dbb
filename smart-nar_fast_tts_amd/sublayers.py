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
attention loss reads the cross-attention maps of ``FFTBlock2.crs_attn``, which ``MultiHeadAttention`` does not cover).

``MultiHeadCrossAttention`` is that other use of the same reference class (csrc/xattngrad.hip, ``ns_xg_*``): ``q`` = mel frames,
``k is v`` = phonemes, the [B, H, T, L] map returned and its gradient accepted.

``PositionwiseFeedForward`` (transformer/SubLayers.py:62-95; csrc/ffngrad.hip, ``ns_fg_*``) is the other sublayer of an FFT block, and
``FFTBlock`` (transformer/Layers.py:39-48) the composite of ``slf_attn``, ``pos_ffn`` and the row mask (``stacks.mask_rows``) in plain
Python.

``Prenet`` (transformer/Layers.py:11-26 with the zeroed first frame and the position add of transformer/Models.py:145-162;
csrc/melencgrad.hip, ``ns_me_*``) and ``FFTBlock2`` (transformer/Layers.py:51-70: ``crs_attn``, ``pos_ffn`` and the row mask) are what
``stacks.MelEncoder`` is made of.

``MelLinear`` (model/fastspeech2_align.py:24,83; csrc/melheadgrad.hip, ``ns_mh_*``) is the ``mel_linear`` between the decoder and the
PostNet of ``training.FastSpeech2Align``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._train import CrossTrainFunction, HipTrainModule, WorkspaceCache, aligned, guard

PARAM_NAMES = ("w_qs.weight", "w_qs.bias", "w_ks.weight", "w_ks.bias", "w_vs.weight", "w_vs.bias", "fc.weight", "fc.bias",
               "layer_norm.weight", "layer_norm.bias")  # order of ns_ag_weights


class _Attention(HipTrainModule):
    """What the two uses of the reference's ``MultiHeadAttention`` share: the constructor (a subclass names the head widths its kernels
    are built for in ``D_K``) and the key lengths of a call."""

    PARAM_NAMES, FIELDS = PARAM_NAMES, _lib.AG_NAMES

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.1):
        super().__init__()
        who, widths = type(self).__name__, [str(w) for w in self.D_K]
        if d_k != d_v:
            raise ValueError(f"{who}: d_k must equal d_v, got {d_k} and {d_v}")
        if n_head * d_k != d_model:
            raise ValueError(f"{who}: n_head * d_k must equal d_model, got {n_head} * {d_k} and {d_model}")
        if d_model not in (256, 512) or d_k not in self.D_K:
            raise ValueError(f"{who}: d_model must be 256 or 512 and d_k {', '.join(widths[:-1])} or {widths[-1]}, got {d_model} and {d_k}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"{who}: dropout must lie in [0, 1), got {dropout}")
        self.n_head, self.d_k, self.d_v, self.d_model = n_head, d_k, d_v, d_model
        self.p_drop = float(dropout)
        self.w_qs = torch.nn.Linear(d_model, n_head * d_k)
        self.w_ks = torch.nn.Linear(d_model, n_head * d_k)
        self.w_vs = torch.nn.Linear(d_model, n_head * d_v)
        self.layer_norm = torch.nn.LayerNorm(d_model)
        self.fc = torch.nn.Linear(n_head * d_v, d_model)
        self.validate_mask = True

    def _key_lengths(self, call, mask, lens, T, L, dims, q, k):
        """``call.lens`` (int64 [B]) from ``lens``, else from the key-padding ``mask`` (bool [B, T, L]), else left None.  The messages
        call the mask's shape ``dims`` ("[B, S, S]") and a query and a key index ``q`` and ``k`` ("i", "j")."""
        dev, B = call.device, call.shape.B
        if lens is not None:
            if not isinstance(lens, torch.Tensor) or tuple(lens.shape) != (B,) or lens.device != dev or lens.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"lens must be an int64 [B] = {(B,)} tensor on {dev}")
            call.lens = lens.to(torch.int64).contiguous()
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, T, L) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
                raise ValueError(f"mask must be a bool {dims} = {(B, T, L)} tensor on {dev}")
            if call.lens is None:
                with guard(dev):
                    m = mask != 0
                    call.lens = (L - m[:, 0, :].sum(-1)).to(torch.int64)
                    if self.validate_mask:
                        want = torch.arange(L, device=dev)[None, None, :] >= call.lens[:, None, None]
                        if not bool((m == want).all()):
                            raise ValueError(f"mask is not a key-padding mask: mask[b, {q}, {k}] must equal {k} >= lens[b] for every {q}")


class MultiHeadAttention(_Attention):
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

    ABI, INPUT, D_K = "ns_ag", "the input", (32, 64, 128)
    WEIGHTS, GRADS = _lib.NsAgWeights, _lib.NsAgGrads
    WORKSPACES = WorkspaceCache("ns_ag_ws_bytes", ("B", "S", "d", "H"))

    def _marshal(self, x, mask, lens, keep_mask):
        call = self._begin(x, self.d_model)
        B, S, d = x.shape
        s = _lib.NsAgShape()
        s.B, s.S, s.d, s.H = B, S, d, self.n_head
        call.shape = s
        self._key_lengths(call, mask, lens, S, S, "[B, S, S]", "i", "j")  # (neither given: a null pointer, every key valid)
        call.p = self.p_drop if self.training else 0.0
        call.keep = self._keep_masks(None if keep_mask is None else (keep_mask,), [(B, S, d)], call.device, call.p)[0]
        return call

    def forward(self, q, k, v, mask=None, lens=None, keep_mask=None):
        if k is not q or v is not q:
            raise NotImplementedError("MultiHeadAttention: self-attention only (q, k and v must be the same tensor); cross-attention is not covered")
        return self._dispatch(self._marshal(q, mask, lens, keep_mask), q), None

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with guard(dev):
            ws, saved = self._workspace(call, save)
            y = torch.empty((s.B, s.S, s.d), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_ag_forward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.lens), _lib.ptr(call.keep), call.p,
                                               _lib.ptr(y), _lib.ptr(saved), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "forward")
        return y, saved

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * y).sum()``: a list (dx, then the ten of PARAM_NAMES) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.S, s.d) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.S, s.d)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        with guard(dev):
            outs, d = self._grad_block(call, need)
            ws, _ = self._workspace(call, save=False)
            self._done(self._lib.ns_ag_backward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.lens), _lib.ptr(call.keep), call.p,
                                                _lib.ptr(saved), _lib.ptr(g), C.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
                       "backward")
        return outs


class MultiHeadCrossAttention(_Attention):
    """Drop-in for ``MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=0.1)`` used as ``FFTBlock2.crs_attn``
    (transformer/Layers.py:61-64): mel-frame queries against phoneme keys, forward AND backward in HIP (csrc/xattngrad.hip, ``ns_xg_*``).
    The same parameter names, so ``mel_encoder.layer_stack.N.crs_attn.*`` loads strictly.

        c = MultiHeadCrossAttention(n_head, d_model, d_k, d_v, dropout).to(device)
        y, attn = c(tgt, src, src, lens=src_lens)        # or mask=crs_attn_mask
        (loss_of(y) + guided_attention_loss(attn)).backward()

    ``forward(q, k, v, mask=None, lens=None, keep_mask=None) -> (output, attn)`` with ``q`` float32 [B, T, d_model], ``k is v`` float32
    [B, L, d_model], ``output = layer_norm(dropout(fc(attention)) + q)`` (NOT masked; FFTBlock2 does that outside) and ``attn`` the
    final probabilities [B, H, T, L] (the reference's shape, transformer/SubLayers.py:48-49), exact 0 at masked keys.
    ``lens`` is the SOURCE lengths, int [B] on the device: keys ``l >=
    lens[b]`` are masked, at no host read.  ``mask`` is the reference's bool [B, T, L] ``crs_attn_mask`` with ``mask[b, t, l] = l >=
    lens[b]`` for every ``t``; from a mask alone the lengths come from ``mask[:, 0, :]`` on the device and, while ``validate_mask`` is
    True, the whole mask is compared with the one those lengths give: one host read per call.  With neither, every key is valid.

    Under ``torch.no_grad()``, or when no input and no parameter requires grad, a call keeps nothing (the map is still returned).
    Otherwise it is one ``torch.autograd.Function`` with two differentiable inputs and two outputs that keeps ``q``, ``kv``, ``ctx``,
    ``z`` (3 B T d + 2 B L d floats) and its own ``attn`` output; the backward accepts the map's gradient (``None`` when the map was
    not used: it is then never read), honours ``needs_input_grad`` and materialises an absent gradient of ``output`` as zeros.

    Raises on what it cannot do: ``k is not v``, ``d_k != d_v``, ``n_head * d_k != d_model``, d_model not 256 or 512, d_k not 64 or
    128, a mask that is not a key-padding mask."""

    ABI, INPUT, D_K, INPUT_GRADS = "ns_xg", "q", (64, 128), ("dtgt", "dsrc")
    WEIGHTS, GRADS = _lib.NsXgWeights, _lib.NsXgGrads
    WORKSPACES = WorkspaceCache("ns_xg_ws_bytes", ("B", "T", "L", "d", "H"))

    def _marshal(self, q, k, mask, lens, keep_mask):
        call = self._begin(q, self.d_model)
        B, T, d = q.shape
        dev = call.device
        if not (isinstance(k, torch.Tensor) and k.device == dev and k.dtype == torch.float32 and k.dim() == 3 and k.shape[0] == B and k.shape[2] == d
                and k.shape[1] > 0):
            raise ValueError(f"k must be a float32 [B, L, {d}] tensor on {dev} with B = {B} and L > 0")
        L = k.shape[1]
        call.src = aligned(k.detach())
        call.inputs.append(call.src)
        s = _lib.NsXgShape()
        s.B, s.T, s.L, s.d, s.H = B, T, L, d, self.n_head
        call.shape = s
        self._key_lengths(call, mask, lens, T, L, "[B, T, L]", "t", "l")
        if call.lens is None:  # (ns_xg_* takes no null pointer: full lengths)
            with guard(dev):
                call.lens = torch.full((B,), L, dtype=torch.int64, device=dev)
        call.p = self.p_drop if self.training else 0.0
        call.keep = self._keep_masks(None if keep_mask is None else (keep_mask,), [(B, T, d)], dev, call.p)[0]
        return call

    def forward(self, q, k, v, mask=None, lens=None, keep_mask=None):
        if k is not v:
            raise ValueError("MultiHeadCrossAttention: k and v must be the same tensor (the keys and values of crs_attn are both the source)")
        call = self._marshal(q, k, mask, lens, keep_mask)
        params = self.ordered_parameters()
        if not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or any(p.requires_grad for p in params))):
            y, attn, _ = self._forward(call, save=False)
            return y, attn
        return CrossTrainFunction.apply(self, call, q, k, *params)

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with guard(dev):
            ws, saved = self._workspace(call, save)
            y = torch.empty((s.B, s.T, s.d), dtype=torch.float32, device=dev)
            attn = torch.empty((s.B, s.H, s.T, s.L), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_xg_forward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.src), _lib.ptr(call.lens),
                                               _lib.ptr(call.keep), call.p, _lib.ptr(y), _lib.ptr(attn), _lib.ptr(saved), _lib.ptr(ws), ws.numel(),
                                               _lib.stream_ptr(dev)), "forward")
        return y, attn, saved

    def _backward(self, call, saved, attn, g, d_attn, need):
        """Gradients of ``(g * y).sum() + (d_attn * attn).sum()``: a list (dtgt, dsrc, then the ten of PARAM_NAMES) with None where
        ``need`` is False.  ``g`` None = zeros; ``d_attn`` None = the map was not used."""
        s, dev = call.shape, call.device
        with guard(dev):
            if g is None:
                g = torch.zeros((s.B, s.T, s.d), dtype=torch.float32, device=dev)
            if tuple(g.shape) != (s.B, s.T, s.d) or g.dtype != torch.float32 or g.device != dev:
                raise ValueError(f"grad_output must be a float32 {(s.B, s.T, s.d)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
            if d_attn is not None and (tuple(d_attn.shape) != (s.B, s.H, s.T, s.L) or d_attn.dtype != torch.float32 or d_attn.device != dev):
                raise ValueError(f"the map's gradient must be a float32 {(s.B, s.H, s.T, s.L)} tensor on {dev}")
            g, attn = aligned(g), aligned(attn.detach())
            d_attn = None if d_attn is None else aligned(d_attn)
            outs, d = self._grad_block(call, need)
            ws, _ = self._workspace(call, save=False)
            self._done(self._lib.ns_xg_backward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.src), _lib.ptr(call.lens),
                                                _lib.ptr(call.keep), call.p, _lib.ptr(saved), _lib.ptr(attn), _lib.ptr(g), _lib.ptr(d_attn),
                                                C.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "backward")
        return outs


FFN_PARAM_NAMES = ("w_1.weight", "w_1.bias", "w_2.weight", "w_2.bias", "layer_norm.weight", "layer_norm.bias")  # order of ns_fg_weights


class PositionwiseFeedForward(HipTrainModule):
    """Drop-in for ``PositionwiseFeedForward(d_in, d_hid, kernel_size, dropout=0.1)`` (transformer/SubLayers.py:62-95) whose forward
    AND backward are HIP (csrc/ffngrad.hip, ``ns_fg_*``): the same parameter names (``w_1``, ``w_2`` as ``nn.Conv1d``, ``layer_norm``),
    so ``encoder.layer_stack.N.pos_ffn.*`` of a reference checkpoint loads strictly.

        f = PositionwiseFeedForward(256, 1024, (9, 1), dropout=0.2).to(device)
        y = f(x)                     # layer_norm(dropout(w_2(relu(w_1(x)))) + x), NOT masked (FFTBlock does that outside)
        y.backward(dy)

    ``forward(x, keep_mask=None)`` with ``x`` float32 [B, S, d_in].  The convolutions run along S inside each utterance: a tap never
    reads the neighbouring utterance's rows.  ``eval()`` means no dropout; the module stays differentiable.  In ``train()`` with
    ``dropout > 0`` the keep-mask is drawn with ``torch.bernoulli`` on the device; ``keep_mask`` (bool or uint8 [B, S, d_in], nonzero =
    kept) supplies it instead.  Under ``torch.no_grad()``, or when neither the input nor a parameter requires grad, a call keeps
    nothing.  Otherwise it is one ``torch.autograd.Function`` (single backward) that keeps ``h = relu(w_1(x))`` and ``z = dropout(w_2(h))
    + x`` ((d_hid + d_in) B S floats) and whose backward honours ``needs_input_grad``.  The ReLU backward gates on the saved ``h``.

    ``matmul`` selects how the six contractions of the layer (``h``, ``u``, the two weight gradients, the two data gradients) are
    computed: ``"fp32"`` (the default) is exact fp32 on the fp32 matrix cores; ``"bf16"`` is opt-in mixed precision with fp32 master
    weights (``ns_fg_*_bf16``, csrc/ffngrad_bf16.hip): both operands of each contraction are rounded to bf16 (nearest even) and summed
    in fp32 on the bf16 matrix cores, while the parameters, their gradients, ``x``, ``h``, ``z``, ``y``, the biases, the LayerNorm, the
    dropout, the residuals, the ReLU gate and every column sum stay as in ``"fp32"``.  The parameter names, ``state_dict()`` and what is
    saved for the backward do not depend on it; ``set_matmul(mode)`` switches a built module (``set_ffn_matmul`` a whole tree).

    Raises on what it cannot do: d_in not 256 or 512, d_hid not a positive multiple of 256, an even kernel size, a ``matmul`` that is
    neither ``"fp32"`` nor ``"bf16"``."""

    ABI, INPUT = "ns_fg", "the input"
    PARAM_NAMES, FIELDS = FFN_PARAM_NAMES, _lib.FG_NAMES
    WEIGHTS, GRADS = _lib.NsFgWeights, _lib.NsFgGrads
    # per matmul mode: the entry points' suffix and the workspace cache (its own size query)
    MATMUL = {"fp32": ("", WorkspaceCache("ns_fg_ws_bytes", ("B", "S", "d", "d_inner", "K1", "K2"))),
              "bf16": ("_bf16", WorkspaceCache("ns_fg_ws_bytes_bf16", ("B", "S", "d", "d_inner", "K1", "K2")))}
    WORKSPACES = MATMUL["fp32"][1]

    def __init__(self, d_in, d_hid, kernel_size, dropout=0.1, matmul="fp32"):
        super().__init__()
        self.set_matmul(matmul)
        who = type(self).__name__
        k1, k2 = (int(k) for k in kernel_size)
        if d_in not in (256, 512):
            raise ValueError(f"{who}: d_in must be 256 or 512, got {d_in}")
        if d_hid <= 0 or d_hid % 256 != 0:
            raise ValueError(f"{who}: d_hid must be a positive multiple of 256, got {d_hid}")
        if k1 <= 0 or k2 <= 0 or k1 % 2 == 0 or k2 % 2 == 0:
            raise ValueError(f"{who}: the kernel sizes must be odd and positive, got {(k1, k2)}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"{who}: dropout must lie in [0, 1), got {dropout}")
        self.d_in, self.d_hid, self.kernel_size = d_in, d_hid, (k1, k2)
        self.p_drop = float(dropout)
        self.w_1 = torch.nn.Conv1d(d_in, d_hid, kernel_size=k1, padding=(k1 - 1) // 2)
        self.w_2 = torch.nn.Conv1d(d_hid, d_in, kernel_size=k2, padding=(k2 - 1) // 2)
        self.layer_norm = torch.nn.LayerNorm(d_in)

    def set_matmul(self, mode):
        """Selects ``"fp32"`` or ``"bf16"`` for the calls from now on (a forward and its backward must run in one mode)."""
        if mode not in self.MATMUL:
            raise ValueError(f"{type(self).__name__}: matmul must be 'fp32' or 'bf16', got {mode!r}")
        self.matmul = mode
        self._suffix, self.WORKSPACES = self.MATMUL[mode]

    def _marshal(self, x, keep_mask):
        call = self._begin(x, self.d_in)
        B, S, d = x.shape
        s = _lib.NsFgShape()
        s.B, s.S, s.d, s.d_inner, s.K1, s.K2 = B, S, d, self.d_hid, self.kernel_size[0], self.kernel_size[1]
        call.shape = s
        call.p = self.p_drop if self.training else 0.0
        call.keep = self._keep_masks(None if keep_mask is None else (keep_mask,), [(B, S, d)], call.device, call.p)[0]
        return call

    def forward(self, x, keep_mask=None):
        return self._dispatch(self._marshal(x, keep_mask), x)

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with guard(dev):
            ws, saved = self._workspace(call, save)
            y = torch.empty((s.B, s.S, s.d), dtype=torch.float32, device=dev)
            entry = "ns_fg_forward" + self._suffix
            self._done(getattr(self._lib, entry)(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.keep), call.p, _lib.ptr(y),
                                                 _lib.ptr(saved), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "forward", entry=entry)
        return y, saved

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * y).sum()``: a list (dx, then the six of FFN_PARAM_NAMES) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.S, s.d) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.S, s.d)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        with guard(dev):
            outs, d = self._grad_block(call, need)
            ws, _ = self._workspace(call, save=False)
            entry = "ns_fg_backward" + self._suffix
            self._done(getattr(self._lib, entry)(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.keep), call.p, _lib.ptr(saved),
                                                 _lib.ptr(g), C.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "backward", entry=entry)
        return outs


def set_ffn_matmul(module, mode) -> int:
    """Switches every ``PositionwiseFeedForward`` under ``module`` — a layer, a stack such as ``model.mel_decoder``, a whole model — to
    ``mode`` (``"fp32"`` or ``"bf16"``) and returns how many it switched; parameters, ``state_dict()`` and checkpoints are untouched.

        sublayers.set_ffn_matmul(model.mel_decoder, "bf16")      # the advised start

    Start at ``mel_decoder``: nothing downstream of it takes a discrete decision, so the rounding only moves the mel by bf16-sized
    amounts.  In the mel encoder (and the text encoder) the feed-forward output feeds the aligner and the duration path, where a
    flipped rounding can move a duration by a frame; switching those is a training-dynamics choice, not an error."""
    if mode not in PositionwiseFeedForward.MATMUL:
        raise ValueError(f"set_ffn_matmul: mode must be 'fp32' or 'bf16', got {mode!r}")
    n = 0
    for m in module.modules():
        if isinstance(m, PositionwiseFeedForward):
            m.set_matmul(mode)
            n += 1
    return n


class FFTBlock(torch.nn.Module):
    """The reference's ``FFTBlock(d_model, n_head, d_k, d_v, d_inner, kernel_size, dropout=0.1)`` (transformer/Layers.py:39-48) as a
    trainable module: ``slf_attn`` is ``MultiHeadAttention`` and ``pos_ffn`` is ``PositionwiseFeedForward``, both HIP in forward and
    backward, composed in plain Python, so ``encoder.layer_stack.N.*`` of a reference checkpoint loads strictly.  The two
    ``masked_fill(mask.unsqueeze(-1), 0)`` between and after the sublayers are ``stacks.mask_rows``: one HIP launch each in the forward
    and one each in the backward (a select on the row's mask byte; ``mask_book`` counts them), so no torch kernel stands between
    ``enc_input`` and ``enc_output``.

    ``forward(enc_input, mask=None, slf_attn_mask=None, lens=None, keep_masks=None) -> (enc_output, None)``: ``mask`` is the bool
    [B, S] padding mask (True = padded; those rows of the output are exactly 0), ``slf_attn_mask`` and ``lens`` follow
    ``MultiHeadAttention``'s rules (the reference's [B, S, S] key-padding mask, or int [B] lengths on the device at no host read, or
    both; with neither every key is valid).  Without ``mask`` no row is zeroed, as in the reference.  ``keep_masks`` supplies the two dropout keep-masks (attention, feed-forward), each [B, S, d_model].  The second return value is
    ``None``: the self-attention map is never written to memory."""

    def __init__(self, d_model, n_head, d_k, d_v, d_inner, kernel_size, dropout=0.1):
        super().__init__()
        self.slf_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForward(d_model, d_inner, kernel_size, dropout=dropout)
        from . import stacks  # (stacks imports this module: resolved here, at first use)

        self._mask_rows, self.mask_book = stacks.mask_rows, stacks.Launches()

    def forward(self, enc_input, mask=None, slf_attn_mask=None, lens=None, keep_masks=None):
        if keep_masks is not None and len(keep_masks) != 2:
            raise ValueError(f"keep_masks must hold 2 masks (attention, feed-forward), got {len(keep_masks)}")
        k_attn, k_ffn = keep_masks if keep_masks is not None else (None, None)
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != tuple(enc_input.shape[:2]) or mask.device != enc_input.device:
                raise ValueError(f"mask must be a bool [B, S] = {tuple(enc_input.shape[:2])} tensor on {enc_input.device}")
            pad = mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0
            pad = pad.contiguous().view(torch.uint8)  # (a bool's bytes are 0 and 1: no kernel)
        else:
            pad = None
        self.mask_book.begin()
        enc_output, _ = self.slf_attn(enc_input, enc_input, enc_input, mask=slf_attn_mask, lens=lens, keep_mask=k_attn)
        if pad is not None:
            enc_output = self._mask_rows(enc_output, mask=pad, book=self.mask_book)
        enc_output = self.pos_ffn(enc_output, keep_mask=k_ffn)
        if pad is not None:
            enc_output = self._mask_rows(enc_output, mask=pad, book=self.mask_book)
        return enc_output, None


PRENET_PARAM_NAMES = ("w_1.weight", "w_1.bias", "w_2.weight", "w_2.bias")  # order of ns_me_weights


class Prenet(HipTrainModule):
    """Drop-in for ``Prenet()`` (transformer/Layers.py:11-26; hard-coded 80 -> 256 -> 256, ``Dropout(0.2)``) together with what
    ``MelEncoder`` does around it, forward AND backward in HIP (csrc/melencgrad.hip, ``ns_me_*``): the zeroed first frame in front
    (transformer/Models.py:145-146) and the position add behind (Models.py:151,162).  The same parameter names (``w_1``, ``w_2`` as
    ``nn.Linear`` with torch's initialisation), so ``mel_encoder.prenet.*`` of a reference checkpoint loads strictly.

        p = Prenet().to(device)
        y = p(mels, pos)             # dropout(relu(w_2(relu(w_1(mels with frame 0 zeroed))))) + pos[:T]
        y.backward(dy)

    ``forward(x, pos, keep_mask=None)`` with ``x`` float32 [B, T, 80], never written, and ``pos`` float32 [>= T, 256], the position
    table of the call, which gets no gradient.  ``x`` gets one only if it requires one; its frame 0 is exactly ``+0.0`` then, and a NaN
    in frame 0 of ``x`` reaches nothing.  The drop probability is 0.2 in ``train()`` and 0 in ``eval()``; the keep-mask is drawn with
    ``torch.bernoulli`` on the device, or ``keep_mask`` (bool or uint8 [B, T, 256], nonzero = kept) supplies it.  Under
    ``torch.no_grad()``, or when neither ``x`` nor a parameter requires grad, a call keeps nothing.  Otherwise it is one
    ``torch.autograd.Function`` (single backward) that keeps the zeroed input and the two activations ((80 + 2 * 256) B T floats) and
    whose backward honours ``needs_input_grad``.  Both ReLU backwards gate on the saved activations."""

    ABI, INPUT, INPUT_GRADS = "ns_me", "x", ("dmels",)
    PARAM_NAMES, FIELDS = PRENET_PARAM_NAMES, _lib.ME_NAMES
    WEIGHTS, GRADS = _lib.NsMeWeights, _lib.NsMeGrads
    WORKSPACES = WorkspaceCache("ns_me_ws_bytes", ("B", "T", "n_mel", "d"))
    N_MEL, D, P_DROP = 80, 256, 0.2

    def __init__(self):
        super().__init__()
        self.p_drop = self.P_DROP
        self.w_1 = torch.nn.Linear(self.N_MEL, self.D)
        self.w_2 = torch.nn.Linear(self.D, self.D)

    def _marshal(self, x, pos, keep_mask):
        call = self._begin(x, self.N_MEL)
        B, T, _ = x.shape
        dev = call.device
        if not isinstance(pos, torch.Tensor) or pos.dim() != 2 or pos.shape[0] < T or pos.shape[1] != self.D or pos.dtype != torch.float32 or pos.device != dev:
            raise ValueError(f"pos must be a float32 [>= {T}, {self.D}] tensor on {dev}")
        call.pos = aligned(pos.detach())
        s = _lib.NsMeShape()
        s.B, s.T, s.n_mel, s.d = B, T, self.N_MEL, self.D
        call.shape = s
        call.p = self.p_drop if self.training else 0.0
        call.keep = self._keep_masks(None if keep_mask is None else (keep_mask,), [(B, T, self.D)], dev, call.p)[0]
        return call

    def forward(self, x, pos, keep_mask=None):
        return self._dispatch(self._marshal(x, pos, keep_mask), x)

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with guard(dev):
            ws, saved = self._workspace(call, save)
            y = torch.empty((s.B, s.T, s.d), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_me_forward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(call.pos), _lib.ptr(call.keep), call.p,
                                               _lib.ptr(y), _lib.ptr(saved), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "forward")
        return y, saved

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * y).sum()``: a list (dmels, then the four of PRENET_PARAM_NAMES) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.T, s.d) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.T, s.d)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        with guard(dev):
            outs, d = self._grad_block(call, need)
            ws, _ = self._workspace(call, save=False)
            self._done(self._lib.ns_me_backward(C.byref(s), C.byref(call.weights), _lib.ptr(call.keep), call.p, _lib.ptr(saved), _lib.ptr(g),
                                                C.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "backward")
        return outs


class MelLinear(HipTrainModule):
    """Drop-in for ``mel_linear = nn.Linear(decoder_hidden, n_mel_channels)`` (model/fastspeech2_align.py:24,83), forward AND backward
    in HIP (csrc/melheadgrad.hip, ``ns_mh_*``): ``weight`` [n_mel, d] and ``bias`` [n_mel] with ``nn.Linear``'s initialisation, so
    ``mel_linear.*`` of a reference checkpoint loads strictly.

        lin = MelLinear(256).to(device)
        y = lin(x)                   # x [B, T, d] -> y [B, T, n_mel] = x weight^T + bias
        y.backward(dy)

    ``d`` is 256 or 512 and ``n_mel`` a multiple of 16 up to 128.  No row is masked: the reference masks none here, a padded row of
    ``y`` equals the bias and feeds the PostNet's batch statistics.  Under ``torch.no_grad()``, or when neither ``x`` nor a parameter
    requires grad, a call is the forward alone.  Otherwise it is one ``torch.autograd.Function`` (single backward) that keeps nothing
    but ``x`` and whose backward honours ``needs_input_grad``: the 80-column weight gradient runs at the padded width 128 (pad, GEMM,
    reduce, copy), the bias gradient is float64 column sums in one order, the data gradient is one pack and the GEMM dispatch."""

    ABI, INPUT = "ns_mh", "x"
    PARAM_NAMES, FIELDS = ("weight", "bias"), _lib.MH_NAMES
    WEIGHTS, GRADS = _lib.NsMhWeights, _lib.NsMhGrads
    WORKSPACES = WorkspaceCache("ns_mh_ws_bytes", ("B", "T", "d", "n_mel"))

    def __init__(self, d, n_mel=80):
        super().__init__()
        self.d, self.n_mel = int(d), int(n_mel)
        if self.d not in (256, 512):
            raise ValueError(f"MelLinear: d must be 256 or 512, got {d}")
        if self.n_mel < 16 or self.n_mel > 128 or self.n_mel % 16:
            raise ValueError(f"MelLinear: n_mel must be a multiple of 16 in [16, 128], got {n_mel}")
        init = torch.nn.Linear(self.d, self.n_mel)  # (nn.Linear's initialisation, its draws in its order)
        self.weight, self.bias = init.weight, init.bias

    def forward(self, x):
        call = self._begin(x, self.d)
        s = _lib.NsMhShape()
        s.B, s.T, s.d, s.n_mel = x.shape[0], x.shape[1], self.d, self.n_mel
        call.shape = s
        return self._dispatch(call, x)

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with guard(dev):
            ws, _ = self._workspace(call, save=False)  # (nothing is saved: the backward reads x and g alone)
            y = torch.empty((s.B, s.T, s.n_mel), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_mh_forward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(y), _lib.ptr(ws), ws.numel(),
                                               _lib.stream_ptr(dev)), "forward")
        return y, None

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * y).sum()``: a list (dx, d_weight, d_bias) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.T, s.n_mel) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.T, s.n_mel)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        with guard(dev):
            outs, d = self._grad_block(call, need)
            ws, _ = self._workspace(call, save=False)
            self._done(self._lib.ns_mh_backward(C.byref(s), C.byref(call.weights), _lib.ptr(call.x), _lib.ptr(g), C.byref(d), _lib.ptr(ws),
                                                ws.numel(), _lib.stream_ptr(dev)), "backward")
        return outs


class FFTBlock2(torch.nn.Module):
    """The reference's ``FFTBlock2(d_model, n_head, d_k, d_v, d_inner, kernel_size, dropout=0.1)`` (transformer/Layers.py:51-70) as a
    trainable module: ``crs_attn`` is ``MultiHeadCrossAttention`` and ``pos_ffn`` is ``PositionwiseFeedForward``, both HIP in forward
    and backward, composed in plain Python as ``FFTBlock`` is, so ``mel_encoder.layer_stack.N.*`` of a reference checkpoint loads
    strictly.  The two ``masked_fill(mask.unsqueeze(-1), 0)`` are ``stacks.mask_rows`` (``mask_book`` counts them).

    ``forward(src_input, tgt_input, mask=None, crs_attn_mask=None, src_lens=None, keep_masks=None) -> (enc_output, attn)``:
    ``src_input`` float32 [B, L, d_model] (the keys and values), ``tgt_input`` float32 [B, T, d_model] (the queries), ``mask`` the bool
    [B, T] padding mask of the target rows (True = padded; those rows of the output are exactly 0; without it no row is zeroed),
    ``crs_attn_mask`` and ``src_lens`` follow ``MultiHeadCrossAttention``'s rules (the reference's [B, T, L] key-padding mask, or int
    [B] source lengths on the device at no host read, or both).  ``keep_masks`` supplies the two dropout keep-masks (attention,
    feed-forward), each [B, T, d_model].  ``attn`` is the [B, H, T, L] map, differentiable."""

    def __init__(self, d_model, n_head, d_k, d_v, d_inner, kernel_size, dropout=0.1):
        super().__init__()
        self.crs_attn = MultiHeadCrossAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForward(d_model, d_inner, kernel_size, dropout=dropout)
        from . import stacks  # (stacks imports this module: resolved here, at first use)

        self._mask_rows, self.mask_book = stacks.mask_rows, stacks.Launches()

    def forward(self, src_input, tgt_input, mask=None, crs_attn_mask=None, src_lens=None, keep_masks=None):
        if keep_masks is not None and len(keep_masks) != 2:
            raise ValueError(f"keep_masks must hold 2 masks (attention, feed-forward), got {len(keep_masks)}")
        k_attn, k_ffn = keep_masks if keep_masks is not None else (None, None)
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != tuple(tgt_input.shape[:2]) or mask.device != tgt_input.device:
                raise ValueError(f"mask must be a bool [B, T] = {tuple(tgt_input.shape[:2])} tensor on {tgt_input.device}")
            pad = mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0
            pad = pad.contiguous().view(torch.uint8)  # (a bool's bytes are 0 and 1: no kernel)
        else:
            pad = None
        self.mask_book.begin()
        enc_output, attn = self.crs_attn(tgt_input, src_input, src_input, mask=crs_attn_mask, lens=src_lens, keep_mask=k_attn)
        if pad is not None:
            enc_output = self._mask_rows(enc_output, mask=pad, book=self.mask_book)
        enc_output = self.pos_ffn(enc_output, keep_mask=k_ffn)
        if pad is not None:
            enc_output = self._mask_rows(enc_output, mask=pad, book=self.mask_book)
        return enc_output, attn
