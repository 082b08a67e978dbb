"""The reference's ``PostNet`` (transformer/Layers.py:107-177, used at model/fastspeech2_align.py:85) as a trainable module whose forward
AND backward are HIP (csrc/postnetgrad.hip, ``ns_pn_*`` in include/nar_fs2.h): five ``Conv1d(k=5)`` + ``BatchNorm1d`` pairs with ``tanh``
and the hard-coded ``dropout(0.5)`` between them, with TRAIN-mode BatchNorm — batch statistics over all ``B * T`` rows, the running
statistics updated by the kernels — behind the loss gradient ``d_postnet`` of ``loss.FastSpeech2TrainingLoss``.

    post = PostNet().to(device)
    post.load_state_dict({k[len("postnet."):]: v for k, v in ckpt["model"].items() if k.startswith("postnet.")})   # strict
    postnet_output = post(mel) + mel            # the residual stays outside, as in the reference
    loss.backward()                             # parameter gradients, and mel.grad when mel requires grad

The parameters and buffers are ordinary torch tensors under the reference's names (``convolutions.{i}.0.conv.weight|bias``,
``convolutions.{i}.1.weight|bias|running_mean|running_var|num_batches_tracked``); every call reads them afresh and a ``state_dict()``
saved after training loads into the inference model, which folds the running statistics into its convolution weights.  There is no
CPU path and no torch kernel between the input and the output or between ``grad_output`` and the gradients."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._train import HipTrainModule, WorkspaceCache, aligned, guard


class _ConvNorm(torch.nn.Module):  # the reference's ConvNorm wrapper (transformer/Layers.py:70-104): a holder of `conv.weight` / `conv.bias`
    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = torch.nn.Conv1d(cin, cout, kernel_size=k, padding=(k - 1) // 2)


class _ByLayer:
    """Lets the training core, which fills a block by ``setattr(block, field, address)``, write the nested blocks of the C ABI:
    ``block.gamma2 = a`` is ``block.layer[2].gamma = a``."""

    def __setattr__(self, name, address):
        if name[-1:].isdigit():
            setattr(self.layer[int(name[-1])], name[:-1], address)
        else:
            super().__setattr__(name, address)


class _Weights(_ByLayer, _lib.NsPnWeights):
    pass


class _Grads(_ByLayer, _lib.NsPnGrads):
    pass


class PostNet(HipTrainModule):
    """Drop-in for ``PostNet(n_mel_channels, postnet_embedding_dim, postnet_kernel_size, postnet_n_convolutions)``: the same parameter
    and buffer names, the same ``forward(x [B, T, n_mel]) -> [B, T, n_mel]`` without the residual.

    ``train()``: every BatchNorm normalises with the mean and the biased variance of its input over all ``B * T`` rows (padded frames
    included: the reference passes no mask) and the forward's kernels update ``running_mean``, ``running_var`` (momentum 0.1, unbiased
    variance) and ``num_batches_tracked`` on the live buffers — once per forward, also under ``torch.no_grad()``, never in the backward.
    Dropout is 0.5 as in the reference; the constructor keyword ``dropout`` (an extension) changes it.  The ``n`` keep-masks are drawn
    with ``torch.bernoulli`` on the device unless ``keep_masks=`` supplies them: ``n - 1`` of shape ``[B, T, emb]`` and one of
    ``[B, T, n_mel]``, bool or uint8, nonzero = kept.  ``eval()``: the running statistics are used and left alone, no dropout; autograd
    stays legal and the backward then treats mean and variance as constants.

    Under ``torch.no_grad()``, or when neither the input nor a parameter requires grad, a call keeps nothing.  Otherwise it is one
    ``torch.autograd.Function`` (single backward) whose saved buffer holds ``u_i = conv_i(h_{i-1}) + b_i`` of every layer, ``h_i`` of
    every layer but the last (fp32) and per layer ``mu_i`` and ``rstd_i`` as float64:
    ``4 * B * T * (2 * (n - 1) * emb + n_mel) + 16 * n * emb`` bytes (270 MB at B = 16, T = 1010, the defaults).  Its backward honours
    ``needs_input_grad``: a tensor that needs no gradient gets no buffer, no write and no launch of its own, and comes back ``None``; the
    walk stops below the lowest layer anything is wanted from.

    Refuses: an input off the GPU, ``B * T == 1`` in ``train()`` (as torch does), ``postnet_embedding_dim`` other than 256 or 512,
    ``n_mel_channels`` not a multiple of 16 in [16, 128], an even kernel size or one above 9, fewer than 2 or more than 5 convolutions."""

    ABI, INPUT = "ns_pn", "x"
    WEIGHTS, GRADS = _Weights, _Grads
    WORKSPACES = WorkspaceCache("ns_pn_ws_bytes", ("B", "T", "n_mel", "emb", "K", "n"))

    def __init__(self, n_mel_channels=80, postnet_embedding_dim=512, postnet_kernel_size=5, postnet_n_convolutions=5, dropout=0.5):
        super().__init__()
        n_mel, emb, k, n = int(n_mel_channels), int(postnet_embedding_dim), int(postnet_kernel_size), int(postnet_n_convolutions)
        if emb not in (256, 512):
            raise ValueError(f"postnet_embedding_dim must be 256 or 512 (the widths the HIP kernels are built for), got {emb}")
        if n_mel % 16 != 0 or not 16 <= n_mel <= 128:
            raise ValueError(f"n_mel_channels must be a multiple of 16 in [16, 128] (16-byte channel groups; the last layer's weight gradient "
                             f"is padded to 128 columns), got {n_mel}")
        if k <= 0 or k % 2 == 0 or k > 9:
            raise ValueError(f"postnet_kernel_size must be odd and at most 9 ('same' padding needs an odd kernel), got {k}")
        if not 2 <= n <= _lib.PN_MAX_LAYERS:
            raise ValueError(f"postnet_n_convolutions must lie in [2, {_lib.PN_MAX_LAYERS}] (a first and a last layer; the C ABI holds five), got {n}")
        self.dropout = float(dropout)
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"dropout must lie in [0, 1), got {self.dropout}")
        self.n_mel, self.emb, self.kernel, self.n = n_mel, emb, k, n
        chans = [n_mel] + [emb] * (n - 1) + [n_mel]
        self.convolutions = torch.nn.ModuleList(
            torch.nn.Sequential(_ConvNorm(chans[i], chans[i + 1], k), torch.nn.BatchNorm1d(chans[i + 1])) for i in range(n))
        self.channels = chans
        self.PARAM_NAMES = tuple(f"convolutions.{i}.{s}" for i in range(n) for s in ("0.conv.weight", "0.conv.bias", "1.weight", "1.bias"))
        self.FIELDS = tuple(f"{p}{i}" for i in range(n) for p in _lib.PN_PARAMS)  # order of ns_pn_grads after dx; p{i} is layer[i].p (_ByLayer)

    def _marshal(self, x, keep_masks):
        call = self._begin(x, self.n_mel)
        B, T, _ = x.shape
        dev = call.device
        call.training = bool(self.training)
        if call.training and B * T == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size " + str(tuple(x.shape)))
        s = _lib.NsPnShape()
        s.B, s.T, s.n_mel, s.emb, s.K, s.n = B, T, self.n_mel, self.emb, self.kernel, self.n
        call.shape = s
        call.buffers = []  # the live buffers, kept alive with the call
        for i in range(self.n):
            bn = self.convolutions[i][1]
            for name in _lib.PN_BUFFERS:
                t = getattr(bn, name)
                want = torch.int64 if name == "num_batches_tracked" else torch.float32
                if t.device != dev or t.dtype != want or not t.is_contiguous() or t.data_ptr() % (8 if want == torch.int64 else 16):
                    raise ValueError(f"convolutions.{i}.1.{name} must be a contiguous, aligned {want} tensor on {dev}: the kernels update it in place")
                setattr(call.weights, f"{name}{i}", t.data_ptr())
                call.buffers.append(t)
        call.p = self.dropout if call.training else 0.0
        call.keep = self._keep_masks(keep_masks, [(B, T, c) for c in self.channels[1:]], dev, call.p)  # one per convolution
        return call

    def _keep_ptrs(self, call):
        if call.keep[0] is None:
            return None
        return (C.c_void_p * self.n)(*[k.data_ptr() for k in call.keep])

    def forward(self, x, keep_masks=None):
        return self._dispatch(self._marshal(x, keep_masks), x)

    def _forward(self, call, save):
        s, dev = call.shape, call.device
        with guard(dev):
            ws, saved = self._workspace(call, save)
            y = torch.empty((s.B, s.T, s.n_mel), dtype=torch.float32, device=dev)
            self._done(self._lib.ns_pn_forward(C.byref(s), C.byref(call.weights), int(call.training), _lib.ptr(call.x), self._keep_ptrs(call), call.p,
                                               _lib.ptr(y), _lib.ptr(saved), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "forward")
        return y, saved

    def _backward(self, call, saved, g, need):
        """Gradients of ``(g * y).sum()``: a list (dx, then the 4 n of PARAM_NAMES) with None where ``need`` is False."""
        s, dev = call.shape, call.device
        if tuple(g.shape) != (s.B, s.T, s.n_mel) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {(s.B, s.T, s.n_mel)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g = aligned(g)
        with guard(dev):
            outs, d = self._grad_block(call, need)
            ws, _ = self._workspace(call, save=False)
            self._done(self._lib.ns_pn_backward(C.byref(s), C.byref(call.weights), int(call.training), _lib.ptr(call.x), self._keep_ptrs(call), call.p,
                                                _lib.ptr(saved), _lib.ptr(g), C.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "backward")
        return outs
