"""The reference's ``TxtEncoder`` and ``MelDecoder`` (transformer/Models.py:33-100, 176-244) as trainable modules: the two stacks of
``sublayers.FFTBlock`` with what stands in front of them, forward AND backward in HIP (csrc/stackgrad.hip, ``ns_st_*`` in
include/nar_fs2.h), under the reference's parameter names; and its ``MelEncoder`` (transformer/Models.py:103-173), the stack of
``sublayers.FFTBlock2`` behind ``sublayers.Prenet`` (csrc/melencgrad.hip, ``ns_me_*``).

    enc = TxtEncoder(model_config).to(device)
    enc.load_state_dict({k[len("txt_encoder."):]: v for k, v in ckpt["model"].items() if k.startswith("txt_encoder.")})
    y = enc(texts, src_mask, lens=src_lens)          # lens: no host read
    dec = MelDecoder(model_config).to(device)
    out, mel_mask = dec(x, mel_mask, lens=mel_lens)
    out.backward(g)

Three pieces are this module's own: ``WordEmbedding`` (``src_word_emb`` + the position add in one launch, the table gradient in one),
the decoder's position add (its gradient is ``grad_output`` itself) and ``mask_rows``, the ``masked_fill(mask.unsqueeze(-1), 0)`` that
an FFT block applies twice.  What stays torch on the way: autograd's own fan-in adds, the [B, S] length derivation (a sum over the mask
and, while ``validate_mask`` is True, one comparison with a host read), and the decoder's slice when it truncates."""
from __future__ import annotations

import torch

from . import _lib, ops
from . import workload as wl
from ._train import aligned, guard, need_gpu
from .sublayers import FFTBlock, FFTBlock2, Prenet


class Launches:
    """Launch bookkeeping of ``ns_st_*`` calls: ``total`` enqueued so far and ``last`` per direction since ``begin()``, as the C side
    counted them (``ns_st_last_launches``)."""

    def __init__(self):
        self.total, self.last = 0, {}

    def begin(self):
        self.last = {}

    def done(self, rc, which, entry, n=None):
        _lib.check(rc, entry)
        n = _lib.load().ns_st_last_launches() if n is None else n
        self.total += n
        self.last[which] = self.last.get(which, 0) + n


def _row_mask(x, mask, lens, book, which):
    """``ns_st_op_row_mask`` on a float32 [B, S, D] tensor; ``mask`` uint8 [B, S] or None, ``lens`` int64 [B] or None."""
    B, S, D = x.shape
    dev = x.device
    x = aligned(x)
    with guard(dev):
        y = torch.empty_like(x)
        rc = _lib.load().ns_st_op_row_mask(_lib.ptr(x), _lib.ptr(mask), _lib.ptr(lens), B, S, D, _lib.ptr(y), _lib.stream_ptr(dev))
    if book is None:
        _lib.check(rc, "ns_st_op_row_mask")
    else:
        book.done(rc, which, "ns_st_op_row_mask")
    return y


class _MaskFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, lens, book):
        ctx.mask, ctx.lens, ctx.book = mask, lens, book
        return _row_mask(x.detach(), mask, lens, book, "forward")

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _row_mask(g, ctx.mask, ctx.lens, ctx.book, "backward"), None, None, None


def mask_rows(x, mask=None, lens=None, book=None):
    """``x.masked_fill(mask.unsqueeze(-1), 0)`` (transformer/Layers.py:43,46) in one HIP launch, out of place; the backward is the same
    launch on ``grad_output``.  ``x`` float32 [B, S, D] on the GPU with D 256 or 512; ``mask`` bool or uint8 [B, S] (nonzero = padded),
    or ``lens`` int [B] (row ``s >= lens[b]`` is padded), or both: then the mask is used.  A padded row is ``+0.0`` whatever ``x`` holds
    there, NaN included.  ``book`` (a ``Launches``) takes the launch counts."""
    need_gpu("mask_rows", "x", x)
    if x.dtype != torch.float32 or x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty float32 [B, S, D] tensor, got {x.dtype} {tuple(x.shape)}")
    B, S, _ = x.shape
    dev = x.device
    if mask is None and lens is None:
        raise ValueError("mask_rows needs mask or lens")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, S) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
            raise ValueError(f"mask must be a bool [B, S] = {(B, S)} tensor on {dev}")
        mask = mask.contiguous().view(torch.uint8)  # (a bool's bytes are 0 and 1: no kernel)
        lens = None
    else:
        if not isinstance(lens, torch.Tensor) or tuple(lens.shape) != (B,) or lens.dtype not in (torch.int64, torch.int32) or lens.device != dev:
            raise ValueError(f"lens must be an int64 [B] = {(B,)} tensor on {dev}")
        lens = lens.to(torch.int64).contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _MaskFunction.apply(x, mask, lens, book)
    return _row_mask(x.detach(), mask, lens, book, "forward")


class _EmbedFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, texts, pos, weight):
        ctx.owner, ctx.texts = owner, texts
        return owner._forward(texts, pos, weight)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return None, None, None, ctx.owner._backward(g, ctx.texts) if ctx.needs_input_grad[3] else None


class WordEmbedding(torch.nn.Module):
    """The reference's ``src_word_emb = nn.Embedding(n_vocab, d, padding_idx=0)`` (transformer/Models.py:56-58; state-dict key
    ``weight``) together with the position add behind it: ``forward(texts, pos) = weight[texts] + pos[:S]`` in one launch, ``texts``
    int64 [B, S], ``pos`` float32 [>= S, d].

    One autograd Function.  ``texts`` and ``pos`` get no gradient.  The table's gradient is one launch (``ns_st_op_embed_grad``: per
    row of the table a float64 sum in ascending row order, rounded once; row 0, PAD, is ``+0.0``), made only when ``weight`` requires
    a gradient: a frozen table makes no launch.

    Deviation from ``nn.Embedding``: a token outside ``[0, n_vocab)`` is treated as PAD in the forward and contributes to no row in the
    backward.  There is no host read on this path, so the module cannot raise an ``IndexError`` as ``nn.Embedding`` would.

    Refuses ``d`` not 256 or 512 and ``n_vocab < 2``."""

    def __init__(self, n_vocab, d):
        super().__init__()
        self.n_vocab, self.d = int(n_vocab), int(d)
        if self.d not in (256, 512):
            raise ValueError(f"WordEmbedding: d must be 256 or 512, got {d}")
        if self.n_vocab < 2:
            raise ValueError(f"WordEmbedding: n_vocab must be at least 2, got {n_vocab}")
        w = torch.randn(self.n_vocab, self.d)  # nn.Embedding's initialisation, the PAD row zeroed
        w[0].zero_()
        self.weight = torch.nn.Parameter(w)
        self._lib = _lib.load()
        self.book = Launches()

    @property
    def launches(self):
        return self.book.total

    @property
    def last_launches(self):
        return dict(self.book.last)

    def forward(self, texts, pos):
        need_gpu("WordEmbedding", "texts", texts)
        dev = texts.device
        if texts.dtype != torch.int64 or texts.dim() != 2 or texts.numel() == 0:
            raise ValueError(f"texts must be a non-empty int64 [B, S] tensor, got {texts.dtype} {tuple(texts.shape)}")
        S = texts.shape[1]
        if not isinstance(pos, torch.Tensor) or pos.dim() != 2 or pos.shape[0] < S or pos.shape[1] != self.d or pos.dtype != torch.float32 or pos.device != dev:
            raise ValueError(f"pos must be a float32 [>= {S}, {self.d}] tensor on {dev}")
        if self.weight.device != dev or self.weight.dtype != torch.float32:
            raise ValueError(f"weight must be a float32 tensor on {dev}, got {self.weight.dtype} on {self.weight.device}")
        self.book.begin()
        if torch.is_grad_enabled() and self.weight.requires_grad:
            return _EmbedFunction.apply(self, texts, pos, self.weight)
        return self._forward(texts, pos, self.weight)

    def _forward(self, texts, pos, weight):
        dev = texts.device
        B, S = texts.shape
        ta, pa, wa = texts.contiguous(), aligned(pos.detach()), aligned(weight.detach())
        with guard(dev):
            out = torch.empty((B, S, self.d), dtype=torch.float32, device=dev)
            self.book.done(self._lib.ns_st_op_embed_pos(_lib.ptr(ta), _lib.ptr(wa), _lib.ptr(pa), B, S, self.d, self.n_vocab, _lib.ptr(out),
                                                        _lib.stream_ptr(dev)), "forward", "ns_st_op_embed_pos")
        return out

    def _backward(self, g, texts):
        dev = texts.device
        if tuple(g.shape) != tuple(texts.shape) + (self.d,) or g.dtype != torch.float32 or g.device != dev:
            raise ValueError(f"grad_output must be a float32 {tuple(texts.shape) + (self.d,)} tensor on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
        g, ta = aligned(g), texts.contiguous()
        with guard(dev):
            dw = torch.empty((self.n_vocab, self.d), dtype=torch.float32, device=dev)
            self.book.done(self._lib.ns_st_op_embed_grad(_lib.ptr(g), _lib.ptr(ta), ta.numel(), self.d, self.n_vocab, _lib.ptr(dw),
                                                         _lib.stream_ptr(dev)), "backward", "ns_st_op_embed_grad")
        return dw


class _AddPosFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, x, pos):
        return owner._add_pos(x.detach(), pos)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return None, g, None  # the add passes the gradient through: the same tensor, no launch


class _Stack(torch.nn.Module):
    """What the three stacks share: ``position_enc``, ``layer_stack``, the position table of a call, the lengths of a call, the walk
    through the layers and the launch bookkeeping.  ``front(d) -> (name, module)`` is what stands in front of the layers
    (``src_word_emb``, ``prenet``), ``block`` the class of a layer and ``attn`` the name of its attention sublayer."""

    def __init__(self, config, side, front=None, block=FFTBlock, attn="slf_attn"):
        super().__init__()
        t = config["transformer"]
        d, n_head = t[f"{side}_hidden"], t[f"{side}_head"]
        if d % n_head:
            raise ValueError(f"{type(self).__name__}: {side}_hidden must be a multiple of {side}_head, got {d} and {n_head}")
        self.max_seq_len, self.d_model = int(config["max_seq_len"]), d
        self._attn = attn
        if front is not None:  # (registered in the reference's order: a state dict lists it ahead of the layers)
            self.add_module(*front(d))
        self.position_enc = torch.nn.Parameter(torch.from_numpy(wl.sinusoid_table(self.max_seq_len + 1, d).copy())[None], requires_grad=False)
        self.layer_stack = torch.nn.ModuleList([
            block(d, n_head, d // n_head, d // n_head, t["conv_filter_size"], t["conv_kernel_size"], dropout=t[f"{side}_dropout"])
            for _ in range(t[f"{side}_layer"])])
        self.validate_mask = True
        self.book = Launches()  # the stack's own launches: the decoder's position add, a regenerated table

    def _hip_modules(self):
        return [m for layer in self.layer_stack for m in (getattr(layer, self._attn), layer.pos_ffn)]

    @property
    def launches(self):
        """kernel launches enqueued so far by the stack and its sublayers, as the C side counted them"""
        return self.book.total + sum(m.launches for m in self._hip_modules()) + sum(layer.mask_book.total for layer in self.layer_stack)

    @property
    def last_launches(self):
        """{"forward": n, "backward": n} of the latest call (the backward once it ran)"""
        books = [self.book] + [layer.mask_book for layer in self.layer_stack]
        return {which: sum(b.last.get(which, 0) for b in books) + sum(m.last_launches.get(which, 0) for m in self._hip_modules())
                for which in ("forward", "backward")}

    def _begin(self):
        self.book.begin()
        for layer in self.layer_stack:  # (a layer's mask_book and the embedding's book begin in their own forward)
            getattr(layer, self._attn).last_launches, layer.pos_ffn.last_launches = {}, {}

    def _table(self, S, dev):
        """The [>= S, d] position table of a call of S rows: ``position_enc``'s, or, in ``eval()`` past ``max_seq_len``, a regenerated
        one (transformer/Models.py:82-87, 218-225; one launch)."""
        if self.position_enc.device != dev:
            raise ValueError(f"position_enc must live on {dev}, got {self.position_enc.device}")
        if not self.training and S > self.max_seq_len:
            with guard(dev):
                table = ops.sinusoid_table(S, self.d_model, device=dev)
            self.book.done(0, "forward", "ns_op_sinusoid_table", n=1)
            return table
        return self.position_enc.detach()[0]

    def _lengths(self, mask, lens, B, S, dev):
        """(uint8 mask [B, S], int64 lens [B]) of a call: ``lens`` as given, else derived from the mask on the device and, while
        ``validate_mask`` is True, compared with it (one host read)."""
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, S) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
            raise ValueError(f"mask must be a bool [B, S] = {(B, S)} tensor on {dev}")
        mask = mask.contiguous()
        if lens is not None:
            if not isinstance(lens, torch.Tensor) or tuple(lens.shape) != (B,) or lens.device != dev or lens.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"lens must be an int64 [B] = {(B,)} tensor on {dev}")
            return mask, lens.to(torch.int64).contiguous()
        with guard(dev):
            m = mask != 0
            lens = (S - m.sum(-1)).to(torch.int64)
            if self.validate_mask and not bool((m == (torch.arange(S, device=dev)[None, :] >= lens[:, None])).all()):
                raise ValueError("mask is not a padding mask: mask[b, s] must equal s >= lens[b]")
        return mask, lens

    def _layers(self, x, mask, lens, keep_masks):
        n = len(self.layer_stack)
        if keep_masks is not None and len(keep_masks) != n:
            raise ValueError(f"keep_masks must hold {n} pairs (one per layer), got {len(keep_masks)}")
        for i, layer in enumerate(self.layer_stack):
            x, _ = layer(x, mask=mask, lens=lens, keep_masks=None if keep_masks is None else keep_masks[i])
        return x


class TxtEncoder(_Stack):
    """Drop-in for ``TxtEncoder(config)`` (transformer/Models.py:33-100) whose forward AND backward are HIP: ``src_word_emb.weight``,
    ``position_enc`` ([1, max_seq_len + 1, d], ``requires_grad=False``, the bits of ``workload.sinusoid_table``) and ``layer_stack.N.*``
    of ``sublayers.FFTBlock``, so the ``txt_encoder.*`` slice of a checkpoint loads with ``strict=True``.

    ``forward(src_seq, mask, return_attns=False, lens=None, keep_masks=None) -> enc_output`` with ``src_seq`` int64 [B, S] and ``mask``
    bool [B, S] (True = padded; those rows of the output are exactly ``+0.0``).  The lengths are derived once per call from ``mask`` on
    the device and, while ``validate_mask`` is True, checked against it: one host read, which passing ``lens`` (int [B] on the device)
    avoids.  Every layer gets ``lens=`` and ``mask=`` and never a [B, S, S] tensor.  ``keep_masks`` is ``n_layers`` pairs (attention,
    feed-forward) of dropout keep-masks; otherwise each sublayer draws its own in ``train()``.  The self-attention maps are never
    written to memory; ``return_attns`` is accepted and changes nothing.

    In ``eval()`` with ``S > max_seq_len`` the position table is regenerated for ``S`` rows (one more launch), as the reference does.
    In ``train()`` with ``S > max_seq_len + 1`` it raises ``ValueError`` (the reference would fail in the broadcast).

    A token id outside ``[0, n_src_vocab)`` is treated as PAD: no host read, so no ``IndexError`` (see ``WordEmbedding``).

    Launches (``launches`` / ``last_launches``, the stack's own plus its sublayers'): forward ``1 + sum over layers (attention forward
    + 1 + FFN forward + 1)``, plus 1 for a regenerated table; backward the mirror plus 1 for the table gradient, which a frozen
    ``src_word_emb`` drops."""

    def __init__(self, config, n_src_vocab=wl.N_SYMBOLS + 1):
        super().__init__(config, "encoder", lambda d: ("src_word_emb", WordEmbedding(n_src_vocab, d)))

    def _hip_modules(self):
        return [self.src_word_emb] + super()._hip_modules()

    def forward(self, src_seq, mask, return_attns=False, lens=None, keep_masks=None):
        need_gpu("TxtEncoder", "src_seq", src_seq)
        if src_seq.dim() != 2 or src_seq.dtype != torch.int64 or src_seq.numel() == 0:
            raise ValueError(f"src_seq must be a non-empty int64 [B, S] tensor, got {src_seq.dtype} {tuple(src_seq.shape)}")
        B, S = src_seq.shape
        if self.training and S > self.max_seq_len + 1:
            raise ValueError(f"TxtEncoder: in train() S must not exceed max_seq_len + 1 = {self.max_seq_len + 1}, got {S}")
        dev = src_seq.device
        self._begin()
        mask, lens = self._lengths(mask, lens, B, S, dev)
        x = self.src_word_emb(src_seq, self._table(S, dev))
        return self._layers(x, mask, lens, keep_masks)


class MelDecoder(_Stack):
    """Drop-in for ``MelDecoder(config)`` (transformer/Models.py:176-244) whose forward AND backward are HIP: ``position_enc`` and
    ``layer_stack.N.*`` of ``sublayers.FFTBlock``, so the ``mel_decoder.*`` slice of a checkpoint loads with ``strict=True``.

    ``forward(enc_seq, mask, return_attns=False, lens=None, keep_masks=None) -> (dec_output, mask)`` with ``enc_seq`` float32 [B, S, d];
    ``mask``, ``lens``, ``keep_masks`` and ``return_attns`` as in ``TxtEncoder``.  The gradient of the position add is ``grad_output``
    itself: no launch.

    When ``S <= max_seq_len``, or in ``train()``, it takes the reference's else-branch: ``max_len = min(S, max_seq_len)``, the input
    and the mask are sliced to ``max_len`` rows and ``lens`` is clamped to it, and the sliced mask is returned.  The slice of
    ``enc_seq`` is torch's own view with torch's backward (zeros past ``max_len``), and the kernels read a contiguous copy of it; this
    is a rare path (a training batch longer than ``max_seq_len``).  In ``eval()`` with ``S > max_seq_len`` the position table is
    regenerated for ``S`` rows (one more launch) and nothing is truncated.

    Launches: forward ``1 + sum over layers (attention forward + 1 + FFN forward + 1)``, plus 1 for a regenerated table; backward the
    mirror (the position add has none)."""

    def __init__(self, config):
        super().__init__(config, "decoder")
        self._lib = _lib.load()

    def _add_pos(self, x, pos):
        B, S, D = x.shape
        dev = x.device
        x, pos = aligned(x), aligned(pos)
        with guard(dev):
            out = torch.empty((B, S, D), dtype=torch.float32, device=dev)
            self.book.done(self._lib.ns_st_op_add_pos(_lib.ptr(x), _lib.ptr(pos), B, S, D, _lib.ptr(out), _lib.stream_ptr(dev)), "forward",
                           "ns_st_op_add_pos")
        return out

    def forward(self, enc_seq, mask, return_attns=False, lens=None, keep_masks=None):
        need_gpu("MelDecoder", "enc_seq", enc_seq)
        if enc_seq.dtype != torch.float32 or enc_seq.dim() != 3 or enc_seq.shape[2] != self.d_model or enc_seq.numel() == 0:
            raise ValueError(f"enc_seq must be a non-empty float32 [B, S, {self.d_model}] tensor, got {enc_seq.dtype} {tuple(enc_seq.shape)}")
        B, S, _ = enc_seq.shape
        dev = enc_seq.device
        self._begin()
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, S):
            raise ValueError(f"mask must be a bool [B, S] = {(B, S)} tensor on {dev}")
        if self.training or S <= self.max_seq_len:
            max_len = min(S, self.max_seq_len)
            if max_len < S:
                enc_seq, mask = enc_seq[:, :max_len, :], mask[:, :max_len]
                if lens is not None:
                    lens = lens.clamp(max=max_len)
                S = max_len
        mask, lens = self._lengths(mask, lens, B, S, dev)
        pos = self._table(S, dev)
        if torch.is_grad_enabled() and enc_seq.requires_grad:
            x = _AddPosFunction.apply(self, enc_seq, pos)
        else:
            x = self._add_pos(enc_seq.detach(), pos)
        return self._layers(x, mask, lens, keep_masks), mask


class MelEncoder(_Stack):
    """Drop-in for ``MelEncoder(config)`` (transformer/Models.py:103-173) whose forward AND backward are HIP: ``prenet.*``
    (``sublayers.Prenet``: the zeroed first frame, the two Linears, the dropout and the position add), ``position_enc`` ([1,
    max_seq_len + 1, d], ``requires_grad=False``, the bits of ``workload.sinusoid_table``) and ``layer_stack.N.{crs_attn,pos_ffn}.*`` of
    ``sublayers.FFTBlock2``, so the ``mel_encoder.*`` slice of a checkpoint loads with ``strict=True`` (``workload.aligner_shapes``
    lists the names).  Raises ``ValueError`` unless ``decoder_hidden == 256``: the Prenet's width is not configurable in the reference.

    ``forward(src_seq, tgt_seq, src_mask, tgt_mask, return_attns=True, src_lens=None, mel_lens=None, keep_masks=None,
    prenet_keep_mask=None) -> (dec_output, [attn per layer])`` with ``src_seq`` float32 [B, L, d] (the text encoder's output, the keys
    and values of every layer), ``tgt_seq`` float32 [B, T, 80] (the reference mel; frame 0 is replaced by zeros and gets a zero
    gradient), ``src_mask`` bool [B, L] and ``tgt_mask`` bool [B, T] (True = padded).  Padded target rows of ``dec_output`` are exactly
    ``+0.0``; each map is [B, H, T, L], differentiable, exact 0 at padded phonemes (an empty list with ``return_attns=False``).  Both
    length vectors are derived once per call from the masks on the device and, while ``validate_mask`` is True, checked against them
    (one host read each), which passing ``src_lens`` / ``mel_lens`` (int [B] on the device) avoids; every layer gets the source lengths
    and the target mask and never a [B, T, L] tensor.  ``keep_masks`` is ``n_layers`` pairs (attention, feed-forward) of dropout
    keep-masks and ``prenet_keep_mask`` the Prenet's; otherwise each sublayer draws its own in ``train()``.

    In ``train()``, or when ``T <= max_seq_len``, it takes the reference's else-branch: ``tgt_seq``, ``tgt_mask`` and ``mel_lens`` are
    cut to ``max_mel_len = min(T, max_seq_len)`` rows (torch's slice with torch's backward, zeros past the cut, as in ``MelDecoder``)
    and the maps are [B, H, max_mel_len, L]; given keep-masks have ``max_mel_len`` rows.  In ``eval()`` with ``T > max_seq_len`` the position table is regenerated for ``T`` rows
    (one more launch) and nothing is cut.

    ``src_seq`` feeds every layer, so its gradient is the sum of the layers' ``dsrc``: autograd's fan-in adds of those are the only
    torch kernels on the data path (apart from the slice of a truncating call).

    Launches: forward ``Prenet forward + sum over layers (cross-attention forward + 1 + FFN forward + 1)``, plus 1 for a regenerated
    table; backward the mirror."""

    def __init__(self, config):
        d = config["transformer"]["decoder_hidden"]
        if d != Prenet.D:
            raise ValueError(f"MelEncoder: decoder_hidden must be {Prenet.D} (Prenet is hard-coded {Prenet.N_MEL} -> {Prenet.D} -> {Prenet.D}, "
                             f"transformer/Layers.py:18-19), got {d}")
        super().__init__(config, "decoder", lambda d: ("prenet", Prenet()), block=FFTBlock2, attn="crs_attn")

    def _hip_modules(self):
        return [self.prenet] + super()._hip_modules()

    def _begin(self):
        super()._begin()
        self.prenet.last_launches = {}

    def forward(self, src_seq, tgt_seq, src_mask, tgt_mask, return_attns=True, src_lens=None, mel_lens=None, keep_masks=None,
                prenet_keep_mask=None):
        need_gpu("MelEncoder", "tgt_seq", tgt_seq)
        if tgt_seq.dtype != torch.float32 or tgt_seq.dim() != 3 or tgt_seq.shape[2] != Prenet.N_MEL or tgt_seq.numel() == 0:
            raise ValueError(f"tgt_seq must be a non-empty float32 [B, T, {Prenet.N_MEL}] tensor, got {tgt_seq.dtype} {tuple(tgt_seq.shape)}")
        B, T, _ = tgt_seq.shape
        dev = tgt_seq.device
        if (not isinstance(src_seq, torch.Tensor) or src_seq.device != dev or src_seq.dtype != torch.float32 or src_seq.dim() != 3
                or src_seq.shape[0] != B or src_seq.shape[2] != self.d_model or src_seq.shape[1] == 0):
            raise ValueError(f"src_seq must be a float32 [B, L, {self.d_model}] tensor on {dev} with B = {B} and L > 0")
        L = src_seq.shape[1]
        n = len(self.layer_stack)
        if keep_masks is not None and len(keep_masks) != n:
            raise ValueError(f"keep_masks must hold {n} pairs (one per layer), got {len(keep_masks)}")
        self._begin()
        if not isinstance(tgt_mask, torch.Tensor) or tuple(tgt_mask.shape) != (B, T):
            raise ValueError(f"tgt_mask must be a bool [B, T] = {(B, T)} tensor on {dev}")
        if self.training or T <= self.max_seq_len:
            max_len = min(T, self.max_seq_len)
            if max_len < T:
                tgt_seq, tgt_mask = tgt_seq[:, :max_len, :], tgt_mask[:, :max_len]
                if mel_lens is not None:
                    mel_lens = mel_lens.clamp(max=max_len)
                T = max_len
        tgt_mask, mel_lens = self._lengths(tgt_mask, mel_lens, B, T, dev)
        src_mask, src_lens = self._lengths(src_mask, src_lens, B, L, dev)
        x = self.prenet(tgt_seq, self._table(T, dev), keep_mask=prenet_keep_mask)
        attns = []
        for i, layer in enumerate(self.layer_stack):
            x, attn = layer(src_seq, x, mask=tgt_mask, src_lens=src_lens, keep_masks=None if keep_masks is None else keep_masks[i])
            if return_attns:
                attns.append(attn)
        return x, attns

    @torch.no_grad()
    def durations(self, attn_last, src_lens, mel_lens):
        """Frames per phoneme, int64 [B, L], from the last layer's map [B, H, T, L]: frame ``t < mel_lens[b]`` goes to the phoneme
        ``l < src_lens[b]`` at which the head-summed map peaks (``ops.aligner_durations``).  The reference's ``_calculate_duration``
        is undefined; this is the rule ``forward_teacher_forced()`` uses in its place."""
        return ops.aligner_durations(attn_last.detach(), src_lens, mel_lens)
