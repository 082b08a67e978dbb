"""Per-operator Python wrappers over the C-ABI's ``ns_op_*`` entry points — one per row of
SURVEY.md §8(a).  They exist so the parity tests can check every stage of the path against
the oracle in isolation, and so ``bench.py`` can time the dominant kernel alone.

Every function takes CUDA tensors, launches on torch's current stream and returns fresh
tensors.  ``model`` is a :class:`smart_nar_fast_tts_amd.model.FastSpeech2Align` with loaded
weights; ``prefix`` is the reference's module path (e.g. ``"mel_decoder.layer_stack.0.slf_attn"``);
``lens`` is the int64 ``[B]`` valid-length vector from which the reference builds its masks.
"""
from __future__ import annotations

import math

import torch

from . import _lib


def _ws(model, B, S):
    n = model._lib.ns_op_ws_bytes(model._h, B, S)
    return model._workspace("op", n)


def _st(t):
    return _lib.stream_ptr(t.device)


def mask_from_lengths(lens: torch.Tensor, max_len: int | None = None) -> torch.Tensor:
    """utils/tools.py:89-97 (True = padding).  max_len=None costs a host sync, as in the reference."""
    lib = _lib.load()
    lens = lens.long().contiguous()
    if max_len is None:
        max_len = int(lens.max().item())
    out = torch.empty(lens.shape[0], max_len, dtype=torch.bool, device=lens.device)
    _lib.check(lib.ns_op_mask_from_lengths(_lib.ptr(lens), lens.shape[0], int(max_len), _lib.ptr(out), _st(lens)), "mask")
    return out


def sinusoid_table(n_position: int, d_hid: int, device="cuda") -> torch.Tensor:
    """transformer/Models.py:10-30."""
    lib = _lib.load()
    out = torch.empty(n_position, d_hid, dtype=torch.float32, device=device)
    _lib.check(lib.ns_op_sinusoid_table(n_position, d_hid, _lib.ptr(out), _st(out)), "sinusoid")
    return out


def txt_encoder(model, texts, lens):
    B, L = texts.shape
    texts, lens = texts.long().contiguous(), lens.long().contiguous()
    out = torch.empty(B, L, model._cfg.d_enc, dtype=torch.float32, device=texts.device)
    ws = _ws(model, B, L)
    _lib.check(model._lib.ns_op_txt_encoder(model._h, _lib.ptr(texts), _lib.ptr(lens), B, L, _lib.ptr(out), _lib.ptr(ws),
                                            ws.numel(), _st(texts)), "txt_encoder")
    return out


def _prefixed(fn_name, model, prefix, x, lens):
    B, S, _ = x.shape
    x = x.contiguous()
    out = torch.empty_like(x)
    ws = _ws(model, B, S)
    fn = getattr(model._lib, fn_name)
    if lens is None:
        rc = fn(model._h, prefix.encode(), _lib.ptr(x), B, S, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _st(x))
    else:
        lens = lens.long().contiguous()
        rc = fn(model._h, prefix.encode(), _lib.ptr(x), _lib.ptr(lens), B, S, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _st(x))
    _lib.check(rc, fn_name)
    return out


def multi_head_attention(model, prefix, x, lens):
    """transformer/SubLayers.py:29-59 (self attention: q = k = v = x); returns LayerNorm(fc(attn) + x)."""
    return _prefixed("ns_op_multi_head_attention", model, prefix, x, lens)


def positionwise_ffn(model, prefix, x):
    """transformer/SubLayers.py:87-95."""
    return _prefixed("ns_op_positionwise_ffn", model, prefix, x, None)


def fft_block(model, prefix, x, lens):
    """transformer/Layers.py:39-48."""
    return _prefixed("ns_op_fft_block", model, prefix, x, lens)


def variance_predictor(model, prefix, x, lens):
    """model/modules.py:278-286; returns [B,S]."""
    B, S, _ = x.shape
    x, lens = x.contiguous(), lens.long().contiguous()
    out = torch.empty(B, S, dtype=torch.float32, device=x.device)
    ws = _ws(model, B, S)
    _lib.check(model._lib.ns_op_variance_predictor(model._h, prefix.encode(), _lib.ptr(x), _lib.ptr(lens), B, S, _lib.ptr(out),
                                                   _lib.ptr(ws), ws.numel(), _st(x)), "variance_predictor")
    return out


def predictor_conv1(model, prefix, x):
    """The first launch of a VariancePredictor alone: h [B,S,filter] = layer_norm_1(relu(conv1d_1(x))) (model/modules.py:245-260)."""
    B, S, _ = x.shape
    x = x.contiguous()
    h = torch.empty(B, S, model._cfg.vp_filter, dtype=torch.float32, device=x.device)
    ws = _ws(model, B, S)
    _lib.check(model._lib.ns_op_predictor_conv1(model._h, prefix.encode(), _lib.ptr(x), B, S, _lib.ptr(h), _lib.ptr(ws), ws.numel(),
                                                _st(x)), "predictor_conv1")
    return h


def predictor_tail(model, prefix, h, lens, control: float = 1.0, target=None, x_in=None, add_pos: bool = False, pred=None, x_out=None):
    """The second launch of a VariancePredictor alone, from hidden rows ``h`` [B,S,filter] the caller supplies: conv1d_2 -> ReLU ->
    layer_norm_2 -> Linear -> masked_fill (-> ``* control`` without a ``target``).  With ``x_in`` [B,S,d] also the pitch / energy
    embedding add of ``prefix`` (from bucketize(target) when a target is given) and, with ``add_pos``, the decoder position rows.
    Returns ``pred`` [B,S], or ``(pred, x_out)`` with ``x_in``.  ``pred`` / ``x_out`` may be passed in (pre-filled) to be written."""
    B, S, _ = h.shape
    h, lens = h.contiguous(), lens.long().contiguous()
    if pred is None:
        pred = torch.empty(B, S, dtype=torch.float32, device=h.device)
    if target is not None:
        target = target.contiguous().float()
    if x_in is not None:
        x_in = x_in.contiguous()
        if x_out is None:
            x_out = torch.empty_like(x_in)
    ws = _ws(model, B, S)
    _lib.check(model._lib.ns_op_predictor_tail(model._h, prefix.encode(), _lib.ptr(h), _lib.ptr(lens), B, S, float(control), _lib.ptr(target),
                                               _lib.ptr(x_in), int(bool(add_pos)), _lib.ptr(pred), _lib.ptr(x_out), _lib.ptr(ws), ws.numel(),
                                               _st(h)), "predictor_tail")
    return pred if x_in is None else (pred, x_out)


def duration_round(log_d, d_control: float = 1.0):
    """model/modules.py:132-135."""
    lib = _lib.load()
    log_d = log_d.contiguous()
    out = torch.empty_like(log_d)
    _lib.check(lib.ns_op_duration_round(_lib.ptr(log_d), log_d.numel(), float(d_control), _lib.ptr(out), _st(log_d)), "duration_round")
    return out


def length_regulate(x, duration, max_len=None):
    """LengthRegulator.forward (model/modules.py:201-230): returns (output [B,T,D], mel_len int64 [B])."""
    lib = _lib.load()
    B, L, D = x.shape
    x, duration = x.contiguous(), duration.contiguous().float()
    cum = torch.empty(B, L, dtype=torch.int32, device=x.device)
    mel_len = torch.empty(B, dtype=torch.long, device=x.device)
    _lib.check(lib.ns_op_duration_scan(_lib.ptr(duration), B, L, _lib.ptr(cum), _lib.ptr(mel_len), _st(x)), "duration_scan")
    T = int(max_len) if max_len else int(mel_len.max().item())
    out = torch.empty(B, T, D, dtype=torch.float32, device=x.device)
    _lib.check(lib.ns_op_length_regulate(_lib.ptr(x), _lib.ptr(cum), B, L, D, T, _lib.ptr(out), _st(x)), "length_regulate")
    return out, mel_len


def duration_target_scan(d_targets, src_lens, texts=None, n_vocab: int = 0):
    """The teacher-forced forward's phase-1 tail alone (model/modules.py:128-130,221-223 with duration_target given): from int64
    ``d_targets`` [B,L] returns (cum int32 [B,L] — inclusive prefix sums of max(d, 0) —, dur_keep float32 [B,L] = d, src_mask bool
    [B,L], mel_lens int64 [B] = the totals).  With ``texts`` [B,L], an utterance holding an id outside [0, n_vocab) reports -1."""
    lib = _lib.load()
    B, L = d_targets.shape
    d_targets, src_lens = d_targets.long().contiguous(), src_lens.long().contiguous()
    if texts is not None:
        texts = texts.long().contiguous()
    dev = d_targets.device
    cum = torch.empty(B, L, dtype=torch.int32, device=dev)
    keep = torch.empty(B, L, dtype=torch.float32, device=dev)
    mask = torch.empty(B, L, dtype=torch.bool, device=dev)
    mel_len = torch.empty(B, dtype=torch.long, device=dev)
    _lib.check(lib.ns_op_duration_target_scan(_lib.ptr(d_targets), _lib.ptr(src_lens), _lib.ptr(texts), int(n_vocab), B, L, _lib.ptr(cum),
                                              _lib.ptr(keep), _lib.ptr(mask), _lib.ptr(mel_len), _st(d_targets)), "duration_target_scan")
    return cum, keep, mask, mel_len


def variance_embedding(model, which: str, x, lens, control: float = 1.0, target=None):
    """get_pitch_embedding / get_energy_embedding + the unmasked add (model/modules.py:80-100,139-149):
    returns (prediction [B,S], x + embedding).  With ``target`` the embedding comes from bucketize(target)."""
    B, S, _ = x.shape
    x, lens = x.contiguous(), lens.long().contiguous()
    pred = torch.empty(B, S, dtype=torch.float32, device=x.device)
    x_out = torch.empty_like(x)
    ws = _ws(model, B, S)
    if target is not None:
        target = target.contiguous().float()
    _lib.check(model._lib.ns_op_variance_embedding(model._h, {"pitch": 0, "energy": 1}[which], _lib.ptr(x), _lib.ptr(lens), B, S,
                                                   float(control), _lib.ptr(target), _lib.ptr(pred), _lib.ptr(x_out),
                                                   _lib.ptr(ws), ws.numel(), _st(x)), "variance_embedding")
    return pred, x_out


def bucketize(values, bins):
    """torch.bucketize(values, bins) with right=False, as model/modules.py:86-88,97-99 calls it."""
    lib = _lib.load()
    values, bins = values.contiguous().float(), bins.contiguous().float()
    out = torch.empty(values.shape, dtype=torch.long, device=values.device)
    _lib.check(lib.ns_op_bucketize(_lib.ptr(values), values.numel(), _lib.ptr(bins), bins.numel(), _lib.ptr(out), _st(values)), "bucketize")
    return out


def gaussian_upsampling(x, durations, max_len=None):
    """GaussianUpsampling.forward (model/modules.py:166-192): returns (output, s [B,1], w [B,L,T])."""
    lib = _lib.load()
    B, L, D = x.shape
    x, durations = x.contiguous(), durations.contiguous().float()
    # torch.arange(0, torch.max(s)) in the reference (also a host sync there): ceil(max s) frames for a fractional sum
    T = int(math.ceil(durations.sum(dim=-1).max().item()))
    T_out = int(max_len) if max_len else T
    out = torch.empty(B, T_out, D, dtype=torch.float32, device=x.device)
    s = torch.empty(B * (L + 1), dtype=torch.float32, device=x.device)
    w = torch.empty(B, L, T, dtype=torch.float32, device=x.device)
    _lib.check(lib.ns_op_gaussian_upsampling(_lib.ptr(x), _lib.ptr(durations), B, L, D, T, T_out, _lib.ptr(out), _lib.ptr(s),
                                             _lib.ptr(w), _st(x)), "gaussian_upsampling")
    return out, s[:B].reshape(B, 1).clone(), w


def mel_decoder(model, x, lens):
    """transformer/Models.py:212-244."""
    B, T, _ = x.shape
    x, lens = x.contiguous(), lens.long().contiguous()
    out = torch.empty_like(x)
    ws = _ws(model, B, T)
    _lib.check(model._lib.ns_op_mel_decoder(model._h, _lib.ptr(x), _lib.ptr(lens), B, T, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                            _st(x)), "mel_decoder")
    return out


def mel_linear(model, x):
    B, T, _ = x.shape
    x = x.contiguous()
    out = torch.empty(B, T, model._cfg.n_mel, dtype=torch.float32, device=x.device)
    _lib.check(model._lib.ns_op_mel_linear(model._h, _lib.ptr(x), B, T, _lib.ptr(out), _st(x)), "mel_linear")
    return out


def postnet(model, mel):
    """PostNet.forward (transformer/Layers.py:169-177), without the residual."""
    B, T, _ = mel.shape
    mel = mel.contiguous()
    out = torch.empty_like(mel)
    ws = _ws(model, B, T)
    _lib.check(model._lib.ns_op_postnet(model._h, _lib.ptr(mel), B, T, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _st(mel)), "postnet")
    return out


def ffn_conv1(model, prefix, x, out=None):
    """The path's dominant kernel alone: relu(w_1(x)) of PositionwiseFeedForward (k=9 Conv1D-as-GEMM)."""
    B, S, _ = x.shape
    if out is None:
        out = torch.empty(B, S, model._cfg.d_inner, dtype=torch.float32, device=x.device)
    _lib.check(model._lib.ns_op_ffn_conv1(model._h, prefix.encode(), _lib.ptr(x), B, S, _lib.ptr(out), _st(x)), "ffn_conv1")
    return out


def plan_attention_dense(B, S, H, dk, scratch_floats: int = 0, has_tickets: bool = False):
    """(kernel 0 k_attention_strip / 1 k_attention, key ranges, merge 0 none / 1 last arriver / 2 k_attention_merge launch, 32-key
    tiles per wave / per range) of the dense attention launch, from the function the launch dispatches on (host only)."""
    import ctypes

    o = (ctypes.c_int32 * 4)()
    _lib.check(_lib.load().ns_plan_attention_dense(int(B), int(S), int(H), int(dk), int(scratch_floats), int(bool(has_tickets)), o),
               "plan_attention_dense")
    return tuple(o)


def attention_dense_scratch(B, S, H, dk, split_scratch=True, tickets: bool = True):
    """(floats of scratch ``attention_core`` allocates, floats of it left to the partials, ticket block carved) for the same
    arguments (host only).  ``True``: 8 ranges' worth of floats in all, the ticket block taken out of them; an int n: room for n key
    ranges plus the ticket block the op takes from the end (16 = ATT_SPLIT_MAX, every split the dispatch can ask for);
    ``"workspace"``: what a model's own workspace holds for this shape; ``False``: none."""
    import ctypes

    lib = _lib.load()
    flags = 0 if tickets else 2

    def carve(total):  # what the op makes of `total` floats, asked of the op's own function
        part, has = ctypes.c_size_t(0), ctypes.c_int32(0)
        _lib.check(lib.ns_op_attention_carve(int(B), int(S), int(H), total * 4, flags, ctypes.byref(part), ctypes.byref(has)), "attention_carve")
        return part.value, bool(has.value)

    one = B * S * H * dk + 2 * B * S * H
    if isinstance(split_scratch, str):
        assert split_scratch == "workspace", split_scratch
        floats = int(lib.ns_op_attention_scratch_bytes(B, S, H, dk)) // 4
    elif split_scratch is True:
        floats = 8 * one
    elif not split_scratch:
        floats = 0
    else:
        big = int(split_scratch) * one + (1 << 28)
        floats = int(split_scratch) * one + (big - carve(big)[0])
    if not floats:
        return 0, 0, False
    return (floats,) + carve(floats)


def attention_core(qkv, lens, n_head: int, split_scratch=True, bf16: bool = False, tickets: bool = True, out=None):
    """ScaledDotProductAttention on already-projected, head-packed q/k/v (transformer/Modules.py:14-25):
    qkv [B,S,3*d] (Q | K | V, head h at h*dk inside each) -> merged heads [B,S,d].  ``split_scratch`` hands the
    kernel the scratch it needs to take its split-key path (``True``: 8 ranges' worth, an int n: room for n ranges, 16 being the
    most the dispatch asks for; see ``attention_dense_scratch``); ``"workspace"`` hands it what a model's own workspace
    holds for this shape (sized by the library, ``ns_op_attention_scratch_bytes``), so the launch splits its keys as the model's
    attention does.  ``tickets=False`` withholds the ticket block (split strips then merge by a launch of their own).  ``bf16`` runs
    the "bf16" precision mode's kernels (what a bf16 model's decoder layers run): Q K^T and P V
    from operands rounded to bf16, the softmax in fp32.  ``out`` (optional): a contiguous [B,S,d] fp32 tensor to write."""
    lib = _lib.load()
    B, S, d3 = qkv.shape
    d = d3 // 3
    qkv = qkv.contiguous()
    if out is None:
        out = torch.empty(B, S, d, dtype=torch.float32, device=qkv.device)
    assert out.shape == (B, S, d) and out.dtype == torch.float32 and out.is_contiguous() and out.device == qkv.device
    lens_p = _lib.ptr(lens.long().contiguous()) if lens is not None else _lib.ptr(None)
    floats = attention_dense_scratch(B, S, n_head, d // n_head, split_scratch, tickets)[0]
    scratch = torch.empty(floats, dtype=torch.float32, device=qkv.device) if floats else None
    args = (_lib.ptr(qkv), lens_p, B, S, n_head, d // n_head, _lib.ptr(out), _lib.ptr(scratch), floats * 4, _st(qkv))
    if bf16 or not tickets:
        _lib.check(lib.ns_op_attention_core_mode(*args, (1 if bf16 else 0) | (0 if tickets else 2)), "attention_core")
    else:
        _lib.check(lib.ns_op_attention_core(*args), "attention_core")
    return out


def gemm(model, name: str, x):
    """One named contraction alone, in ``model``'s precision mode, through the forward's own dispatch: bias and the layer's
    activation (ReLU for ``w_1``, tanh for every PostNet layer but the last), no residual, no LayerNorm.  ``name`` is
    ``<layer prefix>.slf_attn.qkv`` / ``.slf_attn.fc`` / ``.pos_ffn.w_1`` / ``.pos_ffn.w_2``, ``mel_linear`` or
    ``postnet.convolutions.<i>``; x [B,S,Cin] -> [B,S,N] with zero padding per utterance of S rows."""
    B, S, _ = x.shape
    x = x.contiguous()
    n = gemm_shape(model, name)[1]
    out = torch.empty(B, S, n, dtype=torch.float32, device=x.device)
    _lib.check(model._lib.ns_op_gemm(model._h, name.encode(), _lib.ptr(x), B, S, _lib.ptr(out), _st(x)), "gemm")
    return out


def gemm_shape(model, name: str):
    """(Cin, N, KW) of a contraction ``gemm`` accepts (the name itself is validated by the library)."""
    c = model._cfg
    if name == "mel_linear":
        return c.d_dec, c.n_mel, 1
    if name.startswith("postnet.convolutions."):
        i = int(name.rsplit(".", 1)[1])
        return (c.n_mel if i == 0 else c.postnet_dim), (c.n_mel if i == c.postnet_n - 1 else c.postnet_dim), c.postnet_k
    d = c.d_enc if name.startswith("txt_encoder.") else c.d_dec
    for suffix, shape in ((".slf_attn.qkv", (d, 3 * d, 1)), (".slf_attn.fc", (d, d, 1)), (".pos_ffn.w_1", (d, c.d_inner, c.ffn_k1)),
                          (".pos_ffn.w_2", (c.d_inner, d, c.ffn_k2))):
        if name.endswith(suffix):
            return shape
    raise ValueError(f"unknown contraction {name!r}")


def plan_gemm_bf16(M: int, N: int):
    """(rows, columns) of the tile a plain bf16-mode GEMM of M rows and N output channels is launched with."""
    import ctypes

    lib = _lib.load()
    bm, bn = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(lib.ns_plan_gemm_bf16(int(M), int(N), ctypes.byref(bm), ctypes.byref(bn)), "plan_gemm_bf16")
    return bm.value, bn.value


def plan_gemm_bf16_ln(M: int, N: int, Cin: int, KW: int = 1) -> bool:
    """True when a bf16-mode GEMM + LayerNorm of this shape takes the 64 x 256 full-row tile (else plain GEMM + row kernel)."""
    return bool(_lib.load().ns_plan_gemm_bf16_ln(int(M), int(N), int(Cin), int(KW)))


def plan_gemm_b3(M: int, N: int, Cin: int, KW: int = 1, epi: int = 0):
    """What a "bf16x3" model does with a GEMM (``epi`` 0) or GEMM + LayerNorm (``epi`` 1) on a weight that has planes
    (``ns_plan_gemm_b3``; host-side, no GPU): ``(BM, BN, ROWEPI, workgroups)`` of its one bf16x3 launch, or ``None`` when the exact-fp32
    kernels take it.  ``epi`` 1 with ROWEPI 0: the plain bf16x3 GEMM followed by the LayerNorm row kernel."""
    import ctypes

    o = (ctypes.c_int32 * 4)()
    n = _lib.load().ns_plan_gemm_b3(int(M), int(N), int(Cin), int(KW), int(epi), o)
    return tuple(o) if n else None


def plan_gemm_launches(M: int, N: int, Cin: int, KW: int = 1, epi: int = 0):
    """The launches the fp32 Conv1D-as-GEMM dispatch makes for this shape, named by the dispatch itself (``ns_plan_gemm_launches``;
    host-side, no GPU): a tuple of 0, 1 or 2 ``(BM, BN, BK, KS, MF, ROWEPI, TICKET, rows)``.  ``epi``: 0 plain, 1 LayerNorm on the
    full-row tile, 2 LayerNorm on the ticketed ladder."""
    import ctypes

    o = (ctypes.c_int32 * 16)()
    n = _lib.load().ns_plan_gemm_launches(int(M), int(N), int(Cin), int(KW), int(epi), o)
    return tuple(tuple(o[8 * l:8 * l + 8]) for l in range(n))


def cross_attention(q, kv, src_lens, n_head: int):
    """The aligner's ScaledDotProductAttention on already-projected heads (transformer/Modules.py:14-25, key-only mask): q [B,T,d],
    kv [B,L,2*d] (K | V, head h at h*dk inside each) -> (merged heads [B,T,d], attention probabilities [B,H,T,L])."""
    lib = _lib.load()
    B, T, d = q.shape
    L = kv.shape[1]
    q, kv, src_lens = q.contiguous(), kv.contiguous(), src_lens.long().contiguous()
    ctx = torch.empty(B, T, d, dtype=torch.float32, device=q.device)
    attn = torch.empty(B, n_head, T, L, dtype=torch.float32, device=q.device)
    _lib.check(lib.ns_aln_op_cross_attention(_lib.ptr(q), _lib.ptr(kv), _lib.ptr(src_lens), B, T, L, n_head, d // n_head, _lib.ptr(ctx),
                                             _lib.ptr(attn), _st(q)), "cross_attention")
    return ctx, attn


def aligner_input(mels, x):
    """The aligner's decoder input alone (transformer/Models.py:145-146): writes ``x`` = ``mels`` [B, T, C] with frame 0 of every
    utterance replaced by zeros.  Both are the caller's tensors (any view whose memory is [B, T, C] row-major)."""
    lib = _lib.load()
    B, T, C = mels.shape
    _lib.check(lib.ns_aln_op_input(_lib.ptr(mels), _lib.ptr(x), B, T, C, _st(mels)), "aligner_input")
    return x


def aligner_durations(attn_last, src_lens, mel_lens):
    """Frames per phoneme from one [B,H,T,L] alignment (EXTENSION beyond the reference, include/nar_fs2.h): int64 [B,L]."""
    lib = _lib.load()
    B, H, T, L = attn_last.shape
    attn_last = attn_last.contiguous()
    src_lens, mel_lens = src_lens.long().contiguous(), mel_lens.long().contiguous()
    out = torch.empty(B, L, dtype=torch.long, device=attn_last.device)
    _lib.check(lib.ns_aln_op_durations(_lib.ptr(attn_last), _lib.ptr(src_lens), _lib.ptr(mel_lens), B, H, T, L, _lib.ptr(out),
                                       _st(attn_last)), "aligner_durations")
    return out


# ---------------------------------------------------------------------------------------------------- packed rows (test hooks)
class PackedPlan:
    """What ``pack_plan`` built: the device plan (int32, ``None`` for a host-only plan) and the numbers every packed op takes.
    Utterance b owns rows [off[b], off[b] + win[b]) of the ``Mp`` packed rows, win[b] = min(max(lens[b], 0) + guard, S)."""

    def __init__(self, plan, lens, S, H, guard, Mp, att_wgs):
        self.plan, self.lens, self.B, self.S, self.H, self.guard, self.Mp, self.att_wgs = plan, list(lens), len(lens), S, H, guard, Mp, att_wgs

    @property
    def args(self):
        return (_lib.ptr(self.plan), self.B, self.S, self.Mp, self.att_wgs)

    def section(self, name):
        """one array of the device plan (``off``, ``win``, ``att_off``, ``att_order``, ``row_b``, ``row_t``, ``row_w``)"""
        B, Mp = self.B, self.Mp
        start = {"off": 0, "win": B + 1, "att_off": 2 * B + 2, "att_order": 3 * B + 3, "row_b": 4 * B + 4, "row_t": 4 * B + 4 + Mp, "row_w": 4 * B + 4 + 2 * Mp}[name]
        return self.plan[start:start + {"off": B + 1, "win": B, "att_off": B + 1, "att_order": B}.get(name, Mp)]


def pack_plan_ints(B: int, Mp: int) -> int:
    return 4 * B + 4 + 3 * Mp


def pack_plan(lens, S: int, H: int, guard: int, device=None, fill: int = 0) -> PackedPlan:
    """The packing plan of ``lens`` (a list of ints) on an axis of S rows for a stack of H heads (``ns_op_pack_plan``).  With
    ``device=None`` only the host numbers (Mp, att_wgs) — no GPU needed; else also the device plan, its buffer pre-filled with
    ``fill`` so that a caller can tell what the kernels wrote."""
    import ctypes

    lib = _lib.load()
    host = torch.tensor(list(lens), dtype=torch.long)
    mp, wgs = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(lib.ns_op_pack_plan(_lib.ptr(None), _lib.ptr(host), len(lens), int(S), int(H), int(guard), _lib.ptr(None), 0, ctypes.byref(mp),
                                   ctypes.byref(wgs), _lib.ptr(None)), "pack_plan")
    if device is None:
        return PackedPlan(None, lens, S, H, guard, mp.value, wgs.value)
    dev = host.to(device)
    plan = torch.full((pack_plan_ints(len(lens), mp.value),), fill, dtype=torch.int32, device=device)
    _lib.check(lib.ns_op_pack_plan(_lib.ptr(dev), _lib.ptr(host), len(lens), int(S), int(H), int(guard), _lib.ptr(plan), plan.numel(),
                                   ctypes.byref(mp), ctypes.byref(wgs), _st(plan)), "pack_plan")
    return PackedPlan(plan, lens, S, H, guard, mp.value, wgs.value)


def plan_attention_packed(B, S, H, dk, att_wgs, Mp, scratch_floats: int = 0, has_tickets: bool = False):
    """(form 0 strips / 1 work list, key ranges, merge launch 0 / 1, 32-key tiles per range) of the packed attention launch, from
    the function the launch dispatches on (host only)."""
    import ctypes

    o = (ctypes.c_int32 * 4)()
    _lib.check(_lib.load().ns_plan_attention_packed(int(B), int(S), int(H), int(dk), int(att_wgs), int(Mp), int(scratch_floats),
                                                    int(bool(has_tickets)), o), "plan_attention_packed")
    return tuple(o)


def attention_packed_scratch(p: PackedPlan, dk: int, split=True, tickets: bool = True):
    """(floats of scratch ``attention_core_packed`` allocates, floats of it left to the partials, ticket block carved) for the same
    arguments: room for 16 key ranges — ``split="block"``: for as many as ``block_packed`` reserves for its own attention — plus the
    ticket block the op takes from the end."""
    if not split:
        return 0, 0, False
    n = _lib.load().ns_plan_attention_split_packed(p.att_wgs, p.S, p.H, int(dk), p.Mp) if split == "block" else 16
    if n <= 1:
        return 0, 0, False
    import ctypes

    lib = _lib.load()
    flags = 0 if tickets else 2

    def carve(total):  # what the op makes of `total` floats, asked of the op's own function
        part, has = ctypes.c_size_t(0), ctypes.c_int32(0)
        _lib.check(lib.ns_op_attention_packed_carve(p.B, p.S, p.H, total * 4, flags, ctypes.byref(part), ctypes.byref(has)), "attention_packed_carve")
        return part.value, bool(has.value)

    want = n * (p.Mp * p.H * dk + 2 * p.Mp * p.H)
    big = want + (1 << 28)
    floats = want + (big - carve(big)[0])  # + the ticket block the op takes from the end
    return (floats,) + carve(floats)


def attention_core_packed(qkv_p, lens, p: PackedPlan, split=True, tickets: bool = True, bf16: bool = False):
    """``attention_core`` on packed rows: qkv_p [Mp, 3 d] -> [Mp, d].  ``split`` hands the launch scratch for its key ranges,
    ``tickets=False`` withholds the ticket block (the strip form then merges by a launch of its own)."""
    lib = _lib.load()
    Mp, d3 = qkv_p.shape
    assert Mp == p.Mp
    d = d3 // 3
    qkv_p, lens = qkv_p.contiguous(), lens.long().contiguous()
    out = torch.empty(Mp, d, dtype=torch.float32, device=qkv_p.device)
    floats = attention_packed_scratch(p, d // p.H, split, tickets)[0]
    scratch = torch.empty(floats, dtype=torch.float32, device=qkv_p.device) if floats else None
    _lib.check(lib.ns_op_attention_core_packed(_lib.ptr(qkv_p), _lib.ptr(lens), *p.args, p.H, d // p.H, _lib.ptr(out), _lib.ptr(scratch),
                                               floats * 4, _st(qkv_p), (1 if bf16 else 0) | (0 if tickets else 2)), "attention_core_packed")
    return out


def gemm_packed(model, name: str, x_p, p: PackedPlan):
    """``gemm`` on packed rows: x_p [Mp, Cin] -> [Mp, N], zero padding at each window's own edges."""
    x_p = x_p.contiguous()
    assert x_p.shape == (p.Mp, gemm_shape(model, name)[0])
    out = torch.empty(p.Mp, gemm_shape(model, name)[1], dtype=torch.float32, device=x_p.device)
    _lib.check(model._lib.ns_op_gemm_packed(model._h, name.encode(), _lib.ptr(x_p), *p.args, _lib.ptr(out), _st(x_p)), "gemm_packed")
    return out


def block_packed(model, which: str, prefix: str, x_p, lens, p: PackedPlan, mask_rows: bool = False):
    """``positionwise_ffn`` ("ffn"), ``multi_head_attention`` ("mha") or ``fft_block`` ("fft") of the layer ``prefix`` (the
    FFTBlock's prefix) on packed rows x_p [Mp, d]."""
    x_p = x_p.contiguous()
    assert x_p.shape[0] == p.Mp
    out = torch.empty_like(x_p)
    ws = _ws(model, p.B, p.S)
    lens_t = lens.long().contiguous() if lens is not None else None
    _lib.check(model._lib.ns_op_block_packed(model._h, {"ffn": 0, "mha": 1, "fft": 2}[which], prefix.encode(), _lib.ptr(x_p), _lib.ptr(lens_t),
                                             *p.args, int(bool(mask_rows)), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _st(x_p)), "block_packed")
    return out


def length_regulate_packed(x, cum, mel_lens, T: int, H: int, fill: int = 0):
    """``launch_length_regulate_packed`` alone: x [B, L, D], cum int32 [B, L], mel_lens int64 [B] (device) -> (out_p [Mp, D],
    status int32 [B], the PackedPlan it built with guard 20)."""
    lib = _lib.load()
    B, L, D = x.shape
    x, cum, mel_lens = x.contiguous(), cum.int().contiguous(), mel_lens.long().contiguous()
    p = pack_plan(mel_lens.cpu().tolist(), T, H, 20)
    p.plan = torch.full((pack_plan_ints(B, p.Mp),), fill, dtype=torch.int32, device=x.device)
    out = torch.empty(p.Mp, D, dtype=torch.float32, device=x.device)
    status = torch.full((B,), -1, dtype=torch.int32, device=x.device)
    _lib.check(lib.ns_op_length_regulate_packed(_lib.ptr(x), _lib.ptr(cum), _lib.ptr(mel_lens), B, L, D, int(T), p.Mp, int(H), _lib.ptr(out),
                                                _lib.ptr(status), _lib.ptr(p.plan), p.plan.numel(), _st(x)), "length_regulate_packed")
    return out, status, p


def gaussian_regulate(x, durations, own_len, T: int, out, s, p: PackedPlan | None = None, status=None, zero=None, nzero: int | None = None, w=None):
    """``launch_gaussian_upsampling`` alone as the forwards launch it (T_out = T): x [B, L, D], durations [B, L], own_len int64 [B];
    writes ``out`` ([B, T, D], or [Mp, D] with a plan ``p``), ``s`` (B * (L + 1) floats: the sums, then the centres), ``status`` int32
    [B] and the first ``nzero`` words of ``zero`` — all the caller's, pre-filled as it likes, the last two optional."""
    lib = _lib.load()
    B, L, D = x.shape
    assert x.is_contiguous() and durations.is_contiguous() and durations.dtype == torch.float32 and own_len.dtype == torch.long
    if nzero is None:
        nzero = zero.numel() if zero is not None else 0
    plan = (_lib.ptr(p.plan), p.Mp, p.att_wgs) if p is not None else (_lib.ptr(None), 0, 0)
    _lib.check(lib.ns_op_gaussian_regulate(_lib.ptr(x), _lib.ptr(durations), _lib.ptr(own_len), B, L, D, int(T), _lib.ptr(out), _lib.ptr(s),
                                           _lib.ptr(w), _lib.ptr(status), _lib.ptr(zero), int(nzero), *plan, _st(x)), "gaussian_regulate")
    return out


def embed_pos_packed(texts, emb, pos, p: PackedPlan):
    """texts int64 [B, L], emb [n_vocab, D], pos [>= L, D] -> [Mp, D]; also (re)writes the plan's row maps"""
    lib = _lib.load()
    B, L = texts.shape
    assert (B, L) == (p.B, p.S) and pos.shape[0] >= L
    texts, emb, pos = texts.long().contiguous(), emb.contiguous(), pos.contiguous()
    out = torch.empty(p.Mp, emb.shape[1], dtype=torch.float32, device=emb.device)
    _lib.check(lib.ns_op_embed_pos_packed(_lib.ptr(texts), _lib.ptr(emb), _lib.ptr(pos), _lib.ptr(p.plan), B, L, p.Mp, p.att_wgs, emb.shape[1],
                                          emb.shape[0], _lib.ptr(out), _st(emb)), "embed_pos_packed")
    return out


def add_pos_packed(x_p, pos, p: PackedPlan):
    lib = _lib.load()
    assert x_p.shape[0] == p.Mp and pos.shape[0] >= p.S and pos.shape[1] == x_p.shape[1]
    x_p, pos = x_p.contiguous(), pos.contiguous()
    out = torch.empty_like(x_p)
    _lib.check(lib.ns_op_add_pos_packed(_lib.ptr(x_p), _lib.ptr(pos), *p.args, x_p.shape[1], _lib.ptr(out), _st(x_p)), "add_pos_packed")
    return out


def pack_vector(src, p: PackedPlan):
    """src [B, S] -> [Mp]"""
    lib = _lib.load()
    assert src.shape == (p.B, p.S)
    src = src.contiguous().float()
    out = torch.empty(p.Mp, dtype=torch.float32, device=src.device)
    _lib.check(lib.ns_op_pack_vector(_lib.ptr(src), *p.args, _lib.ptr(out), _st(src)), "pack_vector")
    return out


def unpack_rows(src_p, lens, p: PackedPlan):
    """src_p [Mp, D] -> [B, S, D]: rows at t < min(lens[b], win[b]) (lens None: t < win[b]), zeros elsewhere"""
    lib = _lib.load()
    assert src_p.shape[0] == p.Mp
    src_p = src_p.contiguous()
    lens_t = lens.long().contiguous() if lens is not None else None
    D = src_p.shape[1]
    out = torch.full((p.B, p.S, D), float("nan"), dtype=torch.float32, device=src_p.device)
    _lib.check(lib.ns_op_unpack_rows(_lib.ptr(src_p), _lib.ptr(lens_t), *p.args, D, _lib.ptr(out), _st(src_p)), "unpack_rows")
    return out


def unpack_phase1(rows_p, vec_p, lens, p: PackedPlan):
    """rows_p [Mp, D], vec_p [Mp] -> (rows [B, S, D]: zeros past a window; vec [B, S]: zeros at t >= min(lens[b], win[b]))"""
    lib = _lib.load()
    assert rows_p.shape[0] == p.Mp == vec_p.shape[0]
    rows_p, vec_p, lens = rows_p.contiguous(), vec_p.contiguous(), lens.long().contiguous()
    D = rows_p.shape[1]
    rows = torch.full((p.B, p.S, D), float("nan"), dtype=torch.float32, device=rows_p.device)
    vec = torch.full((p.B, p.S), float("nan"), dtype=torch.float32, device=rows_p.device)
    _lib.check(lib.ns_op_unpack_phase1(_lib.ptr(rows_p), _lib.ptr(vec_p), _lib.ptr(lens), *p.args, D, _lib.ptr(rows), _lib.ptr(vec), _st(rows_p)),
               "unpack_phase1")
    return rows, vec


def unpack_outputs(p: PackedPlan, mel_lens, mel_p, post_p, p_p, e_p, mel_bias, post_const, mask: bool = True):
    """``launch_unpack_outputs`` alone; p_p / e_p may be None (no p_pred / e_pred).  Returns (mel, post, p_pred, e_pred, mel_mask)
    on the padded [B, T] grid, outputs pre-filled with NaN / 255 so that an unwritten element shows."""
    lib = _lib.load()
    n_mel = mel_p.shape[1]
    assert mel_p.shape == post_p.shape == (p.Mp, n_mel) and mel_bias.shape == (n_mel,) and post_const.shape == (11, n_mel)
    dev = mel_p.device
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    mel_lens, mel_p, post_p, p_p, e_p, mel_bias, post_const = mel_lens.long().contiguous(), c(mel_p), c(post_p), c(p_p), c(e_p), c(mel_bias), c(post_const)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    mel, post = nan(p.B, p.S, n_mel), nan(p.B, p.S, n_mel)
    pp = nan(p.B, p.S) if p_p is not None else None
    ep = nan(p.B, p.S) if e_p is not None else None
    mm = torch.full((p.B, p.S), 255, dtype=torch.uint8, device=dev) if mask else None
    _lib.check(lib.ns_op_unpack_outputs(*p.args, n_mel, _lib.ptr(mel_lens), _lib.ptr(mel_p), _lib.ptr(post_p), _lib.ptr(p_p), _lib.ptr(e_p),
                                        _lib.ptr(mel_bias), _lib.ptr(post_const), _lib.ptr(mel), _lib.ptr(post), _lib.ptr(pp), _lib.ptr(ep),
                                        _lib.ptr(mm), _st(mel_p)), "unpack_outputs")
    return mel, post, pp, ep, mm
