"""Float64 / numpy restatements of the packed-row stages (csrc/kernels.h RowMap), one at a time.  Shared by
tests/test_packed_ops_host.py (the case tables, and each restatement held against the wrong versions that matter, no GPU) and
tests/test_gpu_packed_ops.py (the kernels against them).

Packed rows: utterance b of a batch on an axis of S rows keeps its WINDOW of win[b] = min(max(len[b], 0) + guard, S) rows, the
windows are laid end to end (off = exclusive scan, Mp = sum) and every stage runs on the [Mp, .] matrix as if each window were an
utterance of its own: a convolution pads with zeros at the window's edges, attention sees the keys t < min(len[b], win[b]) of its
own window.  Nothing here is written from a kernel: the plan follows the sentence above and kernels.h, unpack_outputs the comment
over k_unpack_outputs, the rest the one-line contracts in kernels.h."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from tests import bf16_emu as E


# ---------------------------------------------------------------------------------------------------- plan
@dataclass
class Plan:
    lens: list
    S: int
    H: int
    guard: int
    win: np.ndarray
    off: np.ndarray        # [B + 1]
    att_order: np.ndarray  # [B]
    att_off: np.ndarray    # [B + 1]
    row_b: np.ndarray
    row_t: np.ndarray
    row_w: np.ndarray

    @property
    def B(self):
        return len(self.lens)

    @property
    def Mp(self):
        return int(self.off[-1])

    @property
    def att_wgs(self):
        return int(self.att_off[-1])

    def ints(self, fill=0):
        """the device plan's layout (kernels.h plan_pointers): off [B+1] | win [B], 1 unused | att_off [B+1] | att_order [B], 1 unused |
        row_b | row_t | row_w; the two unused ints keep `fill`"""
        pad = np.array([fill], np.int64)
        return np.concatenate([self.off, self.win, pad, self.att_off, self.att_order, pad, self.row_b, self.row_t, self.row_w]).astype(np.int32)

    def keys(self):
        """valid keys per utterance: min(max(len, 0), win)"""
        return np.minimum(np.maximum(np.asarray(self.lens, np.int64), 0), self.win)


def plan_ref(lens, S, H, guard, clamp=True, ties_by_index=True):
    """clamp=False / ties_by_index=False are the WRONG versions (window not clamped to S; equal windows ranked by descending index)"""
    l = np.asarray(lens, dtype=np.int64)
    win = np.maximum(l, 0) + guard
    if clamp:
        win = np.minimum(win, S)
    B = len(l)
    off = np.concatenate([[0], np.cumsum(win)])
    key = [(-int(win[b]), b if ties_by_index else -b) for b in range(B)]
    att_order = np.array(sorted(range(B), key=lambda b: key[b]), dtype=np.int64)  # stable, descending window
    att_off = np.concatenate([[0], np.cumsum((win[att_order] + 127) // 128 * H)])
    row_b = np.repeat(np.arange(B), win)
    row_t = np.concatenate([np.arange(w) for w in win]) if B else np.zeros(0, np.int64)
    return Plan(list(map(int, l)), S, H, guard, win, off, att_order, att_off, row_b, row_t, win[row_b])


def pack_rows(x, p):
    """[B, S, ...] -> [Mp, ...]: the first win[b] rows of every utterance"""
    return torch.cat([x[b, :int(p.win[b])] for b in range(p.B)], dim=0)


def windows(y_p, p):
    """[Mp, ...] -> the B windows"""
    return [y_p[int(p.off[b]):int(p.off[b + 1])] for b in range(p.B)]


# ---------------------------------------------------------------------------------------------------- contraction
def conv_packed(x_p, w, b, p, dtype=torch.float64, leak=0):
    """each window convolved alone, zero padding at its own edges.  leak = 1 is the WRONG version: the taps of a window's first and
    last row reach one row into the neighbouring windows"""
    out = []
    for u in range(p.B):
        lo, hi = int(p.off[u]), int(p.off[u + 1])
        a, z = max(lo - leak, 0), min(hi + leak, p.Mp)
        y = E.conv_rows(x_p[a:z][None], w, b, dtype)[0]
        out.append(y[lo - a:lo - a + (hi - lo)])
    return torch.cat(out, dim=0)


def gemm_packed_ref(x_p, w, b, p, act=None, round_fn=E.exact, dtype=torch.float64):
    return E.ACTS[act](conv_packed(round_fn(x_p), round_fn(w), b, p, dtype))


def gemm_packed_unit(x_p, w, b, p, round_fn=E.exact):
    return conv_packed(round_fn(x_p).abs(), round_fn(w).abs(), None if b is None else b.abs(), p)


def gemm_packed_check(got_p, x_p, w, b, p, act=None, rel=E.FP32_REL, round_fn=E.exact, ref=None, unit=None):
    """E.gemm_check over every packed row, guard rows included"""
    ref = gemm_packed_ref(x_p, w, b, p, act, round_fn) if ref is None else ref
    unit = gemm_packed_unit(x_p, w, b, p, round_fn) if unit is None else unit
    return E.gemm_check(got_p, x_p, w, b, act=act, rel=rel, ref=ref, unit=unit, round_fn=round_fn)


def gemm_ln_packed_check(got_p, a_p, w, b, resid_p, g, beta, p, rel=E.FP32_REL, round_fn=E.exact, act=None, rows=None):
    """E.gemm_ln_check window by window (its contraction pads per utterance).  rows (bool [Mp], optional): the rows held to the
    bound — the others (masked rows) are the caller's to check."""
    ok, worst = True, 0.0
    for u, (gw, aw, rw) in enumerate(zip(windows(got_p, p), windows(a_p, p), windows(resid_p, p) if resid_p is not None else [None] * p.B)):
        ref, bound = E._ln_ref_bound(aw[None], w, b, None if rw is None else rw[None], g, beta, rel, round_fn, act)
        err = (gw[None].double() - ref).abs()
        keep = torch.ones(gw.shape[0], dtype=torch.bool) if rows is None else rows[int(p.off[u]):int(p.off[u + 1])]
        err, bound, fin = err[0][keep], bound[0][keep], torch.isfinite(gw[keep]).all()
        if err.numel():
            ok = ok and bool((err <= bound).all()) and bool(fin)
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return E.LnCheck(ok, worst)


def ln_packed_ref(a_p, w, b, resid_p, g, beta, p, dtype=torch.float64, act=None):
    """LayerNorm(act(conv(a)) + resid) on packed rows evaluated in dtype (float32: torch's fp32 on the CPU)"""
    z = gemm_packed_ref(a_p, w, b, p, act, dtype=dtype)
    if resid_p is not None:
        z = z + resid_p.to(dtype)
    return E.layernorm_emu(z, g, beta, dtype=dtype)


def valid_rows(p):
    """bool [Mp]: t < len[b]"""
    return torch.from_numpy(p.row_t < np.asarray(p.lens, np.int64)[p.row_b])


# ---------------------------------------------------------------------------------------------------- attention
def ref_attention(qkv, lens, H, dtype=torch.float64):
    """tests/test_gpu_attention.py ref_attention (restated here so that the CPU suite imports no GPU module); dtype = float32:
    torch's fp32 evaluation on the CPU"""
    B, S, d3 = qkv.shape
    d = d3 // 3
    dk = d // H
    x = qkv.to(dtype)
    q, k, v = (x[..., i * d:(i + 1) * d].reshape(B, S, H, dk).permute(0, 2, 1, 3) for i in range(3))
    a = q @ k.transpose(-1, -2) / float(np.power(dk, 0.5))
    pad = torch.arange(S)[None, :] >= lens[:, None]
    a = a.masked_fill(pad[:, None, None, :], -np.inf)
    o = torch.softmax(a, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(B, S, d)


def attention_packed_ref(qkv_p, p, H, keys_at_win=False, dtype=torch.float64):
    """per utterance over its win[b] query rows and its keys < min(len[b], win[b]); NaN rows where no key is valid.
    keys_at_win is the WRONG version: every row of the window is a key"""
    out = []
    for u, xw in enumerate(windows(qkv_p, p)):
        n = int(p.win[u]) if keys_at_win else int(p.keys()[u])
        out.append(ref_attention(xw[None], torch.tensor([n]), H, dtype)[0])
    return torch.cat(out, dim=0)


def key_ranges(p, form, nsplit):
    """per utterance (32-key tiles it has, tiles per key range, number of ranges that own no valid tile) under a launch form
    (0: strips, 4 waves x nsplit ranges; 1: work list, nsplit ranges) — attention.hip's `tps` / `tpr` arithmetic"""
    out = []
    for n in p.keys():
        tiles = (int(n) + 31) // 32
        nr = nsplit * 4 if form == 0 else nsplit
        per = (tiles + nr - 1) // nr
        out.append((tiles, per, sum(1 for r in range(nr) if r * per >= tiles)))
    return out


# ---------------------------------------------------------------------------------------------------- data movement
def length_regulate_packed_ref(x, cum, mel_lens, T, p):
    """(out_p [Mp, D], status [B]) of LengthRegulator.LR into the packed layout: frame t of utterance b copies encoder row
    i = first index with cum[b, i] > t, zeros at t >= cum[b, -1]; status bit 0 = the total exceeds T, bit 1 = mel_lens[b] < 0"""
    xn, cn = x.numpy(), cum.numpy().astype(np.int64)
    out = np.zeros((p.Mp, x.shape[2]), np.float32)
    for m in range(p.Mp):
        b, t = int(p.row_b[m]), int(p.row_t[m])
        if t < cn[b, -1]:
            out[m] = xn[b, int(np.searchsorted(cn[b], t, side="right"))]
    status = np.array([(1 if cn[b, -1] > T else 0) | (2 if int(mel_lens[b]) < 0 else 0) for b in range(p.B)], np.int32)
    return torch.from_numpy(out), torch.from_numpy(status)


def embed_pos_packed_ref(texts, emb, pos, p):
    """emb[token] + pos[t] in fp32; a token id outside [0, n_vocab) reads row 0"""
    tok = texts.numpy()[p.row_b, p.row_t]
    tok = np.where((tok < 0) | (tok >= emb.shape[0]), 0, tok)
    return torch.from_numpy(emb.numpy()[tok] + pos.numpy()[p.row_t])


def add_pos_ref(x_p, pos, p):
    return torch.from_numpy(x_p.numpy() + pos.numpy()[p.row_t])


def pack_vector_ref(src, p):
    return torch.from_numpy(src.numpy()[p.row_b, p.row_t])


def unpack_rows_ref(src_p, lens, p):
    """[B, S, D]: the packed row where t < min(lens[b], win[b]) (lens None: t < win[b]), zeros elsewhere"""
    out = np.zeros((p.B, p.S, src_p.shape[1]), np.float32)
    for b in range(p.B):
        n = int(p.win[b]) if lens is None else int(min(max(int(lens[b]), 0), p.win[b]))
        out[b, :n] = src_p.numpy()[int(p.off[b]):int(p.off[b]) + n]
    return torch.from_numpy(out)


def unpack_phase1_ref(rows_p, vec_p, lens, p):
    """rows [B, S, D]: the packed row where t < win[b], zeros past the window; vec [B, S]: the packed value where
    t < min(lens[b], win[b]), zeros elsewhere"""
    return unpack_rows_ref(rows_p, None, p), unpack_rows_ref(vec_p[:, None], lens, p)[:, :, 0]


def unpack_outputs_ref(p, mel_lens, mel_p, post_p, p_p, e_p, mel_bias, post_const, d_len=0, d_end=0):
    """The comment over k_unpack_outputs (csrc/rowops.hip), frame t of utterance b with window w and length len = the utterance's
    length as the plan takes it, min(max(mel_lens[b], 0), T):
      mel       t < w: the packed row; else mel_bias
      p / e     t < w: the packed value; else 0
      mel_mask  t >= mel_lens[b]
      postnet   w == T: the packed row.  w < T: t < len + 10 the packed row; t >= T - 10 row 1 + t - (T - 10) of post_const; else
                row 0 of post_const.
    d_len / d_end move the two boundaries (the WRONG versions: len + 9, T - 9)."""
    T, n_mel = p.S, mel_p.shape[1]
    mel = np.zeros((p.B, T, n_mel), np.float32)
    post = np.zeros((p.B, T, n_mel), np.float32)
    pp, ep = np.zeros((p.B, T), np.float32), np.zeros((p.B, T), np.float32)
    mask = np.zeros((p.B, T), np.uint8)
    melp, postp, bias, const = mel_p.numpy(), post_p.numpy(), mel_bias.numpy(), post_const.numpy()
    for b in range(p.B):
        w, o = int(p.win[b]), int(p.off[b])
        ln = min(max(int(mel_lens[b]), 0), T)
        for t in range(T):
            mask[b, t] = 1 if t >= int(mel_lens[b]) else 0
            mel[b, t] = melp[o + t] if t < w else bias
            if p_p is not None:
                pp[b, t] = p_p.numpy()[o + t] if t < w else 0.0
            if e_p is not None:
                ep[b, t] = e_p.numpy()[o + t] if t < w else 0.0
            if w == T or t < ln + 10 + d_len:
                post[b, t] = postp[o + t]
            elif t >= T - 10 + d_end:
                post[b, t] = const[1 + t - (T - 10 + d_end)]
            else:
                post[b, t] = const[0]
    f = torch.from_numpy
    return f(mel), f(post), (f(pp) if p_p is not None else None), (f(ep) if e_p is not None else None), f(mask)
