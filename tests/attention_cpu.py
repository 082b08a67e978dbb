"""The yardstick of the dense (grid) self-attention launches (csrc/attention.hip launch_attention with rm == nullptr), plain torch /
numpy, no GPU.  Shared by tests/test_attention_ops_host.py (the case table, the dispatch against its restatement, the wrong versions
the gate must reject) and tests/test_gpu_attention_ops.py (the kernels against it); tests/test_gpu_attention.py imports its float64
attention from here.

  ref_attention        transformer/Modules.py:14-25 on head-packed q | k | v in float64 (dtype=float32: torch's fp32 on the CPU)
  plan_dense_ref       the decision launch_attention made INLINE before it was lifted into attention_plan_dense, restated from that
                       inline code (strip_plan, the small grid's own key split, plan_key_split) — not from the new function
  key_ranges_dense     per utterance: valid 32-key tiles, tiles per range (per wave for strips), ranges that own no valid tile
  xcd_remap            k_attention's workgroup remap (launch index -> position in (batch, head, query tile) order)
  split_merge_ref      the same attention evaluated range by range and merged, in float64, with the wrong merges as options

Forms (the issue's table): A strips, one workgroup per strip; B strips with 2..8 key-range workgroups merged by the last arriver; C the
same merged by a k_attention_merge launch; D k_attention, one sweep, fewer than 128 blocks; E the small grid's own key split + merge
launch; F k_attention, one sweep, 128 blocks or more; G the planner's key split + merge launch."""
from __future__ import annotations

import numpy as np
import torch

ATT_SPLIT_MAX, ATT_SPLIT_MAX_BLOCKS, ATT_STRIP_SPLIT_MAX = 16, 128, 8
STRIP, GRID = 0, 1                 # kernel
NONE, LAST_ARRIVER, MERGE_LAUNCH = 0, 1, 2
SENTINEL = -12345.0                # what a test pre-fills `out` with: finite, and no attention output of N(0, 1) values


# ---------------------------------------------------------------------------------------------------- the function
def ref_attention(qkv, lens, H, dtype=torch.float64):
    """qkv [B, S, 3 d] (Q | K | V, head h at h * dk inside each), lens [B] -> [B, S, d]; keys t >= lens[b] are masked (a length
    above S masks nothing), all S query rows are computed, a zero length gives NaN rows"""
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


def ref_attention_fp32(qkv, lens, H):
    """torch's fp32 evaluation on the CPU: how far plain fp32 is from float64 on the same input (reported, never gated)"""
    return ref_attention(qkv, lens, H, dtype=torch.float32)


def mutant_attention(qkv, lens, H, mask_at_S=False, mask_shift=0, scale_dk=False, head_shift=0):
    """ref_attention in float64 with ONE thing wrong: keys masked at S instead of lens[b]; the mask off by mask_shift keys; the
    scale 1 / dk instead of 1 / sqrt(dk); head h reading head (h + head_shift) % H's K block"""
    B, S, d3 = qkv.shape
    d = d3 // 3
    dk = d // H
    x = qkv.double()
    q, k, v = (x[..., i * d:(i + 1) * d].reshape(B, S, H, dk).permute(0, 2, 1, 3) for i in range(3))
    if head_shift:
        k = torch.roll(k, -head_shift, dims=1)
    a = q @ k.transpose(-1, -2) / (float(dk) if scale_dk else float(np.power(dk, 0.5)))
    edge = torch.full_like(lens, S) if mask_at_S else lens + mask_shift
    pad = torch.arange(S)[None, :] >= edge[:, None]
    a = a.masked_fill(pad[:, None, None, :], -np.inf)
    o = torch.softmax(a, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(B, S, d)


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def _f32(x):
    return np.float32(x)


def plan_key_split_ref(blocks, tiles, dk, M, d):
    """plan_key_split: the cost model in the fp32 arithmetic of the host code (rounds * (3.7 + c * tiles per range) + merge)"""
    c, f = _f32(3.9 if dk == 128 else 2.1 if dk == 64 else 1.2), _f32(3.7)
    rounds = lambda w: _f32((w + 255) // 256)  # noqa: E731
    one = rounds(blocks) * (f + c * _f32(tiles))
    best, best_us = 1, one * _f32(0.94)
    for n in range(2, min(ATT_SPLIT_MAX, tiles) + 1):
        tps = (tiles + n - 1) // n
        if (tiles + tps - 1) // tps != n:
            continue
        us = rounds(blocks * n) * (f + c * _f32(tps)) + _f32(4.0) + _f32(float(n + 1) * float(M) * d * 4.0 / 12e6)
        if us < best_us:
            best, best_us = n, us
    return best


def strip_plan_ref(B, S, H, dk, M, scratch_floats):
    """strip_plan: (taken, key-range workgroups per strip, 32-key tiles per wave)"""
    d, tiles = H * dk, (S + 31) // 32
    part = lambda n: n * (M * d + 2 * M * H)  # noqa: E731
    strips = tiles * H * B
    nsplit = (256 + strips - 1) // strips
    nsplit = min(nsplit, (tiles + 3) // 4, ATT_STRIP_SPLIT_MAX)
    if nsplit > 1 and not scratch_floats:
        nsplit = 1
    if part(nsplit) * 4 >= 1 << 31:
        nsplit = 1
    while nsplit > 1 and part(nsplit) > scratch_floats:
        nsplit -= 1
    tpr = (tiles + 4 * nsplit - 1) // (4 * nsplit)
    nsplit = ((tiles + tpr - 1) // tpr + 3) // 4
    tpr = (tiles + 4 * nsplit - 1) // (4 * nsplit)
    return tpr <= 4, nsplit, tpr


def plan_dense_ref(B, S, H, dk, scratch_floats=0, has_tickets=False, planner=True):
    """(kernel, key ranges, merge, tiles per wave / per range) of the dense launch as launch_attention decided it inline:
    strips first when the launch has fewer than 128 (query tile, head) blocks and a wave sweeps at most 4 tiles; else k_attention
    with the small grid's own split (256 / blocks ranges, no empty one), or the planner's (plan_key_split; planner=False: NS_PLAN=0)"""
    d = H * dk
    qtiles, tiles = (S + 127) // 128, (S + 31) // 32
    blocks, M = qtiles * H * B, B * S
    part = lambda n: n * (M * d + 2 * M * H)  # noqa: E731
    if blocks < ATT_SPLIT_MAX_BLOCKS:
        ok, nsplit, tpr = strip_plan_ref(B, S, H, dk, M, scratch_floats)
        if ok:
            return STRIP, nsplit, (NONE if nsplit == 1 else LAST_ARRIVER if has_tickets else MERGE_LAUNCH), tpr
    nsplit = 1
    if scratch_floats and blocks < ATT_SPLIT_MAX_BLOCKS:
        nsplit = min(256 // blocks, ATT_SPLIT_MAX, tiles)
        while nsplit > 1 and part(nsplit) > scratch_floats:
            nsplit -= 1
        nsplit = max(nsplit, 1)
        tps = (tiles + nsplit - 1) // nsplit
        nsplit = (tiles + tps - 1) // tps
    elif scratch_floats and planner:
        nsplit = plan_key_split_ref(blocks, tiles, dk, M, d)
        while nsplit > 1 and part(nsplit) > scratch_floats:
            nsplit -= 1
        tps = (tiles + nsplit - 1) // nsplit
        nsplit = (tiles + tps - 1) // tps
    return GRID, nsplit, (MERGE_LAUNCH if nsplit > 1 else NONE), (tiles + nsplit - 1) // nsplit


def attention_split_ref(B, S, H, dk, planner=True):
    """ns_plan_attention_split: the ranges a workspace reserves partials for"""
    blocks = (S + 127) // 128 * H * B
    if blocks < ATT_SPLIT_MAX_BLOCKS:
        return ATT_SPLIT_MAX
    return plan_key_split_ref(blocks, (S + 31) // 32, dk, B * S, H * dk) if planner else 1


def blocks_of(B, S, H):
    return (S + 127) // 128 * H * B


def form_of(plan, B, S, H):
    """the issue's letter for a plan (kernel, key ranges, merge, tiles)"""
    kernel, nsplit, merge, _ = plan
    if kernel == STRIP:
        return "A" if nsplit == 1 else {LAST_ARRIVER: "B", MERGE_LAUNCH: "C"}[merge]
    if blocks_of(B, S, H) < ATT_SPLIT_MAX_BLOCKS:
        return "D" if nsplit == 1 else "E"
    return "F" if nsplit == 1 else "G"


def workgroups(plan, B, S, H):
    """workgroups of the main launch: (strips or 128-query tiles) x key ranges x heads x utterances"""
    kernel, nsplit = plan[0], plan[1]
    return ((S + 31) // 32 if kernel == STRIP else (S + 127) // 128) * nsplit * H * B


def key_ranges_dense(lens, S, kernel, nsplit):
    """per utterance (32-key tiles it has, tiles per key range, number of ranges that own no valid tile): the kernels cut the
    VALID tiles of each utterance, ceil(min(max(len, 0), S) / 32), into nsplit ranges (k_attention) or 4 waves x nsplit (strips)"""
    out = []
    for n in lens:
        tiles = (min(max(int(n), 0), S) + 31) // 32
        nr = nsplit * 4 if kernel == STRIP else nsplit
        per = (tiles + nr - 1) // nr
        out.append((tiles, per, sum(1 for r in range(nr) if r * per >= tiles)))
    return out


# ---------------------------------------------------------------------------------------------------- the XCD remap
def xcd_remap(L, nblk, drop_remainder=False):
    """k_attention's remap: workgroup L of nblk (it runs on XCD L % 8) takes position pos of the (batch, head, query tile) order, XCD
    x owning the x-th contiguous slice — the first nblk % 8 slices one longer.  drop_remainder is the WRONG version without that
    branch (every slice nblk // 8 long)"""
    q8, r8, xcd = nblk >> 3, nblk & 7, L & 7
    if drop_remainder:
        return xcd * q8 + (L >> 3)
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + (L >> 3)


def is_bijection(nblk, drop_remainder=False):
    return sorted(xcd_remap(L, nblk, drop_remainder) for L in range(nblk)) == list(range(nblk))


# ---------------------------------------------------------------------------------------------------- range by range
def split_merge_ref(qkv, lens, H, kernel, nsplit, same_reference=False, drop_last=False, first_l_only=False, empty_l_one=False):
    """The attention evaluated as a split launch does, in float64: every utterance's valid key tiles cut into key ranges
    (key_ranges_dense), each range leaving (m, l, O) = (max score, sum 2^(s - m), sum 2^(s - m) v), merged as k_attention_merge
    does: out = sum_r O_r 2^(m_r - m) / sum_r l_r 2^(m_r - m), m = max_r m_r (0 where no range holds a key).  Exact: equals
    ref_attention to rounding.  The WRONG merges: same_reference ignores the difference between the ranges' reference points
    (every weight 1); drop_last leaves out the last partial of the merge (the last range; the last workgroup's four waves for split
    strips); first_l_only divides by the first range's l alone; empty_l_one lets a
    range without keys contribute (m, l, O) = (0, 1, 0) instead of (-inf, 0, 0)."""
    B, S, d3 = qkv.shape
    d = d3 // 3
    dk = d // H
    x = qkv.double()
    q, k, v = (x[..., i * d:(i + 1) * d].reshape(B, S, H, dk).permute(0, 2, 1, 3) for i in range(3))
    out = torch.empty(B, H, S, dk, dtype=torch.float64)
    log2e = 1.4426950408889634
    for b, (tiles, per, _) in enumerate(key_ranges_dense(lens.tolist(), S, kernel, nsplit)):
        n = min(max(int(lens[b]), 0), S)
        nr = nsplit * 4 if kernel == STRIP else nsplit
        s = (q[b] @ k[b].transpose(-1, -2)) * (log2e / float(np.power(dk, 0.5)))  # [H, S, S], in powers of two as the kernels
        ms, ls, os_ = [], [], []
        for r in range(nr - (4 if kernel == STRIP and nsplit > 1 else 1) if drop_last else nr):
            k0, k1 = min(r * per * 32, n), min((r + 1) * per * 32, n)
            if k1 <= k0:
                m = torch.full((H, S, 1), 0.0 if empty_l_one else -np.inf, dtype=torch.float64)
                ms.append(m)
                ls.append(torch.full((H, S, 1), 1.0 if empty_l_one else 0.0, dtype=torch.float64))
                os_.append(torch.zeros(H, S, dk, dtype=torch.float64))
                continue
            sr = s[:, :, k0:k1]
            m = sr.max(dim=-1, keepdim=True).values
            p = torch.exp2(sr - m)
            ms.append(m)
            ls.append(p.sum(dim=-1, keepdim=True))
            os_.append(p @ v[b][:, k0:k1])
        mx = torch.stack(ms).max(dim=0).values
        mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
        acc, l = torch.zeros(H, S, dk, dtype=torch.float64), torch.zeros(H, S, 1, dtype=torch.float64)
        for i, (m, lr, o) in enumerate(zip(ms, ls, os_)):
            w = torch.ones_like(m) if same_reference else torch.exp2(m - mx)
            if same_reference:
                w = torch.where(torch.isinf(m), torch.zeros_like(w), w)
            acc = acc + o * w
            if not first_l_only or i == 0:
                l = l + lr * w
        out[b] = acc / l
    return out.permute(0, 2, 1, 3).reshape(B, S, d)


# ---------------------------------------------------------------------------------------------------- inputs and the rules
def make_qkv(B, S, H, dk, seed, scale=1.0, replica=True):
    """N(0, scale) inputs; the last utterance is a copy of the first (its length is the case's to repeat)"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3 * H * dk, generator=g) * scale
    if replica and B > 1:
        qkv[-1] = qkv[0]
    return qkv


def spike(qkv, lens, H, late_key, early_key=3):
    """The spiked input of a form (inputs at scale 0.5): in utterance 0 (and its copy, the last) head 0's key `late_key` stands far
    above every other key of every query, so the online softmax's reference point must move when the sweep reaches it, in whatever
    range or tile it lies; in the same utterances head 1's key `early_key` (first tile) dominates, so its reference point is set by
    the first tile and must not move again."""
    B, S, d3 = qkv.shape
    d = d3 // 3
    dk = d // H
    assert H >= 2 and early_key < 32 <= late_key < min(int(lens[0]), S)
    for b in {0, B - 1}:
        qkv[b, late_key, d:d + dk] = 6.0
        qkv[b, :, :dk] += 1.0
        qkv[b, early_key, d + dk:d + 2 * dk] = 8.0
        qkv[b, :, dk:2 * dk] = qkv[b, :, dk:2 * dk].abs() + 0.5
    return qkv


def check_output(got, ref, lens):
    """(worst |got - ref| over the rows of utterances with a key, rows of zero-length utterances NaN exactly and all others finite,
    number of values still at the sentinel)"""
    live = torch.tensor([int(n) > 0 for n in lens])
    nan_ok = bool(torch.isnan(got[~live]).all()) and bool(torch.isfinite(got[live]).all())
    err = float((got[live].double() - ref[live].double()).abs().max()) if bool(live.any()) else 0.0
    if not np.isfinite(err):
        err = float("inf")
    return err, nan_ok, int((got == SENTINEL).sum())
