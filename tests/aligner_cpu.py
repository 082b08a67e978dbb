"""Torch-CPU restatement of the reference's ``MelEncoder.forward`` in ``eval()`` (transformer/Models.py:140-173) and of the
aligner's duration rule (an extension beyond the reference, include/nar_fs2.h), in the dtype of the weights it is given
(fp32 or float64).  Written from the reference's behaviour, with line citations; no reference text is copied.  The text encoder
that feeds it is ``oracle.fs2_oracle.txt_encoder``."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import fs2_oracle as orc

LN_EPS = 1e-5  # nn.LayerNorm's default (transformer/SubLayers.py:23,84)


def to_torch_weights(sd_np, dtype=torch.float32):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd_np.items()}


def n_layers(w):
    n = 0
    while f"mel_encoder.layer_stack.{n}.crs_attn.w_qs.weight" in w:
        n += 1
    return n


def cross_attention_core(q, k, v, key_pad, n_head):
    """transformer/SubLayers.py:39-54 + Modules.py:14-25 on projected q [B,T,d], k / v [B,L,d]: heads split, scores divided by
    sqrt(d_k), -inf at padded KEYS (every query row is computed), softmax over keys; returns (merged heads [B,T,d], attn [B,H,T,L])."""
    B, T, d = q.shape
    L = k.shape[1]
    dk = d // n_head
    qh = q.view(B, T, n_head, dk).permute(0, 2, 1, 3)
    kh = k.view(B, L, n_head, dk).permute(0, 2, 1, 3)
    vh = v.view(B, L, n_head, dk).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) / np.power(dk, 0.5)
    s = s.masked_fill(key_pad[:, None, None, :], -np.inf)
    attn = torch.softmax(s, dim=-1)
    out = torch.matmul(attn, vh).permute(0, 2, 1, 3).reshape(B, T, d)
    return out, attn


def mel_encoder(w, src_output, mels, src_mask, mel_mask, n_head, max_seq_len):
    """transformer/Models.py:140-173 in eval(): frame 0 replaced by zeros (:145-146), Prenet (Layers.py:22-26, dropout = identity),
    position rows (the cached table, or the regenerated one for T > max_seq_len, :149-164), then per FFTBlock2 (Layers.py:61-70)
    crs_attn(tgt, src, src) with LayerNorm(fc(.) + tgt) (SubLayers.py:56-57), masked_fill, pos_ffn, masked_fill.
    Returns (tgt_output [B,T,d], [attn [B,H,T,L] per layer])."""
    B, T, _ = mels.shape
    x = torch.cat([torch.zeros_like(mels[:, :1]), mels[:, 1:]], dim=1)
    p = "mel_encoder.prenet"
    x = F.relu(F.linear(F.relu(F.linear(x, w[p + ".w_1.weight"], w[p + ".w_1.bias"])), w[p + ".w_2.weight"], w[p + ".w_2.bias"]))
    d = x.shape[-1]
    pos = orc.sinusoid_table(T, d) if T > max_seq_len else w["mel_encoder.position_enc"][0, :T]
    x = x + pos.to(device=x.device, dtype=x.dtype).unsqueeze(0)
    attns = []
    for i in range(n_layers(w)):
        p = f"mel_encoder.layer_stack.{i}"
        a = p + ".crs_attn"
        q = F.linear(x, w[a + ".w_qs.weight"], w[a + ".w_qs.bias"])
        k = F.linear(src_output, w[a + ".w_ks.weight"], w[a + ".w_ks.bias"])
        v = F.linear(src_output, w[a + ".w_vs.weight"], w[a + ".w_vs.bias"])
        ctx, attn = cross_attention_core(q, k, v, src_mask, n_head)
        y = F.linear(ctx, w[a + ".fc.weight"], w[a + ".fc.bias"])
        y = F.layer_norm(y + x, (d,), w[a + ".layer_norm.weight"], w[a + ".layer_norm.bias"], LN_EPS)
        y = y.masked_fill(mel_mask.unsqueeze(-1), 0)
        y = orc.positionwise_ffn(w, p + ".pos_ffn", y)
        x = y.masked_fill(mel_mask.unsqueeze(-1), 0)
        attns.append(attn)
    return x, attns


def align(w, model_cfg, texts, src_lens, mels, mel_lens):
    """txt_encoder + mel_encoder as model/fastspeech2_align.py:45,56 chains them (w holds both families of weights)."""
    t = model_cfg["transformer"]
    L, T = texts.shape[1], mels.shape[1]
    src_mask = torch.arange(L, device=src_lens.device)[None, :] >= src_lens[:, None]  # utils/tools.py:89-97, True = padding
    mel_mask = torch.arange(T, device=mel_lens.device)[None, :] >= mel_lens[:, None]
    src_output = orc.txt_encoder(w, texts, src_mask, t["encoder_head"], model_cfg["max_seq_len"])
    return mel_encoder(w, src_output, mels, src_mask, mel_mask, t["decoder_head"], model_cfg["max_seq_len"])


def head_sum(attn_last):
    """a[b,t,l] = sum over heads in head order, in the array's own dtype (numpy [B,H,T,L])."""
    a = attn_last[:, 0].copy()
    for h in range(1, attn_last.shape[1]):
        a = a + attn_last[:, h]
    return a


def durations(attn_last, src_lens, mel_lens):
    """durations[b,i] = #{t < mel_len[b] : argmax_{l < src_len[b]} a[t,l] == i}, ties to the lowest l; 0 for i >= src_len; the
    whole row 0 when src_len or mel_len is 0.  numpy in, int64 [B,L] out."""
    attn_last = np.asarray(attn_last)
    B, _, T, L = attn_last.shape
    a = head_sum(attn_last)
    out = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        sl, ml = int(min(max(src_lens[b], 0), L)), int(min(max(mel_lens[b], 0), T))
        if sl == 0 or ml == 0:
            continue
        idx = np.argmax(a[b, :ml, :sl], axis=1)  # first maximum = lowest index
        out[b] = np.bincount(idx, minlength=L)
    return out


# ---- crafted maps for the duration kernel alone (tests/test_gpu_aligner.py; tests/test_aligner_host.py shows what they catch) ---------
DYADIC = np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.75, 1.0], dtype=np.float32)   # head sums of up to 4 of these are exact: ties are real
PLANTS = np.array([8.0, np.inf, np.nan], dtype=np.float32)                       # what must never count: above every valid entry, or NaN
GRIDS = {1: (1, 1), 5: (5, 1), 259: (7, 37)}                                     # B * T -> (B, T); 4 waves per workgroup: 1, 5 and 259 leave a partial one


def crafted_map(H, L, B, T, seed):
    """(attn [B, H, T, L], src_lens [B], mel_lens [B]).  Row kinds by (b T + t) % 8: 0 random dyadic draws (ties everywhere), 1 all
    equal (key 0 wins), 2 all -inf (key 0 wins), 3 the maximum on the last valid key, 4 a tie between l and l + 64 (one lane's two
    keys; the lower wins), 5 a tie between two lanes, 6 a tie that only the head sum creates, 7 dyadic draws with -inf among them.
    Then 8.0, +inf and NaN are planted at every key >= src_len and in every frame >= mel_len."""
    rng = np.random.default_rng(seed)
    src_lens = np.array([L, 0, 1, L + 3, -2, max(1, L // 2), L][:B], dtype=np.int64)
    mel_lens = np.array([max(T - 5, 1), T, T + 4, T, T, 0, -1][:B], dtype=np.int64)
    a = np.empty((B, H, T, L), dtype=np.float32)
    for b in range(B):
        sl = int(min(max(src_lens[b], 0), L))
        for t in range(T):
            kind = (b * T + t) % 8
            row = rng.choice(DYADIC, size=(H, L))
            two = rng.choice(sl, size=2, replace=False) if sl >= 2 else None
            if kind == 1:
                row[:] = rng.choice(DYADIC)
            elif kind == 2:
                row[:] = -np.inf
            elif kind == 3 and sl >= 1:
                row = np.minimum(row, np.float32(0.5))
                row[:, sl - 1] = 1.0
            elif kind == 4 and sl > 64:
                l0 = int(rng.integers(0, sl - 64))
                row = np.minimum(row, np.float32(0.5))
                row[:, l0] = row[:, l0 + 64] = 0.75
            elif kind in (4, 5) and two is not None:
                row = np.minimum(row, np.float32(0.5))
                row[:, two] = 0.75
            elif kind == 6 and two is not None and H >= 2:
                row = np.minimum(row, np.float32(0.125))
                row[0, two], row[1, two] = (0.75, 0.25), (0.25, 0.75)
            elif kind == 7:
                row[rng.random((H, L)) < 0.3] = -np.inf
                row[:] = np.where(np.isinf(row).any(axis=0, keepdims=True), -np.inf, row)   # (a key is -inf in every head or in none)
            a[b, :, t] = row
        ml = int(min(max(mel_lens[b], 0), T))
        a[b, :, :, sl:] = PLANTS[(np.arange(T)[:, None] + np.arange(L - sl)[None, :]) % 3][None]
        a[b, :, ml:, :] = PLANTS[(np.arange(T - ml)[:, None] + np.arange(L)[None, :]) % 3][None]
    return a, src_lens, mel_lens


DURATION_MUTANTS = ("tie_to_highest_key", "later_key_of_a_lane_wins", "src_len_ignored", "mel_len_ignored", "last_valid_key_dropped",
                    "first_head_only", "one_frame_too_many")


def durations_mutant(attn_last, src_lens, mel_lens, mutate):
    """``durations`` with one deliberate mistake of the kind a wave-level argmax can make (64 lanes, lane i walks keys i, i + 64, ...)"""
    assert mutate in DURATION_MUTANTS, mutate
    attn_last = np.asarray(attn_last)
    B, _, T, L = attn_last.shape
    with np.errstate(invalid="ignore"):
        a = attn_last[:, 0] if mutate == "first_head_only" else head_sum(attn_last)
    out = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        sl, ml = int(min(max(src_lens[b], 0), L)), int(min(max(mel_lens[b], 0), T))
        if mutate == "mel_len_ignored":
            ml = T
        if mutate == "one_frame_too_many":
            ml = min(ml + 1, T)
        if sl == 0 or ml == 0:
            continue
        n = L if mutate == "src_len_ignored" else max(sl - 1, 1) if mutate == "last_valid_key_dropped" else sl
        v = a[b, :ml, :n]
        if mutate == "tie_to_highest_key":
            idx = n - 1 - np.argmax(v[:, ::-1], axis=1)
        elif mutate == "later_key_of_a_lane_wins":
            idx = np.empty(ml, dtype=np.int64)
            for t in range(ml):
                best = [max(range(lane, n, 64), key=lambda l: (v[t, l], l)) for lane in range(min(64, n))]   # `>=` inside the lane
                idx[t] = min(best, key=lambda l: (-v[t, l], l))                                             # lowest key across lanes
        else:
            idx = np.argmax(v, axis=1)
        out[b] = np.bincount(idx, minlength=L)
    return out


# ---- the elementwise gate of the cross-attention kernel (tests/test_aligner_host.py proves it both ways) ----------------------
GEMM_EPS = 4e-6   # the project's fp32 GEMM constant (tests/test_fp32_ops_host.py): |fp32 sum - exact| <= GEMM_EPS * sum |a||b|
EXP_EPS = 1e-6    # exp, the division and the row sum of the softmax: a few fp32 roundings on a value <= 1
ABS_FLOOR = 1e-12


def attention_f64(q, kv, src_lens, n_head):
    """float64 evaluation of the fp32 operands: (ctx64 [B,T,d], p64 [B,H,T,L], u [B,H,T], vabs [B,H,L,dk])."""
    q, kv = q.double(), kv.double()
    B, T, d = q.shape
    L = kv.shape[1]
    dk = d // n_head
    key_pad = torch.arange(L)[None, :] >= src_lens[:, None]
    ctx, p = cross_attention_core(q, kv[..., :d], kv[..., d:], key_pad, n_head)
    qh = q.view(B, T, n_head, dk).permute(0, 2, 1, 3).abs()
    kh = kv[..., :d].reshape(B, L, n_head, dk).permute(0, 2, 1, 3).abs()
    mag = torch.matmul(qh, kh.transpose(-1, -2)) / np.power(dk, 0.5)          # sum_c |q_c||k_lc| / sqrt(dk)
    u = mag.masked_fill(key_pad[:, None, None, :], 0).amax(dim=-1)
    vabs = kv[..., d:].reshape(B, L, n_head, dk).permute(0, 2, 1, 3).abs()
    return ctx, p, u, vabs


def attention_gate(q, kv, src_lens, n_head, ctx, attn, skip=()):
    """Worst |error| / bound of the attention probabilities and of the merged-head output against float64, utterances in
    ``skip`` left out (src_len == 0 rows are NaN on both sides):
        |p - p64|     <= p64 (2 GEMM_EPS u + EXP_EPS) + ABS_FLOOR        u = max_l sum_c |q_c||k_lc| / sqrt(dk) over the valid keys:
                         a score is off by <= GEMM_EPS u, the row's log-sum by as much again
        |ctx - ctx64| <= GEMM_EPS sum_l p64 |v_l| + sum_l bound_p[l] |v_l|
    Returns (ratio_p, ratio_ctx); the gate holds when both are <= 1."""
    B, T, d = q.shape
    dk = d // n_head
    ctx64, p64, u, vabs = attention_f64(q, kv, src_lens, n_head)
    keep = [b for b in range(B) if b not in skip]
    bound_p = p64 * (2 * GEMM_EPS * u[..., None] + EXP_EPS) + ABS_FLOOR
    rp = ((attn.double() - p64).abs() / bound_p)[keep]
    bound_c = GEMM_EPS * torch.matmul(p64, vabs) + torch.matmul(bound_p, vabs)      # [B,H,T,dk]
    err_c = (ctx.double() - ctx64).abs().view(B, T, n_head, dk).permute(0, 2, 1, 3)
    rc = (err_c / bound_c)[keep]
    return float(rp.max()), float(rc.max())


def fixture_weights(meta):
    """Both weight families a fixture was generated with, regenerated from its seeds."""
    import smart_nar_fast_tts_amd.workload as wl

    cfg = wl.model_config(meta["config"])
    sd = wl.synth_state_dict(cfg, seed=meta["weight_seed"], frames_per_phoneme=meta["frames_per_phoneme"])
    sd.update(wl.synth_aligner_state_dict(cfg, seed=meta["aligner_seed"]))
    return cfg, sd


def fixture_alignments(name, meta, z, suffix=""):
    """The fixture's per-layer alignments (``suffix`` "" = the reference's fp32, "_f64" = its .double() evaluation)."""
    from tests.util import load_golden

    if meta["split_attn"]:
        return [load_golden(f"{name}_attn{i}")[1]["attn" + suffix] for i in range(meta["n_layer"])]
    return [z[f"attn{i}{suffix}"] for i in range(meta["n_layer"])]
