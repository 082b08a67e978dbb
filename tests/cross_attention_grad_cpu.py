"""The reference's MultiHeadAttention (transformer/SubLayers.py:8-59) used as FFTBlock2.crs_attn — q = tgt [B, T, d], k = v = src
[B, L, d] — and its backward stated independently on the CPU, for the tests of csrc/xattngrad.hip.  No test lives here.

``statement``     the sublayer as one torch expression in the reference's own order of operations (three F.linear, the head split,
                  bmm, / sqrt(dk), masked_fill(-inf at keys >= lens[b]), softmax, bmm, the head merge, fc, the keep-mask times
                  1 / (1 - p) for dropout, + tgt, F.layer_norm) in fp32 or float64, also returning ``attn`` [B, H, T, L];
                  torch's autograd differentiates ``(g * y).sum() + (a * attn).sum()`` (``autograd_ref``; ``a`` None = the map unused).
``closed_form``   the backward written out from SAVED tensors (q [B, T, d], kv [B, L, 2d], ctx, z [B, T, d], attn [B, H, T, L]) cast
                  to the evaluation dtype: the LayerNorm backward from z, du = dz keep / (1 - p), dctx = du Wfc, dA selected away at
                  masked keys, D = dctx . ctx + sum_l A dA per head, dP = dO V^T + dA, dS = A (dP - D), dQ = c dS K, dK = c dS^T Q,
                  dV = A^T dO, the four weight gradients, the bias column sums, dtgt = dQ Wq + dz, dsrc = dK Wk + dV Wv.
                  ``mutate`` names one deliberate mistake (MUTANTS).
``gate``          tests/attention_grad_cpu.py's: per gradient tensor and absolute, 2 x max |ref fp32 - ref float64| + one fp32 ulp of
                  max |ref float64|; a NaN / Inf in the result is an infinite share (``shares``).

d_bk is zero in exact arithmetic here too (sum_l dS_il = 0 also holds with dA: sum_l A_il (dP_il - D_i) = sum_l A_il dO_i . V_l +
sum_l A_il dA_il - D_i = 0), so its values are rounding noise, as in tests/attention_grad_cpu.py.

Weights travel as a dict: wq, wk, wv, wfc [d, d], bq, bk, bv, bfc, ln_g, ln_b [d]."""
import numpy as np
import torch

from tests import attention_grad_cpu as ac
from tests import util

NAMES = ac.NAMES[:10] + ("dtgt", "dsrc")  # order of ns_xg_grads
MUTANTS = ("AdA_missing_from_D", "dA_missing_from_dP", "dA_read_at_masked_keys", "c_applied_once", "dK_without_transpose",
           "heads_swapped_in_dA", "V_branch_missing_from_dsrc", "residual_missing_from_dtgt", "dbq_over_valid_rows_only",
           "keep_scale_dropped")
LN_EPS = ac.LN_EPS
seeded_weights = ac.seeded_weights


def key_mask(lens, L):
    """[B, 1, L] bool: True at keys l >= lens[b]"""
    return ac.key_mask(lens, L)


def statement(tgt, src, w, lens, H, keep=None, p=0.0, dtype=torch.float64, leaves=None):
    """y [B, T, d], attn [B, H, T, L] and the intermediate tensors, differentiable.  leaves: already-cast tensors to use instead of
    tgt, src and w."""
    tgt = torch.as_tensor(tgt).to(dtype) if leaves is None else leaves["tgt"]
    src = torch.as_tensor(src).to(dtype) if leaves is None else leaves["src"]
    w = ac._w(w, dtype) if leaves is None else leaves
    B, T, d = tgt.shape
    L = src.shape[1]
    dk = d // H
    lin = torch.nn.functional.linear
    q, k, v = lin(tgt, w["wq"], w["bq"]), lin(src, w["wk"], w["bk"]), lin(src, w["wv"], w["bv"])
    hb = lambda t, n: t.view(B, n, H, dk).permute(2, 0, 1, 3).contiguous().view(-1, n, dk)  # noqa: E731  (n*b) x len x dk, as the reference
    attn = torch.bmm(hb(q, T), hb(k, L).transpose(1, 2)) / np.power(dk, 0.5)
    mask = key_mask(lens, L).expand(B, T, L).repeat(H, 1, 1)
    attn = attn.masked_fill(mask, -np.inf)
    attn = torch.softmax(attn, dim=2)
    ctx = torch.bmm(attn, hb(v, L)).view(H, B, T, dk).permute(1, 2, 0, 3).contiguous().view(B, T, d)
    u = lin(ctx, w["wfc"], w["bfc"])
    kf = ac._keep(keep, p, dtype)
    z = (u if kf is None else u * kf) + tgt
    y = torch.nn.functional.layer_norm(z, (d,), w["ln_g"], w["ln_b"], LN_EPS)
    return dict(y=y, q=q, kv=torch.cat([k, v], dim=-1), ctx=ctx, z=z, attn=attn.view(H, B, T, L).transpose(0, 1))


def autograd_ref(tgt, src, w, lens, H, g, a=None, keep=None, p=0.0, dtype=torch.float64):
    """torch's CPU autograd of ``statement``: the twelve gradients of (g * y).sum() + (a * attn).sum() as numpy arrays (dict by NAMES),
    and the forward."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in ac._w(w, dtype).items()}
    leaves["tgt"] = torch.as_tensor(tgt).to(dtype).clone().requires_grad_(True)
    leaves["src"] = torch.as_tensor(src).to(dtype).clone().requires_grad_(True)
    out = statement(None, None, None, lens, H, keep, p, dtype, leaves)
    order = [leaves[n] for n in NAMES[:10]] + [leaves["tgt"], leaves["src"]]
    loss = (torch.as_tensor(g).to(dtype) * out["y"]).sum()
    if a is not None:
        loss = loss + (torch.as_tensor(a).to(dtype) * out["attn"]).sum()
    grads = torch.autograd.grad(loss, order)
    return {n: d.detach().numpy() for n, d in zip(NAMES, grads)}, {k: v.detach() for k, v in out.items()}


def attention_backward(q, kv, ctx, attn, dctx, dA, lens, H, dtype=torch.float64, mutate=None):
    """(dq [B, T, d], dkv [B, L, 2d]) from the saved tensors, dctx [B, T, d] and dA [B, H, T, L] or None"""
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    q, kv, ctx, attn, dctx = t(q), t(kv), t(ctx), t(attn), t(dctx)
    B, T, d = q.shape
    L = kv.shape[1]
    c = torch.tensor((d // H) ** -0.5, dtype=dtype)
    Q, K, V = ac.split_heads(q, H), ac.split_heads(kv[..., :d], H), ac.split_heads(kv[..., d:], H)
    dO, O = ac.split_heads(dctx, H), ac.split_heads(ctx, H)
    masked = key_mask(lens, L)[:, None]  # [B, 1, 1, L]
    zero = torch.zeros((), dtype=dtype)
    A = torch.where(masked, zero, attn)
    G = torch.zeros_like(A) if dA is None else t(dA)
    if mutate == "heads_swapped_in_dA":
        G = G.flip(1)
    if mutate != "dA_read_at_masked_keys":
        G = torch.where(masked, zero, G)
    D = (dO * O).sum(-1, keepdim=True)
    if mutate != "AdA_missing_from_D":
        D = D + (A * G).sum(-1, keepdim=True)
    dP = dO @ V.transpose(-1, -2)
    if mutate != "dA_missing_from_dP":
        dP = dP + G
    dS = A * (dP - D)
    dV = A.transpose(-1, -2) @ dO
    dQ = c * (dS @ K)
    dK = (dS.reshape(B, H, L, T) if mutate == "dK_without_transpose" else dS.transpose(-1, -2)) @ Q  # (a view in the transpose's place)
    if mutate != "c_applied_once":
        dK = c * dK
    return ac.merge_heads(dQ), torch.cat([ac.merge_heads(dK), ac.merge_heads(dV)], dim=-1)


def closed_form(tgt, src, w, lens, H, g, a, saved, keep=None, p=0.0, dtype=torch.float64, mutate=None):
    """The twelve gradients (dict by NAMES, numpy arrays of dtype) from saved = (q, kv, ctx, z, attn)."""
    assert mutate is None or mutate in MUTANTS, mutate
    tgt, src = torch.as_tensor(tgt).to(dtype), torch.as_tensor(src).to(dtype)
    B, T, d = tgt.shape
    L = src.shape[1]
    w = ac._w(w, dtype)
    q, kv, ctx, z, attn = (torch.as_tensor(np.asarray(x)).to(dtype) for x in saved)
    q, kv, ctx, z, attn = q.reshape(B, T, d), kv.reshape(B, L, 2 * d), ctx.reshape(B, T, d), z.reshape(B, T, d), attn.reshape(B, H, T, L)
    k = ac._keep(keep, p, dtype)
    if mutate == "keep_scale_dropped" and k is not None:
        k = k * (1.0 - p)
    out = {}
    dz, du, out["ln_g"], out["ln_b"], out["bfc"] = ac.row_backward(torch.as_tensor(g).to(dtype), z, w["ln_g"], k)
    rows = lambda x: x.reshape(-1, x.shape[-1])  # noqa: E731
    out["wfc"] = rows(du).T @ rows(ctx)
    dctx = du @ w["wfc"]
    dq, dkv = attention_backward(q, kv, ctx, attn, dctx, a, lens, H, dtype, mutate)
    dk_, dv_ = dkv[..., :d], dkv[..., d:]
    out["wq"], out["wk"], out["wv"] = rows(dq).T @ rows(tgt), rows(dk_).T @ rows(src), rows(dv_).T @ rows(src)
    # (the mutant's "valid" rows: the first half of the frames, as if the rest were padding)
    out["bq"] = dq[:, :max(1, T // 2)].reshape(-1, d).sum(0) if mutate == "dbq_over_valid_rows_only" else rows(dq).sum(0)
    out["bk"], out["bv"] = rows(dk_).sum(0), rows(dv_).sum(0)
    out["dtgt"] = dq @ w["wq"] if mutate == "residual_missing_from_dtgt" else dq @ w["wq"] + dz
    out["dsrc"] = dk_ @ w["wk"] if mutate == "V_branch_missing_from_dsrc" else dk_ @ w["wk"] + dv_ @ w["wv"]
    out["_dq"], out["_dkv"], out["_dz"], out["_du"], out["_dctx"] = dq, dkv, dz, du, dctx
    return {n: v.detach().numpy() for n, v in out.items()}


def gate(ref32, ref64, names=NAMES):
    return util.gates(ref32, ref64, names)


def shares(got, ref64, gates, names=NAMES):
    return util.shares(got, ref64, gates, names)


def loss_shaped_dA(B, H, T, L, ilens, olens, seed, heads=(0,)):
    """A map gradient shaped like ns_lossg_backward's d_attn: nonzero on the given heads inside t < olens[b], l < ilens[b], +0.0
    elsewhere."""
    rs = np.random.RandomState(seed)
    a = np.zeros((B, H, T, L), dtype=np.float32)
    for b in range(B):
        for h in heads:
            a[b, h, :olens[b], :ilens[b]] = (rs.standard_normal((olens[b], ilens[b])) / (olens[b] * B)).astype(np.float32)
    return a
