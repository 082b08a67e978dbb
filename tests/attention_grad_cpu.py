"""The reference's MultiHeadAttention (transformer/SubLayers.py:8-59) with q = k = v = x and its backward stated independently on the
CPU, for the tests of csrc/attngrad.hip.  No test lives here.

``statement``     the sublayer as one torch expression in the reference's own order of operations (three F.linear, the head split,
                  bmm, / sqrt(dk), masked_fill(-inf at keys >= lens[b]), softmax, bmm, the head merge, fc, the keep-mask times
                  1 / (1 - p) for dropout, + x, F.layer_norm) in fp32 or float64; torch's autograd differentiates it (``autograd_ref``).
``closed_form``   the backward written out from SAVED tensors (qkv [B, S, 3d], ctx, z [B, S, d], lse [B, H, S]) cast to the evaluation
                  dtype: the LayerNorm backward from z, du = dz keep / (1 - p), dctx = du Wfc, D = dctx . ctx per head,
                  P = exp(c S - lse) with exact zeros at masked keys, dV = P^T dO, dP = dO V^T, dS = P (dP - D), dQ = c dS K,
                  dK = c dS^T Q, the four weight gradients, the bias column sums, dx = dqkv [Wq; Wk; Wv] + dz.  ``mutate`` names one
                  deliberate mistake (MUTANTS).
``gate``          per gradient tensor and absolute: 2 x max |ref fp32 - ref float64| + one fp32 ulp of max |ref float64| (the rule of
                  tests/predictor_grad_cpu.py); a NaN / Inf in the result is an infinite share (``shares``).

Weights travel as a dict: wq, wk, wv, wfc [d, d], bq, bk, bv, bfc, ln_g, ln_b [d]."""
import numpy as np
import torch

from tests import util
from tests import predictor_grad_cpu as pc

NAMES = ("wq", "bq", "wk", "bk", "wv", "bv", "wfc", "bfc", "ln_g", "ln_b", "dx")  # order of ns_ag_grads
MUTANTS = ("D_dropped", "c_applied_once", "dK_without_transpose", "masked_keys_exp0", "lse_without_max", "residual_dropped",
           "keep_scale_dropped", "db_over_valid_rows_only", "heads_swapped")
LN_EPS = 1e-5


def _w(w, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items() if k in NAMES[:10]}


def _keep(keep, p, dtype):
    if keep is None or p == 0.0:
        return None
    return torch.as_tensor(np.asarray(keep)).to(dtype) * torch.tensor(1.0 / (1.0 - p), dtype=dtype)


def key_mask(lens, S):
    """[B, 1, S] bool: True at keys j >= lens[b]"""
    return torch.as_tensor(np.arange(S)[None, None, :] >= np.asarray(lens)[:, None, None])


def split_heads(t, H):
    """[B, S, d] -> [B, H, S, dk]"""
    B, S, d = t.shape
    return t.reshape(B, S, H, d // H).permute(0, 2, 1, 3)


def merge_heads(t):
    """[B, H, S, dk] -> [B, S, d]"""
    B, H, S, dk = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, S, H * dk)


def statement(x, w, lens, H, keep=None, p=0.0, dtype=torch.float64, leaves=None):
    """y [B, S, d] and the intermediate tensors, differentiable.  leaves: already-cast tensors to use instead of x and w."""
    x = torch.as_tensor(x).to(dtype) if leaves is None else leaves["x"]
    w = _w(w, dtype) if leaves is None else leaves
    B, S, d = x.shape
    dk = d // H
    lin = torch.nn.functional.linear
    q, k, v = lin(x, w["wq"], w["bq"]), lin(x, w["wk"], w["bk"]), lin(x, w["wv"], w["bv"])
    hb = lambda t: t.view(B, S, H, dk).permute(2, 0, 1, 3).contiguous().view(-1, S, dk)  # noqa: E731  (n*b) x S x dk, as the reference
    attn = torch.bmm(hb(q), hb(k).transpose(1, 2)) / np.power(dk, 0.5)
    mask = key_mask(lens, S).expand(B, S, S).repeat(H, 1, 1)
    attn = attn.masked_fill(mask, -np.inf)
    lse = torch.logsumexp(attn, dim=2).view(H, B, S).permute(1, 0, 2)
    attn = torch.softmax(attn, dim=2)
    ctx = torch.bmm(attn, hb(v)).view(H, B, S, dk).permute(1, 2, 0, 3).contiguous().view(B, S, d)
    u = lin(ctx, w["wfc"], w["bfc"])
    kf = _keep(keep, p, dtype)
    z = (u if kf is None else u * kf) + x
    y = torch.nn.functional.layer_norm(z, (d,), w["ln_g"], w["ln_b"], LN_EPS)
    return dict(y=y, qkv=torch.cat([q, k, v], dim=-1), ctx=ctx, z=z, lse=lse, attn=attn.view(H, B, S, S).transpose(0, 1))


def autograd_ref(x, w, lens, H, g, keep=None, p=0.0, dtype=torch.float64):
    """torch's CPU autograd of ``statement``: the eleven gradients of (g * y).sum() as numpy arrays (dict by NAMES), and the forward."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in _w(w, dtype).items()}
    leaves["x"] = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    out = statement(None, None, lens, H, keep, p, dtype, leaves)
    order = [leaves[n] for n in NAMES[:10]] + [leaves["x"]]
    grads = torch.autograd.grad(out["y"], order, grad_outputs=torch.as_tensor(g).to(dtype))
    return {n: d.detach().numpy() for n, d in zip(NAMES, grads)}, {k: v.detach() for k, v in out.items()}


def lse_of(qkv, lens, H, dtype=torch.float64, with_max=True):
    """lse [B, H, S] from qkv [B, S, 3d]; with_max=False is the naive log(sum(exp)) that overflows"""
    qkv = torch.as_tensor(qkv).to(dtype)
    B, S, d3 = qkv.shape
    d = d3 // 3
    Q, K = split_heads(qkv[..., :d], H), split_heads(qkv[..., d:2 * d], H)
    s = (Q @ K.transpose(-1, -2)) * torch.tensor((d // H) ** -0.5, dtype=dtype)
    s = s.masked_fill(key_mask(lens, S)[:, None], -np.inf)
    if with_max:
        return torch.logsumexp(s, dim=-1)
    return torch.log(torch.exp(s).sum(-1))


def attention_backward(qkv, ctx, lse, dctx, lens, H, dtype=torch.float64, mutate=None):
    """dqkv [B, S, 3d] from the saved tensors and dctx [B, S, d]"""
    t = lambda a: torch.as_tensor(a).to(dtype)  # noqa: E731
    qkv, ctx, lse, dctx = t(qkv), t(ctx), t(lse), t(dctx)
    B, S, d3 = qkv.shape
    d = d3 // 3
    c = torch.tensor((d // H) ** -0.5, dtype=dtype)
    Q, K, V = (split_heads(qkv[..., i * d:(i + 1) * d], H) for i in range(3))
    dO, O = split_heads(dctx, H), split_heads(ctx, H)
    D = (dO * O).sum(-1, keepdim=True)
    if mutate == "D_dropped":
        D = torch.zeros_like(D)
    masked = key_mask(lens, S)[:, None]  # [B, 1, 1, S]
    s = (Q @ K.transpose(-1, -2)) * c
    P = torch.exp(s - lse[..., None])
    P = torch.where(masked, torch.ones((), dtype=dtype) if mutate == "masked_keys_exp0" else torch.zeros((), dtype=dtype), P)
    dV = P.transpose(-1, -2) @ dO
    dP = dO @ V.transpose(-1, -2)
    dS = P * (dP - D)
    dQ = c * (dS @ K)
    dK = (dS if mutate == "dK_without_transpose" else dS.transpose(-1, -2)) @ Q
    if mutate != "c_applied_once":
        dK = c * dK
    if mutate == "heads_swapped":
        dQ, dK, dV = dQ.flip(1), dK.flip(1), dV.flip(1)
    return torch.cat([merge_heads(dQ), merge_heads(dK), merge_heads(dV)], dim=-1)


def row_backward(dy, z, ln_g, k):
    """(dz, du, d_ln_g, d_ln_b, d_bfc) of y = LayerNorm(z), z = u k + x"""
    dz, d_g, d_b, _ = pc.row_backward(dy, z, ln_g, None, relu=False)
    du = dz if k is None else dz * k
    return dz, du, d_g, d_b, du.reshape(-1, du.shape[-1]).sum(0)


def closed_form(x, w, lens, H, g, saved, keep=None, p=0.0, dtype=torch.float64, mutate=None):
    """The eleven gradients (dict by NAMES, numpy arrays of dtype) from saved = (qkv, ctx, z, lse)."""
    assert mutate is None or mutate in MUTANTS, mutate
    x = torch.as_tensor(x).to(dtype)
    B, S, d = x.shape
    w = _w(w, dtype)
    qkv, ctx, z, lse = (torch.as_tensor(np.asarray(a)).to(dtype) for a in saved)
    qkv, ctx, z, lse = qkv.reshape(B, S, 3 * d), ctx.reshape(B, S, d), z.reshape(B, S, d), lse.reshape(B, H, S)
    if mutate == "lse_without_max":
        lse = lse_of(qkv.to(torch.float32), lens, H, torch.float32, with_max=False).to(dtype)
    k = _keep(keep, p, dtype)
    if mutate == "keep_scale_dropped" and k is not None:
        k = k * (1.0 - p)
    out = {}
    dz, du, out["ln_g"], out["ln_b"], out["bfc"] = row_backward(torch.as_tensor(g).to(dtype), z, w["ln_g"], k)
    rows = lambda a: a.reshape(B * S, -1)  # noqa: E731
    out["wfc"] = rows(du).T @ rows(ctx)
    dctx = du @ w["wfc"]
    dqkv = attention_backward(qkv, ctx, lse, dctx, lens, H, dtype, mutate)
    valid = ~key_mask(lens, S)[:, 0, :]  # [B, S] rows t < lens[b]
    for i, n in enumerate("qkv"):
        third = dqkv[..., i * d:(i + 1) * d]
        out["w" + n] = rows(third).T @ rows(x)
        out["b" + n] = third[valid].sum(0) if mutate == "db_over_valid_rows_only" else rows(third).sum(0)
    wqkv = torch.cat([w["wq"], w["wk"], w["wv"]], dim=0)
    out["dx"] = dqkv @ wqkv if mutate == "residual_dropped" else dqkv @ wqkv + dz
    out["_dqkv"], out["_dz"], out["_du"], out["_dctx"] = dqkv, dz, du, dctx
    return {n: v.detach().numpy() for n, v in out.items()}


def gate(ref32, ref64, names=NAMES):
    """The absolute gates (dict by name): twice the reference's own fp32 error plus one fp32 ulp of the largest magnitude."""
    return util.gates(ref32, ref64, names)


def shares(got, ref64, gates, names=NAMES):
    """{name: max |got - ref64| / gate}; inf for a NaN / Inf in got.  A missing (None) gradient is skipped."""
    return util.shares(got, ref64, gates, names)


def seeded_weights(d, seed):
    """weights of about the size the checkpoint's are, with non-trivial LayerNorm parameters and biases"""
    rs = np.random.RandomState(seed)
    n = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    return dict(wq=n(d, d, scale=d ** -0.5), bq=n(d, scale=0.1), wk=n(d, d, scale=d ** -0.5), bk=n(d, scale=0.1), wv=n(d, d, scale=d ** -0.5),
                bv=n(d, scale=0.1), wfc=n(d, d, scale=d ** -0.5), bfc=n(d, scale=0.1), ln_g=1 + n(d, scale=0.2), ln_b=n(d, scale=0.1))
