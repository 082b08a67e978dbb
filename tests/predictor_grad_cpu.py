"""The reference's VariancePredictor (model/modules.py:233-286) and its backward stated independently on the CPU, for the tests of
csrc/predgrad.hip.  No test lives here.

``statement``     the module as one shape-generic torch expression (F.conv1d on the transposed rows, ReLU, F.layer_norm, the keep-mask
                  times 1 / (1 - p) for dropout, Linear, masked_fill) in fp32 or float64; torch's autograd differentiates it
                  (``autograd_ref``).
``closed_form``   the chained backward written out from SAVED activations (v1 = relu(conv1d_1 x + b1), h1 = dropout_1(layer_norm_1 v1),
                  v2 = relu(conv1d_2 h1 + b2)): the statistics, x_hat and the ReLU gates are recomputed from the saved rows cast to
                  the evaluation dtype, dW is formed from the saved x / h1, dX through the weights.  ``mutate`` names one deliberate
                  mistake (MUTANTS).  The rows are written as the kernels see them — y[t] = sum_j x[t + j - pad] w[j], any 0 <= pad <
                  K, output length S — so the data gradient's pad' = K - 1 - pad can be told from pad (they coincide at the module's
                  own pad = (K - 1) / 2; the mutant test uses K = 5, pad = 1).
``gate``          per gradient tensor and absolute: 2 x max |ref fp32 - ref float64| + one fp32 ulp of max |ref float64| (the rule of
                  tests/optim_cpu.py and tests/lossgrad_cpu.py); an all-zero float64 gradient must be matched exactly, a NaN / Inf in
                  the result is an infinite share (``lossgrad_cpu.shares``).

Weights travel as a dict in the layout of tests/test_predictor_ops_host.pred_weights: w1 [F, Cin, K], b1, g1, be1, w2 [F, F, K], b2, g2,
be2 [F], wlin [F], blin []."""
import numpy as np
import torch

from tests import util

NAMES = ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "wlin", "blin", "dx")  # order of ns_pg_grads
MUTANTS = ("dgrad_without_tap_flip", "dgrad_pad_not_flipped", "wgrad_across_utterances", "mean_dy_xhat_dropped", "relu_gate_dropped",
           "mask_multiplied", "keep_scale_dropped", "d_ln_g_without_xhat", "db_over_valid_rows_only")
LN_EPS = 1e-5


def _w(w, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in w.items() if k in NAMES[:10]}


def _keep(keeps, i, p, dtype):
    """the factor dropout applies at site i: keep / (1 - p), or None without dropout"""
    if keeps is None or p == 0.0:
        return None
    return torch.as_tensor(np.asarray(keeps[i])).to(dtype) * torch.tensor(1.0 / (1.0 - p), dtype=dtype)


def statement(x, w, mask, keeps=None, p=0.0, dtype=torch.float64, leaves=None):
    """pred [B, S] and the activations, differentiable.  leaves: already-cast tensors to use instead of x and w (autograd_ref)."""
    x = torch.as_tensor(x).to(dtype) if leaves is None else leaves["x"]
    w = _w(w, dtype) if leaves is None else leaves
    K = w["w1"].shape[2]
    pad = (K - 1) // 2
    conv = lambda t, wt, b: torch.nn.functional.conv1d(t.transpose(1, 2), wt, b, padding=pad).transpose(1, 2)  # noqa: E731
    ln = lambda t, g, b: torch.nn.functional.layer_norm(t, (t.shape[-1],), g, b, LN_EPS)  # noqa: E731
    v1 = conv(x, w["w1"], w["b1"]).relu()
    h1 = ln(v1, w["g1"], w["be1"])
    k1, k2 = _keep(keeps, 0, p, dtype), _keep(keeps, 1, p, dtype)
    if k1 is not None:
        h1 = h1 * k1
    v2 = conv(h1, w["w2"], w["b2"]).relu()
    h2 = ln(v2, w["g2"], w["be2"])
    if k2 is not None:
        h2 = h2 * k2
    pred = h2 @ w["wlin"] + w["blin"]
    if mask is not None:
        pred = pred.masked_fill(torch.as_tensor(mask).bool(), 0.0)
    return dict(pred=pred, v1=v1, h1=h1, v2=v2, h2=h2)


def autograd_ref(x, w, mask, g, keeps=None, p=0.0, dtype=torch.float64):
    """torch's CPU autograd of ``statement``: the eleven gradients of (g * pred).sum() as numpy arrays (dict by NAMES), and the forward."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in _w(w, dtype).items()}
    leaves["x"] = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    out = statement(None, None, mask, keeps, p, dtype, leaves)
    order = [leaves[n] for n in NAMES[:10]] + [leaves["x"]]
    grads = torch.autograd.grad(out["pred"], order, grad_outputs=torch.as_tensor(g).to(dtype), allow_unused=True)
    return {n: (torch.zeros_like(t) if d is None else d).detach().numpy() for n, t, d in zip(NAMES, order, grads)}, {k: v.detach() for k, v in out.items()}


def rows_conv(x, wt, b, pad, cross=False):
    """y[b, t] = sum_j x[b, t + j - pad] @ wt[:, :, j].T + b, rows outside [0, S) read as zero (cross: the WRONG padding, the flat row
    m + j - pad of the neighbouring utterance)"""
    B0, S0, C = x.shape
    N, _, K = wt.shape
    B, S = (1, B0 * S0) if cross else (B0, S0)
    xp = torch.zeros(B, S + K - 1, C, dtype=x.dtype)
    xp[:, pad:pad + S] = x.reshape(B, S, C)
    y = torch.zeros(B, S, N, dtype=x.dtype)
    for j in range(K):
        y = y + xp[:, j:j + S] @ wt[:, :, j].T
    y = y.reshape(B0, S0, N)
    return y if b is None else y + b


def wgrad(dz, x, K, pad, cross=False):
    """dW[n][c][j] = sum_m dz[m, n] x[m + j - pad, c] with the forward's zero padding"""
    B0, S0, C = x.shape
    N = dz.shape[-1]
    B, S = (1, B0 * S0) if cross else (B0, S0)
    xp = torch.zeros(B, S + K - 1, C, dtype=x.dtype)
    xp[:, pad:pad + S] = x.reshape(B, S, C)
    d = dz.reshape(B * S, N)
    return torch.stack([d.T @ xp[:, j:j + S].reshape(B * S, C) for j in range(K)], dim=-1)


def dgrad(dz, wt, pad, mutate=None):
    """dX[m, c] = sum_j sum_n dz[m - j + pad, n] wt[n][c][j]: the forward's rows_conv on the transposed, tap-flipped weight at K - 1 - pad"""
    K = wt.shape[2]
    wf = wt if mutate == "dgrad_without_tap_flip" else wt.flip(2)
    return rows_conv(dz, wf.transpose(0, 1).contiguous(), None, pad if mutate == "dgrad_pad_not_flipped" else K - 1 - pad)


def row_backward(dy_out, v, g, k, mutate=None, relu=True):
    """One LayerNorm + ReLU site from the gradient of its (dropped-out) output: (dz, d_ln_g, d_ln_b, x_hat).  v: the saved pre-LayerNorm
    rows; k: the dropout factor or None."""
    mean = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    xh = (v - mean) * rstd
    dy = dy_out if k is None else dy_out * k
    d_g = dy.reshape(-1, dy.shape[-1]).sum(0) if mutate == "d_ln_g_without_xhat" else (dy * xh).reshape(-1, dy.shape[-1]).sum(0)
    d_b = dy.reshape(-1, dy.shape[-1]).sum(0)
    dyh = dy * g
    m2 = 0.0 if mutate == "mean_dy_xhat_dropped" else (dyh * xh).mean(-1, keepdim=True)
    dv = rstd * (dyh - dyh.mean(-1, keepdim=True) - xh * m2)
    if relu and mutate != "relu_gate_dropped":
        dv = torch.where(v > 0, dv, torch.zeros((), dtype=v.dtype))
    return dv, d_g, d_b, xh


def closed_form(x, w, mask, g, saved, keeps=None, p=0.0, dtype=torch.float64, mutate=None, pad=None):
    """The eleven gradients (dict by NAMES, numpy arrays of dtype) from saved = (v1, h1, v2) [B, S, F] each."""
    assert mutate is None or mutate in MUTANTS, mutate
    x = torch.as_tensor(x).to(dtype)
    w = _w(w, dtype)
    v1, h1, v2 = (torch.as_tensor(t).to(dtype).reshape(x.shape[0], x.shape[1], -1) for t in saved)
    g = torch.as_tensor(g).to(dtype)
    K = w["w1"].shape[2]
    pad = (K - 1) // 2 if pad is None else pad
    k1 = _keep(keeps, 0, p, dtype) if keeps is not None and p > 0 else None
    k2 = _keep(keeps, 1, p, dtype) if keeps is not None and p > 0 else None
    if mutate == "keep_scale_dropped" and k1 is not None:
        k1, k2 = k1 * (1.0 - p), k2 * (1.0 - p)
    zero = torch.zeros((), dtype=dtype)
    if mask is None:
        dp = g
    elif mutate == "mask_multiplied":
        dp = g * (~torch.as_tensor(mask).bool()).to(dtype)
    else:
        dp = torch.where(torch.as_tensor(mask).bool(), zero, g)
    cross = mutate == "wgrad_across_utterances"
    out = {}
    # tail: Linear(F, 1) then site 2
    dz2, out["g2"], out["be2"], xh2 = row_backward(dp[..., None] * w["wlin"], v2, w["g2"], k2, mutate)
    h2 = xh2 * w["g2"] + w["be2"]
    if k2 is not None:
        h2 = h2 * (_keep(keeps, 1, p, dtype))
    out["wlin"] = (dp[..., None] * h2).reshape(-1, h2.shape[-1]).sum(0)
    out["blin"] = dp.sum()
    valid = torch.ones_like(dp, dtype=torch.bool) if mask is None else ~torch.as_tensor(mask).bool()
    rows = lambda dz: dz[valid] if mutate == "db_over_valid_rows_only" else dz.reshape(-1, dz.shape[-1])  # noqa: E731
    out["b2"] = rows(dz2).sum(0)
    out["w2"] = wgrad(dz2, h1, K, pad, cross)
    dh1 = dgrad(dz2, w["w2"], pad, mutate)
    dz1, out["g1"], out["be1"], _ = row_backward(dh1, v1, w["g1"], k1, mutate)
    out["b1"] = rows(dz1).sum(0)
    out["w1"] = wgrad(dz1, x, K, pad, cross)
    out["dx"] = dgrad(dz1, w["w1"], pad, mutate)
    out["_dh1"] = dh1
    return {k: v.detach().numpy() for k, v in out.items()}


def gate(ref32, ref64):
    """The eleven absolute gates (dict by NAMES): twice the reference's own fp32 error plus one fp32 ulp of the largest magnitude."""
    return util.gates(ref32, ref64, NAMES)


def shares(got, ref64, gates, names=NAMES):
    """{name: max |got - ref64| / gate}; inf for a NaN / Inf in got.  A missing (None) gradient is skipped."""
    return util.shares(got, ref64, gates, names)


def seeded_weights(Cin, F, K, seed):
    """weights of about the size the checkpoint's are, with non-trivial LayerNorm parameters and biases"""
    rs = np.random.RandomState(seed)
    n = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    return dict(w1=n(F, Cin, K, scale=(Cin * K) ** -0.5), b1=n(F, scale=0.1), g1=1 + n(F, scale=0.2), be1=n(F, scale=0.1),
                w2=n(F, F, K, scale=(F * K) ** -0.5), b2=n(F, scale=0.1), g2=1 + n(F, scale=0.2), be2=n(F, scale=0.1),
                wlin=n(F, scale=F ** -0.5), blin=np.float32(0.3))


def mask_of(lens, S):
    return np.arange(S)[None, :] >= np.asarray(lens)[:, None]
