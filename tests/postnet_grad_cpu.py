"""The reference's PostNet (transformer/Layers.py:107-177) with train-mode BatchNorm and its backward stated independently on the CPU,
for the tests of csrc/postnetgrad.hip.  No test lives here.

``autograd_ref``   the module in the torch ops the reference itself runs — F.conv1d on the transposed rows, F.batch_norm (momentum 0.1,
                   eps 1e-5, which also updates the running statistics), tanh, the keep-mask as ``x * keep / (1 - p)`` — in fp32 or
                   float64, differentiated by torch's autograd.  In fp32 it is what the gate is built from.
``forward_form``   the same forward written out: u = rows_conv(h) + b, mu and the BIASED variance over all M = B * T rows, the running
                   statistics by hand, n = gamma (u - mu) rstd + beta, tanh, keep.  Returns y, the saved (u_i, h_i, mu_i, rstd_i) and the
                   buffers after the call.
``closed_form``    the chained backward written out from those saved tensors: dy = dh keep scale (1 - t^2) with t = h / scale, d_beta,
                   d_gamma, dz = gamma rstd (dy - mean dy - xhat mean(dy xhat)) (eval: gamma rstd dy), d_bias, dW from the saved
                   h_{i-1}, dh_{i-1} through the tap-flipped weights.  ``mutate`` names one deliberate mistake (MUTANTS); forward
                   mistakes are made in ``forward_form``, backward mistakes in ``closed_form`` (``evaluate`` runs both).
``gate``           per tensor and absolute, the rule of tests/predictor_grad_cpu.gate: 2 x max |ref fp32 - ref float64| + one fp32 ulp
                   of max |ref float64|; an all-zero float64 tensor must be matched exactly, a NaN / Inf is an infinite share.  The
                   buffers after a forward and y are gated the same way.

Under train-mode BatchNorm a conv bias cancels, so d_b{i} is exactly zero in real arithmetic: the fp32 and the float64 reference
values are both rounding noise, and the gate of that tensor is a small multiple of the reference's own noise.

Weights travel as a dict: per layer i  w{i} [C_out, C_in, K], b{i}, g{i}, be{i}, rm{i}, rv{i} [C_out], nbt{i} [] (int64)."""
import numpy as np
import torch

from tests import util
from tests.predictor_grad_cpu import dgrad, rows_conv, wgrad

BN_EPS, MOMENTUM = 1e-5, 0.1
PARAMS = ("w", "b", "g", "be")  # order of ns_pn_layer_grads
MUTANTS = ("unbiased_var_in_normalisation", "biased_running_var", "momentum_swapped", "mean_dy_dropped", "mean_dy_xhat_dropped",
           "tanh_gate_dropped", "tanh_on_last_layer", "keep_scale_dropped", "stats_over_valid_rows_only", "eps_outside_sqrt",
           "dgrad_without_tap_flip", "wgrad_across_utterances", "eval_backward_with_batch_terms")
FORWARD_MUTANTS = ("unbiased_var_in_normalisation", "biased_running_var", "momentum_swapped", "tanh_on_last_layer", "stats_over_valid_rows_only",
                   "eps_outside_sqrt")


def grad_names(n):
    """the gradients in the order of ns_pn_grads, dx last"""
    return tuple(f"{p}{i}" for i in range(n) for p in PARAMS) + ("dx",)


def buffer_names(n):
    return tuple(f"{p}{i}" for i in range(n) for p in ("rm", "rv"))


def all_names(n):
    return ("y",) + grad_names(n) + buffer_names(n)


def n_layers(w):
    return sum(1 for k in w if k[0] == "w" and k[1:].isdigit())


def _t(v, dtype):
    return torch.as_tensor(np.asarray(v)).to(dtype)


def _keep(keeps, i, p, dtype):
    if keeps is None or p == 0.0:
        return None
    return _t(keeps[i], dtype)


def autograd_ref(x, w, g, keeps=None, p=0.0, training=True, dtype=torch.float64):
    """The reference's own ops under torch's CPU autograd: ({name: numpy} for y, the gradients of (g * y).sum() and the buffers after the
    call, the saved activations).  The weights dict is not modified."""
    n = n_layers(w)
    K = np.asarray(w["w0"]).shape[2]
    leaves = {f"{q}{i}": _t(w[f"{q}{i}"], dtype).clone().requires_grad_(True) for i in range(n) for q in PARAMS}
    leaves["dx"] = _t(x, dtype).clone().requires_grad_(True)
    rm = [_t(w[f"rm{i}"], dtype).clone() for i in range(n)]
    rv = [_t(w[f"rv{i}"], dtype).clone() for i in range(n)]
    h = leaves["dx"].transpose(1, 2)
    us, hs = [], []
    for i in range(n):
        u = torch.nn.functional.conv1d(h, leaves[f"w{i}"], leaves[f"b{i}"], padding=(K - 1) // 2)
        us.append(u.transpose(1, 2).detach())
        v = torch.nn.functional.batch_norm(u, rm[i], rv[i], leaves[f"g{i}"], leaves[f"be{i}"], training, MOMENTUM, BN_EPS)
        if i < n - 1:
            v = torch.tanh(v)
        k = _keep(keeps, i, p, dtype)
        if k is not None:
            v = v * k.transpose(1, 2) / (1.0 - p)
        h = v
        hs.append(h.transpose(1, 2).detach())
    y = h.transpose(1, 2)
    names = grad_names(n)
    grads = torch.autograd.grad(y, [leaves[k] for k in names], grad_outputs=_t(g, dtype), allow_unused=True)
    out = {k: (torch.zeros_like(leaves[k]) if d is None else d).detach().numpy() for k, d in zip(names, grads)}
    out["y"] = y.detach().numpy()
    for i in range(n):
        out[f"rm{i}"], out[f"rv{i}"] = rm[i].numpy(), rv[i].numpy()
    return out, dict(u=us, h=hs)


def forward_form(x, w, keeps=None, p=0.0, training=True, dtype=torch.float64, mutate=None, lens=None):
    """y, saved = (u, h, mu, rstd lists) and the buffers after the call, written out.  lens: only for stats_over_valid_rows_only."""
    n = n_layers(w)
    x = _t(x, dtype)
    B, T, _ = x.shape
    K = np.asarray(w["w0"]).shape[2]
    pad = (K - 1) // 2
    h = x
    us, hs, mus, rstds, out = [], [], [], [], {}
    for i in range(n):
        wt, b, gam, bet = (_t(w[f"{q}{i}"], dtype) for q in PARAMS)
        rm, rv = _t(w[f"rm{i}"], dtype), _t(w[f"rv{i}"], dtype)
        u = rows_conv(h, wt, b, pad)
        if training:
            rows = u.reshape(B * T, -1)
            if mutate == "stats_over_valid_rows_only":
                rows = u[torch.arange(T)[None, :] < torch.as_tensor(np.asarray(lens))[:, None]]
            M = rows.shape[0]
            mu = rows.mean(0)
            var_b = ((rows - mu) ** 2).mean(0)
            var_u = var_b * (M / (M - 1.0))
            var = var_u if mutate == "unbiased_var_in_normalisation" else var_b
            mom = 1.0 - MOMENTUM if mutate == "momentum_swapped" else MOMENTUM
            rm = (1.0 - mom) * rm + mom * mu
            rv = (1.0 - mom) * rv + mom * (var_b if mutate == "biased_running_var" else var_u)
        else:
            mu, var = rm, rv
        rstd = 1.0 / (torch.sqrt(var) + BN_EPS) if mutate == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + BN_EPS)
        v = gam * ((u - mu) * rstd) + bet
        if i < n - 1 or mutate == "tanh_on_last_layer":
            v = torch.tanh(v)
        k = _keep(keeps, i, p, dtype)
        if k is not None:
            v = v * k / (1.0 - p)
        h = v
        us.append(u), hs.append(h), mus.append(mu), rstds.append(rstd)
        out[f"rm{i}"], out[f"rv{i}"] = rm.numpy(), rv.numpy()
    out["y"] = h.numpy()
    return out, dict(u=us, h=hs, mu=mus, rstd=rstds)


def closed_form(x, w, g, saved, keeps=None, p=0.0, training=True, dtype=torch.float64, mutate=None):
    """The 4 n + 1 gradients (dict by grad_names, numpy arrays of dtype) from saved = dict(u, h, mu, rstd) as the forward left them."""
    assert mutate is None or mutate in MUTANTS, mutate
    n = n_layers(w)
    x = _t(x, dtype)
    B, T, _ = x.shape
    K = np.asarray(w["w0"]).shape[2]
    pad = (K - 1) // 2
    scale = 1.0 / (1.0 - p) if (keeps is not None and p > 0) else 1.0
    cross = mutate == "wgrad_across_utterances"
    out = {}
    dh = _t(g, dtype)
    for i in reversed(range(n)):
        wt, gam = _t(w[f"w{i}"], dtype), _t(w[f"g{i}"], dtype)
        u, h = (_t(saved[q][i], dtype).reshape(B, T, -1) for q in ("u", "h"))
        mu, rstd = _t(saved["mu"][i], dtype), _t(saved["rstd"][i], dtype)
        xh = (u - mu) * rstd
        k = _keep(keeps, i, p, dtype)
        dy = dh
        if k is not None:
            dy = dy * k * (1.0 if mutate == "keep_scale_dropped" else scale)
        if (i < n - 1 or mutate == "tanh_on_last_layer") and mutate != "tanh_gate_dropped":
            t = h / scale  # where keep is 0, h is 0 and so is dy
            dy = dy * (1.0 - t * t)
        flat = lambda a: a.reshape(B * T, -1)  # noqa: E731
        out[f"be{i}"] = flat(dy).sum(0)
        out[f"g{i}"] = flat(dy * xh).sum(0)
        if training or mutate == "eval_backward_with_batch_terms":
            m1 = 0.0 if mutate == "mean_dy_dropped" else flat(dy).mean(0)
            m2 = 0.0 if mutate == "mean_dy_xhat_dropped" else flat(dy * xh).mean(0)
            dz = gam * rstd * (dy - m1 - xh * m2)
        else:
            dz = gam * rstd * dy
        out[f"b{i}"] = flat(dz).sum(0)
        h_in = x if i == 0 else _t(saved["h"][i - 1], dtype).reshape(B, T, -1)
        out[f"w{i}"] = wgrad(dz, h_in, K, pad, cross)
        dh = dgrad(dz, wt, pad, mutate)
    out["dx"] = dh
    return {k: v.detach().numpy() for k, v in out.items()}


def evaluate(x, w, g, keeps=None, p=0.0, training=True, dtype=torch.float64, mutate=None, lens=None):
    """forward_form + closed_form: every tensor of all_names(n) as numpy; a forward mutant changes the forward (and what it saves), any
    other the backward."""
    fwd_mut = mutate if mutate in FORWARD_MUTANTS else None
    out, saved = forward_form(x, w, keeps, p, training, dtype, fwd_mut, lens)
    out.update(closed_form(x, w, g, saved, keeps, p, training, dtype, mutate))
    return out


gate = util.gates  # the absolute gates {name: value}, over the tensors both evaluations hold unless names are given
shares = util.shares  # {name: max |got - ref64| / gate}


def classes(sh):
    """the worst share per tensor class: y, w, b, gamma, beta, dx, running_mean, running_var"""
    out = {}
    for k, v in sh.items():
        c = k.rstrip("0123456789")
        c = {"g": "gamma", "be": "beta", "rm": "running_mean", "rv": "running_var"}.get(c, c)
        out[c] = max(out.get(c, 0.0), v)
    return out


def seeded_weights(n_mel, emb, K, n, seed):
    """weights of about the size the checkpoint's are, non-trivial BatchNorm parameters and running statistics"""
    rs = np.random.RandomState(seed)
    nrm = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    chans = [n_mel] + [emb] * (n - 1) + [n_mel]
    w = {}
    for i in range(n):
        ci, co = chans[i], chans[i + 1]
        w[f"w{i}"], w[f"b{i}"] = nrm(co, ci, K, scale=(ci * K) ** -0.5), nrm(co, scale=0.1)
        w[f"g{i}"], w[f"be{i}"] = 1 + nrm(co, scale=0.2), nrm(co, scale=0.1)
        w[f"rm{i}"], w[f"rv{i}"] = nrm(co, scale=0.2), (0.5 + rs.rand(co)).astype(np.float32)
        w[f"nbt{i}"] = np.int64(3 + i)
    return w


def keep_masks(B, T, n_mel, emb, n, p, seed):
    rs = np.random.RandomState(seed)
    chans = [emb] * (n - 1) + [n_mel]
    return [(rs.rand(B, T, c) >= p).astype(np.uint8) for c in chans]
