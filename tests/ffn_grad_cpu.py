"""The reference's PositionwiseFeedForward (transformer/SubLayers.py:62-95) and its backward stated independently on the CPU, for the
tests of csrc/ffngrad.hip.  No test lives here.

``statement``     the sublayer as one torch expression in the reference's own order of operations (transpose, conv1d w_1 with padding
                  (K1 - 1) / 2, relu, conv1d w_2, transpose, the keep-mask times 1 / (1 - p) for dropout, + x, F.layer_norm) in fp32 or
                  float64; torch's autograd differentiates it (``autograd_ref``).
``closed_form``   the backward written out from SAVED tensors (h = relu(w_1 x) [B, S, d_inner], z [B, S, d]) cast to the evaluation
                  dtype: the LayerNorm backward from z, du = dz keep / (1 - p), dW2 = wgrad(du, h), da = dgrad(du, w2), the ReLU gate
                  dh = where(h > 0, da, 0) taken from the saved h, d_b1 = column sums of dh, dW1 = wgrad(dh, x), dx = dgrad(dh, w1) + dz.
                  The convolutions and their gradients are tests/predictor_grad_cpu.py's (zero padding inside each utterance).
                  ``mutate`` names one deliberate mistake (MUTANTS).
``gate``          per gradient tensor and absolute: 2 x max |ref fp32 - ref float64| + one fp32 ulp of max |ref float64| (the rule of
                  tests/attention_grad_cpu.py), both references being ``closed_form`` on the same saved tensors; a NaN / Inf in the
                  result is an infinite share (``shares``).

Why from the saved tensors: a pre-activation within an fp32 rounding of zero can have the other sign in float64, which moves one
element of dh by O(1) and a weight gradient far past any rounding gate.  That is a property of the input, not a kernel error, so a
device gradient is never compared with a float64 autograd run of its own forward.

Weights travel as a dict: w1 [d_inner, d, K1], b1 [d_inner], w2 [d, d_inner, K2], b2, ln_g, ln_b [d]."""
import numpy as np
import torch

from tests import attention_grad_cpu as ac
from tests import predictor_grad_cpu as pc
from tests import util

NAMES = ("w1", "b1", "w2", "b2", "ln_g", "ln_b", "dx")  # order of ns_fg_grads
MUTANTS = ("relu_gate_dropped", "gate_from_preactivation_sign_of_da", "dgrad_without_tap_flip", "wgrad_across_utterances", "residual_dropped",
           "keep_scale_dropped", "db1_before_gate")
LN_EPS = 1e-5


def _w(w, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items() if k in NAMES[:6]}


def statement(x, w, keep=None, p=0.0, dtype=torch.float64, leaves=None):
    """y [B, S, d] and the intermediate tensors, differentiable.  leaves: already-cast tensors to use instead of x and w."""
    x = torch.as_tensor(x).to(dtype) if leaves is None else leaves["x"]
    w = _w(w, dtype) if leaves is None else leaves
    d = x.shape[-1]
    conv = torch.nn.functional.conv1d
    k1, k2 = w["w1"].shape[2], w["w2"].shape[2]
    h = torch.relu(conv(x.transpose(1, 2), w["w1"], w["b1"], padding=(k1 - 1) // 2))
    u = conv(h, w["w2"], w["b2"], padding=(k2 - 1) // 2).transpose(1, 2)
    kf = ac._keep(keep, p, dtype)
    z = (u if kf is None else u * kf) + x
    y = torch.nn.functional.layer_norm(z, (d,), w["ln_g"], w["ln_b"], LN_EPS)
    return dict(y=y, h=h.transpose(1, 2), u=u, z=z)


def autograd_ref(x, w, g, keep=None, p=0.0, dtype=torch.float64):
    """torch's CPU autograd of ``statement``: the seven gradients of (g * y).sum() as numpy arrays (dict by NAMES), and the forward."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in _w(w, dtype).items()}
    leaves["x"] = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    out = statement(None, None, keep, p, dtype, leaves)
    order = [leaves[n] for n in NAMES[:6]] + [leaves["x"]]
    grads = torch.autograd.grad(out["y"], order, grad_outputs=torch.as_tensor(g).to(dtype))
    return {n: t.detach().numpy() for n, t in zip(NAMES, grads)}, {k: v.detach() for k, v in out.items()}


def relu_gate(da, h, mutate=None):
    """dh from the data gradient through w_2 and the SAVED activation: a select, so what da holds where h <= 0 reaches nothing"""
    if mutate == "relu_gate_dropped":
        return da
    if mutate == "gate_from_preactivation_sign_of_da":
        return torch.where(da > 0, da, torch.zeros((), dtype=da.dtype))
    return torch.where(h > 0, da, torch.zeros((), dtype=da.dtype))


def closed_form(x, w, g, saved, keep=None, p=0.0, dtype=torch.float64, mutate=None):
    """The seven gradients (dict by NAMES, numpy arrays of dtype) from saved = (h, z)."""
    assert mutate is None or mutate in MUTANTS, mutate
    x = torch.as_tensor(x).to(dtype)
    B, S, d = x.shape
    w = _w(w, dtype)
    h, z = (torch.as_tensor(np.asarray(a)).to(dtype) for a in saved)
    h, z = h.reshape(B, S, -1), z.reshape(B, S, d)
    K1, K2 = w["w1"].shape[2], w["w2"].shape[2]
    pad1, pad2 = (K1 - 1) // 2, (K2 - 1) // 2
    k = ac._keep(keep, p, dtype)
    if mutate == "keep_scale_dropped" and k is not None:
        k = k * (1.0 - p)
    cross = mutate == "wgrad_across_utterances"
    flip = mutate if mutate == "dgrad_without_tap_flip" else None
    rows = lambda a: a.reshape(B * S, -1)  # noqa: E731
    out = {}
    dz, du, out["ln_g"], out["ln_b"], out["b2"] = ac.row_backward(torch.as_tensor(g).to(dtype), z, w["ln_g"], k)
    out["w2"] = pc.wgrad(du, h, K2, pad2, cross)
    da = pc.dgrad(du, w["w2"], pad2, flip)
    dh = relu_gate(da, h, mutate)
    out["b1"] = rows(da if mutate == "db1_before_gate" else dh).sum(0)
    out["w1"] = pc.wgrad(dh, x, K1, pad1, cross)
    dx = pc.dgrad(dh, w["w1"], pad1, flip)
    out["dx"] = dx if mutate == "residual_dropped" else dx + dz
    out["_dz"], out["_du"], out["_da"], out["_dh"] = dz, du, da, dh
    return {n: v.detach().numpy() for n, v in out.items()}


def gate(ref32, ref64, names=NAMES):
    """The absolute gates (dict by name): twice the reference's own fp32 error plus one fp32 ulp of the largest magnitude."""
    return util.gates(ref32, ref64, names)


def shares(got, ref64, gates, names=NAMES):
    """{name: max |got - ref64| / gate}; inf for a NaN / Inf in got.  A missing (None) gradient is skipped."""
    return util.shares(got, ref64, gates, names)


def seeded_weights(d, d_inner, K1, K2, seed):
    """weights of about the size the checkpoint's are, with non-trivial LayerNorm parameters and biases"""
    rs = np.random.RandomState(seed)
    n = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    return dict(w1=n(d_inner, d, K1, scale=(d * K1) ** -0.5), b1=n(d_inner, scale=0.1), w2=n(d, d_inner, K2, scale=(d_inner * K2) ** -0.5),
                b2=n(d, scale=0.1), ln_g=1 + n(d, scale=0.2), ln_b=n(d, scale=0.1))


def fft_block(x, wa, wf, lens, H, keeps=None, p=0.0, dtype=torch.float64, leaves=None):
    """The reference's FFTBlock (transformer/Layers.py:39-48) as the composite of the two yardsticks: attention_grad_cpu.statement,
    masked_fill at rows t >= lens[b], ``statement``, masked_fill.  leaves: (attention leaves with "x", feed-forward leaves)."""
    ka, kf = keeps if keeps is not None else (None, None)
    a = ac.statement(x, wa, lens, H, ka, p, dtype, None if leaves is None else leaves[0])
    pad = torch.as_tensor(pc.mask_of(lens, a["y"].shape[1]))[..., None]
    mid = a["y"].masked_fill(pad, 0.0)
    f = statement(None if leaves is not None else mid, wf, kf, p, dtype, None if leaves is None else dict(leaves[1], x=mid))
    return f["y"].masked_fill(pad, 0.0)
