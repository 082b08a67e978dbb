"""The reference's MelEncoder (transformer/Models.py:103-173: the zeroed first frame, Prenet, the position add, a stack of FFTBlock2) and
the two kernels of csrc/melencgrad.hip stated independently on the CPU, for tests/test_mel_encoder_host.py and
tests/test_gpu_mel_encoder.py.  No test lives here.

``drop_pos``          the forward kernel's bits: fl32(f64(h2) k + f64(pos[m % T])) in numpy float64, one rounding; k = scale where the keep
                      byte is nonzero and 0 where it is zero (``scale_of``: 1 / (1 - p) in fp32, as the C side computes it).
``drop_relu_gate``    the backward kernel's bits: where(keep != 0 and h2 > 0, fl32(f64(g) scale), +0.0), a select; and the exact float64
                      column sums of those fp32 values (``colsum_bound`` is what one rounding of a float64 sum over M rows may differ by:
                      tests/stacks_cpu.embed_grad_bound's form, 0.5 ulp32(|s|) + M 2^-53 sum |dh|).  ``mutate`` names one deliberate
                      mistake (MUTANTS).
``prenet_statement``  the Prenet with what MelEncoder does around it as one torch expression in fp32 or float64.
``prenet_closed_form``  its backward written out from the SAVED activations (h1, h2) cast to the evaluation dtype: a device gradient is
                      judged against this, never against a float64 forward of its own (a pre-activation within a rounding of zero
                      can change sign in float64: tests/ffn_grad_cpu.py states the rule).
``statement``         the whole stack: ``prenet_statement``, then per layer cross_attention_grad_cpu.statement, masked_fill of the padded
                      target rows (tests/stacks_cpu.pad_of), ffn_grad_cpu.statement, masked_fill; the table and the truncation are
                      tests/stacks_cpu.position_table's.  torch's autograd differentiates (g * y).sum() + sum_i (a_i * attn_i).sum()
                      (``autograd_ref``).
``KERNEL_CASES`` / ``kernel_case``   the case table of the two kernels' GPU tests; the host test proves on it that bit-equality rejects
                      the mutants.

Weights travel as dicts: the Prenet's w1 [256, 80], b1, w2 [256, 256], b2; a layer's as cross_attention_grad_cpu's and ffn_grad_cpu's."""
import numpy as np
import torch

from tests import attention_grad_cpu as ac
from tests import cross_attention_grad_cpu as xc
from tests import ffn_grad_cpu as fc
from tests import stacks_cpu as sc

N_MEL, D_PRENET, P_PRENET = 80, 256, 0.2
PRENET_NAMES = ("w1", "b1", "w2", "b2", "dmels")
MUTANTS = ("keep_byte_ignored", "gate_on_h2_ge_0", "multiply_not_select", "frame0_not_zeroed", "pos_indexed_by_m")
ROWS = (0, 1, 127, 255)  # the rows of a [256, *] weight gradient the fixture stores


def scale_of(p):
    """1 / (1 - p) as the C side computes it: in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


# ---- the two kernels ------------------------------------------------------------------------------------------------------------------
def _factor(keep, p, shape):
    k = np.full(shape, np.float64(scale_of(p)))
    return k if keep is None else np.where(np.asarray(keep) != 0, k, 0.0)


def drop_pos(h2, pos, keep, p, T, mutate=None):
    """fp32 [M, F]: the forward kernel's bits from h2 [M, F], pos [>= T, F] (the pos_indexed_by_m mutant needs >= M rows), keep uint8
    [M, F] or None"""
    h2 = np.asarray(h2, dtype=np.float32)
    M = h2.shape[0]
    k = _factor(None if mutate == "keep_byte_ignored" else keep, p, h2.shape)
    rows = np.arange(M) if mutate == "pos_indexed_by_m" else np.arange(M) % T
    with np.errstate(invalid="ignore", over="ignore"):
        return (h2.astype(np.float64) * k + np.asarray(pos, dtype=np.float32)[rows].astype(np.float64)).astype(np.float32)


def drop_relu_gate(g, h2, keep, p, mutate=None):
    """(dh fp32 [M, F], the float64 column sums of dh): the backward kernel's bits"""
    g, h2 = np.asarray(g, dtype=np.float32), np.asarray(h2, dtype=np.float32)
    k = _factor(None if mutate == "keep_byte_ignored" else keep, p, g.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        open_ = (h2 >= 0) if mutate == "gate_on_h2_ge_0" else (h2 > 0)  # (a NaN compares false either way)
        scaled = g.astype(np.float64) * np.float64(scale_of(p))
        if mutate == "multiply_not_select":
            dh = (scaled * ((k != 0) & open_)).astype(np.float32)
        else:
            dh = np.where((k != 0) & open_, scaled, 0.0).astype(np.float32)
        return dh, dh.astype(np.float64).sum(0)


def colsum_bound(dh):
    """float64 [F]: what the device's column sum (float64 partials per 64 rows, added in ascending order, rounded once) may differ from
    the exact sum of the fp32 dh by: the one rounding, plus M float64 adds each wrong by at most 2^-53 of a partial sum <= sum |dh|"""
    a = np.asarray(dh, dtype=np.float64)
    s = a.sum(0)
    return 0.5 * np.spacing(np.abs(s).astype(np.float32)).astype(np.float64) + a.shape[0] * 2.0 ** -53 * np.abs(a).sum(0)


KERNEL_SHAPES = ((1, 1), (3, 33), (2, 70))  # (B, T): one row, a partial 64-row block, past one block
KERNEL_WIDTHS = (256, 512)
KERNEL_CASES = ("plain", "keep", "nan_g", "nan_h2")
# the case on which each kernel-level mutant must change a bit (frame0_not_zeroed is a mutant of the Prenet's backward, not of a kernel)
CATCHER = {"keep_byte_ignored": "keep", "gate_on_h2_ge_0": "plain", "multiply_not_select": "nan_g", "pos_indexed_by_m": "plain"}


def kernel_case(name, B, T, F, seed=0):
    """dict(g, h2 [M, F] fp32, pos [M, F] fp32, keep uint8 [M, F] or None, p) of one case.  h2 is a ReLU output: about half exact
    zeros.  "keep": p = 0.2 with a given mask; "nan_g": that, with NaN and infinities planted in g behind dropped and behind gated
    elements only; "nan_h2": NaN in h2 (it gates like a zero in the backward; the forward's output carries it)."""
    assert name in KERNEL_CASES, name
    rs = np.random.RandomState(3000 + seed + 17 * B + T + F)
    M = B * T
    g = rs.standard_normal((M, F)).astype(np.float32)
    h2 = np.maximum(rs.standard_normal((M, F)), 0.0).astype(np.float32)
    pos = rs.standard_normal((M, F)).astype(np.float32)
    keep, p = None, 0.0
    if name != "plain":
        keep, p = (rs.random_sample((M, F)) >= P_PRENET).astype(np.uint8), P_PRENET
        keep.reshape(-1)[:4] = (1, 0, 1, 0)  # both kinds in the first group, whatever the draw
        h2.reshape(-1)[:4] = (1.5, 2.5, 0.0, 0.0)
    if name == "nan_g":
        closed = (keep == 0) | ~(h2 > 0)
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        idx = np.flatnonzero(closed)
        g.reshape(-1)[idx] = bad[np.arange(idx.size) % 3]
    if name == "nan_h2":
        h2.reshape(-1)[rs.choice(M * F, size=max(1, M * F // 50), replace=False)] = np.nan
    return dict(g=g, h2=h2, pos=pos, keep=keep, p=p)


# ---- the Prenet -----------------------------------------------------------------------------------------------------------------------
def seeded_prenet(seed):
    """weights of about the size torch's initialisation gives, biases included"""
    rs = np.random.RandomState(seed)
    n = lambda *s, scale=1.0: (rs.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    return dict(w1=n(D_PRENET, N_MEL, scale=N_MEL ** -0.5), b1=n(D_PRENET, scale=0.1), w2=n(D_PRENET, D_PRENET, scale=D_PRENET ** -0.5),
                b2=n(D_PRENET, scale=0.1))


def _pw(w, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items() if k in PRENET_NAMES[:4]}


def _kfactor(keep, p, dtype):
    if keep is None or p == 0.0:
        return None
    return (torch.as_tensor(np.asarray(keep)) != 0).to(dtype) * torch.tensor(float(scale_of(p)), dtype=dtype)


def zero_frame0(mels):
    """transformer/Models.py:145-146: a replacement of frame 0, not a shift"""
    return torch.cat([torch.zeros_like(mels[:, :1]), mels[:, 1:]], dim=1)


def prenet_statement(mels, w, pos, keep=None, p=0.0, dtype=torch.float64, leaves=None):
    """y [B, T, 256] = dropout(relu(w_2(relu(w_1(mels with frame 0 zeroed))))) + pos[:T] and the intermediate tensors, differentiable.
    leaves: already-cast tensors (w1, b1, w2, b2, mels) to use instead of mels and w."""
    mels = torch.as_tensor(np.asarray(mels)).to(dtype) if leaves is None else leaves["mels"]
    w = _pw(w, dtype) if leaves is None else leaves
    T = mels.shape[1]
    lin = torch.nn.functional.linear
    xin = zero_frame0(mels)
    h1 = torch.relu(lin(xin, w["w1"], w["b1"]))
    h2 = torch.relu(lin(h1, w["w2"], w["b2"]))
    k = _kfactor(None if keep is None else np.asarray(keep).reshape(h2.shape), p, dtype)
    y = (h2 if k is None else h2 * k) + torch.as_tensor(np.asarray(pos)).to(dtype)[:T][None]
    return dict(y=y, xin=xin, h1=h1, h2=h2)


def prenet_closed_form(mels, w, g, saved, keep=None, p=0.0, dtype=torch.float64, mutate=None):
    """The five gradients (dict by PRENET_NAMES, numpy arrays of dtype) of (g * y).sum() from saved = (h1, h2)."""
    assert mutate is None or mutate in MUTANTS, mutate
    mels = torch.as_tensor(np.asarray(mels)).to(dtype)
    B, T, _ = mels.shape
    w = _pw(w, dtype)
    h1, h2 = (torch.as_tensor(np.asarray(a)).to(dtype).reshape(B * T, -1) for a in saved)
    xin = zero_frame0(mels).reshape(B * T, -1)
    g = torch.as_tensor(np.asarray(g)).to(dtype).reshape(B * T, -1)
    zero = torch.zeros((), dtype=dtype)
    kept = torch.ones_like(h2, dtype=torch.bool) if keep is None or p == 0.0 or mutate == "keep_byte_ignored" else \
        torch.as_tensor(np.asarray(keep)).reshape(h2.shape) != 0
    open2 = (h2 >= 0) if mutate == "gate_on_h2_ge_0" else (h2 > 0)
    scaled = g * torch.tensor(float(scale_of(p)), dtype=dtype)
    dh2 = scaled * (kept & open2).to(dtype) if mutate == "multiply_not_select" else torch.where(kept & open2, scaled, zero)
    out = {"b2": dh2.sum(0), "w2": dh2.T @ h1}
    dh1 = torch.where(h1 > 0, dh2 @ w["w2"], zero)
    out["b1"], out["w1"] = dh1.sum(0), dh1.T @ xin
    dx = (dh1 @ w["w1"]).reshape(B, T, -1)
    out["dmels"] = dx if mutate == "frame0_not_zeroed" else zero_frame0(dx)
    return {n: v.detach().numpy() for n, v in out.items()}


# ---- the stack ------------------------------------------------------------------------------------------------------------------------
def seeded_stack(d, d_inner, kernel, n_layers, seed):
    """dict(prenet, layers [(cross-attention weights, feed-forward weights)])"""
    return dict(prenet=seeded_prenet(seed), layers=[(xc.seeded_weights(d, seed + 10 + 2 * i), fc.seeded_weights(d, d_inner, kernel[0], kernel[1], seed + 11 + 2 * i))
                                                    for i in range(n_layers)])


def leaves_of(w, dtype, src, mels):
    """the differentiable leaves of the stack: dict(prenet, layers [(attention leaves, feed-forward leaves)], src, mels)"""
    leaf = lambda v: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)  # noqa: E731
    return dict(prenet={k: leaf(v) for k, v in _pw(w["prenet"], dtype).items()}, src=leaf(src), mels=leaf(mels),
                layers=[({k: leaf(v) for k, v in ac._w(wa, dtype).items()}, {k: leaf(v) for k, v in fc._w(wf, dtype).items()}) for wa, wf in w["layers"]])


def statement(leaves, src_lens, mel_lens, H, max_seq_len, training=True, keeps=None, prenet_keep=None, p=0.0, p_prenet=0.0, dtype=torch.float64):
    """(y [B, T', d], [attn per layer], the mel lens the layers saw) from ``leaves_of``; T' = min(T, max_seq_len) outside eval() past
    max_seq_len (the reference's else-branch), else T."""
    T, d = leaves["mels"].shape[1], D_PRENET
    table, rows = sc.position_table(T, d, max_seq_len, training)
    mel_lens = [min(int(n), rows) for n in mel_lens]
    x = prenet_statement(None, None, table, prenet_keep, p_prenet, dtype, dict(leaves["prenet"], mels=leaves["mels"][:, :rows]))["y"]
    pad = torch.as_tensor(sc.pad_of(mel_lens, rows))[..., None]
    attns = []
    for i, (la, lf) in enumerate(leaves["layers"]):
        ka, kf = keeps[i] if keeps is not None else (None, None)
        a = xc.statement(None, None, None, src_lens, H, ka, p, dtype, dict(la, tgt=x, src=leaves["src"]))
        mid = a["y"].masked_fill(pad, 0.0)
        x = fc.statement(None, None, kf, p, dtype, dict(lf, x=mid))["y"].masked_fill(pad, 0.0)
        attns.append(a["attn"])
    return x, attns, mel_lens


def grad_names(n_layers):
    names = ["dsrc", "dmels"] + [f"P_{n}" for n in PRENET_NAMES[:4]]
    for i in range(n_layers):
        names += [f"L{i}_a_{n}" for n in ac.NAMES[:10]] + [f"L{i}_f_{n}" for n in fc.NAMES[:6]]
    return names


def autograd_ref(w, src, mels, src_lens, mel_lens, H, g, a, max_seq_len, training=True, keeps=None, prenet_keep=None, p=0.0, p_prenet=0.0,
                 dtype=torch.float64):
    """torch's CPU autograd of ``statement``: (y, [attn], {name: gradient of (g * y).sum() + sum_i (a[i] * attn_i).sum()}) as numpy
    arrays; g and a[i] are cut to the rows the call keeps"""
    leaves = leaves_of(w, dtype, src, mels)
    y, attns, _ = statement(leaves, src_lens, mel_lens, H, max_seq_len, training, keeps, prenet_keep, p, p_prenet, dtype)
    rows = y.shape[1]
    loss = (torch.as_tensor(np.asarray(g)).to(dtype)[:, :rows] * y).sum()
    for ai, attn in zip(a, attns):
        loss = loss + (torch.as_tensor(np.asarray(ai)).to(dtype)[:, :, :rows] * attn).sum()
    tensors = [leaves["src"], leaves["mels"]] + [leaves["prenet"][n] for n in PRENET_NAMES[:4]]
    for la, lf in leaves["layers"]:
        tensors += [la[n] for n in ac.NAMES[:10]] + [lf[n] for n in fc.NAMES[:6]]
    grads = torch.autograd.grad(loss, tensors)
    return (y.detach().numpy(), [t.detach().numpy() for t in attns],
            {n: t.detach().numpy().copy() for n, t in zip(grad_names(len(leaves["layers"])), grads)})


def fixture_inputs(meta, case):
    """(src [B, L, d], mels [B, T, 80], g [B, T, d], [a per layer, [B, H, T, L]]) of one fixture case, regenerated from its seed (the
    fixture stores no input)"""
    c = meta["cases"][case]
    rs = np.random.RandomState(c["seed"])
    B, L, T, d, H = meta["B"], meta["L"], c["T"], meta["d"], meta["H"]
    src = rs.standard_normal((B, L, d)).astype(np.float32)
    mels = (rs.standard_normal((B, T, N_MEL)) * 2.0 - 3.0).astype(np.float32)
    g = rs.standard_normal((B, T, d)).astype(np.float32)
    a = [rs.standard_normal((B, H, T, L)).astype(np.float32) for _ in range(meta["n_layers"])]
    return src, mels, g, a
