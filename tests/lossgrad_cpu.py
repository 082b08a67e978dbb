"""The gradients of FastSpeech2Loss (model/loss.py:149-250) stated independently on the CPU, for the tests of csrc/lossgrad.hip:

``closed_form``   the nine gradients of ``(g * seven).sum()`` written out per element in float64 — a coefficient times sign(x - y),
                  2 (x - y) or W — never through autograd of the ``where`` statement of loss_cpu._parts, whose ``abs`` backward
                  turns a NaN behind a mask into ``0 * NaN``.  ``mutate`` names one deliberate mistake (MUTANTS).
``autograd_ref``  the reference's own statement — ``masked_select`` then L1Loss / MSELoss, W zero outside the selected region — with
                  torch's CPU autograd, in fp32 or float64: the yardstick of the gate on the seeded cases.
``gate``          per gradient tensor and absolute: 2 x max |ref fp32 - ref float64| + one fp32 ulp of max |ref float64| ("twice the
                  reference's own fp32 error plus one ulp", as tests/optim_cpu.py); the four maps add 4 * 2^-24 * ALPHA * |g[0] + g[6]| /
                  n_attn for the device's expf against the host's in W = 1 - exp(.), which the reference's own error cannot show because
                  it builds W in fp32 in both runs.

The guided-attention weights W and the duration target log(d.float() + 1) are fp32 at every dtype, as in the reference."""
import numpy as np
import torch

from tests import loss_cpu as lc
from tests.util import gate_value, share_of, ulp32  # noqa: F401  (ulp32: callers use lg.ulp32)

NAMES = ("mel", "postnet", "pitch", "energy", "log_d", "attn0", "attn1", "attn2", "attn3")
MUTANTS = ("mean_over_all_elements", "factor_2_dropped", "g0_only", "W_on_every_head", "alpha_dropped", "log_without_plus_one",
           "mask_off_by_one", "multiply_by_mask")
G_TOTAL = np.array([1, 0, 0, 0, 0, 0, 0], dtype=np.float32)  # total.backward()


def nine(predictions):
    """The nine differentiated tensors of a prediction tuple in the order of NAMES."""
    return list(predictions[:5]) + list(predictions[10][:4])


def seeded_g(name, level):
    """A random grad_output for one of loss_cpu.CASES: every one of the seven takes part, with both signs."""
    rng = np.random.default_rng(100 + 2 * list(lc.CASES).index(name) + lc.LEVELS.index(level))
    return (rng.standard_normal(7) + np.array([1.0, 0, 0, 0, 0, 0, 0])).astype(np.float32)


def _region(src_lens, mel_lens, L, T):
    ilen, olen = lc._clamped(src_lens, L), lc._clamped(mel_lens, T)
    region = (torch.arange(T)[None, :, None] < olen[:, None, None]) & (torch.arange(L)[None, None, :] < ilen[:, None, None])
    gx = torch.arange(T).float()[None, :, None] / olen.float()[:, None, None]
    gy = torch.arange(L).float()[None, None, :] / ilen.float()[:, None, None]
    W = 1.0 - torch.exp(-((gy - gx) ** 2) / (2 * (lc.SIGMA ** 2)))  # fp32 (model/loss.py:104-108)
    return ilen, olen, region, W


def closed_form(inputs, predictions, pitch_level, energy_level, g, mutate=None):
    """The nine gradients as float64 numpy arrays, shaped like the predictions."""
    assert mutate is None or mutate in MUTANTS, mutate
    src_lens, _, mel_targets, mel_lens, _, p_tgt, e_tgt = inputs[4:11]
    mel, post, p_pred, e_pred, log_d, _, src_masks, mel_masks, _, _, attn, d_tgt = predictions
    B, T, n_mel = mel.shape
    H, L = attn[0].shape[1], log_d.shape[1]
    f = lambda t: torch.as_tensor(t).double()  # noqa: E731
    g = [float(v) for v in np.asarray(g, dtype=np.float64)]
    keep_t, keep_l = ~torch.as_tensor(mel_masks), ~torch.as_tensor(src_masks)
    ilen, olen, region, W = _region(src_lens, mel_lens, L, T)
    if mutate == "mask_off_by_one":
        keep_t = torch.arange(T)[None] <= (T - torch.as_tensor(mel_masks).sum(1))[:, None]
        keep_l = torch.arange(L)[None] <= ilen[:, None]
        ilen, olen, region, W = _region((ilen + 1).clamp(max=L), (olen + 1).clamp(max=T), L, T)
    w = lambda i: g[0] if mutate == "g0_only" else g[0] + g[i]  # noqa: E731
    two = 1.0 if mutate == "factor_2_dropped" else 2.0
    zero = torch.zeros((), dtype=torch.float64)

    def select(term, keep, c_of_count):
        """where(keep, c * term, +0) with c = c_of_count(selected count); the coefficient of an empty selection is never applied."""
        k = keep.expand_as(term)
        n = int(k.sum()) if mutate != "mean_over_all_elements" else term.numel()
        if mutate == "multiply_by_mask":
            return (c_of_count(n) if n else 0.0) * term * k
        if not k.any():
            return torch.zeros_like(term)
        return torch.where(k, c_of_count(n) * term, zero)

    out = []
    tgt = f(mel_targets)[:, :T]
    for i, x in ((1, f(mel)), (2, f(post))):
        out.append(select(torch.sign(x - tgt), keep_t[:, :, None], lambda n, i=i: w(i) / n))  # (n counts the n_mel columns)
    for i, x, y, level in ((3, f(p_pred), f(p_tgt), pitch_level), (4, f(e_pred), f(e_tgt), energy_level)):
        out.append(select(x - y, keep_t if level == "frame_level" else keep_l, lambda n, i=i: two * w(i) / n))
    d = torch.as_tensor(d_tgt)[:, :L].float()
    log_t = torch.log(d if mutate == "log_without_plus_one" else d + 1).double()  # fp32 log, as the reference's .float()
    out.append(select(f(log_d) - log_t, keep_l, lambda n: two * w(5) / n))
    alpha = 1.0 if mutate == "alpha_dropped" else lc.ALPHA
    n_attn = int(region.sum()) if mutate != "mean_over_all_elements" else B * T * L
    head0 = torch.zeros(B, T, L, dtype=torch.float64)
    if n_attn:
        c = alpha * w(6) / n_attn
        head0 = c * W.double() * region if mutate == "multiply_by_mask" else torch.where(region, c * W.double(), zero)
    m = torch.zeros(B, H, T, L, dtype=torch.float64)
    m[:, :] = head0[:, None] if mutate == "W_on_every_head" else 0.0
    m[:, 0] = head0
    out += [m.clone() for _ in range(4)]
    return [o.numpy() for o in out]


def statement(inputs, predictions, pitch_level, energy_level):
    """The reference's forward (model/loss.py:164-250) as one torch statement on the tensors' device: masked_select, then L1Loss / MSELoss,
    and W * attn[k][:, 0] with W zero outside {t < olen, l < ilen} (``_make_guided_attention_masks`` fills a zero tensor).  Differs from
    the reference only where it must: lengths are clamped to the tensors' shapes (the DEVIATION of loss.FastSpeech2Loss), and an
    utterance with a zero length contributes no cell.  Returns the seven values stacked, differentiable."""
    src_lens, _, mel_targets, mel_lens, _, p_tgt, e_tgt = inputs[4:11]
    mel, post, p_pred, e_pred, log_d, _, src_masks, mel_masks, _, _, attn, d_tgt = predictions
    dev = mel.device
    T, L = mel.shape[1], log_d.shape[1]
    keep_t, keep_l = ~mel_masks, ~src_masks
    log_t = torch.log(d_tgt.float() + 1)[:, :L].masked_select(keep_l)
    by = lambda level: keep_t if level == "frame_level" else keep_l  # noqa: E731
    l1, l2 = torch.nn.functional.l1_loss, torch.nn.functional.mse_loss
    tgt = mel_targets[:, :T].masked_select(keep_t[:, :, None])
    v_mel = l1(mel.masked_select(keep_t[:, :, None]), tgt)
    v_post = l1(post.masked_select(keep_t[:, :, None]), tgt)
    v_pitch = l2(p_pred.masked_select(by(pitch_level)), p_tgt.masked_select(by(pitch_level)))
    v_energy = l2(e_pred.masked_select(by(energy_level)), e_tgt.masked_select(by(energy_level)))
    v_dur = l2(log_d.masked_select(keep_l), log_t.to(log_d.dtype))
    ar = lambda n: torch.arange(n, device=dev)  # noqa: E731
    ilen, olen = lc._clamped(src_lens, L, dev), lc._clamped(mel_lens, T, dev)
    region = (ar(T)[None, :, None] < olen[:, None, None]) & (ar(L)[None, None, :] < ilen[:, None, None])
    gx = ar(T).float()[None, :, None] / olen.float()[:, None, None]
    gy = ar(L).float()[None, None, :] / ilen.float()[:, None, None]
    W = torch.where(region, 1.0 - torch.exp(-((gy - gx) ** 2) / (2 * (lc.SIGMA ** 2))), torch.zeros((), device=dev))
    v_attn = 0
    for k in range(4):
        v_attn = v_attn + lc.ALPHA * torch.mean((W * attn[k][:, 0]).masked_select(region))
    total = v_mel + v_post + v_dur + v_pitch + v_energy + v_attn
    return torch.stack([total, v_mel, v_post, v_pitch, v_energy, v_dur, v_attn])


def autograd_ref(inputs, predictions, pitch_level, energy_level, g, dtype):
    """torch's CPU autograd of ``statement`` in ``dtype``: the nine gradients as numpy arrays of that dtype."""
    cast = lambda t: t.detach().to(dtype).clone().requires_grad_(True)  # noqa: E731
    leaves = [cast(t) for t in nine(predictions)]
    tcast = lambda t: torch.as_tensor(t).to(dtype)  # noqa: E731
    i2 = tuple(inputs[:6]) + (tcast(inputs[6]),) + tuple(inputs[7:9]) + (tcast(inputs[9]), tcast(inputs[10]))
    p2 = tuple(leaves[:5]) + tuple(predictions[5:10]) + (leaves[5:], predictions[11])
    seven = statement(i2, p2, pitch_level, energy_level)
    grads = torch.autograd.grad(seven, leaves, grad_outputs=torch.as_tensor(np.asarray(g)).to(dtype), allow_unused=True)
    return [(torch.zeros_like(x) if d is None else d).numpy() for x, d in zip(leaves, grads)]


def n_attn_of(inputs, predictions):
    T, L = predictions[0].shape[1], predictions[4].shape[1]
    return int((lc._clamped(inputs[4], L) * lc._clamped(inputs[7], T)).sum())


def gate(ref32, ref64, g, n_attn):
    """The nine absolute gates.  An all-zero float64 gradient has a gate of one denormal: it must be matched exactly."""
    out = []
    for i, (a, w) in enumerate(zip(ref32, ref64)):
        v = gate_value(a, w)
        if i >= 5 and n_attn > 0:
            v += 4.0 * 2.0 ** -24 * lc.ALPHA * abs(float(g[0]) + float(g[6])) / n_attn
        out.append(v)
    return np.array(out)


def shares(got, want64, gates):
    """Per tensor (max |got - want| / gate, flat index of the worst element); a NaN or Inf anywhere in ``got`` gives inf."""
    pairs = [share_of(a, w, q) for a, w, q in zip(got, want64, gates)]
    return np.array([s for s, _ in pairs]), [i for _, i in pairs]


_CACHE = {}


def case(name, level):
    """One of loss_cpu.CASES at one level with its seeded g: (inputs, predictions, g, float64 closed form, gates, n_attn), computed
    once and shared (never modified).  The gate's yardstick is ``autograd_ref`` in fp32 against float64."""
    key = (name, level)
    if key not in _CACHE:
        inputs, predictions, _, _ = lc.case(name, level)
        g = seeded_g(name, level)
        r32 = autograd_ref(inputs, predictions, level, level, g, torch.float32)
        r64 = autograd_ref(inputs, predictions, level, level, g, torch.float64)
        n = n_attn_of(inputs, predictions)
        _CACHE[key] = (inputs, predictions, g, closed_form(inputs, predictions, level, level, g), gate(r32, r64, g, n), n, r32, r64)
    return _CACHE[key]


def hidden(inputs, predictions, pitch_level, energy_level):
    """Per tensor of NAMES the boolean array of the positions a mask hides (where the gradient must be exactly +0.0)."""
    mel, log_d, attn = predictions[0], predictions[4], predictions[10]
    B, T, n_mel = mel.shape
    H, L = attn[0].shape[1], log_d.shape[1]
    pad_t, pad_l = np.asarray(predictions[7]), np.asarray(predictions[6])
    _, _, region, _ = _region(inputs[4], inputs[7], L, T)
    m = np.ones((B, H, T, L), dtype=bool)
    m[:, 0] = ~region.numpy()
    by = lambda level: pad_t if level == "frame_level" else pad_l  # noqa: E731
    frames = np.broadcast_to(pad_t[:, :, None], (B, T, n_mel))
    return [frames, frames, by(pitch_level), by(energy_level), pad_l, m, m, m, m]
