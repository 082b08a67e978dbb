"""The reference's VarianceAdaptor (model/modules.py:17-159, teacher-forced branch) and its backward stated independently on the CPU, for
the tests of csrc/adaptorgrad.hip and smart_nar_fast_tts_amd/adaptor.py.  No test lives here.

``autograd_ref``   the adaptor in torch ops — tests/predictor_grad_cpu.statement for the three predictors, torch.bucketize + indexing for the
                   two embeddings, repeat_interleave + pad / crop for the length regulator — in fp32 or float64, differentiated by torch's
                   autograd.  In fp32 it is what the gate is built from.
``forward_form``   the same forward written out (prefix sums and a search for the length regulator), keeping what a backward needs.
``closed_form``    the chained backward written out: per stage in reverse the embedding's segment sum over ALL rows, the predictor's
                   closed form (tests/predictor_grad_cpu.closed_form), the fan-in add; the length regulator's sum over each phoneme's
                   frames below T.  ``mutate`` names one deliberate mistake (MUTANTS); forward mistakes are made in ``forward_form``.
``gate``           per tensor and absolute: 2 x max |ref fp32 - ref float64| + one fp32 ulp of max |ref float64|; an all-zero float64
                   tensor must be matched exactly, a NaN / Inf is an infinite share.

A mix is two letters, pitch level then energy level: p = phoneme_level, f = frame_level.  Weights travel as a dict: "dur", "pitch",
"energy" (each a predictor dict of tests/predictor_grad_cpu), "pitch_emb", "energy_emb" [n_bins, d], "pitch_bins", "energy_bins"
[n_bins - 1].  Inputs travel as a dict: x [B, L, d], src_lens [B], duration [B, L] int64, T, pitch_t / energy_t (at the mix's level),
g_out [B, T, d], g_pitch / g_energy (at the mix's level), g_log_d [B, L]."""
import numpy as np
import torch

from tests import util
from tests import predictor_grad_cpu as pg

PRED = ("dur", "pitch", "energy")
PRED_KEY = {"dur": "duration_predictor", "pitch": "pitch_predictor", "energy": "energy_predictor"}
MIXES = ("pp", "pf", "fp", "ff")
LEVEL = {"p": "phoneme_level", "f": "frame_level"}
HEAD = ("y", "pitch", "energy", "log_d", "dx", "d_pitch_emb", "d_energy_emb")
NAMES = HEAD + tuple(f"{p}.{n}" for p in PRED for n in pg.NAMES[:10])
FIXTURE_NAMES = HEAD + tuple(f"{p}.{n}" for p in PRED for n in ("wlin", "b1"))  # what the golden file records
MUTANTS = ("embed_skips_padded_rows", "bucketize_right", "lr_first_frame_skipped", "lr_one_frame_too_many", "cropped_frames_counted",
           "energy_reads_x", "frame_embedding_summed_per_phoneme")
FORWARD_MUTANTS = ("bucketize_right", "energy_reads_x")


def order(mix):
    """the stages after the duration predictor, in forward order"""
    o = [s for s, c in zip(("pitch", "energy"), mix) if c == "p"] + ["lr"]
    return o + [s for s, c in zip(("pitch", "energy"), mix) if c == "f"]


def _t(v, dtype):
    return torch.as_tensor(np.asarray(v)).to(dtype)


def masks(inp):
    """src_mask [B, L], mel_mask [B, T] (True = padded) and mel_len [B] (uncropped)"""
    d = np.maximum(np.asarray(inp["duration"]), 0)
    mel_len = d.sum(1).astype(np.int64)
    return pg.mask_of(inp["src_lens"], d.shape[1]), pg.mask_of(mel_len, int(inp["T"])), mel_len


def regulate(x, duration, T):
    """LengthRegulator.LR + pad (model/modules.py:201-226, utils/tools.py:288-306), differentiable"""
    B, L, d = x.shape
    rows = []
    for b in range(B):
        rep = torch.repeat_interleave(torch.arange(L), torch.as_tensor(np.maximum(np.asarray(duration[b]), 0)))
        e = x[b][rep][:T]
        rows.append(torch.cat([e, torch.zeros(T - e.shape[0], d, dtype=x.dtype)]))
    return torch.stack(rows)


def autograd_ref(inp, w, mix, dtype=torch.float64):
    """{name: numpy} for every tensor of NAMES: the four outputs and the gradients of
    (g_out y).sum() + (g_pitch pitch).sum() + (g_energy energy).sum() + (g_log_d log_d).sum()"""
    src_mask, mel_mask, _ = masks(inp)
    x = _t(inp["x"], dtype).clone().requires_grad_(True)
    wl = {p: {k: v.clone().requires_grad_(True) for k, v in pg._w(w[p], dtype).items()} for p in PRED}
    emb = {s: _t(w[f"{s}_emb"], dtype).clone().requires_grad_(True) for s in ("pitch", "energy")}
    pred = {"dur": pg.statement(None, None, src_mask, leaves=dict(wl["dur"], x=x))["pred"]}
    cur, mask = x, src_mask
    for st in order(mix):
        if st == "lr":
            cur, mask = regulate(cur, inp["duration"], int(inp["T"])), mel_mask
            continue
        pred[st] = pg.statement(None, None, mask, leaves=dict(wl[st], x=cur))["pred"]
        idx = torch.bucketize(_t(inp[f"{st}_t"], dtype), _t(w[f"{st}_bins"], dtype))
        cur = cur + emb[st][idx]
    leaves = [x, emb["pitch"], emb["energy"]] + [wl[p][n] for p in PRED for n in pg.NAMES[:10]]
    grads = torch.autograd.grad([cur, pred["pitch"], pred["energy"], pred["dur"]], leaves,
                                grad_outputs=[_t(inp[k], dtype) for k in ("g_out", "g_pitch", "g_energy", "g_log_d")])
    out = dict(y=cur, pitch=pred["pitch"], energy=pred["energy"], log_d=pred["dur"])
    out.update(zip(NAMES[4:], grads))
    return {k: v.detach().numpy() for k, v in out.items()}


def forward_form(inp, w, mix, dtype=torch.float64, mutate=None):
    """The four outputs and mel_len, written out; saved: per stage the predictor's input, mask and activations and the bucket indices,
    and the length regulator's prefix sums."""
    src_mask, mel_mask, mel_len = masks(inp)
    T = int(inp["T"])
    x = _t(inp["x"], dtype)
    saved, out = {}, {"mel_len": mel_len}

    def predict(name, xin, mask):
        with torch.no_grad():
            f = pg.statement(xin, w[name], mask, dtype=dtype)
        saved[name] = dict(x=xin, mask=mask, saved=(f["v1"], f["h1"], f["v2"]))
        return f["pred"]

    out["log_d"] = predict("dur", x, src_mask)
    cur, mask, before = x, src_mask, None
    for st in order(mix):
        if st == "lr":
            cum = np.cumsum(np.maximum(np.asarray(inp["duration"]), 0), axis=1)
            B, L, d = cur.shape
            y = torch.zeros(B, T, d, dtype=dtype)
            for b in range(B):
                for t in range(min(T, int(cum[b, -1]))):
                    y[b, t] = cur[b, int(np.searchsorted(cum[b], t, side="right"))]  # the first l with cum[l] > t
            saved["lr"] = dict(cum=cum, L=L)
            cur, mask, before = y, mel_mask, None
            continue
        xin = before if (mutate == "energy_reads_x" and st == "energy" and before is not None) else cur
        out[st] = predict(st, xin, mask)
        idx = torch.bucketize(_t(inp[f"{st}_t"], dtype), _t(w[f"{st}_bins"], dtype), right=mutate == "bucketize_right")
        saved[st]["idx"] = idx
        before = cur
        cur = cur + _t(w[f"{st}_emb"], dtype)[idx]
    out["y"] = cur
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}, saved


def lr_backward(g, cum, L, T, mutate=None):
    """d_x[b, l] = the sum of g[b, t] over t in [cum[l-1], min(cum[l], T))"""
    B, _, d = g.shape
    flat = g.reshape(B * T, d)
    dx = torch.zeros(B, L, d, dtype=g.dtype)
    for b in range(B):
        for l in range(L):
            s, e = (int(cum[b, l - 1]) if l else 0), int(cum[b, l])
            if e <= s:
                continue
            if mutate == "lr_first_frame_skipped":
                s += 1
            if mutate == "lr_one_frame_too_many":
                e += 1
            if mutate == "cropped_frames_counted":  # no min(., T): the frames past T are the next utterance's rows
                rows = flat[b * T + s:min(b * T + e, B * T)]
            else:
                rows = g[b, min(s, T):min(e, T)]
            dx[b, l] = rows.sum(0)
    return dx


def embed_backward(g, idx, n_bins, skip=None):
    """d_table[k] = the sum of g's rows with idx == k, over all rows (skip: a bool mask of rows the WRONG sum leaves out)"""
    d = g.shape[-1]
    rows, k = g.reshape(-1, d), idx.reshape(-1)
    if skip is not None:
        keep = ~torch.as_tensor(np.asarray(skip)).reshape(-1)
        rows, k = rows[keep], k[keep]
    return torch.zeros(n_bins, d, dtype=g.dtype).index_add_(0, k, rows)


def closed_form(inp, w, mix, saved, dtype=torch.float64, mutate=None):
    """every gradient of NAMES[4:] from what forward_form saved"""
    assert mutate is None or mutate in MUTANTS, mutate
    T = int(inp["T"])
    n_bins = np.asarray(w["pitch_emb"]).shape[0]
    out = {}
    g = _t(inp["g_out"], dtype)
    after_lr = True
    for st in reversed(["dur"] + order(mix)):
        if st == "lr":
            g = lr_backward(g, saved["lr"]["cum"], saved["lr"]["L"], T, mutate)
            after_lr = False
            continue
        s = saved[st]
        if st != "dur":
            if mutate == "frame_embedding_summed_per_phoneme" and after_lr:
                cum, L = saved["lr"]["cum"], saved["lr"]["L"]
                dt = torch.zeros(n_bins, g.shape[-1], dtype=dtype)
                for b in range(g.shape[0]):
                    for l in range(L):
                        a, e = min(int(cum[b, l - 1]) if l else 0, T), min(int(cum[b, l]), T)
                        if e > a:
                            dt[int(s["idx"][b, a])] += g[b, a:e].sum(0)  # the bucket of the phoneme's first frame for all its frames
                out[f"d_{st}_emb"] = dt
            else:
                out[f"d_{st}_emb"] = embed_backward(g, s["idx"], n_bins, s["mask"] if mutate == "embed_skips_padded_rows" else None)
        gr = pg.closed_form(s["x"], w[st], s["mask"], inp["g_log_d" if st == "dur" else f"g_{st}"], s["saved"], dtype=dtype)
        for n in pg.NAMES[:10]:
            out[f"{st}.{n}"] = torch.as_tensor(gr[n])
        g = g + torch.as_tensor(gr["dx"])
    out["dx"] = g
    return {k: v.detach().numpy() for k, v in out.items()}


def evaluate(inp, w, mix, dtype=torch.float64, mutate=None):
    """forward_form + closed_form: every tensor of NAMES (and mel_len) as numpy"""
    out, saved = forward_form(inp, w, mix, dtype, mutate if mutate in FORWARD_MUTANTS else None)
    out.update(closed_form(inp, w, mix, saved, dtype, mutate))
    return out


def gate(ref32, ref64, names=None):
    """The absolute gates {name: value}: twice the reference's own fp32 error plus one fp32 ulp of the largest magnitude."""
    return util.gates(ref32, ref64, names or [k for k in ref64 if k in ref32 and k != "mel_len"])


shares = util.shares  # {name: max |got - ref64| / gate}


def classes(sh):
    """the worst share per tensor class: the heads by name, the predictors' gradients per predictor"""
    out = {}
    for k, v in sh.items():
        c = k.split(".")[0] + ".*" if "." in k else k
        out[c] = max(out.get(c, 0.0), v)
    return out


# ------------------------------------------------------------------------------------------------------------ weights and inputs
def config(d=32, F=256, K=3, n_bins=8):
    return dict(d=d, F=F, K=K, n_bins=n_bins)


def synth_weights(cfg, seed):
    """every weight from a numpy RandomState: three predictors, two tables about the size nn.Embedding draws, fixed linear bin edges"""
    rs = np.random.RandomState(seed)
    w = {p: pg.seeded_weights(cfg["d"], cfg["F"], cfg["K"], int(rs.randint(1 << 30))) for p in PRED}
    for s in ("pitch", "energy"):
        w[f"{s}_emb"] = rs.standard_normal((cfg["n_bins"], cfg["d"])).astype(np.float32)
    w["pitch_bins"] = np.linspace(-1.5, 1.5, cfg["n_bins"] - 1).astype(np.float32)
    w["energy_bins"] = np.linspace(-1.0, 2.0, cfg["n_bins"] - 1).astype(np.float32)
    return w


def state_dict(w):
    """the weights under the reference's ``variance_adaptor.*`` names (without the prefix), numpy arrays in checkpoint layout"""
    from smart_nar_fast_tts_amd.predictor import PARAM_NAMES

    sd = {"pitch_bins": w["pitch_bins"], "energy_bins": w["energy_bins"], "pitch_embedding.weight": w["pitch_emb"],
          "energy_embedding.weight": w["energy_emb"]}
    for p in PRED:
        for key, n in zip(PARAM_NAMES, pg.NAMES[:10]):
            v = np.asarray(w[p][n], dtype=np.float32)
            sd[f"{PRED_KEY[p]}.{key}"] = v.reshape(1, -1) if n == "wlin" else v.reshape(1) if n == "blin" else v
    return sd


def grad_key(name):
    """NAMES[4:] -> the parameter's state-dict key (None for dx)"""
    from smart_nar_fast_tts_amd.predictor import PARAM_NAMES

    if name == "dx":
        return None
    if name.startswith("d_"):
        return f"{name[2:-4]}_embedding.weight"
    p, n = name.split(".")
    return f"{PRED_KEY[p]}.{PARAM_NAMES[pg.NAMES.index(n)]}"


def synth_inputs(cfg, B, L, T, src_lens, seed, max_dur=9):
    """Both levels of every target and gradient: {x, src_lens, duration, T, pitch_t_p, pitch_t_f, energy_t_p, energy_t_f, g_out, g_log_d,
    g_pitch_p, g_pitch_f, g_energy_p, g_energy_f}.  Padded phonemes have duration 0; padded targets are 0, as a collated batch holds."""
    rs = np.random.RandomState(seed)
    src_lens = np.asarray(src_lens, dtype=np.int64)
    src_mask = pg.mask_of(src_lens, L)
    z = dict(x=rs.standard_normal((B, L, cfg["d"])).astype(np.float32), src_lens=src_lens, T=np.int64(T))
    dur = rs.randint(0, max_dur + 1, size=(B, L)).astype(np.int64)
    dur[src_mask] = 0
    z["duration"] = dur
    mel_mask = pg.mask_of(dur.sum(1), T)
    for s in ("pitch", "energy"):
        for c, (shape, mask) in (("p", ((B, L), src_mask)), ("f", ((B, T), mel_mask))):
            t = (rs.standard_normal(shape) * 1.2).astype(np.float32)
            t[mask] = 0.0
            z[f"{s}_t_{c}"] = t
            z[f"g_{s}_{c}"] = rs.standard_normal(shape).astype(np.float32)
    z["g_out"] = rs.standard_normal((B, T, cfg["d"])).astype(np.float32)
    z["g_log_d"] = rs.standard_normal((B, L)).astype(np.float32)
    return z


def inputs_for(z, mix):
    """the inputs dict of one mix out of the both-levels arrays (a fixture file or synth_inputs)"""
    inp = {k: np.asarray(z[k]) for k in ("x", "src_lens", "duration", "T", "g_out", "g_log_d")}
    for s, c in zip(("pitch", "energy"), mix):
        inp[f"{s}_t"], inp[f"g_{s}"] = np.asarray(z[f"{s}_t_{c}"]), np.asarray(z[f"g_{s}_{c}"])
    return inp
