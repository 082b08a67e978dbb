"""Float64 numpy restatement of the optimiser half of the reference's training step — nn.utils.clip_grad_norm_ (train.py:91), Adam
under ScheduledOptim's schedule (model/optimizer.py) and zero_grad — with the seeded cases of the GPU tests, the same loop on torch's
own CPU Adam (the yardstick of the gate), the gate, and the mutants the gate must reject.

A case is a dict: ``params`` (list of fp32 arrays), ``grads`` (per step a list of fp32 arrays or None = ``p.grad is None``), ``lrs``
(per step), ``betas``, ``eps``, ``weight_decay``, ``max_norm`` (None = no clip), and for the GPU tests ``misaligned_params`` /
``misaligned_grads`` (indices held as ``base[1:]`` views).  A trajectory is a list with one snapshot per step:
``{"p": [...], "m": [...], "v": [...], "step": [...], "norm": float}``; ``m`` / ``v`` of a never-updated tensor are zeros, its step 0.

THE GATE.  For each of p, m, v (per tensor) and the norm, the allowed distance from the float64 trajectory is
    2 x the distance of torch's own fp32 single-tensor Adam (foreach=False, CPU) on the same case + one fp32 ulp of the tensor's
    largest magnitude.
The torch error is computed where the gate is used, never stored.  The factor 2 covers an equally valid rounding order (fused
multiply-add inside lerp / addcmul, a different association of step_size * m / denom).  The ulp term keeps the gate from collapsing
where torch's error is exactly zero (one-element tensors, the first step)."""
import numpy as np

from tests.util import gate_value

CHUNK = 4096  # NS_OPT_CHUNK
MUTANTS = ("no_bias_correction", "eps_inside_sqrt", "betas_swapped", "clip_without_1e-6", "step_off_by_one", "decoupled_weight_decay")
QUANTITIES = ("p", "m", "v")

SHIPPED = dict(warm_up_step=4000, anneal_steps=[], anneal_rate=1.0)          # config/LJSpeech/train.yaml
ANNEALED = dict(warm_up_step=4000, anneal_steps=[3000, 5000, 9000], anneal_rate=0.3)
ENCODER_HIDDEN = 256                                                           # config/LJSpeech/model.yaml
BETAS, EPS, GRAD_CLIP = (0.9, 0.98), 1e-9, 1.0                                  # train.yaml


# ---- the schedule (model/optimizer.py:20, 33-51) -------------------------------------------------------------------------------------
def lr_at(step, warm_up_step, anneal_steps, anneal_rate, encoder_hidden=ENCODER_HIDDEN):
    """The learning rate ScheduledOptim writes when its current_step has just become ``step``: float64, the reference's operation order."""
    init_lr = np.power(encoder_hidden, -0.5)
    scale = np.min([np.power(step, -0.5), np.power(warm_up_step, -1.5) * step])
    for s in anneal_steps:
        if step > s:
            scale = scale * anneal_rate
    return init_lr * scale


def schedule(first, last, **cfg):
    return np.array([lr_at(s, **cfg) for s in range(first, last + 1)], dtype=np.float64)


# ---- clip + Adam in float64 -------------------------------------------------------------------------------------------------------------
def total_norm(grads):
    sq = 0.0
    for g in grads:
        if g is not None:
            sq += float(np.sum(np.asarray(g, dtype=np.float64) ** 2))
    return float(np.sqrt(sq))


def run(case, mutate=None):
    """The float64 trajectory of a case.  ``mutate`` names one deliberate mistake (MUTANTS)."""
    assert mutate is None or mutate in MUTANTS, mutate
    b1, b2 = case["betas"]
    if mutate == "betas_swapped":
        b1, b2 = b2, b1
    eps, wd, max_norm = case["eps"], case["weight_decay"], case["max_norm"]
    p = [np.asarray(x, dtype=np.float64).copy() for x in case["params"]]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    step = [0] * len(p)
    out = []
    for grads, lr in zip(case["grads"], case["lrs"]):
        grads = [None if g is None else np.asarray(g, dtype=np.float64) for g in grads]
        norm = total_norm(grads)
        coef = 1.0
        if max_norm is not None:
            coef = min(1.0, max_norm / (norm + (0.0 if mutate == "clip_without_1e-6" else 1e-6)))
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g * coef
            step[i] += 1
            t = step[i] + (1 if mutate == "step_off_by_one" else 0)
            if wd != 0 and mutate != "decoupled_weight_decay":
                g = g + wd * p[i]
            m[i] = m[i] + (1 - b1) * (g - m[i])
            v[i] = v[i] * b2 + (1 - b2) * g * g
            bc1, bc2 = (1.0, 1.0) if mutate == "no_bias_correction" else (1 - b1 ** t, 1 - b2 ** t)
            if mutate == "eps_inside_sqrt":
                denom = np.sqrt(v[i] / bc2 + eps)
            else:
                denom = np.sqrt(v[i]) / np.sqrt(bc2) + eps
            if wd != 0 and mutate == "decoupled_weight_decay":
                p[i] = p[i] * (1 - lr * wd)
            p[i] = p[i] - (lr / bc1) * m[i] / denom
        out.append({"p": [x.copy() for x in p], "m": [x.copy() for x in m], "v": [x.copy() for x in v], "step": list(step), "norm": norm})
    return out


# ---- the same loop on torch's own CPU optimiser ---------------------------------------------------------------------------------------
def torch_run(case, dtype="float32", make_optimizer=None):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False).step() on the CPU in ``dtype``; a never-updated tensor reports zeros and
    step 0.  ``make_optimizer(params) -> (optimizer, set_lr)`` substitutes another driver of the same loop (the golden generator
    passes the reference's ScheduledOptim)."""
    import torch

    td = getattr(torch, dtype)
    params = [torch.nn.Parameter(torch.from_numpy(np.asarray(x)).to(td).clone()) for x in case["params"]]
    if make_optimizer is None:
        opt = torch.optim.Adam(params, lr=1e-3, betas=tuple(case["betas"]), eps=case["eps"], weight_decay=case["weight_decay"], foreach=False)

        def set_lr(lr):
            opt.param_groups[0]["lr"] = float(lr)
    else:
        opt, set_lr = make_optimizer(params)
    out = []
    for grads, lr in zip(case["grads"], case["lrs"]):
        for q, g in zip(params, grads):
            q.grad = None if g is None else torch.from_numpy(np.asarray(g)).to(td).clone()
        if case["max_norm"] is not None:
            norm = torch.nn.utils.clip_grad_norm_(params, case["max_norm"], foreach=False)
        else:
            norm = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in params if q.grad is not None)).to(td)
        set_lr(lr)
        opt.step()
        snap = {"p": [], "m": [], "v": [], "step": [], "norm": norm.item() if dtype == "float64" else np.float32(norm.item())}
        for q in params:
            s = opt.state.get(q, {})
            snap["p"].append(q.detach().numpy().copy())
            snap["m"].append(s["exp_avg"].numpy().copy() if "exp_avg" in s else np.zeros(q.shape, dtype=dtype))
            snap["v"].append(s["exp_avg_sq"].numpy().copy() if "exp_avg_sq" in s else np.zeros(q.shape, dtype=dtype))
            snap["step"].append(int(s["step"]) if "step" in s else 0)
        out.append(snap)
    return out


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
def gate_of(torch32, want64):
    """2 x max |torch fp32 - float64| + one fp32 ulp of max |float64| (an array or a scalar); 1 for an empty array."""
    return 1.0 if np.size(want64) == 0 else gate_value(torch32, want64)


def shares(got, torch32, want64):
    """Per step the largest share of the gate over the tensors, for p, m, v and the norm: ``{"p": [...], "m": [...], "v": [...],
    "norm": [...]}``.  A NaN anywhere gives a share of inf."""
    out = {q: [] for q in QUANTITIES + ("norm",)}
    for g, t, w in zip(got, torch32, want64):
        for q in QUANTITIES:
            worst = 0.0
            for gi, ti, wi in zip(g[q], t[q], w[q]):
                if wi.size == 0:
                    continue
                err = np.max(np.abs(np.asarray(gi, dtype=np.float64) - wi))
                worst = max(worst, float(err / gate_of(ti, wi)) if np.isfinite(err) else float("inf"))
            out[q].append(worst)
        err = abs(float(g["norm"]) - w["norm"])
        out["norm"].append(float(err / gate_of(t["norm"], w["norm"])) if np.isfinite(err) else float("inf"))
    return out


def worst(sh):
    return {q: max(v) if v else 0.0 for q, v in sh.items()}


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def _case(sizes, steps, seed, lrs=None, grad_scale=None, none_at=(), weight_decay=0.0, max_norm=GRAD_CLIP, step_scale=None, eps=EPS, **extra):
    """Seeded N(0, 0.1) parameters and N(0, 1) gradients times grad_scale[i] (per tensor) times step_scale[s] (per step);
    ``none_at`` holds (step, tensor) pairs whose gradient is None."""
    rng = np.random.default_rng(seed)
    shapes = [s if isinstance(s, tuple) else (s,) for s in sizes]
    params = [(0.1 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    grads = []
    for k in range(steps):
        row = []
        for i, s in enumerate(shapes):
            g = rng.standard_normal(s) * (1.0 if grad_scale is None else grad_scale[i]) * (1.0 if step_scale is None else step_scale[k])
            row.append(None if (k, i) in none_at else g.astype(np.float32))
        grads.append(row)
    # the plateau of the shipped schedule (steps 3999, 4000, ...): about 1e-3, large enough for a wrong update to show in fp32
    lrs = list(schedule(3999, 3998 + steps, **SHIPPED)) if lrs is None else list(lrs)
    case = dict(params=params, grads=grads, lrs=lrs, betas=BETAS, eps=eps, weight_decay=weight_decay, max_norm=max_norm,
                misaligned_params=(), misaligned_grads=())
    case.update(extra)
    return case


TINY_SIZES = [1, 3, 4, 5, (6, 7), 8]          # the last one never gets a gradient
TINY_GRAD_SCALE = [1.0, 1.0, 1e-6, 1.0, 1.0, 1.0]  # tensor 2: gradients far below sqrt(eps), where eps's place in the denominator shows
TINY_STEP_SCALE = [1.0, 1.0, 1e-2, 1.0, 1.0]  # step 2: a norm below the threshold
TINY_NONE = tuple((k, 5) for k in range(5)) + ((3, 1),)  # tensor 1 has no gradient at step 3 and comes back at step 4


def tiny_case(weight_decay=0.0):
    """What tests/golden/optim_tiny.npz was generated from (make_golden_optim.py); the reference started at current_step = 3998."""
    return _case(TINY_SIZES, 5, seed=14, grad_scale=TINY_GRAD_SCALE, step_scale=TINY_STEP_SCALE, none_at=TINY_NONE, weight_decay=weight_decay)


def _exact_threshold():
    c = _case([5, 4, CHUNK + 1], 2, seed=3)
    for row in c["grads"]:
        for g in row:
            g[...] = 0
        row[2][CHUNK] = 1.0  # the norm is exactly max_norm: the coefficient is 1 / (1 + 1e-6), not 1
    return c


CASES = {
    # every size at which the kernel takes another path: empty, below / at / above one 16-byte group, around one chunk, past two
    "edges": lambda: _case([0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3], 3, seed=1, step_scale=[1.0, 1e-3, 1.0],
                           misaligned_params=(2, 7), misaligned_grads=(3, 8)),
    # more tensors than a workgroup has threads
    "many_small": lambda: _case([1 + (i * 5) % 7 for i in range(300)], 2, seed=2, weight_decay=0.01),
    # a None gradient that comes and goes (table rebuild, per-tensor lag), first-step None, a never-updated tensor
    "none_comes_and_goes": lambda: _case([100, 1000, 37, CHUNK + 5, 16], 5, seed=4, step_scale=[1.0, 1e-3, 1.0, 1.0, 1.0],
                                         none_at=((2, 1), (3, 1), (0, 3)) + tuple((k, 4) for k in range(5))),
    "exact_threshold": _exact_threshold,
    "weight_decay": lambda: _case([7, (33, 65), CHUNK + 2], 3, seed=5, weight_decay=0.01, misaligned_params=(1,)),
}

_BUILT = {}


def case(name):
    """(case, float64 trajectory, torch fp32 trajectory), computed once and shared; callers must not modify them."""
    if name not in _BUILT:
        c = tiny_case(0.01 if name == "tiny_wd" else 0.0) if name.startswith("tiny") else CASES[name]()
        _BUILT[name] = (c, run(c), torch_run(c))
    return _BUILT[name]
