"""The optimiser half of the reference's training step on the device: ``nn.utils.clip_grad_norm_``, ``ScheduledOptim`` (Adam under the
Noam warm-up / anneal schedule, model/optimizer.py) and ``zero_grad()`` — train.py:91-95 — as a fixed handful of HIP launches
(csrc/optim.hip; ``ns_opt_*`` in include/nar_fs2.h).  It acts on ordinary ``torch.nn.Parameter``s and their ``.grad``s, so it drops into
a training loop that runs the reference model under PyTorch-ROCm; the model's backward stays torch's (the loss's own: loss.py).

    optimizer = ScheduledOptim(model, train_config, model_config, restore_step)          # utils/model.py:27-29
    ...
    total_loss.backward()
    nn.utils.clip_grad_norm_(model.parameters(), grad_clip_thresh)                       # train.py:91   } or, in three launches:
    optimizer.step_and_update_lr()                                                       # train.py:94   } optimizer.step_and_update_lr(
    optimizer.zero_grad()                                                                # train.py:95   }     grad_clip_thresh, zero_grad=True)

Out of scope: ``amsgrad``, ``maximize``, several parameter groups, parameters that are not fp32, graph capture of a step (lr, the betas
and the step number are kernel arguments), any backward pass, any change to ``checkpoint.get_model``.  One optimiser is used from one
stream at a time (it owns one workspace and one norm record)."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._train import guard

CHUNK = _lib.NS["NS_OPT_CHUNK"]


def _check_params(params):
    """fp32, contiguous, one cuda device; returns the device."""
    if len(params) == 0:
        raise ValueError("optimizer got an empty parameter list")
    for i, p in enumerate(params):
        if not torch.is_tensor(p):
            raise ValueError(f"parameter {i} must be a tensor, got {type(p).__name__}")
        if p.dtype != torch.float32:
            raise ValueError(f"parameter {i} must be float32, got {p.dtype} (non-fp32 parameters are out of scope)")
        if not p.is_contiguous():
            raise ValueError(f"parameter {i} must be contiguous (it is updated in place), got strides {tuple(p.stride())}")
    for i, p in enumerate(params):
        if not p.is_cuda:
            raise RuntimeError(f"parameter {i} must live on the MI355X (cuda) device; there is no CPU path")
    dev = params[0].device
    for i, p in enumerate(params):
        if p.device != dev:
            raise ValueError(f"parameter {i} is on {p.device}, parameter 0 on {dev}: one device per optimizer")
    return dev


class _Table:
    """The device chunk table of one parameter list with its workspace and norm record.  ``refresh`` rebuilds and uploads the table
    only when the tuple of gradient pointers (0 = skipped) or the lags changed: a steady-state step uploads nothing."""

    def __init__(self, params):
        self.params = list(params)
        self.device = _check_params(self.params)
        self.lib = _lib.load()
        n = len(self.params)
        self.n = n
        self.numels = (C.c_int64 * n)(*[p.numel() for p in self.params])
        self.plan = _lib.NsOptPlan()
        _lib.check(self.lib.ns_opt_plan_sizes(self.numels, n, C.byref(self.plan)), "ns_opt_plan_sizes")
        self.param_ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in self.params])
        with guard(self.device):
            self.table = torch.empty(int(self.plan.table_bytes), dtype=torch.uint8, device=self.device)
            self.ws = torch.empty(int(self.plan.ws_bytes), dtype=torch.uint8, device=self.device)
            self.record = torch.zeros(4, dtype=torch.float32, device=self.device)  # ns_opt_record: float64 norm, total_norm, clip_coef
        self.total_norm = self.record[2]
        self._key = None
        self.uploads = 0

    def _grad_ptr(self, i, p):
        g = p.grad
        if g is None:
            return 0
        if g.dtype != torch.float32 or g.device != p.device or g.is_sparse or not g.is_contiguous() or g.shape != p.shape:
            raise ValueError(f"the gradient of parameter {i} must be a dense contiguous float32 tensor of the parameter's shape on {p.device}")
        return g.data_ptr()

    def refresh(self, lags=None):
        """Returns the tuple of gradient pointers the table now holds."""
        if any(p.data_ptr() != (q or 0) for p, q in zip(self.params, self.param_ptrs)):  # (a NULL reads back as None)
            raise RuntimeError("a parameter's storage moved since the optimizer was built (assign to .data in place, or build a new optimizer)")
        grads = tuple(self._grad_ptr(i, p) for i, p in enumerate(self.params))
        key = (grads, tuple(lags) if lags is not None else None)
        if key != self._key:
            host = np.zeros(int(self.plan.table_bytes) // 8, dtype=np.int64)
            gp = (C.c_void_p * self.n)(*grads)
            lg = (C.c_int32 * self.n)(*lags) if lags is not None else None
            _lib.check(self.lib.ns_opt_build_table(self.numels, self.param_ptrs, gp, lg, self.n, C.c_void_p(host.ctypes.data), host.nbytes), "ns_opt_build_table")
            with guard(self.device):
                self.table.copy_(torch.from_numpy(host).view(torch.uint8))  # stream-ordered; returns once the host rows are consumed
            self._key = key
            self.uploads += 1
        return grads

    def st(self):
        return _lib.stream_ptr(self.device)

    def grad_norm(self, max_norm: float):
        with guard(self.device):
            _lib.check(self.lib.ns_opt_grad_norm(C.byref(self.plan), _lib.ptr(self.table), self.table.numel(), float(max_norm), _lib.ptr(self.ws),
                                                 self.ws.numel(), _lib.ptr(self.record, _lib.NsOptRecord), self.st()), "ns_opt_grad_norm")

    def scale(self):
        with guard(self.device):
            _lib.check(self.lib.ns_opt_scale_grads(C.byref(self.plan), _lib.ptr(self.table), self.table.numel(), _lib.ptr(self.record, _lib.NsOptRecord), self.st()),
                       "ns_opt_scale_grads")

    def zero(self):
        with guard(self.device):
            _lib.check(self.lib.ns_opt_zero_grads(C.byref(self.plan), _lib.ptr(self.table), self.table.numel(), self.st()), "ns_opt_zero_grads")


_CLIP_TABLES = OrderedDict()  # (parameter pointers, sizes) -> _Table, least recently used first
_MAX_CLIP_TABLES = 4


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """``torch.nn.utils.clip_grad_norm_`` (train.py:91) in three launches: the 2-norm of all gradients, then ``g *= min(1, max_norm /
    (norm + 1e-6))`` in place — multiplied even when the coefficient is 1, as torch does.  Parameters whose ``.grad`` is None are
    skipped.  Returns the 0-dim fp32 device ``total_norm`` without reading it; it is a view of the table's record and holds its value
    until the next call on the same parameter list.  2-norm only."""
    if float(norm_type) != 2.0:
        raise ValueError(f"only the 2-norm is implemented (the reference's default), got norm_type={norm_type}")
    if float(max_norm) < 0:
        raise ValueError(f"max_norm must be >= 0, got {max_norm}")
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = list(parameters)
    key = tuple((p.data_ptr(), p.numel()) for p in params if torch.is_tensor(p))
    t = _CLIP_TABLES.get(key)
    if t is None or len(t.params) != len(params) or any(a is not b for a, b in zip(t.params, params)):
        t = _Table(params)
        _CLIP_TABLES[key] = t
    _CLIP_TABLES.move_to_end(key)
    while len(_CLIP_TABLES) > _MAX_CLIP_TABLES:
        _CLIP_TABLES.popitem(last=False)
    t.refresh()
    t.grad_norm(max_norm)
    t.scale()
    return t.total_norm


class Adam:
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` for one group of fp32, contiguous parameters on one cuda device, as
    one launch per step.  The arithmetic is torch's single-tensor order (``_single_tensor_adam``, non-capturable) per element.

    ``param_groups`` is one dict with torch's keys; ``lr`` is read from it at every ``step()`` (the reference writes it there,
    optimizer.py:50-51).  ``state_dict()`` / ``load_state_dict()`` use torch's own layout, so a ``torch.optim.Adam.state_dict()`` saved
    by the reference (train.py:150-154) loads here and ours loads into ``torch.optim.Adam``.

    DEVIATION from today's torch: ``zero_grad()`` defaults to ``set_to_none=False`` — the torch behaviour of the reference's day.  It
    keeps the gradient pointers stable, so the device table is built once; with ``set_to_none=True`` every step rebuilds and uploads it.
    A parameter whose ``.grad`` is None at a step is skipped and keeps its own step count, as in torch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False):
        params = list(params)
        if len(params) > 0 and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError(f"one parameter group is supported, got {len(params)}")
            group = dict(params[0])
            params = list(group.pop("params"))
            lr, betas, eps = group.pop("lr", lr), group.pop("betas", betas), group.pop("eps", eps)
            weight_decay, amsgrad, maximize = group.pop("weight_decay", weight_decay), group.pop("amsgrad", amsgrad), group.pop("maximize", maximize)
        if amsgrad or maximize:
            raise ValueError("amsgrad and maximize are out of scope")
        self._validate(lr, betas, eps, weight_decay)
        self._t = _Table(params)
        self.param_groups = [self._group(lr, betas, eps, weight_decay, params)]
        dev = self._t.device
        with guard(dev):
            self._exp_avg = torch.zeros(int(self._t.plan.state_floats), dtype=torch.float32, device=dev)
            self._exp_avg_sq = torch.zeros(int(self._t.plan.state_floats), dtype=torch.float32, device=dev)
        self._offsets = []
        off = 0
        for p in params:
            self._offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self._steps = [0] * len(params)  # torch's per-parameter `step`
        self._global_step = 0

    @staticmethod
    def _validate(lr, betas, eps, weight_decay):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= float(eps):
            raise ValueError(f"Invalid epsilon value: {eps}")
        if len(betas) != 2 or not 0.0 <= float(betas[0]) < 1.0 or not 0.0 <= float(betas[1]) < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= float(weight_decay):
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")

    @staticmethod
    def _group(lr, betas, eps, weight_decay, params):
        g = dict(torch.optim.Adam([torch.zeros(1)]).defaults)  # torch's keys, whatever this torch version has
        g.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        g["params"] = params
        return g

    # ---- state views -----------------------------------------------------------------------------
    def _view(self, arena, i):
        p = self._t.params[i]
        return arena[self._offsets[i]:self._offsets[i] + p.numel()].view(p.shape)

    def _present(self):
        return [p.grad is not None for p in self._t.params]  # an empty tensor with a gradient counts its steps, as in torch

    def _lags(self):
        """global_step - step for the tensors that take part; 0 for the skipped ones (never read), so a tensor that stays skipped
        does not change the table."""
        return [self._global_step - s if here else 0 for s, here in zip(self._steps, self._present())]

    # ---- the step --------------------------------------------------------------------------------
    def step(self, closure=None, grad_clip_thresh=None, zero_grad=False):
        """One Adam step in one launch.  EXTENSION: with ``grad_clip_thresh`` the gradients' norm is taken first (two launches) and the
        clip coefficient is applied inside the update — bitwise what ``clip_grad_norm_`` followed by ``step()`` gives, the gradients
        themselves staying unscaled — and the 0-dim device ``total_norm`` is returned; ``zero_grad=True`` also zeroes the gradients in
        the same pass.  Nothing is read back."""
        if closure is not None:
            raise ValueError("a closure is not supported (the reference passes none)")
        if len(self.param_groups) != 1:
            raise ValueError(f"one parameter group is supported, got {len(self.param_groups)}")
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("amsgrad and maximize are out of scope")
        self._validate(g["lr"], g["betas"], g["eps"], g["weight_decay"])
        t = self._t
        # a tensor that is skipped at this step falls one step further behind the global count
        self._global_step += 1
        for i, here in enumerate(self._present()):
            if here:
                self._steps[i] += 1
        t.refresh(self._lags())
        h = _lib.NsOptHyper()
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])
        h.global_step, h.fuse_clip, h.zero_grads = self._global_step, int(grad_clip_thresh is not None), int(bool(zero_grad))
        if grad_clip_thresh is not None:
            if float(grad_clip_thresh) < 0:
                raise ValueError(f"grad_clip_thresh must be >= 0, got {grad_clip_thresh}")
            t.grad_norm(grad_clip_thresh)
        with guard(t.device):
            _lib.check(t.lib.ns_opt_adam_step(C.byref(t.plan), _lib.ptr(t.table), t.table.numel(), C.byref(h), _lib.ptr(self._exp_avg),
                                              _lib.ptr(self._exp_avg_sq), self._exp_avg.numel(), _lib.ptr(t.record, _lib.NsOptRecord), t.st()), "ns_opt_adam_step")
        return t.total_norm if grad_clip_thresh is not None else None

    def zero_grad(self, set_to_none: bool = False):
        """``set_to_none=False`` (the default HERE, unlike today's torch): one launch writes zeros into every gradient in place."""
        if set_to_none:
            for p in self._t.params:
                p.grad = None
            return
        if all(p.grad is None for p in self._t.params):
            return
        self._t.refresh(self._lags())
        self._t.zero()

    # ---- torch's state_dict layout ---------------------------------------------------------------
    def state_dict(self):
        state = {}
        for i, s in enumerate(self._steps):
            if s > 0:
                state[i] = {"step": torch.tensor(float(s)), "exp_avg": self._view(self._exp_avg, i), "exp_avg_sq": self._view(self._exp_avg_sq, i)}
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._t.params)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"one parameter group is supported, the state dict has {len(groups)}")
        saved = groups[0]
        n = len(self._t.params)
        if len(saved["params"]) != n:
            raise ValueError(f"the state dict holds {len(saved['params'])} parameters, this optimizer {n}")
        if saved.get("amsgrad") or saved.get("maximize"):
            raise ValueError("amsgrad and maximize are out of scope")
        self._validate(saved["lr"], saved["betas"], saved["eps"], saved["weight_decay"])
        index = {pid: i for i, pid in enumerate(saved["params"])}
        staged = {}
        for pid, s in state_dict["state"].items():
            if pid not in index:
                raise ValueError(f"the state dict has state for parameter id {pid}, which its group does not list")
            i = index[pid]
            p = self._t.params[i]
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(s[k].shape) != tuple(p.shape):
                    raise ValueError(f"{k} of parameter {i} has shape {tuple(s[k].shape)}, the parameter {tuple(p.shape)}")
            if "max_exp_avg_sq" in s:
                raise ValueError("amsgrad state is out of scope")
            staged[i] = (int(float(s["step"])), s["exp_avg"], s["exp_avg_sq"])
        with guard(self._t.device):
            self._exp_avg.zero_()
            self._exp_avg_sq.zero_()
            self._steps = [0] * n
            for i, (step, m, v) in staged.items():
                self._view(self._exp_avg, i).copy_(m)
                self._view(self._exp_avg_sq, i).copy_(v)
                self._steps[i] = step
        self._global_step = max(self._steps)
        for k in ("lr", "betas", "eps", "weight_decay"):
            self.param_groups[0][k] = tuple(saved[k]) if k == "betas" else saved[k]


class ScheduledOptim:
    """The reference's ``ScheduledOptim`` (model/optimizer.py:5-51) over ``optim.Adam``: the same constructor, attributes
    (``_optimizer``, ``n_warmup_steps``, ``anneal_steps``, ``anneal_rate``, ``current_step``, ``init_lr``) and methods.  The schedule
    is host float64 arithmetic in the reference's operation order, so the learning rates agree bit for bit."""

    def __init__(self, model, train_config, model_config, current_step):
        cfg = train_config["optimizer"]
        self._optimizer = Adam(model.parameters(), betas=cfg["betas"], eps=cfg["eps"], weight_decay=cfg["weight_decay"])
        self.n_warmup_steps = cfg["warm_up_step"]
        self.anneal_steps = cfg["anneal_steps"]
        self.anneal_rate = cfg["anneal_rate"]
        self.current_step = current_step
        self.init_lr = np.power(model_config["transformer"]["encoder_hidden"], -0.5)  # optimizer.py:20

    def step_and_update_lr(self, grad_clip_thresh=None, zero_grad=False):
        """optimizer.py:22-24.  EXTENSION: ``grad_clip_thresh`` folds train.py:91 and ``zero_grad=True`` folds train.py:95 into the
        step: norm, then the fused clip / Adam / zero update, three launches; returns the 0-dim device ``total_norm`` (else None)."""
        self._update_learning_rate()
        return self._optimizer.step(grad_clip_thresh=grad_clip_thresh, zero_grad=zero_grad)

    def zero_grad(self):
        """optimizer.py:26-28; in place (``set_to_none=False``)."""
        self._optimizer.zero_grad()

    def load_state_dict(self, path):
        """optimizer.py:30-31: takes the optimizer's state dict (the reference names the argument ``path``)."""
        self._optimizer.load_state_dict(path)

    def _get_lr_scale(self):
        """min(step ** -0.5, warm_up ** -1.5 * step), times anneal_rate for every anneal step behind us (optimizer.py:33-43)."""
        step = self.current_step
        scale = np.min([np.power(step, -0.5), np.power(self.n_warmup_steps, -1.5) * step])
        for boundary in self.anneal_steps:
            if step > boundary:
                scale = scale * self.anneal_rate
        return scale

    def _update_learning_rate(self):
        """optimizer.py:45-51: advance the step, write the new rate into the group."""
        self.current_step += 1
        lr = self.init_lr * self._get_lr_scale()
        for group in self._optimizer.param_groups:
            group["lr"] = lr
