#!/usr/bin/env python3
"""Golden values for the optimiser step — runs ONLY where the reference lives read-only at /root/reference (the import recipe of
make_golden_aligner.py).  It imports the reference's ``model.optimizer.ScheduledOptim`` and drives it as train.py:89-95 does:
``nn.utils.clip_grad_norm_`` -> ``step_and_update_lr()`` -> ``zero_grad()``.

    python tests/golden/make_golden_optim.py

optim_schedule.npz   the learning rate of steps 1..12000 under the shipped train.yaml (warm-up 4000, no anneal) and under anneal steps
                     [3000, 5000, 9000] at rate 0.3, plus a restart from current_step = 7000 (steps 7001..7100); float64
optim_tiny.npz       tests/optim_cpu.tiny_case (six tensors of 1, 3, 4, 5, 6x7 and 8 elements, the last never updated; five steps from
                     current_step = 3998, one with a norm below the threshold, one with a gradient set to None) at weight_decay 0 and
                     0.01: after every step the parameters, exp_avg, exp_avg_sq, step and the returned total_norm, once from the
                     reference's loop in fp32 and once from the same loop cast to float64
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import optim_cpu as oc  # noqa: E402

MODEL_CONFIG = {"transformer": {"encoder_hidden": oc.ENCODER_HIDDEN}}
RESTART, RESTART_STEPS, TINY_START = 7000, 100, 3998


def train_config(schedule, weight_decay=0.0):
    return {"optimizer": dict(betas=list(oc.BETAS), eps=oc.EPS, weight_decay=weight_decay, grad_clip_thresh=oc.GRAD_CLIP, **schedule)}


class Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.items = torch.nn.ParameterList(params)


def reference_lrs(schedule, current_step, n):
    from model.optimizer import ScheduledOptim  # the reference class

    so = ScheduledOptim(Holder([torch.nn.Parameter(torch.zeros(1))]), train_config(schedule), MODEL_CONFIG, current_step)
    out = []
    for _ in range(n):
        so._update_learning_rate()
        out.append(so._optimizer.param_groups[0]["lr"])
    assert so.current_step == current_step + n
    return np.array(out, dtype=np.float64)


def make_schedule():
    arrays = {}
    for name, cfg in (("shipped", oc.SHIPPED), ("annealed", oc.ANNEALED)):
        arrays["lr_" + name] = reference_lrs(cfg, 0, 12000)
        arrays["restart_" + name] = reference_lrs(cfg, RESTART, RESTART_STEPS)
        assert np.array_equal(arrays["restart_" + name], arrays["lr_" + name][RESTART:RESTART + RESTART_STEPS])
    mga.save("optim_schedule", dict(shipped=oc.SHIPPED, annealed=oc.ANNEALED, encoder_hidden=oc.ENCODER_HIDDEN, restart=RESTART), **arrays)


class Driver:
    """What tests/optim_cpu.torch_run drives in place of a bare torch.optim.Adam: the reference's ScheduledOptim."""

    def __init__(self, params, weight_decay):
        from model.optimizer import ScheduledOptim

        self.so = ScheduledOptim(Holder(params), train_config(oc.SHIPPED, weight_decay), MODEL_CONFIG, TINY_START)
        self.state = self.so._optimizer.state
        self.lrs = []

    def step(self):
        self.so.step_and_update_lr()
        self.lrs.append(self.so._optimizer.param_groups[0]["lr"])
        self.so.zero_grad()


def flat(snaps, q):
    return np.stack([np.concatenate([np.asarray(x).reshape(-1) for x in s[q]]) for s in snaps])


def make_tiny():
    arrays, meta = {}, dict(sizes=[list(s) if isinstance(s, tuple) else [s] for s in oc.TINY_SIZES], start=TINY_START, steps=5,
                            weight_decays=[0.0, 0.01], betas=list(oc.BETAS), eps=oc.EPS, max_norm=oc.GRAD_CLIP)
    for key, wd in (("wd0", 0.0), ("wd1", 0.01)):
        case = oc.tiny_case(wd)
        if key == "wd0":
            arrays["params"] = np.concatenate([x.reshape(-1) for x in case["params"]])
            arrays["grads"] = np.stack([np.concatenate([(np.full(p.shape, np.nan, np.float32) if g is None else g).reshape(-1)
                                                        for g, p in zip(row, case["params"])]) for row in case["grads"]])  # NaN = None
        for dtype, tag in (("float32", "ref32"), ("float64", "ref64")):
            drivers = []

            def make(params, wd=wd):
                drivers.append(Driver(params, wd))
                return drivers[0], (lambda lr: None)

            snaps = oc.torch_run(case, dtype, make_optimizer=make)
            assert np.array_equal(np.array(drivers[0].lrs), np.array(case["lrs"])), "the case's learning rates are the reference's"
            for q in oc.QUANTITIES:
                arrays[f"{tag}_{key}_{q}"] = flat(snaps, q)
            arrays[f"{tag}_{key}_step"] = np.array([s["step"] for s in snaps], dtype=np.int64)
            arrays[f"{tag}_{key}_norm"] = np.array([s["norm"] for s in snaps], dtype=dtype)
            print(key, tag, "norms", arrays[f"{tag}_{key}_norm"], "steps", arrays[f"{tag}_{key}_step"][-1])
        arrays[f"lrs_{key}"] = np.array(case["lrs"], dtype=np.float64)
    mga.save("optim_tiny", meta, **arrays)


if __name__ == "__main__":
    make_schedule()
    make_tiny()
