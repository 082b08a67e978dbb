#!/usr/bin/env python3
"""Golden gradients for the training loss — runs ONLY where the reference lives read-only at /root/reference (the import recipe of
make_golden_loss.py).  It imports the reference's ``model.loss.FastSpeech2Loss``, feeds it the fp32 tuples stored in teacher_tiny.npz
and teacher_tiny_phoneme_level.npz (make_golden_teacher.py: B = 2, L = 12, T = 40, four layers, both feature levels) with
``requires_grad`` on the five predictions and the four alignment maps, and calls ``total.backward()`` (train.py:88) — once in fp32 and
once with the SAME fp32 tuple cast to float64, so the two runs differentiate the same function at the same point and differ in
arithmetic only (the stored ``_f64`` tuple is another point: the float64 model's own predictions).  The guided-attention weights and
the duration target are fp32 in both runs (``.float()``, model/loss.py:104-108,190).  torch's MSELoss backward refuses a float64
prediction against that fp32 target ("Found dtype Float but expected Double"), so in the float64 run the reference's ``mse_loss``
member is wrapped to cast its target to the prediction's dtype — the target's VALUES stay the fp32 ones; nothing else is touched.

    python tests/golden/make_golden_lossgrad.py

lossgrad_tiny.npz                  the nine gradients (mel, postnet, pitch, energy, log_d, attn0..3) of both runs, and the seven values
lossgrad_tiny_phoneme_level.npz    the same at phoneme_level
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402
from tests import loss_cpu, lossgrad_cpu  # noqa: E402
from tests.util import load_golden  # noqa: E402


class _CastTargetMSE(torch.nn.MSELoss):
    def forward(self, x, y):
        return super().forward(x, y.to(x.dtype))


def make(name, source):
    from model.loss import FastSpeech2Loss  # the reference class

    meta, z = load_golden(source)
    ref = FastSpeech2Loss(wl.preprocess_config(meta["pitch"], meta["energy"]), wl.model_config(meta["config"]))
    arrays = {}
    for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
        inputs, predictions = loss_cpu.fixture_case(z, meta, "")
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in lossgrad_cpu.nine(predictions)]
        inputs = tuple(t.to(dtype).clone() if torch.is_tensor(t) and t.dtype.is_floating_point else t for t in inputs)
        predictions = tuple(leaves[:5]) + tuple(predictions[5:10]) + (leaves[5:], predictions[11])
        ref.mse_loss = _CastTargetMSE() if suffix else torch.nn.MSELoss()
        with contextlib.redirect_stdout(io.StringIO()):
            out = ref(inputs, predictions)
        assert all(o.dtype == dtype for o in out)
        out[0].backward()
        arrays["values" + suffix] = np.array([o.item() for o in out], dtype=np.float64 if suffix else np.float32)
        for n, x in zip(lossgrad_cpu.NAMES, leaves):
            assert x.grad is not None and x.grad.dtype == dtype and x.grad.shape == x.shape
            arrays[n + suffix] = x.grad.numpy()
        print(name, suffix or "fp32", {n: float(np.abs(arrays[n + suffix]).max()) for n in lossgrad_cpu.NAMES})
    mga.save(name, dict(source=source, names=list(lossgrad_cpu.NAMES), pitch=meta["pitch"], energy=meta["energy"], B=meta["B"], L=meta["L"],
                        T=meta["T"], n_layer=meta["n_layer"], grad_output=[1, 0, 0, 0, 0, 0, 0]), **arrays)


if __name__ == "__main__":
    make("lossgrad_tiny", "teacher_tiny")
    make("lossgrad_tiny_phoneme_level", "teacher_tiny_phoneme_level")
