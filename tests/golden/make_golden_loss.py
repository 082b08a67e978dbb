#!/usr/bin/env python3
"""Golden values for the validation loss — runs ONLY where the reference lives read-only at /root/reference (the import recipe of
make_golden_aligner.py).  It imports the reference's ``model.loss.FastSpeech2Loss`` and feeds it the tuples already stored in
teacher_tiny.npz and teacher_tiny_phoneme_level.npz (make_golden_teacher.py: B = 2, L = 12, T = 40, four layers, both feature
levels): the fp32 arrays for the fp32 run, the ``_f64`` arrays for the float64 run.  The guided-attention weights are fp32 in both
runs (``.float()`` grids, model/loss.py:104-108).

    python tests/golden/make_golden_loss.py

loss_tiny.npz                  the seven values (total, mel, postnet, pitch, energy, duration, attn) in fp32 and float64
loss_tiny_phoneme_level.npz    the same at phoneme_level
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
from tests import loss_cpu  # noqa: E402
from tests.util import load_golden  # noqa: E402


def make(name, source):
    from model.loss import FastSpeech2Loss  # the reference class

    meta, z = load_golden(source)
    ref = FastSpeech2Loss(wl.preprocess_config(meta["pitch"], meta["energy"]), wl.model_config(meta["config"]))
    values = {}
    for suffix in ("", "_f64"):
        inputs, predictions = loss_cpu.fixture_case(z, meta, suffix)
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            out = ref(inputs, predictions)
        assert all(o.dtype == (torch.float64 if suffix else torch.float32) for o in out)
        values["values" + suffix] = np.array([o.item() for o in out], dtype=np.float64 if suffix else np.float32)
        print(name, suffix or "fp32", [float(v) for v in values["values" + suffix]])
    mga.save(name, dict(source=source, names=list(loss_cpu.NAMES), pitch=meta["pitch"], energy=meta["energy"], B=meta["B"], L=meta["L"],
                        T=meta["T"], n_layer=meta["n_layer"]), **values)


if __name__ == "__main__":
    make("loss_tiny", "teacher_tiny")
    make("loss_tiny_phoneme_level", "teacher_tiny_phoneme_level")
