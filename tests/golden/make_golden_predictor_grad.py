#!/usr/bin/env python3
"""Golden gradients of the VariancePredictor — runs ONLY where the reference lives read-only at /root/reference (the import recipe of
make_golden_aligner.py).  It imports the reference's ``model.modules.VariancePredictor``, builds it from a config with ``dropout`` set
to 0.0, keeps it in ``train()``, loads seeded weights (tests/predictor_grad_cpu.seeded_weights), and runs ``pred = module(x, mask)``,
``(g * pred).sum().backward()`` — once in fp32 and once with the same weights and inputs cast to float64.  The upstream gradient g is
nonzero at masked positions too.  Two small configs (K = 3): hidden = filter = 32, and hidden 48 -> filter 32; B = 4, S = 9, lens
[9, 0, 5, 9].

    python tests/golden/make_golden_predictor_grad.py

predictor_grad_tiny.npz    per config c in (a, b): {c}_x, {c}_g, {c}_mask, the ten weights {c}_w_*, {c}_pred, and the ten parameter
                           gradients + dx of the reference's own autograd as {c}_d_* (fp32) and {c}_d_*_f64
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import predictor_grad_cpu as pc  # noqa: E402

B, S, LENS, K = 4, 9, [9, 0, 5, 9], 3
CONFIGS = {"a": (32, 32), "b": (48, 32)}  # name -> (encoder_hidden, filter_size)
KEYS = {"w1": "conv_layer.conv1d_1.conv.weight", "b1": "conv_layer.conv1d_1.conv.bias", "g1": "conv_layer.layer_norm_1.weight",
        "be1": "conv_layer.layer_norm_1.bias", "w2": "conv_layer.conv1d_2.conv.weight", "b2": "conv_layer.conv1d_2.conv.bias",
        "g2": "conv_layer.layer_norm_2.weight", "be2": "conv_layer.layer_norm_2.bias", "wlin": "linear_layer.weight", "blin": "linear_layer.bias"}


def make():
    from model.modules import VariancePredictor  # the reference class

    arrays = {}
    for i, (c, (hidden, filt)) in enumerate(CONFIGS.items()):
        cfg = {"transformer": {"encoder_hidden": hidden}, "variance_predictor": {"filter_size": filt, "kernel_size": K, "dropout": 0.0}}
        w = pc.seeded_weights(hidden, filt, K, seed=20 + i)
        rs = np.random.RandomState(40 + i)
        x = rs.standard_normal((B, S, hidden)).astype(np.float32)
        g = rs.standard_normal((B, S)).astype(np.float32)
        mask = pc.mask_of(LENS, S)
        ref = VariancePredictor(cfg).train()
        sd = {KEYS[k]: torch.as_tensor(np.asarray(v)).reshape(ref.state_dict()[KEYS[k]].shape) for k, v in w.items()}
        ref.load_state_dict(sd)
        arrays.update({f"{c}_x": x, f"{c}_g": g, f"{c}_mask": mask})
        arrays.update({f"{c}_w_{k}": np.asarray(v) for k, v in w.items()})
        for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
            m = copy.deepcopy(ref).to(dtype).train()
            xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
            pred = m(xt, torch.from_numpy(mask))
            assert pred.dtype == dtype and pred.shape == (B, S)
            (torch.from_numpy(g).to(dtype) * pred).sum().backward()
            arrays[f"{c}_pred{suffix}"] = pred.detach().numpy()
            named = dict(m.named_parameters())
            for k in pc.NAMES[:10]:
                arrays[f"{c}_d_{k}{suffix}"] = named[KEYS[k]].grad.numpy().reshape(np.asarray(w[k]).shape)
            arrays[f"{c}_d_dx{suffix}"] = xt.grad.numpy()
        print(c, {k: float(np.abs(arrays[f"{c}_d_{k}"]).max()) for k in pc.NAMES})
    mga.save("predictor_grad_tiny", dict(B=B, S=S, lens=LENS, K=K, configs={c: list(v) for c, v in CONFIGS.items()}, names=list(pc.NAMES)), **arrays)


if __name__ == "__main__":
    make()
