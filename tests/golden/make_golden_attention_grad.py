#!/usr/bin/env python3
"""Golden gradients of the self-attention sublayer — runs ONLY where the reference lives read-only at /root/reference (the import
recipe of make_golden_aligner.py).  It imports the reference's ``transformer.SubLayers.MultiHeadAttention``, builds it with
``dropout=0.0``, keeps it in ``train()``, loads seeded weights (tests/attention_grad_cpu.seeded_weights), and runs
``y, attn = module(x, x, x, mask=mask)`` with the key-padding mask ``mask[b, i, j] = j >= lens[b]``, then ``(g * y).sum().backward()`` —
once in fp32 and once with the same weights and inputs cast to float64.  The upstream gradient g is nonzero on padded query rows too.
Two small configs: d = 32 with H = 2 and H = 4; B = 4, S = 9, lens [9, 1, 5, 9] (no zero length: the reference's softmax over an
all -inf row is NaN, and so would every weight gradient be).

    python tests/golden/make_golden_attention_grad.py

attention_grad_tiny.npz    per config c in (a, b): {c}_x, {c}_g, the ten weights {c}_w_*, {c}_y, and the ten parameter gradients + dx of
                           the reference's own autograd as {c}_d_* (fp32) and {c}_d_*_f64
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import attention_grad_cpu as ac  # noqa: E402

B, S, LENS, D = 4, 9, [9, 1, 5, 9], 32
CONFIGS = {"a": 2, "b": 4}  # name -> n_head
KEYS = {"wq": "w_qs.weight", "bq": "w_qs.bias", "wk": "w_ks.weight", "bk": "w_ks.bias", "wv": "w_vs.weight", "bv": "w_vs.bias",
        "wfc": "fc.weight", "bfc": "fc.bias", "ln_g": "layer_norm.weight", "ln_b": "layer_norm.bias"}


def make():
    from transformer.SubLayers import MultiHeadAttention  # the reference class

    arrays = {}
    for i, (c, H) in enumerate(CONFIGS.items()):
        w = ac.seeded_weights(D, seed=60 + i)
        rs = np.random.RandomState(80 + i)
        x = rs.standard_normal((B, S, D)).astype(np.float32)
        g = rs.standard_normal((B, S, D)).astype(np.float32)
        mask = ac.key_mask(LENS, S).expand(B, S, S)
        ref = MultiHeadAttention(H, D, D // H, D // H, dropout=0.0).train()
        ref.load_state_dict({KEYS[k]: torch.as_tensor(np.asarray(v)) for k, v in w.items()})
        arrays.update({f"{c}_x": x, f"{c}_g": g})
        arrays.update({f"{c}_w_{k}": np.asarray(v) for k, v in w.items()})
        for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
            m = copy.deepcopy(ref).to(dtype).train()
            xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
            y, attn = m(xt, xt, xt, mask=mask)
            assert y.dtype == dtype and y.shape == (B, S, D) and attn.shape == (B, H, S, S)
            (torch.from_numpy(g).to(dtype) * y).sum().backward()
            arrays[f"{c}_y{suffix}"] = y.detach().numpy()
            named = dict(m.named_parameters())
            for k in ac.NAMES[:10]:
                arrays[f"{c}_d_{k}{suffix}"] = named[KEYS[k]].grad.numpy()
            arrays[f"{c}_d_dx{suffix}"] = xt.grad.numpy()
        print(c, {k: float(np.abs(arrays[f"{c}_d_{k}"]).max()) for k in ac.NAMES})
    mga.save("attention_grad_tiny", dict(B=B, S=S, lens=LENS, d=D, configs=dict(CONFIGS), names=list(ac.NAMES)), **arrays)


if __name__ == "__main__":
    make()
