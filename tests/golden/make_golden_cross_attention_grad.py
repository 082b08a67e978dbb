#!/usr/bin/env python3
"""Golden gradients of the cross-attention sublayer — runs ONLY where the reference lives read-only at /root/reference (the import
recipe of make_golden_aligner.py).  It imports the reference's ``transformer.SubLayers.MultiHeadAttention``, builds it with
``dropout=0.0``, keeps it in ``train()``, loads seeded weights (tests/attention_grad_cpu.seeded_weights), and runs
``y, attn = module(tgt, src, src, mask=mask)`` as FFTBlock2.crs_attn does (transformer/Layers.py:61-64) with the key-padding mask
``mask[b, t, l] = l >= src_lens[b]``, then ``((g * y).sum() + (a * attn).sum()).backward()`` — once in fp32 and once with the same
weights and inputs cast to float64.  g is nonzero on every query row.  Two variants of the map's upstream gradient: ``h0`` nonzero on
head 0 only (what the guided-attention loss gives), ``all`` nonzero on every head.
Two small configs: d = 32 with H = 2 and H = 4; B = 3, T = 9, L = 7, src_lens [7, 1, 4] (no zero length: the reference's softmax over
an all -inf row is NaN).

    python tests/golden/make_golden_cross_attention_grad.py

cross_attention_grad_tiny.npz    per config c in (a, b): {c}_tgt, {c}_src, {c}_g, {c}_a_h0, {c}_a_all, the ten weights {c}_w_*, {c}_y,
                                 {c}_attn [B, H, T, L], and per variant v the ten parameter gradients + dtgt + dsrc of the reference's own
                                 autograd as {c}_{v}_d_* (fp32) and {c}_{v}_d_*_f64; {c}_y_f64, {c}_attn_f64
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import cross_attention_grad_cpu as xc  # noqa: E402

B, T, L, LENS, D = 3, 9, 7, [7, 1, 4], 32
CONFIGS = {"a": 2, "b": 4}  # name -> n_head
KEYS = {"wq": "w_qs.weight", "bq": "w_qs.bias", "wk": "w_ks.weight", "bk": "w_ks.bias", "wv": "w_vs.weight", "bv": "w_vs.bias",
        "wfc": "fc.weight", "bfc": "fc.bias", "ln_g": "layer_norm.weight", "ln_b": "layer_norm.bias"}


def make():
    from transformer.SubLayers import MultiHeadAttention  # the reference class

    arrays = {}
    for i, (c, H) in enumerate(CONFIGS.items()):
        w = xc.seeded_weights(D, seed=160 + i)
        rs = np.random.RandomState(180 + i)
        tgt = rs.standard_normal((B, T, D)).astype(np.float32)
        src = rs.standard_normal((B, L, D)).astype(np.float32)
        g = rs.standard_normal((B, T, D)).astype(np.float32)
        a_all = rs.standard_normal((B, H, T, L)).astype(np.float32)
        a_h0 = a_all.copy()
        a_h0[:, 1:] = 0.0
        mask = xc.key_mask(LENS, L).expand(B, T, L)
        ref = MultiHeadAttention(H, D, D // H, D // H, dropout=0.0).train()
        ref.load_state_dict({KEYS[k]: torch.as_tensor(np.asarray(v)) for k, v in w.items()})
        arrays.update({f"{c}_tgt": tgt, f"{c}_src": src, f"{c}_g": g, f"{c}_a_h0": a_h0, f"{c}_a_all": a_all})
        arrays.update({f"{c}_w_{k}": np.asarray(v) for k, v in w.items()})
        for v, a in (("h0", a_h0), ("all", a_all)):
            for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
                m = copy.deepcopy(ref).to(dtype).train()
                tt = torch.from_numpy(tgt).to(dtype).requires_grad_(True)
                st = torch.from_numpy(src).to(dtype).requires_grad_(True)
                y, attn = m(tt, st, st, mask=mask)
                assert y.dtype == dtype and y.shape == (B, T, D) and attn.shape == (B, H, T, L)
                ((torch.from_numpy(g).to(dtype) * y).sum() + (torch.from_numpy(a).to(dtype) * attn).sum()).backward()
                arrays[f"{c}_y{suffix}"] = y.detach().numpy()
                arrays[f"{c}_attn{suffix}"] = attn.detach().numpy()
                named = dict(m.named_parameters())
                for k in xc.NAMES[:10]:
                    arrays[f"{c}_{v}_d_{k}{suffix}"] = named[KEYS[k]].grad.numpy()
                arrays[f"{c}_{v}_d_dtgt{suffix}"] = tt.grad.numpy()
                arrays[f"{c}_{v}_d_dsrc{suffix}"] = st.grad.numpy()
            print(c, v, {k: float(np.abs(arrays[f"{c}_{v}_d_{k}"]).max()) for k in xc.NAMES})
    mga.save("cross_attention_grad_tiny", dict(B=B, T=T, L=L, lens=LENS, d=D, configs=dict(CONFIGS), variants=["h0", "all"], names=list(xc.NAMES)),
             **arrays)


if __name__ == "__main__":
    make()
