#!/usr/bin/env python3
"""Golden gradients of the position-wise feed-forward sublayer and of one FFT block — runs ONLY where the reference lives read-only at
/root/reference (the import recipe of make_golden_aligner.py).  It imports the reference's ``transformer.SubLayers.PositionwiseFeedForward``
and ``transformer.Layers.FFTBlock``, builds them with ``dropout=0.0``, keeps them in ``train()``, loads seeded weights
(tests/ffn_grad_cpu.seeded_weights, tests/attention_grad_cpu.seeded_weights) and runs the forward, then ``(g * y).sum().backward()`` —
once in fp32 and once with the same weights and inputs cast to float64.

PositionwiseFeedForward: d = 32, d_hid = 64, kernel sizes (9, 1) and (3, 3); B = 4, S = 9, so that with K1 = 9 every tap leaves the
utterance somewhere.  FFTBlock: d = 32, H = 2, d_inner = 64, (9, 1), lens [9, 1, 5, 9], with both masks (mask[b, t] = t >= lens[b],
slf_attn_mask[b, i, j] = j >= lens[b]); the upstream gradient is nonzero on padded rows too.

    python tests/golden/make_golden_ffn_grad.py

ffn_grad_tiny.npz    per feed-forward config c in (a, b): {c}_x, {c}_g, {c}_y, and the six parameter gradients + dx of the reference's
                     own autograd as {c}_d_* (fp32) and {c}_d_*_f64; for the block: blk_x, blk_g, blk_y, blk_d_a_* (attention),
                     blk_d_f_* (feed-forward), blk_d_dx, each with its _f64 twin.  The weights are not stored: the meta record holds
                     the seeds of seeded_weights (numpy's RandomState stream is fixed), which keeps the file well below the size limit
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden_attention_grad import KEYS as ATTN_KEYS  # noqa: E402
from tests import attention_grad_cpu as ac  # noqa: E402
from tests import ffn_grad_cpu as fc  # noqa: E402

B, S, LENS, D, D_HID, H = 4, 9, [9, 1, 5, 9], 32, 64, 2
CONFIGS = {"a": (9, 1), "b": (3, 3)}  # name -> kernel sizes
SEEDS = {"a": 160, "b": 161, "blk_attn": 170, "blk_ffn": 171}  # of the seeded weights: the fixture stores the seeds, not the weights
KEYS = {"w1": "w_1.weight", "b1": "w_1.bias", "w2": "w_2.weight", "b2": "w_2.bias", "ln_g": "layer_norm.weight", "ln_b": "layer_norm.bias"}


def _both(arrays, prefix, ref, run, grads_of):
    """runs ``run(module, dtype) -> (y, x leaf)`` in fp32 and float64 and records y and the gradients ``grads_of(module)`` names"""
    for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
        m = copy.deepcopy(ref).to(dtype).train()
        y, xt, g = run(m, dtype)
        (g * y).sum().backward()
        arrays[f"{prefix}_y{suffix}"] = y.detach().numpy()
        for name, p in grads_of(m).items():
            arrays[f"{prefix}_d_{name}{suffix}"] = p.grad.numpy()
        arrays[f"{prefix}_d_dx{suffix}"] = xt.grad.numpy()


def make():
    from transformer.Layers import FFTBlock  # the reference classes
    from transformer.SubLayers import PositionwiseFeedForward

    arrays = {}
    for i, (c, ks) in enumerate(CONFIGS.items()):
        w = fc.seeded_weights(D, D_HID, ks[0], ks[1], seed=SEEDS[c])
        rs = np.random.RandomState(180 + i)
        x = rs.standard_normal((B, S, D)).astype(np.float32)
        g = rs.standard_normal((B, S, D)).astype(np.float32)
        ref = PositionwiseFeedForward(D, D_HID, list(ks), dropout=0.0).train()
        ref.load_state_dict({KEYS[k]: torch.as_tensor(np.asarray(v)) for k, v in w.items()})
        arrays.update({f"{c}_x": x, f"{c}_g": g})

        def run(m, dtype, x=x, g=g):
            xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
            y = m(xt)
            assert y.dtype == dtype and y.shape == (B, S, D)
            return y, xt, torch.from_numpy(g).to(dtype)

        _both(arrays, c, ref, run, lambda m: {k: dict(m.named_parameters())[KEYS[k]] for k in fc.NAMES[:6]})
        print(c, {k: float(np.abs(arrays[f"{c}_d_{k}"]).max()) for k in fc.NAMES})

    wa, wf = ac.seeded_weights(D, seed=SEEDS["blk_attn"]), fc.seeded_weights(D, D_HID, 9, 1, seed=SEEDS["blk_ffn"])
    rs = np.random.RandomState(190)
    x = rs.standard_normal((B, S, D)).astype(np.float32)
    g = rs.standard_normal((B, S, D)).astype(np.float32)
    ref = FFTBlock(D, H, D // H, D // H, D_HID, [9, 1], dropout=0.0).train()
    sd = {"slf_attn." + ATTN_KEYS[k]: torch.as_tensor(np.asarray(v)) for k, v in wa.items()}
    sd.update({"pos_ffn." + KEYS[k]: torch.as_tensor(np.asarray(v)) for k, v in wf.items()})
    ref.load_state_dict(sd)
    mask = torch.as_tensor(np.arange(S)[None, :] >= np.asarray(LENS)[:, None])
    slf_attn_mask = ac.key_mask(LENS, S).expand(B, S, S)
    arrays.update({"blk_x": x, "blk_g": g})

    def run_block(m, dtype):
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        y, _ = m(xt, mask=mask, slf_attn_mask=slf_attn_mask)
        assert y.dtype == dtype and y.shape == (B, S, D)
        return y, xt, torch.from_numpy(g).to(dtype)

    def block_grads(m):
        named = dict(m.named_parameters())
        out = {f"a_{k}": named["slf_attn." + ATTN_KEYS[k]] for k in ac.NAMES[:10]}
        out.update({f"f_{k}": named["pos_ffn." + KEYS[k]] for k in fc.NAMES[:6]})
        return out

    _both(arrays, "blk", ref, run_block, block_grads)
    mga.save("ffn_grad_tiny", dict(B=B, S=S, lens=LENS, d=D, d_hid=D_HID, H=H, configs={c: list(ks) for c, ks in CONFIGS.items()},
                                   block_kernel=[9, 1], seeds=dict(SEEDS), names=list(fc.NAMES), attention_names=list(ac.NAMES)), **arrays)


if __name__ == "__main__":
    make()
