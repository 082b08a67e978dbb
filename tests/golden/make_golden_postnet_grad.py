#!/usr/bin/env python3
"""Golden outputs, gradients and BatchNorm buffers of the PostNet — runs ONLY where the reference lives read-only at /root/reference
(the import recipe of make_golden_aligner.py).  It imports the reference's ``transformer.Layers.PostNet``, builds ``PostNet(16, 32, 5, 3)``,
loads seeded weights with non-trivial running statistics (tests/postnet_grad_cpu.seeded_weights), and runs ``y = module(x)`` followed
by ``(g * y).sum().backward()`` — once in fp32 and once with the same weights and inputs cast to float64 — in two modes:

  train()  the reference ties its dropout to ``self.training``; for the duration of the call ``torch.nn.functional.dropout`` is
           replaced by a function that applies recorded, seeded keep-masks as ``x * keep / (1 - p)``.  The masks are stored.
  eval()   running statistics, no dropout.

B = 3, T = 7 (lens [7, 4, 5] are stored for the yardstick's valid-rows mutant; the module itself sees no mask).

    python tests/golden/make_golden_postnet_grad.py

postnet_grad_tiny.npz   x, g, keep0 .. keep2, the weights and buffers before the call as w_*, and per mode m in (train, eval):
                        {m}_y, {m}_d_* (the 4 n parameter gradients and dx) as fp32 and *_f64; train_rm{i}, train_rv{i}, train_nbt{i}:
                        the buffers after the train-mode call
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import postnet_grad_cpu as pc  # noqa: E402

N_MEL, EMB, K, N = 16, 32, 5, 3
B, T, LENS, P = 3, 7, [7, 4, 5], 0.5
# Seeds chosen on the CPU so that the yardstick's mutants stay sharp on this fixture: of weight seeds 250, 253, ..., 289 (inputs and masks at
# +1, +2) this one has the largest smallest mutant share, 25 (eps_outside_sqrt, the mildest mistake: it moves rstd by about 5e-6 relative).
WEIGHT_SEED, INPUT_SEED, MASK_SEED = 259, 260, 261


def state_dict(w, dtype):
    sd = {}
    for i in range(N):
        for q, key in (("w", "0.conv.weight"), ("b", "0.conv.bias"), ("g", "1.weight"), ("be", "1.bias"), ("rm", "1.running_mean"), ("rv", "1.running_var")):
            sd[f"convolutions.{i}.{key}"] = torch.as_tensor(np.asarray(w[f"{q}{i}"])).to(dtype)
        sd[f"convolutions.{i}.1.num_batches_tracked"] = torch.as_tensor(np.asarray(w[f"nbt{i}"]))
    return sd


def make():
    from transformer.Layers import PostNet  # the reference class

    w = pc.seeded_weights(N_MEL, EMB, K, N, WEIGHT_SEED)
    rs = np.random.RandomState(INPUT_SEED)
    x = rs.standard_normal((B, T, N_MEL)).astype(np.float32)
    g = rs.standard_normal((B, T, N_MEL)).astype(np.float32)
    keeps = pc.keep_masks(B, T, N_MEL, EMB, N, P, MASK_SEED)
    arrays = {"x": x, "g": g}
    arrays.update({f"keep{i}": k for i, k in enumerate(keeps)})
    arrays.update({f"w_{k}": np.asarray(v) for k, v in w.items()})
    real_dropout = torch.nn.functional.dropout
    for mode in ("train", "eval"):
        for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
            m = PostNet(N_MEL, EMB, K, N).to(dtype)
            m.load_state_dict(state_dict(w, dtype))  # strict
            m.train(mode == "train")
            queue = list(keeps)

            def recorded(t, p=0.5, training=True, inplace=False):
                assert training and p == P
                k = torch.from_numpy(queue.pop(0)).to(t.dtype).transpose(1, 2)  # the module runs on [B, C, T]
                return t * k / (1 - p)

            xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
            if mode == "train":
                torch.nn.functional.dropout = recorded
            try:
                y = m(xt)
            finally:
                torch.nn.functional.dropout = real_dropout
            assert y.dtype == dtype and y.shape == (B, T, N_MEL) and (mode == "eval" or not queue)
            (torch.from_numpy(g).to(dtype) * y).sum().backward()
            arrays[f"{mode}_y{suffix}"] = y.detach().numpy()
            named = dict(m.named_parameters())
            for i in range(N):
                for q, key in (("w", "0.conv.weight"), ("b", "0.conv.bias"), ("g", "1.weight"), ("be", "1.bias")):
                    arrays[f"{mode}_d_{q}{i}{suffix}"] = named[f"convolutions.{i}.{key}"].grad.numpy()
                bn = m.convolutions[i][1]
                if mode == "train":
                    arrays[f"train_rm{i}{suffix}"] = bn.running_mean.detach().numpy()
                    arrays[f"train_rv{i}{suffix}"] = bn.running_var.detach().numpy()
                    arrays[f"train_nbt{i}{suffix}"] = bn.num_batches_tracked.numpy()
                else:
                    assert torch.equal(bn.running_mean, torch.as_tensor(w[f"rm{i}"]).to(dtype)) and int(bn.num_batches_tracked) == int(w[f"nbt{i}"])
            arrays[f"{mode}_d_dx{suffix}"] = xt.grad.numpy()
        print(mode, {k: float(np.abs(arrays[f"{mode}_d_{k}"]).max()) for k in pc.grad_names(N)})
    mga.save("postnet_grad_tiny", dict(B=B, T=T, lens=LENS, n_mel=N_MEL, emb=EMB, K=K, n=N, p=P, seeds=[WEIGHT_SEED, INPUT_SEED, MASK_SEED],
                                       names=list(pc.grad_names(N))), **arrays)


if __name__ == "__main__":
    make()
