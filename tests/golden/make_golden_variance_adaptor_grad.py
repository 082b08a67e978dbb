#!/usr/bin/env python3
"""Golden outputs and gradients of the VarianceAdaptor's teacher-forced branch — runs ONLY where the reference lives read-only at
/root/reference (the import recipe of make_golden_aligner.py).  It imports the reference's ``model.modules.VarianceAdaptor``, builds it
at encoder_hidden 32, filter 256, kernel 3, n_bins 8 (a temporary ``stats.json`` stands in for the preprocessed data; the bin edges
are then loaded with the weights), loads the seeded weights of tests/variance_adaptor_grad_cpu.synth_weights with ``strict=True`` and
runs, in ``eval()`` (no dropout), the forward with all three targets followed by

    torch.autograd.backward([x_out, pitch, energy, log_d], [g_out, g_pitch, g_energy, g_log_d])

once in fp32 and once with the same weights and inputs cast to float64, for the four mixes of phoneme_level / frame_level.

B = 3, L = 7, src_lens [7, 4, 5], max_len T = 12 with totals [14, 9, 6]: utterance 0 is cropped by two frames, 1 and 2 are padded.
The durations hold zeros at valid phonemes (a leading one too); every target array holds one value below the first edge, one above
the last and one exactly on an edge.

    python tests/golden/make_golden_variance_adaptor_grad.py

variance_adaptor_grad_tiny.npz   the inputs (both levels of every target and gradient: tests/variance_adaptor_grad_cpu.synth_inputs)
                                 and per mix m in (pp, pf, fp, ff): {m}_{name} as fp32 and {m}_{name}_f64 for the names of
                                 FIXTURE_NAMES — y, the three predictions, dx, both d_embedding.weight and, of each predictor, only
                                 d linear_layer.weight and d conv1d_1 bias — and {m}_mel_len.  No weights: both sides draw them from
                                 the seed.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402
from tests import variance_adaptor_grad_cpu as vc  # noqa: E402

CFG = vc.config(d=32, F=256, K=3, n_bins=8)
B, L, T, SRC_LENS = 3, 7, 12, [7, 4, 5]
DURATION = [[0, 3, 2, 0, 4, 1, 4], [2, 0, 3, 4, 0, 0, 0], [1, 1, 0, 2, 2, 0, 0]]  # totals 14 (cropped at 12), 9, 6
WEIGHT_SEED, INPUT_SEED = 41, 42


def inputs(w):
    z = vc.synth_inputs(CFG, B, L, T, SRC_LENS, INPUT_SEED)
    z["duration"] = np.asarray(DURATION, dtype=np.int64)
    mel_mask = np.arange(T)[None, :] >= z["duration"].sum(1)[:, None]
    for s in ("pitch", "energy"):
        z[f"{s}_t_f"][mel_mask] = 0.0
        for c in "pf":  # below the first edge, above the last, exactly on an edge — at valid positions of utterance 0
            t, bins = z[f"{s}_t_{c}"], w[f"{s}_bins"]
            t[0, 1], t[0, 2], t[0, 3] = bins[0] - 3.0, bins[-1] + 3.0, bins[3]
    return z


def model_config():
    mc = wl.model_config("tiny")
    mc["transformer"]["encoder_hidden"] = CFG["d"]
    mc["variance_predictor"].update(filter_size=CFG["F"], kernel_size=CFG["K"])
    mc["variance_embedding"]["n_bins"] = CFG["n_bins"]
    return mc


def make():
    from model.modules import VarianceAdaptor  # the reference class

    w = vc.synth_weights(CFG, WEIGHT_SEED)
    z = inputs(w)
    arrays = dict(z)
    sd = vc.state_dict(w)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "stats.json"), "w") as f:
            json.dump(wl.SYNTH_STATS, f)
        for mix in vc.MIXES:
            pc = wl.preprocess_config(vc.LEVEL[mix[0]], vc.LEVEL[mix[1]])
            pc["path"]["preprocessed_path"] = tmp
            inp = vc.inputs_for(z, mix)
            for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
                m = VarianceAdaptor(pc, model_config())
                m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})  # strict
                m = m.to(dtype).eval()
                x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
                src_mask = torch.arange(L)[None] >= torch.from_numpy(inp["src_lens"])[:, None]
                mel_mask = torch.arange(T)[None] >= torch.from_numpy(inp["duration"]).sum(1)[:, None]
                y, p, e, log_d, d_r, mel_len, mm = m(x, src_mask, mel_mask, T, torch.from_numpy(inp["pitch_t"]).to(dtype),
                                                     torch.from_numpy(inp["energy_t"]).to(dtype), torch.from_numpy(inp["duration"]))
                assert y.dtype == dtype and y.shape == (B, T, CFG["d"]) and mm is mel_mask
                torch.autograd.backward([y, p, e, log_d], [torch.from_numpy(inp[k]).to(dtype) for k in ("g_out", "g_pitch", "g_energy", "g_log_d")])
                named = dict(m.named_parameters())
                got = dict(y=y, pitch=p, energy=e, log_d=log_d, dx=x.grad)
                for name in vc.FIXTURE_NAMES[5:]:
                    got[name] = named[vc.grad_key(name)].grad
                for name in vc.FIXTURE_NAMES:
                    arrays[f"{mix}_{name}{suffix}"] = got[name].detach().numpy()
                arrays[f"{mix}_mel_len"] = mel_len.numpy()
            print(mix, {k: float(np.abs(arrays[f"{mix}_{k}"]).max()) for k in vc.FIXTURE_NAMES})
    mga.save("variance_adaptor_grad_tiny", dict(B=B, L=L, T=T, src_lens=SRC_LENS, cfg=CFG, seeds=[WEIGHT_SEED, INPUT_SEED], mixes=list(vc.MIXES),
                                                names=list(vc.FIXTURE_NAMES)), **arrays)


if __name__ == "__main__":
    make()
