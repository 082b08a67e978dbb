#!/usr/bin/env python3
"""Golden gradients of the Gaussian length regulator — runs ONLY where the reference lives read-only at /root/reference (the import
recipe of make_golden_aligner.py).  Two parts, both from the reference's own ``model.modules.GaussianUpsampling`` under torch's autograd,
once in fp32 and once in float64:

  plain    the module alone in its plain form (rows past an utterance's own length NOT zeroed) on the case
           "odd_L_partial_tile 2x7x24" of tests/gaussian_grad_cpu.CASES (B 2, L 7, D 24): out, w, and d_x of (g out).sum()
  adaptor  the reference's ``VarianceAdaptor`` with that module wired where it instantiates ``LengthRegulator``, exactly as
           make_golden.gaussian_wired_case wires it (mel_len = the sum of the durations, frames at or past it zeroed), in ``eval()``
           (dropout 0), teacher-forced, at the configuration and seeded weights of make_golden_variance_adaptor_grad.py, B 2, L 7,
           src_lens [7, 4], T 20 with totals [17, 11], for the two mixed mixes MIXES = (pf, fp) — each has a predictor and an
           embedding on either side of the regulator, and two mixes keep the file at half the hard regulator's: per mix m the tensors
           of variance_adaptor_grad_cpu.FIXTURE_NAMES as {m}_{name} (fp32) and {m}_{name}_f64, and {m}_mel_len

    python tests/golden/make_golden_gaussian_grad.py

gaussian_grad_tiny.npz holds numbers only; no weights: both sides draw them from the seed."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_aligner as mga  # noqa: E402  (sets up sys.path and the stub modules the reference's imports need)
import make_golden_variance_adaptor_grad as mva  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402
from tests import gaussian_grad_cpu as gg  # noqa: E402
from tests import variance_adaptor_grad_cpu as vc  # noqa: E402

PLAIN_CASE = "odd_L_partial_tile 2x7x24"
CFG = mva.CFG
B, L, T, SRC_LENS = 2, 7, 20, [7, 4]
DURATION = [[2, 0, 5, 1, 3, 4, 2], [3, 6, 0, 2, 0, 0, 0]]  # totals 17 and 11: both padded at T = 20
WEIGHT_SEED, INPUT_SEED = mva.WEIGHT_SEED, 52
MIXES = ("pf", "fp")


def plain(arrays):
    import model.modules as mm

    mm.device = torch.device("cpu")
    x, d, own_len, g = gg.CASES[PLAIN_CASE]()
    assert own_len is None and x.shape == (2, 7, 24)
    arrays.update(plain_x=x, plain_d=d, plain_g=g)
    for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        out, s, w = mm.GaussianUpsampling()(xt, torch.from_numpy(d).to(dtype), torch.ones(2, 7), None)
        assert out.dtype == dtype and out.shape == g.shape
        out.backward(torch.from_numpy(g).to(dtype))
        arrays.update({f"plain_out{suffix}": out.detach().numpy(), f"plain_w{suffix}": w.detach().numpy(), f"plain_dx{suffix}": xt.grad.numpy()})


def wired():
    import model.modules as mm

    mm.device = torch.device("cpu")
    gu = mm.GaussianUpsampling()

    class Wired(torch.nn.Module):  # make_golden.gaussian_wired_case's three wiring lines, the integer targets cast to x's type first
        def forward(self, x, duration, max_len):
            duration = duration.to(x.dtype)
            out, s, _ = gu(x, duration, torch.ones_like(duration), max_len)
            mel_len = s.reshape(-1).long()
            pad = torch.arange(out.shape[1])[None, :] >= mel_len[:, None]
            return out.masked_fill(pad.unsqueeze(-1), 0.0), mel_len

    return Wired()


def adaptor(arrays):
    from model.modules import VarianceAdaptor  # the reference class

    w = vc.synth_weights(CFG, WEIGHT_SEED)
    z = vc.synth_inputs(CFG, B, L, T, SRC_LENS, INPUT_SEED)
    z["duration"] = np.asarray(DURATION, dtype=np.int64)
    mel_mask = np.arange(T)[None, :] >= z["duration"].sum(1)[:, None]
    for s in ("pitch", "energy"):
        z[f"{s}_t_f"][mel_mask] = 0.0
    arrays.update(z)
    sd = vc.state_dict(w)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "stats.json"), "w") as f:
            json.dump(wl.SYNTH_STATS, f)
        for mix in MIXES:
            pc = wl.preprocess_config(vc.LEVEL[mix[0]], vc.LEVEL[mix[1]])
            pc["path"]["preprocessed_path"] = tmp
            inp = vc.inputs_for(z, mix)
            for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
                m = VarianceAdaptor(pc, mva.model_config())
                m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})  # strict
                m = m.to(dtype).eval()
                m.length_regulator = wired()
                x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
                src_mask = torch.arange(L)[None] >= torch.from_numpy(inp["src_lens"])[:, None]
                mm_ = torch.from_numpy(mel_mask)
                y, p, e, log_d, d_r, mel_len, _ = m(x, src_mask, mm_, T, torch.from_numpy(inp["pitch_t"]).to(dtype),
                                                    torch.from_numpy(inp["energy_t"]).to(dtype), torch.from_numpy(inp["duration"]))
                assert y.dtype == dtype and y.shape == (B, T, CFG["d"])
                torch.autograd.backward([y, p, e, log_d], [torch.from_numpy(inp[k]).to(dtype) for k in ("g_out", "g_pitch", "g_energy", "g_log_d")])
                named = dict(m.named_parameters())
                got = dict(y=y, pitch=p, energy=e, log_d=log_d, dx=x.grad)
                for name in vc.FIXTURE_NAMES[5:]:
                    got[name] = named[vc.grad_key(name)].grad
                for name in vc.FIXTURE_NAMES:
                    arrays[f"{mix}_{name}{suffix}"] = got[name].detach().numpy()
                arrays[f"{mix}_mel_len"] = mel_len.numpy()
            print(mix, {k: float(np.abs(arrays[f"{mix}_{k}"]).max()) for k in vc.FIXTURE_NAMES})


def make():
    arrays = {}
    plain(arrays)
    adaptor(arrays)
    mga.save("gaussian_grad_tiny", dict(plain_case=PLAIN_CASE, B=B, L=L, T=T, src_lens=SRC_LENS, cfg=CFG, seeds=[WEIGHT_SEED, INPUT_SEED],
                                        mixes=list(MIXES), names=list(vc.FIXTURE_NAMES)), **arrays)


if __name__ == "__main__":
    make()
