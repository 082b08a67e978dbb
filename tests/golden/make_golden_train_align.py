#!/usr/bin/env python3
"""Golden predictions, losses and gradients of one training step of the whole model — runs ONLY where the reference is checked out
(make_golden_aligner.REF; the import recipe of make_golden_aligner.py).  It imports the reference's
``model.fastspeech2_align.FastSpeech2Align`` and ``model.loss.FastSpeech2Loss``, builds the model in ``train()`` with every dropout at
0 — the config's three rates, ``mel_encoder.prenet.dropout.p`` set on the instance, and PostNet's hard-coded ``F.dropout`` replaced by
the identity while the forward runs (the device of make_golden_postnet_grad.py; no reference file is changed) — sets the INSTANCE's
``_calculate_duration`` (undefined in the reference) to ``make_golden_teacher.duration_rule``, and runs

    out = model(speakers, texts, src_lens, max_src_len, mels, mel_lens, max_mel_len, p_targets, e_targets)
    losses = FastSpeech2Loss(...)(batch, out);  losses[0].backward()

once in fp32 and once cast to ``.double()``, the float64 run's durations forced to the fp32 run's.

Config: d 256, 2 heads, 1 encoder layer, 4 decoder layers (the loss reads the maps 0-3), conv_filter_size 256 (the narrowest the
trainable PositionwiseFeedForward takes: the GPU test runs this very config), kernels (3, 1), predictor filter 256 / kernel 3,
max_seq_len 32; B = 2, L = 7 with lengths [7, 4], T = 20 with lengths [20, 13].

Two discrete hazards are checked here, on the CPU, and recorded in ``meta``; (aligner seed, input seed) pairs are searched until both
hold: the smallest float64 top-two gap of the head-summed last map is at least 1000 x that map's fp32-vs-float64 distance (the argmax
of the duration rule), and min |prediction - target| over the valid mel / PostNet elements is at least 1000 x that prediction's
fp32-vs-float64 distance (the sign in the L1 gradient).  A third condition guards the three one-element gradients (``linear_layer.bias`` of
the duration, pitch and energy predictor), whose gate is made from ONE sample of the reference's fp32 error: d_b = (2 / N) sum (pred -
target) over the N valid positions, so its fp32 error is the mean of N prediction errors times 2, about 2 rms(pred fp32 - pred float64)
/ sqrt(N); a recorded distance below that single standard deviation means the reference's fp32 value happened to land next to the
float64 one, and twice it would understate what any other fp32 evaluation of the same sum is off by.  Such a seed is passed over.

    python tests/golden/make_golden_train_align.py

train_align_tiny.npz   the five predictions and the seven loss values in fp32 and (suffix _f64) float64, d_targets, and in float64:
                       every 1-D parameter gradient, mel_linear.weight's whole gradient, rows ROWS = {0, 1, 127, 255} of one weight
                       gradient per stack (g__<name>, dots as in the state dict).  The fp32 run's gradients are not stored: meta
                       ["grad_dist"] holds max |fp32 - float64| per stored gradient, which is all the gate reads of them.  Neither the
                       weights nor the inputs are stored: meta holds their seeds (tests/train_align_cpu.fixture_state_dict,
                       fixture_batch) and the reference's state-dict names and shapes in its order.
"""
import copy
import contextlib
import io
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
from make_golden_lossgrad import _CastTargetMSE  # noqa: E402
from make_golden_teacher import GAP_FACTOR, duration_rule, head_sum_valid  # noqa: E402
from tests import train_align_cpu as tc  # noqa: E402

BASE = dict(d=256, H=2, encoder_layer=1, decoder_layer=4, conv_filter_size=256, kernel=[3, 1], predictor_filter=256, predictor_kernel=3,
            max_seq_len=32, B=2, L=7, src_lens=[7, 4], T=20, mel_lens=[20, 13], pitch="frame_level", energy="frame_level", weight_seed=400)


def build(meta):
    from model.fastspeech2_align import FastSpeech2Align  # the reference class

    pc, cfg = tc.fixture_config(meta)
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "stats.json"), "w") as f:
        json.dump(wl.SYNTH_STATS, f)
    pc["path"]["preprocessed_path"] = d
    model = FastSpeech2Align(pc, cfg).train()
    model.mel_encoder.prenet.dropout.p = 0.0
    names = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.fixture_state_dict(meta).items()}, strict=True)
    return model, pc, cfg, names


def run(model, pc, cfg, batch, double, forced=None):
    from model.loss import FastSpeech2Loss  # the reference class

    dtype = torch.float64 if double else torch.float32
    model = copy.deepcopy(model).to(dtype).train()
    _, _, speakers, texts, sl, L, mels, ml, T, pt, et = batch
    if forced is None:
        model._calculate_duration = duration_rule
    else:
        rows = iter(torch.from_numpy(forced))
        model._calculate_duration = lambda attn, src_len, mel_len, max_src_len: next(rows)
    tt = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    inputs = (None, None, tt(speakers), tt(texts), tt(sl), L, tt(mels).to(dtype), tt(ml), T, tt(pt).to(dtype), tt(et).to(dtype))
    real_dropout = torch.nn.functional.dropout

    def identity(t, p=0.5, training=True, inplace=False):
        assert training  # PostNet's hard-coded F.dropout(..., 0.5, self.training) in train()
        return t

    torch.nn.functional.dropout = identity
    try:
        out = model(*inputs[2:])
    finally:
        torch.nn.functional.dropout = real_dropout
    loss = FastSpeech2Loss(pc, cfg)
    loss.mse_loss = _CastTargetMSE() if double else torch.nn.MSELoss()
    with contextlib.redirect_stdout(io.StringIO()):
        seven = loss(inputs, out)
    assert all(o.dtype == dtype for o in seven) and all(out[i].dtype == dtype for i in range(5))
    seven[0].backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad).numpy() for k, p in model.named_parameters() if p.requires_grad}
    res = {n: out[i].detach().numpy() for i, n in enumerate(tc.PRED_NAMES)}
    res.update(d_targets=out[11].numpy(), seven=np.array([o.item() for o in seven], dtype=np.float64 if double else np.float32))
    return res, [a.detach().numpy() for a in out[10]], grads


def hazards(meta, batch, r32, r64, al32, al64, g32, g64):
    """(ok, record): the two discrete hazards of this (weights, inputs) pair and the floor of the one-element gradients' distances"""
    sl, ml, mels = batch[4], batch[7], batch[6]
    v32, v64 = head_sum_valid(al32[-1], sl, ml), head_sum_valid(al64[-1], sl, ml)
    dist = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(v32, v64))
    gap = min(float((np.sort(b, axis=1)[:, -1] - np.sort(b, axis=1)[:, -2]).min()) if b.shape[1] > 1 else np.inf for b in v64)
    rec = dict(min_top2_gap_f64=gap, head_sum_dist_fp32_f64=dist)
    ok = gap >= GAP_FACTOR * dist
    valid = np.arange(meta["T"])[None, :] < np.asarray(ml)[:, None]
    for n in ("output", "postnet_output"):
        d = float(np.abs(r32[n].astype(np.float64) - r64[n])[valid].max())
        m = float(np.abs(r64[n] - mels.astype(np.float64))[valid].min())
        rec[f"{n}_dist_fp32_f64"], rec[f"{n}_min_abs_error_f64"] = d, m
        ok = ok and m >= GAP_FACTOR * d
    valid_l = np.arange(meta["L"])[None, :] < np.asarray(sl)[:, None]
    rec["one_element_grad_floor"] = {}
    for name, pred, level in (("duration", "log_d_predictions", "phoneme_level"), ("pitch", "p_predictions", meta["pitch"]),
                              ("energy", "e_predictions", meta["energy"])):
        sel = valid if (level == "frame_level" and name != "duration") else valid_l
        e = (r32[pred].astype(np.float64) - r64[pred])[sel]
        floor = 2.0 * float(np.sqrt(np.mean(e * e))) / float(np.sqrt(e.size))
        k = f"variance_adaptor.{name}_predictor.linear_layer.bias"
        rec["one_element_grad_floor"][k] = floor
        ok = ok and float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) >= floor
    return ok, rec


def make(name="train_align_tiny"):
    for aligner_seed, input_seed in [(a, i) for i in range(410, 474) for a in range(4)]:
        meta = dict(BASE, aligner_seed=aligner_seed, input_seed=input_seed)
        batch = tc.fixture_batch(meta)
        model, pc, cfg, names = build(meta)
        r32, al32, g32 = run(model, pc, cfg, batch, False)
        r64, al64, g64 = run(model, pc, cfg, batch, True, forced=r32["d_targets"])
        ok, rec = hazards(meta, batch, r32, r64, al32, al64, g32, g64)
        print(f"aligner seed {aligner_seed}, input seed {input_seed}: {json.dumps(rec)} -> {'ok' if ok else 'searching on'}")
        if ok:
            break
    else:
        raise SystemExit("no (aligner seed, input seed) pair clears both hazards")
    L = meta["L"]
    d64 = np.stack([duration_rule(torch.from_numpy(al64[-1][b]), batch[4][b], batch[7][b], L).numpy() for b in range(meta["B"])])
    assert np.array_equal(d64, r32["d_targets"]) and np.array_equal(r32["d_targets"], r64["d_targets"])
    assert len(al32) == 4 and np.isfinite(r32["seven"]).all()
    sd = tc.fixture_state_dict(meta)
    s32, s64 = tc.stored_gradients(g32, sd), tc.stored_gradients(g64, sd)
    meta.update(rec, gap_factor=GAP_FACTOR, rows=list(tc.ROWS), state_dict=names, pred_names=list(tc.PRED_NAMES),
                grad_dist={k: float(np.abs(s32[k].astype(np.float64) - s64[k]).max()) for k in s64},
                attn_dist=[mga.dist(a, b) for a, b in zip(al32, al64)])
    arrays = dict(d_targets=r32["d_targets"], seven=r32["seven"], seven_f64=r64["seven"])
    for n in tc.PRED_NAMES:
        arrays[n], arrays[n + "_f64"] = r32[n], r64[n]
    arrays.update({"g__" + k: v for k, v in s64.items()})
    mga.save(name, meta, **arrays)
    size = os.path.getsize(os.path.join(HERE, name + ".npz"))
    assert size < os.path.getsize(os.path.join(HERE, "mel_encoder_tiny.npz")), size
    print("losses", r32["seven"], r64["seven"])


if __name__ == "__main__":
    make()
