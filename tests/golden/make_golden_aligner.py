#!/usr/bin/env python3
"""Golden vectors for the reference-mel aligner — runs ONLY where the reference lives read-only at /root/reference.  It imports
the reference's ``transformer.TxtEncoder`` / ``transformer.MelEncoder`` (recipe: SURVEY.md §8c), loads the seeded synthetic
weights (``workload.synth_state_dict`` + ``workload.synth_aligner_state_dict``) and runs what
``model/fastspeech2_align.py:45,56`` chains — ``mel_encoder(txt_encoder(texts, src_masks), mels, src_masks, mel_masks)`` — in
``eval()``, once as it is (fp32) and once cast to ``.double()``.

The fixtures hold numbers only (inputs, both evaluations, the reference's own fp32-vs-float64 distances); the weights are NOT
stored, both sides regenerate them from the seed.

    python tests/golden/make_golden_aligner.py

aligner_tiny.npz              B = 2, L = 12, T = 40, src_lens [12, 7], mel_lens [40, 23]: every layer, every row
aligner_T_above_1000.npz      B = 1, L = 24, T = 1030: inputs, distances, tgt_output rows 0-15 and 992-1029
aligner_T_above_1000_attn{i}.npz   the alignment of layer i of that case, fp32 and float64 (one file per layer: a committed file
                              stays below 1 MiB)
"""
import copy
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
for _name, _attr in (("unidecode", "unidecode"), ("inflect", "engine")):
    _m = types.ModuleType(_name)
    setattr(_m, _attr, (lambda s: s) if _name == "unidecode" else (lambda: None))
    sys.modules[_name] = _m

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402

torch.set_num_threads(8)
CONFIG = "ljspeech"
ROWS_LONG = list(range(0, 16)) + list(range(992, 1030))


def build(cfg, weight_seed, aligner_seed):
    from transformer import MelEncoder, TxtEncoder  # the reference classes

    sd = wl.synth_state_dict(cfg, seed=weight_seed)
    asd = wl.synth_aligner_state_dict(cfg, seed=aligner_seed)
    enc, mel = TxtEncoder(cfg).eval(), MelEncoder(cfg).eval()
    enc.load_state_dict({k[len("txt_encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith("txt_encoder.")})
    mel.load_state_dict({k[len("mel_encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in asd.items()})
    return enc, mel


def inputs(B, L, T, src_lens, mel_lens, seed):
    _, texts, sl, _ = wl.synth_inputs(B, L, seed=seed, src_lens=src_lens)
    rs = np.random.RandomState(seed + 99)
    mels = (rs.standard_normal((B, T, wl.N_MEL)) * 2.0 - 3.0).astype(np.float32)  # log-mel-like range
    ml = np.asarray(mel_lens, dtype=np.int64)
    for b in range(B):
        mels[b, ml[b]:] = 0.0  # what a collated batch holds past an utterance's end (utils/tools.py pad_2D)
    return texts, sl, mels, ml


def run(enc, mel, texts, sl, mels, ml, double):
    L, T = texts.shape[1], mels.shape[1]
    sm = torch.arange(L)[None] >= torch.from_numpy(sl)[:, None]
    mm = torch.arange(T)[None] >= torch.from_numpy(ml)[:, None]
    x = torch.from_numpy(mels)
    if double:
        enc, mel, x = copy.deepcopy(enc).double(), copy.deepcopy(mel).double(), x.double()
    with torch.no_grad():
        out, al = mel(enc(torch.from_numpy(texts), sm), x, sm, mm)
    return out.numpy(), [a.numpy() for a in al]


def frame_argmax(al_last, sl, ml):
    a = al_last[:, 0].copy()
    for h in range(1, al_last.shape[1]):
        a = a + al_last[:, h]
    return [np.argmax(a[b, :ml[b], :sl[b]], axis=1) for b in range(a.shape[0]) if sl[b] > 0 and ml[b] > 0]


def dist(a32, a64):
    d = np.abs(np.asarray(a32, dtype=np.float64) - a64).reshape(-1)
    return {"max": float(d.max()), "p999": float(np.quantile(d, 0.999))}


def make(name, B, L, T, src_lens, mel_lens, rows=None, split_attn=False, input_seed=1):
    cfg = wl.model_config(CONFIG)
    for aligner_seed in range(8):
        enc, mel = build(cfg, 0, aligner_seed)
        texts, sl, mels, ml = inputs(B, L, T, src_lens, mel_lens, input_seed)
        out32, al32 = run(enc, mel, texts, sl, mels, ml, False)
        out64, al64 = run(enc, mel, texts, sl, mels, ml, True)
        i32, i64 = np.concatenate(frame_argmax(al32[-1], sl, ml)), np.concatenate(frame_argmax(al64[-1], sl, ml))
        agree = float((i32 == i64).mean())
        print(f"{name}: aligner seed {aligner_seed}: fp32 / float64 per-frame argmax agree on {agree:.4f} of {i32.size} frames")
        if agree >= 0.99:
            break
    else:
        raise SystemExit(f"{name}: no seed with >= 99 % argmax agreement")
    meta = dict(config=CONFIG, weight_seed=0, frames_per_phoneme=8.0, aligner_seed=aligner_seed, B=B, L=L, T=T, n_layer=len(al32),
                argmax_agreement=agree, rows=rows, split_attn=bool(split_attn),
                attn_dist=[dist(a, b) for a, b in zip(al32, al64)], tgt_dist=dist(out32, out64))
    sel = slice(None) if rows is None else np.asarray(rows)
    arrays = dict(texts=texts, src_lens=sl, mels=mels, mel_lens=ml, tgt_output=out32[:, sel], tgt_output_f64=out64[:, sel])
    if not split_attn:
        for i, (a, b) in enumerate(zip(al32, al64)):
            arrays[f"attn{i}"], arrays[f"attn{i}_f64"] = a, b
    save(name, meta, **arrays)
    if split_attn:
        for i, (a, b) in enumerate(zip(al32, al64)):
            save(f"{name}_attn{i}", dict(layer=i, of=name), attn=a, attn_f64=b)
    print(name, json.dumps({k: meta[k] for k in ("attn_dist", "tgt_dist")}))


def save(name, meta, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}  {size / 1024:.0f} KiB")
    assert size < (1 << 20), "a committed file must stay below 1 MiB"


if __name__ == "__main__":
    make("aligner_tiny", 2, 12, 40, [12, 7], [40, 23])
    make("aligner_T_above_1000", 1, 24, 1030, [24], [1030], rows=ROWS_LONG, split_attn=True)
