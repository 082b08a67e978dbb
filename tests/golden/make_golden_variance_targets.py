#!/usr/bin/env python3
"""Golden vectors for the variance targets and dataset statistics — runs ONLY where the reference lives read-only at /root/reference.
It runs the reference's own ``Preprocessor.build_from_path`` over a temporary directory with the stub-module recipe of
make_golden_melfront.py: ``tgt``, ``librosa``, ``pyworld`` and the reference's ``audio`` package are stubbed so that
``tgt.io.read_textgrid``, ``librosa.load``, ``pw.dio`` / ``pw.stonemask`` and ``Audio.tools.get_mel_from_wav`` hand back the fixture's
durations, f0 (already rounded to fp32, so the comparison is arithmetic only) and energy.  sampling_rate == hop_length makes the
TextGrid times the frame prefix sums, so ``get_alignment`` recovers the durations exactly.

    python tests/golden/make_golden_variance_targets.py

variance_targets_tiny.npz    B 6, L 12, T 40, the four level combinations; alias-free durations, so the reference runs on all of it
variance_targets_edges.npz   B 4, L 300, T 1030; the aliasing utterances (printed) carry the restatement's values only
Each holds numbers only: the inputs, the reference's raw and normalised .npy contents, its stats.json values and the float64
restatement (tests/variance_targets_cpu.py).  Asserts the discrete preconditions the tests restate.
"""
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import variance_targets_cpu as vc  # noqa: E402

CUR = {}  # what the stubs hand back: the utterance whose TextGrid was read last


class _Interval:
    def __init__(self, s, e):
        self.start_time, self.end_time, self.text = float(s), float(e), "a"


class _Tier:
    def __init__(self, d):
        c = np.concatenate([[0], np.cumsum(d)])
        self._objects = [_Interval(c[i], c[i + 1]) for i in range(len(d))]


class _Grid:
    def __init__(self, d):
        self.tier = _Tier(d)

    def get_tier_by_name(self, name):
        return self.tier


def _stub_modules():
    """Installed once, before the reference module is imported (it binds these names at import); the batch travels through CUR."""
    def read_textgrid(path):
        b = int(os.path.basename(path).split(".")[0][1:])
        CUR["b"] = b
        return _Grid(CUR["batch"]["durations"][b, :CUR["batch"]["src_lens"][b]])

    tgt, tio = types.ModuleType("tgt"), types.ModuleType("tgt.io")
    tio.read_textgrid = read_textgrid
    tgt.io = tio
    librosa = types.ModuleType("librosa")
    librosa.load = lambda path: (np.zeros(CUR["batch"]["pitch"].shape[1], np.float32), 1)
    pw = types.ModuleType("pyworld")
    pw.dio = lambda wav, sr, frame_period: (CUR["batch"]["pitch"][CUR["b"]].astype(np.float64), None)
    pw.stonemask = lambda wav, f0, t, sr: f0
    audio, stft, tools = types.ModuleType("audio"), types.ModuleType("audio.stft"), types.ModuleType("audio.tools")
    stft.TacotronSTFT = lambda *a, **k: None
    tools.get_mel_from_wav = lambda wav, fn: (np.zeros((4, CUR["batch"]["pitch"].shape[1]), np.float32), CUR["batch"]["energy"][CUR["b"]].copy())
    audio.stft, audio.tools = stft, tools
    sys.modules.update({"tgt": tgt, "tgt.io": tio, "librosa": librosa, "pyworld": pw, "audio": audio, "audio.stft": stft, "audio.tools": tools})


def run_reference(batch, utts, p_level, e_level):
    """The reference's build_from_path over the utterances ``utts`` -> (raw {name: {b: array}}, normalised, stats.json dict)."""
    from preprocessor.preprocessor import Preprocessor  # the reference class

    with tempfile.TemporaryDirectory() as tmp:
        raw_dir, out_dir = os.path.join(tmp, "raw"), os.path.join(tmp, "out")
        os.makedirs(os.path.join(raw_dir, "spk"))
        os.makedirs(os.path.join(out_dir, "TextGrid", "spk"))
        for b in utts:
            for path in (os.path.join(raw_dir, "spk", f"u{b}.wav"), os.path.join(out_dir, "TextGrid", "spk", f"u{b}.TextGrid")):
                open(path, "w").close()
            with open(os.path.join(raw_dir, "spk", f"u{b}.lab"), "w") as f:
                f.write("text\n")
        cfg = {"path": {"data_path": raw_dir, "preprocessed_path": out_dir},
               "preprocessing": {"val_size": 0, "audio": {"sampling_rate": 256}, "stft": {"filter_length": 1024, "hop_length": 256, "win_length": 1024},
                                 "mel": {"n_mel_channels": 4, "mel_fmin": 0, "mel_fmax": 8000},
                                 "pitch": {"feature": p_level, "normalization": True}, "energy": {"feature": e_level, "normalization": True}}}
        pre = Preprocessor(cfg)
        raw = {"pitch": {}, "energy": {}}
        inner = pre.normalize

        def normalize(in_dir, mean, std):  # keep the raw files' contents before the reference overwrites them
            kind = os.path.basename(in_dir)
            for name in os.listdir(in_dir):
                raw[kind][int(name.split("-")[-1].split(".")[0][1:])] = np.load(os.path.join(in_dir, name))
            return inner(in_dir, mean, std)

        pre.normalize = normalize
        pre.build_from_path()
        norm = {"pitch": {}, "energy": {}}
        for kind in norm:
            for name in os.listdir(os.path.join(out_dir, kind)):
                norm[kind][int(name.split("-")[-1].split(".")[0][1:])] = np.load(os.path.join(out_dir, kind, name))
        with open(os.path.join(out_dir, "stats.json")) as f:
            stats = json.load(f)
    return raw, norm, stats


def save(name, meta, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}  {size / 1024:.0f} KiB")
    assert size < (1 << 20), "a committed file must stay below 1 MiB"


def make(cfg, seed, combos):
    batch = vc.fixture_batch(cfg, seed)
    B, T = batch["pitch"].shape
    L = batch["durations"].shape[1]
    CUR["batch"] = batch
    free = [b for b in range(B) if vc.alias_free(batch["durations"][b], int(batch["src_lens"][b]))]
    print(f"{cfg}: alias-free utterances {free}; aliasing (restatement values only) {[b for b in range(B) if b not in free]}")
    if cfg == "tiny":
        assert free == list(range(B)), "the tiny fixture must be alias-free"
    arrays = {"pitch": batch["pitch"], "energy": batch["energy"], "durations_padded": batch["durations_padded"], "src_lens": batch["src_lens"],
              "ref_utts": np.array(free, dtype=np.int64)}
    meta = {"config": cfg, "seed": seed, "B": B, "L": L, "T": T, "combos": [list(c) for c in combos], "replica": batch["replica"], "ref_stats": {}}
    for p_level, e_level in combos:
        key = vc.combo_key(p_level, e_level)
        full = vc.pipeline(batch, p_level, e_level)
        # discrete preconditions: no value within relative 1e-5 of an outlier bound, no `valid` decision at its threshold's mercy
        vc.check_preconditions(batch, full)
        raw, norm, stats = run_reference(batch, free, p_level, e_level)
        sub = vc.pipeline(batch, p_level, e_level, only=free)  # the restatement on what the reference saw
        kept = [b for b in free if full["valid"][b]]
        assert sorted(raw["pitch"]) == kept == sorted(raw["energy"]), (sorted(raw["pitch"]), kept)
        meta["ref_stats"][key] = stats
        for name, level in (("pitch", p_level), ("energy", e_level)):
            W = T if level == "frame_level" else L
            r_raw, r_norm, r_len = np.zeros((B, W)), np.zeros((B, W)), np.zeros(B, dtype=np.int64)
            for b in kept:
                v = raw[name][b]
                r_len[b] = len(v)
                assert len(v) == sub[name]["n"][b], (name, b, len(v), sub[name]["n"][b])
                r_raw[b, :len(v)], r_norm[b, :len(v)] = v, norm[name][b]
                # the restatement reproduces the reference: float64 pitch to 1e-12, fp32 energy to n 2^-24 (n = the longest segment)
                want = sub[name]["raw64"][b, :len(v)]
                if v.dtype == np.float64:
                    assert np.all(np.abs(v - want) <= 1e-12 * np.abs(want)), (cfg, key, name, b)
                else:
                    nseg = max(1, int(batch["durations"][b, :batch["src_lens"][b]].max()))
                    assert np.all(np.abs(v.astype(np.float64) - want) <= nseg * vc.U24 * np.abs(want)), (cfg, key, name, b)
            arrays.update({f"ref_{key}_{name}_raw": r_raw, f"ref_{key}_{name}_norm": r_norm, f"ref_{key}_{name}_len": r_len,
                           f"ref_{key}_{name}_is_f64": np.array(all(raw[name][b].dtype == np.float64 for b in kept)),
                           f"cpu_{key}_{name}_raw": full[name]["raw64"], f"cpu_{key}_{name}_norm": full[name]["norm"],
                           f"cpu_{key}_{name}_stats": np.array(full["stats"][name]), f"cpu_sub_{key}_{name}_stats": np.array(sub["stats"][name])})
            s, r = sub["stats"][name], stats[name]
            scale = max(abs(r[2]), r[3])
            print(f"  {key} {name}: reference stats {r}; restatement (fp32-rounded values) off by "
                  f"mean {abs(s[2] - r[2]) / scale:.2e} std {abs(s[3] - r[3]) / scale:.2e} (gate 1e-6)")
            assert abs(s[2] - r[2]) <= 1e-6 * scale and abs(s[3] - r[3]) <= 1e-6 * scale
        arrays.update({f"cpu_{key}_frame_lens": full["frame_lens"], f"cpu_{key}_valid": full["valid"]})
    save("variance_targets_" + cfg, meta, **arrays)


if __name__ == "__main__":
    _stub_modules()
    make("tiny", 21, vc.COMBOS)
    make("edges", 22, (("phoneme_level", "phoneme_level"), ("frame_level", "frame_level")))
