#!/usr/bin/env python3
"""Golden batches for the device-resident training set — runs ONLY where the reference lives read-only at /root/reference.  It writes a
synthetic preprocessed directory (train.txt, val.txt, speakers.json, mel/, pitch/, energy/ ``*.npy``) to a temp dir and runs the
reference's OWN ``Dataset(sort=True, drop_last=True)`` under ``DataLoader(batch_size=3 * 4, shuffle=True, collate_fn=...)`` with
``to_device(batch, cpu)`` (dataset.py, train.py:27-38, utils/tools.py:18-54) for one epoch, and then ``Dataset(sort=False,
drop_last=False)`` under ``DataLoader(batch_size=3, shuffle=False)`` as the validation pass.  ``text.text_to_sequence`` is replaced by a
stub that reads space-separated integers (the text front end is out of scope: SURVEY.md), ``unidecode`` / ``inflect`` are stubbed as in
make_golden_aligner.py.

    python tests/golden/make_golden_dataset.py

dataset_tiny.npz   29 utterances, n_mel 80, frame-level pitch and energy, L in [1, 9] with many ties, T in [1, 70] with 1, 63, 64, 65
                   among them (most are short, so that the file stays small), random fp32 with some -0.0 and denormals.  Stored: the
                   utterance arrays (packed, with their lengths), the permutation the loader drew (recovered from the ids the loader
                   handed ``collate_fn``, in its order), and every batch's tensors, ids and maxima of both passes.
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
for _name, _attr in (("unidecode", "unidecode"), ("inflect", "engine")):
    _m = types.ModuleType(_name)
    setattr(_m, _attr, (lambda s: s) if _name == "unidecode" else (lambda: None))
    sys.modules[_name] = _m
_text = types.ModuleType("text")
_text.text_to_sequence = lambda text, cleaners: [int(t) for t in text.split()]  # "{12 7 301}" is written as "12 7 301"
sys.modules["text"] = _text

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402
from tests import dataset_cpu as dc  # noqa: E402

N, N_MEL, BATCH, GROUP, SEED = 29, 80, 3, 4, 20
SPEAKERS = {"ann": 0, "bob": 1, "cyd": 2}
T_EDGES = (1, 63, 64, 65, 70)


def utterances():
    rs = np.random.RandomState(SEED)
    L = rs.randint(1, 10, size=N)
    L[:4] = (1, 9, 9, 1)
    T = rs.randint(2, 32, size=N)
    T[rs.permutation(N)[:len(T_EDGES)]] = T_EDGES
    utts = dc.make_set(list(zip(L.tolist(), T.tolist())), n_mel=N_MEL, seed=SEED + 1)
    names = sorted(SPEAKERS)
    utts["speaker_names"] = [names[s] for s in utts["speakers"]]
    return utts


def write_dir(root, utts):
    for d in ("mel", "pitch", "energy"):
        os.makedirs(os.path.join(root, d))
    with open(os.path.join(root, "speakers.json"), "w") as f:
        json.dump(SPEAKERS, f)
    lines = []
    for i, name in enumerate(utts["ids"]):
        s = utts["speaker_names"][i]
        lines.append("|".join((name, s, " ".join(str(int(t)) for t in utts["texts"][i]), utts["raw_texts"][i])))
        for kind, key in (("mel", "mels"), ("pitch", "pitches"), ("energy", "energies")):
            np.save(os.path.join(root, kind, f"{s}-{kind}-{name}.npy"), utts[key][i])
    for fn in ("train.txt", "val.txt"):
        with open(os.path.join(root, fn), "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")


def run_pass(root, filename, sort, drop_last, loader_batch, shuffle):
    """(the ids in the order the loader handed them to collate_fn, the list of to_device'd batches)"""
    from dataset import Dataset  # the reference's
    from utils.tools import to_device

    pcfg = wl.preprocess_config()
    pcfg["dataset"] = "tiny"
    pcfg["path"]["preprocessed_path"] = root
    pcfg["preprocessing"]["text"] = {"text_cleaners": ["english_cleaners"]}
    ds = Dataset(filename, pcfg, {"optimizer": {"batch_size": BATCH}}, sort=sort, drop_last=drop_last)
    seen = []

    def collate(data):
        seen.extend(d["id"] for d in data)
        return ds.collate_fn(data)

    out = []
    for batchs in DataLoader(ds, batch_size=loader_batch, shuffle=shuffle, collate_fn=collate):
        for batch in batchs:
            out.append(to_device(batch, torch.device("cpu")))
    return seen, out


def main():
    utts = utterances()
    index = {name: i for i, name in enumerate(utts["ids"])}
    with tempfile.TemporaryDirectory() as root:
        write_dir(root, utts)
        torch.manual_seed(SEED)
        seen, train = run_pass(root, "train.txt", True, True, BATCH * GROUP, True)
        seen_val, val = run_pass(root, "val.txt", False, False, BATCH, False)
    perm = np.array([index[n] for n in seen], dtype=np.int64)
    assert sorted(perm.tolist()) == list(range(N)) and [index[n] for n in seen_val] == list(range(N))
    store = dc.pack(utts)
    arrays = dict(perm=perm, mel=store["mel"], pitch=np.concatenate(utts["pitches"]), energy=np.concatenate(utts["energies"]),
                  text=np.concatenate(utts["texts"]).astype(np.int64), speaker=store["speaker"], text_len=store["text_len"], mel_len=store["mel_len"])
    meta = dict(N=N, n_mel=N_MEL, batch_size=BATCH, group_size=GROUP, pitch="frame_level", energy="frame_level", seed=SEED, ids=utts["ids"],
                raw_texts=utts["raw_texts"], passes={})
    for tag, batches in (("train", train), ("val", val)):
        recs = []
        for k, b in enumerate(batches):
            assert len(b) == 11
            recs.append(dict(ids=list(b[0]), raw_texts=list(b[1]), max_src_len=int(b[5]), max_mel_len=int(b[8]),
                             dtypes={name: str(b[pos].dtype) for pos, name in dc.TENSORS.items()}))
            for pos, name in dc.TENSORS.items():
                arrays[f"{tag}{k}_{name}"] = b[pos].numpy()
        meta["passes"][tag] = recs
        print(tag, len(batches), "batches:", [len(r["ids"]) for r in recs], "T:", [r["max_mel_len"] for r in recs])
    path = os.path.join(HERE, "dataset_tiny.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}  {size / 1024:.0f} KiB")
    assert size < (1 << 20), "a committed file must stay below 1 MiB"


if __name__ == "__main__":
    main()
