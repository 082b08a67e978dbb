"""The device-resident training set on the GPU (csrc/dataset.hip through ns_ds_*, smart_nar_fast_tts_amd.data, training.fit).

The gather alone first: ``ns_ds_gather`` and ``ns_ds_op_gather`` at grid caps 1 and 2 on every case of tests/dataset_cpu.py (n_mel 4, 16
and 80; B 1 and 3; T 1, 63, 64 and 65 in one batch; the first and the last utterance of the store; an utterance twice; axes wider than
the batch needs; phoneme-level slots), outputs pre-filled with 0xFF bytes, bit-equal to ``collate_statement`` — the reference's collate
and ``to_device`` restated on the unpacked utterances.  Then ``DeviceDataset.epoch()`` on tests/golden/dataset_tiny.npz against the
batches the reference's own ``Dataset`` / ``DataLoader`` / ``to_device`` produced, both passes: ids, dtypes, shapes, maxima and bits, one
launch per batch, no host read.  Then ``training.fit`` for four steps against a hand loop of ``train_step`` over the same batches:
parameters and buffers bit-equal.  All comparisons are exact."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from tests import dataset_cpu as dc
from tests import optim_cpu as oc
from tests import train_align_cpu as tc
from tests.util import ROOT, dev, load_golden, native_lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def so():
    return native_lib()


@pytest.fixture(scope="module")
def golden():
    return load_golden("dataset_tiny")


@pytest.fixture(scope="module")
def tb():
    spec = importlib.util.spec_from_file_location("_ns_tools_bench", os.path.join(ROOT, "tools", "_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture_utterances(meta, z):
    tl, ml = z["text_len"], z["mel_len"]
    cut = lambda a, lens: np.split(a, np.cumsum(lens)[:-1])  # noqa: E731
    level = lambda name: ml if meta[name] == "frame_level" else tl  # noqa: E731
    return dict(ids=list(meta["ids"]), raw_texts=list(meta["raw_texts"]), speakers=[int(s) for s in z["speaker"]], texts=cut(z["text"], tl),
                mels=cut(z["mel"], ml), pitches=cut(z["pitch"], level("pitch")), energies=cut(z["energy"], level("energy")))


def _fixture_set(meta, z, **kw):
    from smart_nar_fast_tts_amd import data

    u = fixture_utterances(meta, z)
    return data.DeviceDataset.from_arrays(u["ids"], u["raw_texts"], u["speakers"], u["texts"], u["mels"], u["pitches"], u["energies"],
                                          wl.preprocess_config(meta["pitch"], meta["energy"]), "cuda", **kw)


# ---------------------------------------------------------------------------------------------------- the gather alone
FIELDS = ("mel", "pitch", "energy", "text", "speaker", "mel_off", "pitch_off", "energy_off", "text_off", "text_len", "mel_len", "pitch_len", "energy_len")
OUT_DTYPES = dict(mels=torch.float32, pitches=torch.float32, energies=torch.float32, texts=torch.int64, speakers=torch.int64, src_lens=torch.int64,
                  mel_lens=torch.int64)


def _canaries(B, T, P, E, Lm, n_mel):
    shapes = dict(mels=(B, T, n_mel), pitches=(B, P), energies=(B, E), texts=(B, Lm), speakers=(B,), src_lens=(B,), mel_lens=(B,))
    out = {}
    for k, shape in shapes.items():
        n = int(np.prod(shape)) * (4 if OUT_DTYPES[k] == torch.float32 else 8)
        out[k] = torch.full((n,), dc.CANARY, dtype=torch.uint8, device="cuda").view(OUT_DTYPES[k]).reshape(shape)
    return out


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_gather_is_the_collate_statement_bit_for_bit(so, name):
    L, lib = so
    utts, store, idxs, caps = dc.case_store(name)
    n_mel = store["mel"].shape[1]
    held = {f: dev(store[f]) for f in FIELDS}
    s, lens = L.STRUCTS["ns_ds_store"](), L.STRUCTS["ns_ds_lens"]()
    for f in FIELDS:
        setattr(s, f, held[f].data_ptr())
    s.mel_rows, s.pitch_elems, s.energy_elems, s.text_elems = store["mel"].shape[0], store["pitch"].size, store["energy"].size, store["text"].size
    s.N, s.n_mel = len(store["speaker"]), n_mel
    for f in ("text", "mel", "pitch", "energy"):
        setattr(lens, f, store[f + "_len"].ctypes.data)
    # the batch sits in the middle of a longer order: `first` is honoured on the device and on the host
    order = np.array([0, 9] + list(idxs) + [4], dtype=np.int32)
    order_d = dev(order)
    want = dc.collate_statement(utts, idxs, *caps)
    assert all(dc.same_bits(want[pos], dc.case_want(name)[n]) for pos, n in dc.TENSORS.items())
    before = {f: held[f].cpu().numpy().tobytes() for f in FIELDS}
    for cap in (None,) + dc.GRID_CAPS:
        out = _canaries(len(idxs), *caps, n_mel)
        o = L.STRUCTS["ns_ds_batch"](*(out[k].data_ptr() for k in OUT_DTYPES), len(idxs), *caps)
        args = (C.byref(s), C.byref(lens), L.ptr(order_d), order.ctypes.data, order.size, 2, C.byref(o))
        if cap is None:
            L.check(lib.ns_ds_gather(*args, L.stream_ptr()), "ns_ds_gather")
        else:
            L.check(lib.ns_ds_op_gather(*args, cap, L.stream_ptr()), "ns_ds_op_gather")
        assert lib.ns_ds_last_launches() == 1
        for pos, n in dc.TENSORS.items():
            got = out[n].cpu().numpy()
            assert dc.same_bits(got, want[pos]), (name, cap, n)
    assert all(held[f].cpu().numpy().tobytes() == before[f] for f in FIELDS), "the store is only read"


# ---------------------------------------------------------------------------------------------------- epoch() against the reference's loader
@pytest.mark.parametrize("tag", ["train", "val"])
def test_epoch_is_the_reference_loader_bit_for_bit(golden, tb, tag):
    meta, z = golden
    ds = _fixture_set(meta, z)
    assert len(ds) == meta["N"] and ds.skipped == [] and ds.launches == 0
    assert ds.upload_bytes == z["mel"].nbytes + 4 * (2 * dc.layout(z["mel_len"])[1] + dc.layout(z["text_len"])[1] + meta["N"]) + 8 * 4 * (meta["N"] + 1) + 16 * meta["N"]
    recs = meta["passes"][tag]
    got = []

    def run():
        it = ds.epoch(meta["batch_size"], meta["group_size"], perm=z["perm"]) if tag == "train" else ds.validation(meta["batch_size"])
        for batch in it:
            got.append((batch, ds.last_launches))

    torch.cuda.synchronize()
    n_reads, msgs = tb.host_reads(run)
    assert n_reads == 0, msgs
    torch.cuda.synchronize()
    assert len(got) == len(recs) and ds.launches == len(recs), "one launch per batch"
    for k, ((batch, launched), rec) in enumerate(zip(got, recs)):
        assert launched == 1 and len(batch) == 11
        assert batch[0] == rec["ids"] and batch[1] == rec["raw_texts"]
        assert type(batch[5]) is int and type(batch[8]) is int and (batch[5], batch[8]) == (rec["max_src_len"], rec["max_mel_len"])
        for pos, name in dc.TENSORS.items():
            want = z[f"{tag}{k}_{name}"]
            t = batch[pos]
            assert t.is_cuda and str(t.dtype) == rec["dtypes"][name] and tuple(t.shape) == want.shape, (tag, k, name)
            assert dc.same_bits(t.cpu().numpy(), want), (tag, k, name)


def test_max_frames_leaves_out_and_lists(golden):
    meta, z = golden
    ds = _fixture_set(meta, z, max_frames=32)
    long = [n for n, t in zip(meta["ids"], z["mel_len"]) if t > 32]
    assert ds.skipped == long and len(long) == 4 and len(ds) == meta["N"] - 4 and int(ds.mel_lens.max()) <= 32
    batch = next(iter(ds.validation(5)))
    keep = [i for i, t in enumerate(z["mel_len"]) if t <= 32][:5]
    want = dc.collate_statement(fixture_utterances(meta, z), keep)
    assert batch[0] == want[0] and all(dc.same_bits(batch[pos].cpu().numpy(), want[pos]) for pos in dc.TENSORS)


def test_from_preprocessed_reads_the_reference_directory(golden, tmp_path):
    """the directory dataset.py:21-86 reads, written from the fixture's utterances: the validation pass is the reference's"""
    import json

    from smart_nar_fast_tts_amd import data

    meta, z = golden
    u = fixture_utterances(meta, z)
    root = tmp_path / "preprocessed"
    names = {0: "ann", 1: "bob", 2: "cyd"}
    for d in ("mel", "pitch", "energy"):
        os.makedirs(root / d)
    (root / "speakers.json").write_text(json.dumps({v: k for k, v in names.items()}))
    lines = []
    for i, name in enumerate(u["ids"]):
        s = names[u["speakers"][i]]
        lines.append("|".join((name, s, " ".join(str(int(t)) for t in u["texts"][i]), u["raw_texts"][i])))
        for kind, key in (("mel", "mels"), ("pitch", "pitches"), ("energy", "energies")):
            np.save(root / kind / f"{s}-{kind}-{name}.npy", u[key][i])
    (root / "val.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    pcfg = wl.preprocess_config(meta["pitch"], meta["energy"])
    pcfg["path"]["preprocessed_path"] = str(root)
    pcfg["preprocessing"]["text"] = {"text_cleaners": ["english_cleaners"]}
    seen = []

    def text_to_sequence(text, cleaners):
        seen.append(cleaners)
        return [int(t) for t in text.split()]

    ds = data.DeviceDataset.from_preprocessed("val.txt", pcfg, {"optimizer": {"batch_size": meta["batch_size"]}}, text_to_sequence, "cuda")
    assert len(ds) == meta["N"] == len(seen) and seen[0] == ["english_cleaners"] and ds.ids == u["ids"] and ds.raw_texts == u["raw_texts"]
    recs = meta["passes"]["val"]
    for k, (batch, rec) in enumerate(zip(ds.validation(meta["batch_size"]), recs)):
        assert batch[0] == rec["ids"] and batch[1] == rec["raw_texts"]
        assert all(dc.same_bits(batch[pos].cpu().numpy(), z[f"val{k}_{name}"]) for pos, name in dc.TENSORS.items()), k
    assert ds.launches == len(recs)


# ---------------------------------------------------------------------------------------------------- fit()
def _model(pcfg, cfg, sd):
    from smart_nar_fast_tts_amd import training

    m = training.FastSpeech2Align(pcfg, cfg)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m.mel_encoder.prenet.p_drop, m.postnet.dropout = 0.0, 0.0  # dropout 0 everywhere (the config's three are 0 already)
    return m.cuda().train()


def test_fit_is_a_hand_loop_of_train_step(golden, tmp_path):
    from smart_nar_fast_tts_amd import optim, training
    from smart_nar_fast_tts_amd.loss import FastSpeech2TrainingLoss

    meta, z = golden
    tmeta, _ = load_golden("train_align_tiny")
    pcfg, cfg = tc.fixture_config(tmeta)
    assert (tmeta["pitch"], tmeta["energy"]) == (meta["pitch"], meta["energy"]) and cfg["transformer"]["encoder_dropout"] == 0.0
    sd = tc.fixture_state_dict(tmeta)
    ds = _fixture_set(meta, z, max_frames=cfg["max_seq_len"])  # train() refuses a mel past max_seq_len: those utterances stay out
    assert len(ds) >= 4 * 3 * 2
    train_config = {"optimizer": dict(batch_size=3, betas=list(oc.BETAS), eps=oc.EPS, weight_decay=0.0, grad_clip_thresh=oc.GRAD_CLIP, grad_acc_step=1, **oc.SHIPPED),
                    "step": dict(total_step=4, log_step=2, val_step=4, save_step=4), "path": {"ckpt_path": str(tmp_path / "ckpt")}}
    loss = FastSpeech2TrainingLoss(pcfg, cfg)

    logged = []
    a = _model(pcfg, cfg, sd)
    opt_a = optim.ScheduledOptim(a, train_config, cfg, 0)
    torch.manual_seed(77)
    before = ds.launches
    last = training.fit(a, loss, opt_a, ds, train_config, val_set=ds, on_log=lambda step, values, kind: logged.append((step, kind, values)))
    assert last == 4 and a.training and opt_a.current_step == 4
    assert ds.launches - before == 4 + -(-len(ds) // 3), "four training batches and one validation pass, one launch each"
    assert [(s, k) for s, k, _ in logged] == [(2, "train"), (4, "train"), (4, "val")]
    assert all(len(v) == 7 and all(np.isfinite(x) and type(x) is float for x in v) for _, _, v in logged)
    ckpt = torch.load(str(tmp_path / "ckpt" / "4.pth.tar"), map_location="cpu", weights_only=True)
    assert sorted(ckpt) == ["model", "optimizer"] and not os.path.exists(str(tmp_path / "ckpt" / "2.pth.tar"))

    b = _model(pcfg, cfg, sd)
    opt_b = optim.ScheduledOptim(b, train_config, cfg, 0)
    torch.manual_seed(77)
    seen = []
    for step, batch in enumerate(itertools.islice(ds.epoch(3), 4), start=1):
        losses = training.train_step(b, loss, opt_b, batch, step, 1, oc.GRAD_CLIP)
        seen.append(torch.stack([v.detach() for v in losses]).cpu().tolist())
    torch.cuda.synchronize()
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].cpu().numpy().tobytes() == sb[k].cpu().numpy().tobytes(), k
    assert all(ckpt["model"][k].numpy().tobytes() == sb[k].cpu().numpy().tobytes() for k in sb), "the checkpoint of step 4 is the final state"
    assert logged[0][2] == seen[1] and logged[1][2] == seen[3], "the logged losses are the steps' own"
    w0 = torch.as_tensor(np.asarray(sd["mel_linear.weight"]))
    assert not torch.equal(sa["mel_linear.weight"].cpu(), w0), "four steps moved the weights"
    # restore_step continues the count: one more step from 4 ends at 5
    again = dict(train_config, step=dict(train_config["step"], total_step=5, log_step=100, val_step=100, save_step=100))
    assert training.fit(a, loss, opt_a, ds, again, restore_step=4) == 5 and opt_a.current_step == 5
    with pytest.raises(ValueError, match="restore_step"):
        training.fit(a, loss, opt_a, ds, again, restore_step=5)
