"""The device-resident training set on the CPU (no GPU): ``data.plan_epoch`` against the batches the reference's own loader produced
(tests/golden/dataset_tiny.npz, both passes) and against tests/dataset_cpu.py's independent ``plan_statement`` on a sweep;
``ns_ds_host_gather`` (the inline function the kernel compiles) against the reference's tensors and the yardstick's cases, bit for bit;
each mutant of the yardstick caught on its named case; every refusal of the ns_ds_* family through the library and through a plain-C
caller; the header's declarations; ``DeviceDataset.from_arrays``' raises; no spill.  All comparisons are exact.

Ties among equal text lengths fall as numpy's default ``argsort`` lets them: the fixture was recorded through that same call (the
reference's), and ``plan_epoch`` makes it again."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import dataset_cpu as dc
from tests.util import ROOT, assert_no_spill, built_lib, expect_refusals, load_golden, run_c_caller


@pytest.fixture(scope="module")
def lib():
    return built_lib()


@pytest.fixture(scope="module")
def golden():
    return load_golden("dataset_tiny")


def fixture_utterances(meta, z):
    """the utterances of dataset_tiny.npz as the lists ``from_arrays`` and the yardstick take"""
    tl, ml = z["text_len"], z["mel_len"]
    cut = lambda a, lens: np.split(a, np.cumsum(lens)[:-1])  # noqa: E731
    level = lambda name: ml if meta[name] == "frame_level" else tl  # noqa: E731
    return dict(ids=list(meta["ids"]), raw_texts=list(meta["raw_texts"]), speakers=[int(s) for s in z["speaker"]], texts=cut(z["text"], tl),
                mels=cut(z["mel"], ml), pitches=cut(z["pitch"], level("pitch")), energies=cut(z["energy"], level("energy")))


def _structs(L, store, n_mel=None):
    """(ns_ds_store over the yardstick's packed host arrays, ns_ds_lens, the arrays kept alive)"""
    s, lens = L.STRUCTS["ns_ds_store"](), L.STRUCTS["ns_ds_lens"]()
    for f in ("mel", "pitch", "energy", "text", "speaker", "mel_off", "pitch_off", "energy_off", "text_off", "text_len", "mel_len", "pitch_len", "energy_len"):
        assert store[f].flags["C_CONTIGUOUS"]
        setattr(s, f, store[f].ctypes.data)
    s.mel_rows, s.pitch_elems, s.energy_elems, s.text_elems = store["mel"].shape[0], store["pitch"].size, store["energy"].size, store["text"].size
    s.N, s.n_mel = len(store["speaker"]), store["mel"].shape[1] if n_mel is None else n_mel
    for f in ("text", "mel", "pitch", "energy"):
        setattr(lens, f, store[f + "_len"].ctypes.data)
    return s, lens


def _batch(L, out, caps):
    o = L.STRUCTS["ns_ds_batch"]()
    for f in ("mels", "pitches", "energies", "texts", "speakers", "src_lens", "mel_lens"):
        setattr(o, f, out[f].ctypes.data)
    o.B, (o.Tmax, o.Pmax, o.Emax, o.Lmax) = out["speakers"].shape[0], caps
    return o


def host_gather(L, so, store, idxs, caps, order=None, first=0):
    """the seven outputs of ns_ds_host_gather, started as canaries"""
    s, lens = _structs(L, store)
    order = np.asarray(idxs if order is None else order, dtype=np.int32)
    out = dc.empty_outputs(len(idxs), *caps, store["mel"].shape[1])
    L.check(so.ns_ds_host_gather(C.byref(s), C.byref(lens), order.ctypes.data, order.size, first, C.byref(_batch(L, out, caps))), "ns_ds_host_gather")
    assert so.ns_ds_last_launches() == 0
    return out


def _same(got, want):
    return all(dc.same_bits(got[k], want[k]) for k in want) and got.keys() == want.keys()


# ---------------------------------------------------------------------------------------------------- the epoch's batches
@pytest.mark.parametrize("tag", ["train", "val"])
def test_plan_epoch_reproduces_the_reference_loader(golden, tag):
    from smart_nar_fast_tts_amd import data

    meta, z = golden
    ids = meta["ids"]
    kw = dict(perm=z["perm"]) if tag == "train" else dict(group_size=1, sort=False, drop_last=False, perm=np.arange(meta["N"]))
    batches = data.plan_epoch(z["text_len"], meta["batch_size"], **(dict(group_size=meta["group_size"], **kw) if tag == "train" else kw))
    want = [rec["ids"] for rec in meta["passes"][tag]]
    assert [[ids[i] for i in b] for b in batches] == want and all(b.dtype == np.int64 for b in batches)
    state = dc.plan_statement(z["text_len"], meta["batch_size"], meta["group_size"] if tag == "train" else 1, tag == "train", tag == "train",
                              z["perm"] if tag == "train" else np.arange(meta["N"]))
    assert [[ids[i] for i in b] for b in state] == want
    assert len(want) == (9 if tag == "train" else 10) and sum(len(b) for b in want) == (27 if tag == "train" else 29)  # 2 dropped of the last group


def test_plan_epoch_agrees_with_the_statement_on_a_sweep():
    from smart_nar_fast_tts_amd import data

    for n, bs, gs in dc.PLAN_SWEEP:
        rs = np.random.RandomState(1000 * n + 10 * bs + gs)
        lens, perm = rs.randint(1, 4, size=n), rs.permutation(n)
        for sort in (True, False):
            for drop_last in (True, False):
                got = [b.tolist() for b in data.plan_epoch(lens, bs, gs, sort, drop_last, perm)]
                assert got == dc.plan_statement(lens, bs, gs, sort, drop_last, perm), (n, bs, gs, sort, drop_last)
                used = sorted(i for b in got for i in b)
                assert len(set(used)) == len(used) and (drop_last or used == list(range(n))) and all(len(b) == bs for b in got[:-1])
    assert data.plan_epoch([3, 1], 3) == [] and [b.tolist() for b in data.plan_epoch([3, 1], 3, drop_last=False, perm=[1, 0])] == [[0, 1]]  # n < batch_size
    assert len(data.plan_epoch(np.ones(24), 3, perm=np.arange(24))) == 8  # an empty tail
    import torch

    g = torch.Generator().manual_seed(5)
    want = torch.randperm(13, generator=torch.Generator().manual_seed(5)).numpy()
    assert np.concatenate(data.plan_epoch(np.ones(13), 13, 1, sort=False, generator=g)).tolist() == want.tolist()
    for bad in (dict(batch_size=0), dict(batch_size=2, group_size=0), dict(batch_size=2, perm=[0, 5])):
        with pytest.raises(ValueError):
            data.plan_epoch([1, 2, 3], **bad)


# ---------------------------------------------------------------------------------------------------- the gather on the host
@pytest.mark.parametrize("tag", ["train", "val"])
def test_host_gather_is_the_reference_batch_bit_for_bit(lib, golden, tag):
    L, so = lib
    meta, z = golden
    utts = fixture_utterances(meta, z)
    store = dc.pack(utts)
    index = {n: i for i, n in enumerate(meta["ids"])}
    recs = meta["passes"][tag]
    order = np.array([index[n] for rec in recs for n in rec["ids"]], dtype=np.int32)
    first = 0
    for k, rec in enumerate(recs):
        idxs = order[first:first + len(rec["ids"])].tolist()
        caps = dc.batch_maxima(store, idxs)
        assert (caps[3], caps[0]) == (rec["max_src_len"], rec["max_mel_len"])
        got = host_gather(L, so, store, idxs, caps, order=order, first=first)
        state = dc.collate_statement(utts, idxs)
        for pos, name in dc.TENSORS.items():
            want = z[f"{tag}{k}_{name}"]
            assert str(want.dtype) == rec["dtypes"][name].replace("torch.", "") and dc.same_bits(got[name], want), (tag, k, name)
            assert dc.same_bits(state[pos], want), ("collate_statement", tag, k, name)
            if want.dtype == np.float32:
                assert got[name].view(np.int32).tobytes() == want.view(np.int32).tobytes()
        first += len(idxs)


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_host_gather_is_the_yardstick(lib, name):
    L, so = lib
    utts, store, idxs, caps = dc.case_store(name)
    got = host_gather(L, so, store, idxs, caps)
    assert _same(got, dc.case_want(name)), name
    state = dc.collate_statement(utts, idxs, *caps)
    assert all(dc.same_bits(got[n], state[pos]) for pos, n in dc.TENSORS.items()), name


@pytest.mark.parametrize("mutate", dc.MUTANTS)
def test_each_mutant_is_caught_on_its_named_case(lib, mutate):
    from smart_nar_fast_tts_amd import data

    L, so = lib
    name = dc.CATCHER[mutate]
    if name in dc.CASES:
        _, store, idxs, caps = dc.case_store(name)
        good, bad = dc.case_want(name), dc.case_want(name, mutate)
        assert not _same(bad, good), (mutate, name)
        assert _same(host_gather(L, so, store, idxs, caps), good)
    else:
        c = dc.plan_case(name)
        good = dc.plan_statement(sort=True, drop_last=True, **c)
        bad = dc.plan_statement(sort=True, drop_last=True, mutate=mutate, **c)
        assert bad != good, (mutate, name)
        assert [b.tolist() for b in data.plan_epoch(c["text_lens"], c["batch_size"], c["group_size"], perm=c["perm"])] == good


def test_plan_layout(lib):
    L, so = lib
    tl, ml = np.array([1, 4, 5, 9, 3], dtype=np.int32), np.array([1, 63, 64, 65, 2], dtype=np.int32)
    lens = L.STRUCTS["ns_ds_lens"](tl.ctypes.data, ml.ctypes.data, tl.ctypes.data, ml.ctypes.data)
    off = np.full((4, 6), -1, dtype=np.int64)
    nbytes = (C.c_uint64 * 4)()
    L.check(so.ns_ds_plan(C.byref(lens), 5, 80, C.byref(L.STRUCTS["ns_ds_offsets"](*(off[k].ctypes.data for k in range(4)))), nbytes), "ns_ds_plan")
    assert off[0].tolist() == [0, 1, 64, 128, 193, 195] and nbytes[0] == 195 * 320
    assert off[1].tolist() == dc.layout(tl)[0].tolist() == [0, 4, 8, 16, 28, 32] and off[3].tolist() == off[1].tolist()
    assert off[2].tolist() == dc.layout(ml)[0].tolist() == [0, 4, 68, 132, 200, 204]
    assert all(o % 4 == 0 for o in off[1:].reshape(-1)) and [int(b) for b in nbytes[1:]] == [128, 816, 128]


# ---------------------------------------------------------------------------------------------------- the C ABI
NAMES = ("ns_ds_abi_version", "ns_ds_last_launches", "ns_ds_plan", "ns_ds_gather", "ns_ds_op_gather", "ns_ds_host_gather")


def test_abi_is_declared_everywhere(lib):
    L, so = lib
    assert so.ns_ds_abi_version() == 1 == L.NS["NS_DS_ABI_VERSION"]
    header = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    assert re.findall(r"^#define NS_DS_ABI_VERSION (\d+)\b", header, re.M) == ["1"]
    assert re.findall(r"^#define NS_DS_GRID_CAP (\d+)\b", header, re.M) == [str(L.NS["NS_DS_GRID_CAP"])]
    for name in NAMES:
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    assert L.fields("ns_ds_lens") == ("text", "mel", "pitch", "energy") and L.fields("ns_ds_offsets") == ("mel", "pitch", "energy", "text")
    assert L.fields("ns_ds_batch") == ("mels", "pitches", "energies", "texts", "speakers", "src_lens", "mel_lens", "B", "Tmax", "Pmax", "Emax", "Lmax")
    assert C.sizeof(L.STRUCTS["ns_ds_store"]) == 13 * 8 + 4 * 8 + 8 and C.sizeof(L.STRUCTS["ns_ds_batch"]) == 7 * 8 + 5 * 4 + 4
    build = open(os.path.join(ROOT, "smart-nar_fast_tts_amd", "build.py")).read()
    assert '"dataset.hip"' in build and '"dataset_api.hip"' in build
    # one text for the kernel and the host: both sources take the item functions from dataset.h and define none of their own
    csrc = os.path.join(ROOT, "smart-nar_fast_tts_amd", "csrc")
    assert open(os.path.join(csrc, "dataset.h")).read().count("__host__ __device__ inline void ds_mel_item(") == 1
    for f in ("dataset.hip", "dataset_api.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "dataset.h"' in text and "ds_mel_item(a, " in text and "ds_tail_item(a, " in text and "inline void ds_" not in text, f


def test_every_refusal_precedes_the_first_hip_call(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    utts, store, _, _ = dc.case_store("edges_80")
    idxs = [1, 2, 3, 9]
    caps = dc.batch_maxima(store, idxs[:3])
    DEV = 0x1000000  # a made-up device address: never dereferenced

    def gather(which="host", first=0, B=3, order=idxs, order_len=None, caps=caps, store_edit=None, out_edit=None, n_mel=None, null=None, grid_cap=7,
               order_dev=DEV, table_edit=None):
        st = dict(store)
        if table_edit:
            name, i, v = table_edit
            st[name] = st[name].copy()
            st[name][i] = v
        s, lens = _structs(L, st, n_mel=n_mel)[0], _structs(L, store)[1]  # (the host lengths stay the plan's)
        out = dc.empty_outputs(B if B > 0 else 1, *[max(c, 1) if c < (1 << 20) else 1 for c in caps], store["mel"].shape[1])
        o = _batch(L, out, caps)
        o.B = B
        for obj, edit in ((s, store_edit), (o, out_edit)):
            if edit:
                setattr(obj, edit[0], edit[1] if not callable(edit[1]) else edit[1](getattr(obj, edit[0])))
        od = np.asarray(order, dtype=np.int32)
        a = dict(store=C.byref(s), lens=C.byref(lens), order=od.ctypes.data, out=C.byref(o))
        if null:
            a[null] = None
        n = od.size if order_len is None else order_len
        if which == "host":
            rc = so.ns_ds_host_gather(a["store"], a["lens"], a["order"], n, first, a["out"])
            assert rc != 0 and all((v.view(np.uint8) == dc.CANARY).all() for v in out.values()), "a refused host gather writes nothing"
            return rc
        if which == "gather":
            return so.ns_ds_gather(a["store"], a["lens"], order_dev, a["order"], n, first, a["out"], None)
        return so.ns_ds_op_gather(a["store"], a["lens"], order_dev, a["order"], n, first, a["out"], grid_cap, None)

    T, P, E, Lm = caps
    shared = (
        (dict(null="store"), "null argument"), (dict(null="lens"), "null argument"), (dict(null="order"), "null argument"), (dict(null="out"), "null argument"),
        (dict(store_edit=("pitch", None)), "null pointer in the store"), (dict(store_edit=("text_off", None)), "null pointer in the store"),
        (dict(store_edit=("mel_len", None)), "null pointer in the store"), (dict(out_edit=("mels", None)), "null pointer in the batch"),
        (dict(out_edit=("src_lens", None)), "null pointer in the batch"),
        (dict(store_edit=("mel", lambda p: p + 4)), "store->mel must be 16-byte aligned"), (dict(store_edit=("text", lambda p: p + 8)), "store->text must be 16-byte aligned"),
        (dict(store_edit=("pitch_off", lambda p: p + 4)), "store->pitch_off must be 8-byte aligned"),
        (dict(store_edit=("speaker", lambda p: p + 2)), "store->speaker must be 4-byte aligned"),
        (dict(out_edit=("mels", lambda p: p + 8)), "out->mels must be 16-byte aligned"), (dict(out_edit=("texts", lambda p: p + 4)), "out->texts must be 8-byte aligned"),
        (dict(out_edit=("pitches", lambda p: p + 1)), "out->pitches must be 4-byte aligned"),
        (dict(n_mel=6), "n_mel must be a multiple of 4 in [4, 128], got 6"), (dict(n_mel=0), "n_mel must be a multiple of 4"), (dict(n_mel=132), "n_mel must be a multiple of 4"),
        (dict(store_edit=("N", 0)), "N must be positive"), (dict(store_edit=("N", -2)), "N must be positive"),
        (dict(B=0), "B must be positive"), (dict(B=-1), "B must be positive"),
        (dict(first=2), "first + B must not pass the order's length: first 2, B 3, order_len 4"), (dict(first=-1), "first + B must not pass"),
        (dict(order_len=2), "first + B must not pass"), (dict(first=1 << 40), "first + B must not pass"),
        (dict(order=[1, 10, 3]), "order[1] = 10 is outside [0, N = 10)"), (dict(order=[-1, 2, 3]), "order[0] = -1 is outside"),
        (dict(caps=(T - 1, P, E, Lm)), f"Tmax = {T - 1} is below the batch's own maximum {T}"), (dict(caps=(T, P - 1, E, Lm)), f"Pmax = {P - 1} is below"),
        (dict(caps=(T, P, 0, Lm)), "Emax = 0 is below"), (dict(caps=(T, P, E, Lm - 1)), f"Lmax = {Lm - 1} is below the batch's own maximum {Lm}"),
        (dict(caps=((1 << 31) // (3 * 80) + 1, P, E, Lm)), "every output must stay below 2^31 elements"),
        (dict(caps=(T, (1 << 31) // 3 + 1, E, Lm)), "every output must stay below 2^31 elements"),
        (dict(store_edit=("mel_rows", 0)), "the store's sizes must be positive"))
    for which in ("host", "gather", "op"):
        expect_refusals(err, lambda **kw: gather(which=which, **kw), shared)  # noqa: B023
        assert so.ns_ds_last_launches() == 0
    expect_refusals(err, lambda **kw: gather(which="host", **kw), (
        (dict(table_edit=("pitch_off", 2, 67)), "store->pitch_off is not one ns_ds_plan wrote (entry 2 is 67"),
        (dict(table_edit=("mel_off", 0, 1)), "store->mel_off is not one ns_ds_plan wrote (entry 0 is 1, the plan's is 0)"),
        (dict(table_edit=("text_off", 10, 0)), "store->text_off is not one ns_ds_plan wrote (entry 10"),
        (dict(table_edit=("energy_len", 4, 3)), "store->energy_len[4] is not the positive length lens states"),
        (dict(store_edit=("text_elems", 8)), "store->text is stated shorter")))
    expect_refusals(err, lambda **kw: gather(which="gather", **kw), ((dict(order_dev=None), "null argument"), (dict(order_dev=DEV + 2), "order_dev must be 4-byte aligned")))
    expect_refusals(err, lambda **kw: gather(which="op", **kw), ((dict(grid_cap=0), "grid_cap must lie in [1, 2048], got 0"), (dict(grid_cap=2049), "grid_cap must lie in"),
                                                                 (dict(order_dev=None), "null argument")))
    assert so.ns_ds_last_launches() == 0

    # ns_ds_plan
    tl, ml = store["text_len"], store["mel_len"]
    off = np.zeros((4, len(tl) + 1), dtype=np.int64)
    nbytes = (C.c_uint64 * 4)()

    def plan(N=len(tl), n_mel=80, lens=True, offs=True, out=True, null_len=None, null_off=None, bad=None):
        v = dict(text=tl, mel=ml, pitch=ml, energy=ml)
        if bad:
            v[bad[0]] = v[bad[0]].copy()
            v[bad[0]][bad[1]] = bad[2]
        ls = L.STRUCTS["ns_ds_lens"](*(None if null_len == k else v[k].ctypes.data for k in ("text", "mel", "pitch", "energy")))
        of = L.STRUCTS["ns_ds_offsets"](*(None if null_off == k else off[k].ctypes.data for k in range(4)))
        return so.ns_ds_plan(C.byref(ls) if lens else None, N, n_mel, C.byref(of) if offs else None, nbytes if out else None)

    expect_refusals(err, plan, ((dict(lens=False), "null argument"), (dict(offs=False), "null argument"), (dict(out=False), "null argument"),
                                (dict(null_len="pitch"), "null argument"), (dict(null_off=2), "null argument"), (dict(N=0), "N must be positive"),
                                (dict(N=-1), "N must be positive"), (dict(n_mel=2), "n_mel must be a multiple of 4 in [4, 128], got 2"),
                                (dict(n_mel=129), "n_mel must be a multiple of 4"), (dict(bad=("mel", 3, 0)), "lens->mel[3] must be positive, got 0"),
                                (dict(bad=("text", 0, -4)), "lens->text[0] must be positive, got -4")))
    assert plan() == 0 and plan(n_mel=4) == 0 and plan(n_mel=128) == 0


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    out = run_c_caller("ds_host_only", lib[0].LIB_PATH, tmp_path)
    assert "gathered on the host" in out


def test_the_kernel_does_not_spill():
    assert_no_spill("dataset.hip", kernels=("k_ds_gather",))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_from_arrays_raises(lib, golden):
    import torch

    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import data, training

    assert pkg.data is data and pkg.DeviceDataset is data.DeviceDataset and "data" in pkg.__all__ and callable(training.fit)
    meta, z = golden
    u = fixture_utterances(meta, z)
    pcfg = wl.preprocess_config(meta["pitch"], meta["energy"])

    def build(pcfg=pcfg, device="cuda", **edit):
        v = dict(u, **edit)
        return data.DeviceDataset.from_arrays(v["ids"], v["raw_texts"], v["speakers"], v["texts"], v["mels"], v["pitches"], v["energies"], pcfg, device)

    short = list(u["pitches"])
    short[4] = short[4][:-1] if len(short[4]) > 1 else np.zeros(2, dtype=np.float32)
    with pytest.raises(ValueError, match=r"utterance 'utt0004': pitch is frame_level, so it must hold \d+ values \(T\)"):
        build(pitches=short)
    with pytest.raises(ValueError, match=r"utterance 'utt0004': energy is frame_level"):
        build(energies=short)
    with pytest.raises(ValueError, match=r"utterance 'utt000\d': pitch is phoneme_level, so it must hold \d+ values \(L\)"):
        build(pcfg=wl.preprocess_config("phoneme_level", meta["energy"]))  # the set's pitch is frame level: T values, not L
    narrow = list(u["mels"])
    narrow[2] = narrow[2][:, :64]
    with pytest.raises(ValueError, match=r"utterance 'utt0002': the mel must be \[T, n_mel = 80\]"):
        build(mels=narrow)
    pc2 = wl.preprocess_config(meta["pitch"], meta["energy"])
    pc2["preprocessing"]["mel"]["n_mel_channels"] = 64
    with pytest.raises(ValueError, match=r"utterance 'utt0000': the mel must be \[T, n_mel = 64\]"):
        build(pcfg=pc2)
    with pytest.raises(ValueError, match="must have one length"):
        build(ids=u["ids"][:-1])
    pc3 = wl.preprocess_config(meta["pitch"], meta["energy"])
    pc3["preprocessing"]["energy"]["feature"] = "word_level"
    with pytest.raises(ValueError, match="preprocessing.energy.feature"):
        build(pcfg=pc3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        build(device=torch.device("cpu"))
    with pytest.raises(TypeError, match="from_arrays"):
        data.DeviceDataset()
