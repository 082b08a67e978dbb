"""The keep-mask generator on the CPU (no GPU): tests/keepmask_cpu.py's yardstick against the known answers and against the library's
host entry points (ns_km_op_philox, ns_km_host_draw: the inline functions the kernel compiles), every refusal of the ns_km_* family
through the library and through a plain-C caller, the plan's layout, the Python state's round trip, and the statistics of the
definition.

The statistics are conditions on the yardstick: a keep rate within 5 sigma of thr / 2^32 (sigma = sqrt(q (1 - q) / n)) over 72 draws
of 512000 elements (measured worst when written: 2.93 sigma), and an agreement within 5 sigma of one half (sigma = 0.5 / sqrt(n))
between a p = 0.5 mask and five neighbours (measured: at most 1.6 sigma)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import keepmask_cpu as kc
from tests.util import ROOT, assert_no_spill, built_lib, expect_refusals, run_c_caller


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def _plan(L, so, masks):
    """(table bytes as a numpy array, arena bytes) of ns_km_plan"""
    n = len(masks)
    arr = (L.NsKmMask * n)()
    for i, (cnt, stream, thr) in enumerate(masks):
        arr[i].n, arr[i].stream, arr[i].thr = cnt, stream, thr
    nbytes = so.ns_km_table_bytes(n)
    assert nbytes == (n + 1) * 32
    table = np.zeros(nbytes, dtype=np.uint8)
    need = C.c_uint64(0)
    L.check(so.ns_km_plan(arr, n, table.ctypes.data, nbytes, C.byref(need)), "ns_km_plan")
    return table, int(need.value)


def _host_draw(L, so, masks, seed, call, slack=0):
    table, need = _plan(L, so, masks)
    a = np.full(need + slack, kc.CANARY, dtype=np.uint8)
    L.check(so.ns_km_host_draw(table.ctypes.data, len(masks), seed, call, a.ctypes.data, a.size), "ns_km_host_draw")
    return a


# ---------------------------------------------------------------------------------------------------- the definition
def test_known_answers_through_the_yardstick_and_the_library(lib):
    L, so = lib
    U4, U2 = C.c_uint32 * 4, C.c_uint32 * 2
    for ctr, key, want in kc.KNOWN:
        got = [int(v) for v in kc.philox(*ctr, *key)]
        assert tuple(got) == want, [hex(v) for v in got]
        out = U4()
        assert so.ns_km_op_philox(U4(*ctr), U2(*key), out) == 0
        assert tuple(out) == want, [hex(v) for v in out]
    assert tuple(kc.mask(1234, 1, 0, 32, kc.threshold(0.2))) == kc.FIRST_32


def test_thresholds(lib):
    L, so = lib
    for p, want in kc.THRESHOLDS:
        thr = C.c_uint32(0)
        assert so.ns_km_threshold(p, C.byref(thr)) == 0 and thr.value == want == kc.threshold(p), p
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    thr = C.c_uint32(0)

    def call(p=0.2, out=True):
        return so.ns_km_threshold(p, C.byref(thr) if out else None)

    expect_refusals(err, call, ((dict(out=False), "null argument"), (dict(p=0.0), "p must lie in (0, 1)"), (dict(p=1.0), "p must lie in (0, 1)"),
                                (dict(p=-0.1), "p must lie in (0, 1)"), (dict(p=1.5), "p must lie in (0, 1)"), (dict(p=float("nan")), "p must lie in (0, 1)"),
                                (dict(p=1.0 - 2.0 ** -33), "the threshold would be 0"), (dict(p=2.0 ** -60), "does not fit 32 bits")))
    for p in (0.0, 1.0, 1.0 - 2.0 ** -33, 2.0 ** -60, float("nan")):
        with pytest.raises(ValueError):
            kc.threshold(p)


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_host_draw_is_the_yardstick(lib, name):
    L, so = lib
    c = kc.CASES[name]
    got = _host_draw(L, so, c["masks"], c["seed"], c["call"], slack=48)
    want = kc.case_arena(name, slack=48)
    assert got.tobytes() == want.tobytes(), name
    assert (got[-48:] == kc.CANARY).all() and so.ns_km_last_launches() == 0


def test_a_mask_does_not_depend_on_its_neighbours(lib):
    L, so = lib
    c = kc.CASES["mixed"]
    whole = _host_draw(L, so, c["masks"], c["seed"], c["call"])
    offs, _ = kc.layout([m[0] for m in c["masks"]])
    for off, m in zip(offs, c["masks"]):
        alone = _host_draw(L, so, [m], c["seed"], c["call"])
        assert whole[off:off + alone.size].tobytes() == alone.tobytes(), m


@pytest.mark.parametrize("mutate", kc.MUTANTS)
def test_each_mutant_differs_on_its_named_case(lib, mutate):
    L, so = lib
    name = kc.CATCHER[mutate]
    c = kc.CASES[name]
    good, bad = kc.case_arena(name), kc.case_arena(name, mutate)
    assert good.tobytes() != bad.tobytes(), (mutate, name)
    assert _host_draw(L, so, c["masks"], c["seed"], c["call"]).tobytes() == good.tobytes()


def test_plan_layout(lib):
    L, so = lib
    ns = (1, 15, 16, 17, 4095, 4096, 4097, 100000)
    table, need = _plan(L, so, [(n, 10 + i, 7 + i) for i, n in enumerate(ns)])
    offs, total = kc.layout(ns)
    rows = table.view(np.dtype([("offset", "<u8"), ("n", "<u8"), ("stream", "<u4"), ("thr", "<u4"), ("chunk_begin", "<u8")]))
    assert need == total == sum((n + 15) // 16 * 16 for n in ns) and len(rows) == len(ns) + 1
    assert [int(o) for o in rows["offset"][:-1]] == offs and all(o % 16 == 0 for o in offs)
    assert [int(v) for v in rows["n"][:-1]] == list(ns) and [int(v) for v in rows["stream"][:-1]] == [10 + i for i in range(len(ns))]
    assert [int(v) for v in rows["thr"][:-1]] == [7 + i for i in range(len(ns))]
    chunks = np.cumsum([0] + [(n + 4095) // 4096 for n in ns])
    assert [int(v) for v in rows["chunk_begin"]] == [int(v) for v in chunks]
    assert int(rows["offset"][-1]) == total and int(rows["n"][-1]) == 0
    assert L.KM_MAX_MASKS >= 256 and so.ns_km_table_bytes(L.KM_MAX_MASKS) == (L.KM_MAX_MASKS + 1) * L.KM_TABLE_ROW_BYTES


# ---------------------------------------------------------------------------------------------------- the C ABI
NAMES = ("ns_km_abi_version", "ns_km_last_launches", "ns_km_threshold", "ns_km_table_bytes", "ns_km_plan", "ns_km_draw", "ns_km_op_philox",
         "ns_km_host_draw")


def test_abi_is_declared_everywhere(lib):
    L, so = lib
    assert so.ns_km_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    assert re.findall(r"^#define NS_KM_ABI_VERSION (\d+)\b", header, re.M) == ["1"]
    for macro, value in (("NS_KM_MAX_MASKS", L.KM_MAX_MASKS), ("NS_KM_GRID_CAP", L.KM_GRID_CAP), ("NS_KM_TABLE_ROW_BYTES", L.KM_TABLE_ROW_BYTES)):
        assert re.findall(rf"^#define {macro} (\d+)\b", header, re.M) == [str(value)], macro
    for name in NAMES:
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\(", header), name
    assert [f for f, _ in L.NsKmMask._fields_] == ["n", "stream", "thr"] and C.sizeof(L.NsKmMask) == 16
    build = open(os.path.join(ROOT, "smart-nar_fast_tts_amd", "build.py")).read()
    assert '"keepmask.hip"' in build and '"keepmask_api.hip"' in build
    # one text for the kernel and the host: both sources take the round function from the header and define none of their own
    csrc = os.path.join(ROOT, "smart-nar_fast_tts_amd", "csrc")
    assert open(os.path.join(csrc, "keepmask.h")).read().count("__host__ __device__ inline KmWords km_philox4x32_10(") == 1
    for f in ("keepmask.hip", "keepmask_api.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "keepmask.h"' in text and "0xD2511F53" not in text and "km_draw16(" in text, f


def test_every_refusal_precedes_the_first_hip_call(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    good = [(100, 0, 5), (17, 1, 6)]
    buf = np.zeros(32 * 3, dtype=np.uint8)
    need = C.c_uint64(0)

    def plan(masks=good, n=None, table=True, nbytes=None, out=True, null_masks=False):
        arr = (L.NsKmMask * max(len(masks), 1))()
        for i, (cnt, stream, thr) in enumerate(masks):
            arr[i].n, arr[i].stream, arr[i].thr = cnt, stream, thr
        return so.ns_km_plan(None if null_masks else arr, len(masks) if n is None else n, buf.ctypes.data if table else None,
                             buf.size if nbytes is None else nbytes, C.byref(need) if out else None)

    expect_refusals(err, plan, (
        (dict(null_masks=True), "null argument"), (dict(table=False), "null argument"), (dict(out=False), "null argument"),
        (dict(n=0), "n_masks must lie in [1, 1024]"), (dict(n=-1), "n_masks must lie in"), (dict(n=1025), "n_masks must lie in [1, 1024]"),
        (dict(masks=[(100, 0, 5), (0, 1, 6)]), "masks[1].n must be positive"), (dict(masks=[(1 << 34, 0, 5)]), "masks[0].n must stay below 2^34"),
        (dict(masks=[(100, 0, 0)]), "masks[0].thr must not be 0"), (dict(nbytes=95), "table too small (ns_km_table_bytes)"),
        (dict(nbytes=0), "table too small")))
    assert plan() == 0 and need.value == 112 + 32
    assert plan(masks=[((1 << 34) - 1, 0, 1)], nbytes=64) == 0 and need.value == 1 << 34
    for n in (0, -3, 1025):
        assert so.ns_km_table_bytes(n) == 0 and "n_masks must lie in [1, 1024]" in err()

    def draw(table=0x1000000, n=2, arena=0x2000000, nbytes=144):
        return so.ns_km_draw(P(table), n, 1, 1, P(arena), nbytes, None)

    expect_refusals(err, draw, (
        (dict(table=0), "null argument"), (dict(arena=0), "null argument"), (dict(n=0), "n_masks must lie in [1, 1024]"),
        (dict(n=1025), "n_masks must lie in"), (dict(table=0x1000004), "the table must be 8-byte aligned"),
        (dict(arena=0x2000008), "the arena must be 16-byte aligned"), (dict(nbytes=31), "arena too small"), (dict(nbytes=0), "arena too small")))
    assert so.ns_km_last_launches() == 0

    U4, U2 = C.c_uint32 * 4, C.c_uint32 * 2
    for args in ((None, U2(), U4()), (U4(), None, U4()), (U4(), U2(), None)):
        assert so.ns_km_op_philox(*args) != 0 and "null argument" in err()

    table, total = _plan(L, so, good)
    arena = np.zeros(total, dtype=np.uint8)

    def host(t=None, n=2, a=True, nbytes=None, edit=None):
        t = table.copy() if t is None else t
        if edit:
            rows = t.view(np.dtype([("offset", "<u8"), ("n", "<u8"), ("stream", "<u4"), ("thr", "<u4"), ("chunk_begin", "<u8")]))
            row, field, value = edit
            rows[field][row] = value
        return so.ns_km_host_draw(t.ctypes.data if t is not False else None, n, 1, 1, arena.ctypes.data if a else None, total if nbytes is None else nbytes)

    expect_refusals(err, host, (
        (dict(t=False), "null argument"), (dict(a=False), "null argument"), (dict(n=0), "n_masks must lie in"), (dict(nbytes=total - 1), "arena too small"),
        (dict(edit=(1, "offset", 96)), "not one ns_km_plan wrote"), (dict(edit=(0, "n", 0)), "masks[0].n must be positive"),
        (dict(edit=(1, "thr", 0)), "masks[1].thr must not be 0"), (dict(edit=(0, "n", 1 << 34)), "must stay below 2^34")))
    assert not arena.any(), "a refused host draw writes nothing"


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    out = run_c_caller("km_host_only", lib[0].LIB_PATH, tmp_path)
    assert "first 32" in out


def test_the_kernel_does_not_spill():
    assert_no_spill("keepmask.hip", kernels=("k_km_draw",))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_rng_state_round_trip(lib, tmp_path):
    import torch

    import smart_nar_fast_tts_amd as pkg
    from smart_nar_fast_tts_amd import dropout, training

    assert pkg.dropout is dropout and pkg.KeepMaskRNG is dropout.KeepMaskRNG and "dropout" in pkg.__all__
    rng = dropout.KeepMaskRNG((1 << 63) + 5)
    assert rng.state_dict() == {"version": 1, "seed": (1 << 63) + 5, "call": 0, "stream": 0} and rng.launches == 0
    rng.next_call()
    rng.next_call()
    rng.stream = 7
    rng.call += 1 << 40
    path = str(tmp_path / "rng.pt")
    torch.save({"keep_mask_rng": rng.state_dict()}, path)
    state = torch.load(path, weights_only=True)["keep_mask_rng"]
    assert all(type(v) is int for v in state.values())
    other = dropout.KeepMaskRNG(0)
    other.load_state_dict(state)
    assert other.state_dict() == rng.state_dict() and other.call == (1 << 40) + 2
    other.next_call()
    assert (other.call, other.stream) == ((1 << 40) + 3, 0)
    with pytest.raises(ValueError, match="version"):
        other.load_state_dict(dict(state, version=2))
    with pytest.raises(ValueError, match="out of range"):
        other.load_state_dict(dict(state, stream=1 << 32))
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed must lie in"):
            dropout.KeepMaskRNG(seed)
    for p, want in kc.THRESHOLDS:
        assert dropout.threshold(p) == want
    with pytest.raises(RuntimeError, match="p must lie in"):
        dropout.threshold(0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rng.take([(2, 3, 4)], 0.2, torch.device("cpu"))

    # attach / detach reach every trainable HIP layer and the model; save_checkpoint writes the third key only with rng
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd._train import HipTrainModule

    m = training.FastSpeech2Align(wl.preprocess_config(), wl.model_config("tiny"))
    layers = [x for x in m.modules() if isinstance(x, HipTrainModule)]
    assert len(layers) >= 12 and {"Prenet", "PostNet", "VariancePredictor", "MultiHeadAttention"} <= {type(x).__name__ for x in layers} and all(x._keep_mask_rng is None for x in layers) and m._keep_mask_rng is None
    assert dropout.attach(m, rng) is m and all(x._keep_mask_rng is rng for x in layers) and m._keep_mask_rng is rng
    assert "_keep_mask_rng" not in m.state_dict() and not any("keep_mask" in k for k in m.state_dict())
    dropout.detach(m)
    assert all(x._keep_mask_rng is None for x in layers) and m._keep_mask_rng is None
    with pytest.raises(TypeError, match="KeepMaskRNG"):
        dropout.attach(m, torch.Generator())
    with pytest.raises(ValueError, match="no trainable HIP layer"):
        dropout.attach(torch.nn.Linear(2, 2), rng)

    class Opt:
        class _optimizer:
            @staticmethod
            def state_dict():
                return {"state": {}, "param_groups": [{"lr": np.float64(0.5), "betas": (0.9, 0.98)}]}

    training.save_checkpoint(m, Opt, str(tmp_path / "a.pt"))
    training.save_checkpoint(m, Opt, str(tmp_path / "b.pt"), rng=rng)
    a, b = (torch.load(str(tmp_path / f), weights_only=True) for f in ("a.pt", "b.pt"))
    assert sorted(a) == ["model", "optimizer"] and sorted(b) == ["keep_mask_rng", "model", "optimizer"] and b["keep_mask_rng"] == rng.state_dict()


def test_the_models_mask_list(lib):
    """training.FastSpeech2Align._step_masks on the ljspeech config: the 40 masks of the issue's table, in the forward's order"""
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import training

    cfg = wl.model_config("ljspeech")
    m = training.FastSpeech2Align(wl.preprocess_config(), cfg).train()
    B, L, T = 16, 128, 1000
    got = m._step_masks({}, B, L, T, T)
    t, F = cfg["transformer"], cfg["variance_predictor"]["filter_size"]
    pe, pd, pv = t["encoder_dropout"], t["decoder_dropout"], cfg["variance_predictor"]["dropout"]
    levels = (m.variance_adaptor.pitch_feature_level, m.variance_adaptor.energy_feature_level)
    rows = [L if lv == "phoneme_level" else T for lv in levels]
    preds = [("pitch", rows[0], levels[0]), ("energy", rows[1], levels[1])]
    preds = [x for x in preds if x[2] == "phoneme_level"] + [x for x in preds if x[2] == "frame_level"]
    n_enc, n_dec = t["encoder_layer"], t["decoder_layer"]  # (the aligner has decoder_layer layers as well)
    want = ([((B, L, 256), pe)] * (2 * n_enc) + [((B, T, 256), 0.2)] + [((B, T, 256), pd)] * (2 * n_dec)
            + [((B, L, F), pv)] * 2 + [((B, r, F), pv) for _, r, _ in preds for _ in range(2)] + [((B, T, 256), pd)] * (2 * n_dec)
            + [((B, T, c), 0.5) for c in (512, 512, 512, 512, 80)])
    total = 2 * n_enc + 1 + 2 * n_dec + 6 + 2 * n_dec + 5  # 36 at this project's ljspeech config (4 + 4 + 4 layers)
    assert len(m.mel_encoder.layer_stack) == len(m.mel_decoder.layer_stack) == n_dec
    assert got == want and len(got) == total == 36
    # a part whose masks are given, or that is in eval(), asks for none
    assert len(m._step_masks({"postnet": [None] * 5, "prenet": object()}, B, L, T, T)) == total - 5 - 1
    assert len(m._step_masks({"variance_adaptor": {"pitch": (1, 2)}}, B, L, T, T)) == total - 2
    m.postnet.eval()
    assert len(m._step_masks({}, B, L, T, T)) == total - 5
    assert m.eval()._step_masks({}, B, L, T, T) == []
    # a train() stack cuts its rows at max_seq_len
    m.train()
    cutoff = cfg["max_seq_len"]
    long = m._step_masks({}, B, L, cutoff + 9, cutoff + 9)
    assert long[2 * n_enc] == ((B, cutoff, 256), 0.2) and long[-1] == ((B, cutoff, 80), 0.5)
    assert (((B, cutoff + 9, F), pv) in long) == ("frame_level" in levels)  # the regulator's rows are not cut; the decoder's are


# ---------------------------------------------------------------------------------------------------- statistics of the definition
N_STAT = 512000


def test_keep_rate():
    worst = 0.0
    for seed in (0, 1234, (1 << 63) + 5):
        for p in kc.PS:
            thr = kc.threshold(p)
            q = thr / 2.0 ** 32
            sigma = np.sqrt(q * (1.0 - q) / N_STAT)
            for stream in range(4):
                for call in (1, 2):
                    rate = kc.mask(seed, call, stream, N_STAT, thr).mean()
                    worst = max(worst, abs(rate - q) / sigma)
    print("worst keep-rate deviation, sigma:", worst)
    assert worst <= 5.0, worst


def test_agreement_with_neighbours():
    thr = kc.threshold(0.5)
    base = kc.mask(1234, 1, 0, N_STAT, thr)
    sigma = 0.5 / np.sqrt(N_STAT)
    other = {"stream 1": kc.mask(1234, 1, 1, N_STAT, thr), "call 2": kc.mask(1234, 2, 0, N_STAT, thr), "seed 1235": kc.mask(1235, 1, 0, N_STAT, thr)}
    dev = {k: abs((base == v).mean() - 0.5) / sigma for k, v in other.items()}
    for shift in (1, 256):
        dev[f"shift {shift}"] = abs((base[shift:] == base[:-shift]).mean() - 0.5) / (0.5 / np.sqrt(N_STAT - shift))
    print("agreement deviations, sigma:", dev)
    assert max(dev.values()) <= 5.0, dev
