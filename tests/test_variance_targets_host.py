"""Variance targets and dataset statistics, everything that needs no GPU: the float64 restatement (tests/variance_targets_cpu.py) against
the values captured from the reference's own Preprocessor.build_from_path, the in-place loop against the closed form, every mutant
rejected by its gate, the ns_vt_* C ABI's host side (versions, size function, every refusal), the plain-C caller, the stats.json
round trip and the kernels' register hygiene."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from smart_nar_fast_tts_amd import _lib
from tests import variance_targets_cpu as vc
from tests.util import assert_no_spill, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("variance_targets_tiny", "variance_targets_edges")


def batch_of(z, L):
    return {"pitch": z["pitch"], "energy": z["energy"], "durations_padded": z["durations_padded"], "durations": z["durations_padded"][:, :L],
            "src_lens": z["src_lens"]}


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_what_fixture_batch_builds_and_meets_the_preconditions(name):
    meta, z = load_golden(name)
    fb = vc.fixture_batch(meta["config"], meta["seed"])
    for k in ("pitch", "energy", "durations_padded", "src_lens"):
        assert np.array_equal(fb[k], z[k]), k
    batch = batch_of(z, meta["L"])
    free = [b for b in range(meta["B"]) if vc.alias_free(batch["durations"][b], int(batch["src_lens"][b]))]
    assert free == z["ref_utts"].tolist()
    for p_level, e_level in meta["combos"]:
        full = vc.pipeline(batch, p_level, e_level)
        vc.check_preconditions(batch, full)  # no value within relative 1e-5 of an outlier bound, no valid decision at its mercy
    if meta["config"] == "edges":
        d, sl = batch["durations"], batch["src_lens"]
        assert meta["replica"] == [0, 1] and np.array_equal(z["pitch"][0], z["pitch"][1]) and np.array_equal(d[0], d[1])
        assert d[0, 0] == 0 and d[0, 150] == 0 and d[0, 299] == 0 and d[0].sum() == meta["T"] and d[2, :sl[2]].sum() < meta["T"]
        c = np.cumsum(d[0])
        i = int(np.searchsorted(c, 256, side="right"))
        assert c[i] - d[0, i] < 256 < c[i], "a phoneme straddles the first 256-frame tile"
        assert np.all(z["pitch"][0, 500:530] == 0) and z["pitch"][0, 499] != 0 and z["pitch"][0, 530] != 0, "an unvoiced run straddles frame 512"
        assert sl[2] < meta["L"] and int(np.sum(z["pitch"][3, :900] != 0)) == 1
        assert full["valid"].tolist() == [1, 1, 1, 0]
    else:
        assert int(np.sum(z["pitch"][3] != 0)) == 2 and full["valid"].all()


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    """Raw: the reference's float64 pitch files to 1e-12 relative, its fp32 energy files to n 2^-24 (n = the longest segment).
    stats.json: mean / std to 1e-6 of max(|mean|, std); min / max and the normalised files under the normalised-value gate."""
    meta, z = load_golden(name)
    batch = batch_of(z, meta["L"])
    free = z["ref_utts"].tolist()
    for p_level, e_level in meta["combos"]:
        key = vc.combo_key(p_level, e_level)
        sub = vc.pipeline(batch, p_level, e_level, only=free)
        full = vc.pipeline(batch, p_level, e_level)
        assert np.array_equal(full["frame_lens"], z[f"cpu_{key}_frame_lens"]) and np.array_equal(full["valid"], z[f"cpu_{key}_valid"])
        for f in ("pitch", "energy"):
            assert np.array_equal(full[f]["raw64"], z[f"cpu_{key}_{f}_raw"]) or np.allclose(full[f]["raw64"], z[f"cpu_{key}_{f}_raw"], rtol=1e-14, atol=0)
            ref_raw, ref_norm, ref_len = z[f"ref_{key}_{f}_raw"], z[f"ref_{key}_{f}_norm"], z[f"ref_{key}_{f}_len"]
            rs = meta["ref_stats"][key][f]
            mean, std = rs[2], rs[3]
            scale = max(abs(mean), std)
            s = sub["stats"][f]
            assert abs(s[2] - mean) <= 1e-6 * scale and abs(s[3] - std) <= 1e-6 * scale, (key, f, s, rs)
            worst = 0.0
            for b in range(meta["B"]):
                n = int(ref_len[b])
                assert n == int(sub[f]["n"][b]), (key, f, b)
                if n == 0:
                    continue
                want = sub[f]["raw64"][b, :n]
                if bool(z[f"ref_{key}_{f}_is_f64"]):
                    tol = 1e-12 * np.abs(want)
                else:
                    tol = max(1, int(batch["durations"][b, :batch["src_lens"][b]].max())) * vc.U24 * np.abs(want)
                assert np.all(np.abs(ref_raw[b, :n] - want) <= tol), (key, f, b)
                gate = vc.norm_gate(sub[f]["raw32"][b, :n], mean, std)
                err = np.abs(sub[f]["norm"][b, :n] - ref_norm[b, :n])
                # the reference normalises its own (unrounded, or fp32-summed) raw values: add that distance, scaled by 1 / std
                slack = np.abs(ref_raw[b, :n] - sub[f]["raw32"][b, :n]) / std
                worst = max(worst, float(np.max(err / (gate + slack + 1e-300))))
                assert np.all(err <= gate + slack), (key, f, b)
            # |min a - min b| <= the larger per-value bound at the two argmins (the restatement's and the reference's); max alike
            sel = np.arange(ref_norm.shape[1])[None, :] < ref_len[:, None]
            bound = (vc.norm_gate(sub[f]["raw32"], mean, std) + np.abs(ref_raw - sub[f]["raw32"]) / std)[sel]
            for k, arg in ((0, np.argmin), (1, np.argmax)):
                g = max(bound[arg(sub[f]["norm"][sel])], bound[arg(ref_norm[sel])])
                print(name, key, f, "min" if k == 0 else "max", "vs reference: error", abs(s[k] - rs[k]), "bound", g)
                assert abs(s[k] - rs[k]) <= g, (key, f, k, s, rs)
            print(name, key, f, "normalised vs reference, worst share of the gate:", round(worst, 4))


def test_inplace_form_equals_closed_form_exactly_where_alias_free():
    for name in FIXTURES:
        meta, z = load_golden(name)
        batch = batch_of(z, meta["L"])
        L = meta["L"]
        for b in range(meta["B"]):
            Ls = int(batch["src_lens"][b])
            d = batch["durations"][b, :Ls]
            n = vc.frame_count(batch["durations"][b], Ls, meta["T"])
            e = batch["energy"][b, :n].astype(np.float64)
            closed = vc.phoneme_mean(e, batch["durations"][b], Ls, L)[:Ls]
            if vc.alias_free(d, Ls):
                assert np.array_equal(vc.phoneme_mean_inplace(e, d), closed), (name, b)
            else:
                assert not np.array_equal(vc.phoneme_mean_inplace(e, d), closed), (name, b)
    # sum(d) < Ls: the reference's loop raises where the closed form is defined
    with pytest.raises(IndexError):
        vc.phoneme_mean_inplace(np.arange(3, dtype=np.float64), np.array([1, 1, 1, 0, 0]))
    assert not vc.alias_free(np.array([1, 1, 1, 0, 0]), 5)


# mutant -> (level of both features, the part of the result it must push out of its gate)
MUTANT_PART = {"segment_off_by_one": ("phoneme_level", "raw"), "zero_duration_nan": ("phoneme_level", "raw"), "no_interpolation": ("phoneme_level", "raw_pitch"),
               "nearest_interpolation": ("phoneme_level", "raw_pitch"), "zero_edge_fill": ("phoneme_level", "raw_pitch"), "no_trim": ("frame_level", "raw"),
               "nonstrict_outlier": ("frame_level", "meanstd"), "nearest_percentile": ("frame_level", "meanstd"), "ddof_1": ("frame_level", "meanstd"),
               "minmax_filtered": ("frame_level", "minmax"), "divide_by_variance": ("frame_level", "norm")}


@pytest.mark.parametrize("mutant", [m for m in vc.MUTANTS if m != "multiply_by_mask"])
def test_gate_rejects_mutant(mutant):
    level, part = MUTANT_PART[mutant]
    hit = False
    for name in FIXTURES:
        meta, z = load_golden(name)
        batch = batch_of(z, meta["L"])
        good, bad = vc.pipeline(batch, level, level), vc.pipeline(batch, level, level, mutate=mutant)
        for f in ("pitch", "energy"):
            if part == "raw_pitch" and f == "energy":
                continue
            if part.startswith("raw"):
                with np.errstate(invalid="ignore"):
                    ok = vc.raw_gate_ok(bad[f]["raw64"].astype(np.float32), good[f]["raw64"])
                hit |= not ok.all() or not np.array_equal(bad["frame_lens"], good["frame_lens"])
            elif part == "meanstd":
                hit |= (abs(bad[f]["mean_raw"] - good[f]["mean_raw"]) > 1e-10 * abs(good[f]["mean_raw"])
                        or abs(bad[f]["std_raw"] - good[f]["std_raw"]) > 1e-10 * good[f]["std_raw"])
            else:
                mean, std = good["stats"][f][2:]
                if part == "minmax":
                    g = vc.extrema_gates(good[f], mean, std)
                    hit |= abs(bad["stats"][f][0] - good["stats"][f][0]) > g[0] or abs(bad["stats"][f][1] - good["stats"][f][1]) > g[1]
                else:
                    hit |= bool(np.any(np.abs(bad[f]["norm"] - good[f]["norm"]) > vc.norm_gate(good[f]["raw32"], mean, std)))
    assert hit, mutant


def test_gate_rejects_multiply_by_mask_on_nan_padding():
    meta, z = load_golden("variance_targets_tiny")
    batch = batch_of(z, meta["L"])
    good = vc.pipeline(batch, "phoneme_level", "frame_level")
    bad_in = vc.poison(batch, good["frame_lens"])
    again = vc.pipeline(bad_in, "phoneme_level", "frame_level")
    for f in ("pitch", "energy"):
        assert np.array_equal(again[f]["raw64"], good[f]["raw64"])  # the selection does not see the poison
    with np.errstate(invalid="ignore"):
        bad = vc.targets(bad_in["pitch"], bad_in["energy"], bad_in["durations"], bad_in["src_lens"], "phoneme_level", "frame_level", mutate="multiply_by_mask")
    assert np.isnan(bad["energy"]).any() or not vc.raw_gate_ok(bad["energy"], good["energy"]["raw64"]).all()


# ---- the C ABI's host side ----------------------------------------------------------------------------------------------------------
def test_abi_versions_header_against_lib():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    for macro, fn, want in (("NS_VT_ABI_VERSION", lib.ns_vt_abi_version, 1), ("NS_LOSS_ABI_VERSION", lib.ns_loss_abi_version, 1), ("NS_ABI_VERSION", lib.ns_abi_version, 6),
                            ("NS_VOC_ABI_VERSION", lib.ns_voc_abi_version, 1), ("NS_ALN_ABI_VERSION", lib.ns_aln_abi_version, 1),
                            ("NS_MEL_ABI_VERSION", lib.ns_mel_abi_version, 1), ("NS_GL_ABI_VERSION", lib.ns_gl_abi_version, 1)):
        have = int(re.search(rf"#define {macro} (\d+)", text).group(1))
        assert have == fn() == want, macro
    from smart_nar_fast_tts_amd import targets

    assert int(re.search(r"#define NS_VT_SORT_CAPACITY (\d+)", text).group(1)) == vc.SORT_CAPACITY == targets.SORT_CAPACITY >= 8192


def test_structs_match_header():
    text = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ns_vt_args \{(.*?)\} ns_vt_args;", text, flags=re.S).group(1), flags=re.S)
    fields = [f.strip().lstrip("*") for decl in re.findall(r"(?:const )?\w+\*? ([^;]+);", body) for f in decl.split(",")]
    assert fields == [f for f, _ in _lib.NsVtArgs._fields_]
    assert C.sizeof(_lib.NsVtArgs) == 4 * 8 + 8 + 8 * 8 and C.sizeof(_lib.NsVtState) == 80


def test_ws_bytes_positive_and_monotone():
    lib = _lib.load()
    assert lib.ns_vt_ws_bytes(0, 0, 0) > 0 and lib.ns_vt_ws_bytes(1, 0, 0) > 0 and lib.ns_vt_ws_bytes(-1, -1, -1) > 0
    for axis in range(3):
        prev = 0
        for v in (0, 1, 15, 16, 17, 255, 256, 257, 1030, 4000, 8192):
            dims = [4, 96, 300]
            dims[axis] = v
            n = lib.ns_vt_ws_bytes(*dims)
            assert n >= prev > -1, (axis, v)
            prev = n


def _args(**over):
    """A well-formed argument block over made-up (never dereferenced) device addresses: validation runs before any HIP call."""
    a = _lib.NsVtArgs()
    a.B, a.L, a.T, a.pitch_frame_level, a.energy_frame_level, a.pitch_normalization, a.energy_normalization = 2, 12, 40, 0, 1, 1, 1
    a.durations_stride = 12
    for i, (f, _) in enumerate(_lib.NsVtArgs._fields_[8:]):
        setattr(a, f, 0x10000 * (i + 1))
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_every_refusal_is_reached_without_a_gpu():
    lib = _lib.load()
    ws, state = C.c_void_p(0x2000000), C.c_void_p(0x3000000)
    need = lib.ns_vt_ws_bytes(2, 12, 40)
    calls = {"ns_vt_targets": lambda a, w, n, s: lib.ns_vt_targets(a, w, n, None), "ns_vt_fit": lambda a, w, n, s: lib.ns_vt_fit(a, s, w, n, None),
             "ns_vt_normalize": lambda a, w, n, s: lib.ns_vt_normalize(a, s, w, n, None)}

    def refused(which, a, match, ws=ws, n=need, state=state):
        state = C.cast(state, C.POINTER(_lib.NsVtState)) if state is not None else None  # the header types it: ns_vt_state*
        for name in which:
            rc = calls[name](C.byref(a) if a is not None else None, ws, n, state)
            msg = lib.ns_last_error().decode()
            assert rc != 0 and msg.startswith(name) and re.search(match, msg), (name, match, rc, msg)

    every = tuple(calls)
    refused(every, None, "null argument")
    refused(every, _args(), "null argument", ws=None)
    for f in ("B", "L", "T"):
        refused(every, _args(**{f: -1}), "negative size")
    refused(every, _args(B=1 << 20, T=1 << 12), "problem too large", n=1 << 44)
    for f in ("src_lens", "frame_lens", "pitch_targets", "energy_targets"):
        refused(every, _args(**{f: None}), "null " + f)
    refused(every, _args(), r"workspace too small \(ns_vt_ws_bytes\)", n=need - 1)
    refused(every, _args(), "workspace must be 16-byte aligned", ws=C.c_void_p(0x2000008))
    refused(("ns_vt_fit", "ns_vt_normalize"), _args(), "null state", state=None)
    refused(("ns_vt_fit", "ns_vt_normalize"), _args(), "state must be 8-byte aligned", state=C.c_void_p(0x3000004))
    refused(("ns_vt_targets", "ns_vt_fit"), _args(valid=None), "null valid")
    for f in ("pitch", "energy"):
        refused(("ns_vt_targets",), _args(**{f: None}), "null pitch or energy")
    refused(("ns_vt_targets",), _args(durations=None), "null durations")
    refused(("ns_vt_targets",), _args(durations_stride=11), "durations_stride must be at least L")
    # n above the LDS sort capacity: T at frame_level, L at phoneme_level
    big = lib.ns_vt_ws_bytes(2, 8193, 8193)
    refused(("ns_vt_fit",), _args(T=8193), "exceed the LDS sort capacity NS_VT_SORT_CAPACITY = 8192", n=big)
    refused(("ns_vt_fit",), _args(L=8193, durations_stride=8193), "exceed the LDS sort capacity", n=big)
    assert lib.ns_vt_state_init(None, None) != 0 and "null state" in lib.ns_last_error().decode()


def test_header_is_plain_c_and_validation_works_from_c(tmp_path):
    run_c_caller("vt_host_only", _lib.LIB_PATH, tmp_path)


def test_python_surface_without_a_gpu(tmp_path):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align
    from smart_nar_fast_tts_amd.targets import VarianceTargets

    assert pkg.VarianceTargets is VarianceTargets
    pc = wl.preprocess_config("phoneme_level", "frame_level")
    vt = VarianceTargets(pc)
    p, e = torch.zeros(2, 7), torch.zeros(2, 7)
    d, sl = torch.ones(2, 3, dtype=torch.long), torch.tensor([3, 2])
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        vt.process(p, e, d, sl)
    with pytest.raises(ValueError, match="pitch must be torch.float32"):
        vt.process(p.double(), e, d, sl)
    with pytest.raises(ValueError, match="energy must have shape"):
        vt.process(p, e[:, :5], d, sl)
    with pytest.raises(ValueError, match="durations must be torch.int64"):
        vt.process(p, e, d.int(), sl)
    with pytest.raises(ValueError, match="src_lens must have shape"):
        vt.process(p, e, d, sl[:1])
    with pytest.raises(ValueError, match="exceed the sort capacity"):
        vt.process(torch.zeros(1, 8193), torch.zeros(1, 8193), d[:1], sl[:1])
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        vt.normalize(torch.zeros(2, 3), torch.zeros(2, 7), sl, sl)
    with pytest.raises(RuntimeError, match="nothing has been processed"):
        vt.stats()
    bad = wl.preprocess_config("frame_level", "frame_level")
    bad["preprocessing"]["pitch"]["feature"] = "word_level"
    with pytest.raises(ValueError, match="preprocessing.pitch.feature"):
        VarianceTargets(bad)
    # stats.json round trip: a state as the device would leave it -> write_stats -> FastSpeech2Align.__init__ -> the same bin edges
    vt._state = torch.tensor([50.0, 80.0, 180.0, 30.0, 50.0 * 40.0 ** 2, 80.0 * 9.0 ** 2, -2.5, -3.0, 4.0, 9.5], dtype=torch.float64)
    pc["path"]["preprocessed_path"] = str(tmp_path)
    s = vt.write_stats(str(tmp_path))
    assert s == {"pitch": [-2.5, 4.0, 180.0, 40.0], "energy": [-3.0, 9.5, 30.0, 9.0]}
    assert json.load(open(tmp_path / "stats.json")) == s
    mc = wl.model_config("tiny")
    mc["variance_embedding"]["pitch_quantization"] = "linear"  # normalised pitch is negative: "log" bins need a positive range
    m = FastSpeech2Align(pc, mc)
    assert m._stats == s
    pb, eb = wl.variance_bins(mc, s)
    init = m._default_init()
    assert np.array_equal(init["variance_adaptor.pitch_bins"], pb) and np.array_equal(init["variance_adaptor.energy_bins"], eb)
    assert vt.reset() is vt and vt._state is None


def test_vartargets_kernels_do_not_spill():
    assert_no_spill("vartargets.hip", kernels=("k_vt_targets", "k_vt_fit_partial", "k_vt_fit_merge", "k_vt_normalize", "k_vt_minmax_merge", "k_vt_state_init"))
