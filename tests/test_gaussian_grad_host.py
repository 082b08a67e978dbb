"""The yardstick of the Gaussian length regulator's backward, proved both ways without a GPU (tests/gaussian_grad_cpu.py): the numpy-fp32
emulation of k_gu_bwd's arithmetic stays inside the bound on the fixture and on every case the GPU test runs, the 102-frame band changes
no bit, every mutant leaves the bound on a named case, the float64 reference restates the reference module's own autograd
(tests/golden/gaussian_grad_tiny.npz).  Also the host side of ns_va_gu_* / ns_va_op_gu_*: every refusal comes before any device work,
through the library and through a C99 caller; the ``length_regulator`` key of adaptor.VarianceAdaptor; no spill."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import gaussian_cpu as gc
from tests import gaussian_grad_cpu as gg
from tests.util import assert_no_spill, built_lib, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def case(name):
    """(x, d, own_len, g, Reference) of a case, built once"""
    if name not in _REF:
        x, d, own_len, g = gg.CASES[name]()
        _REF[name] = (x, d, own_len, g, gg.reference(x, d, g, own_len))
    return _REF[name]


def tiles(name):
    """per (utterance, 32-phoneme tile): (t_lo, t_hi, lim)"""
    x, d, own_len, g, ref = case(name)
    c, _ = gc.centres(d)
    return [(b, l0) + gg.band(c[b, l0:l0 + gg.PHONEME_TILE], ref.lim[b]) + (ref.lim[b],) for b in range(d.shape[0])
            for l0 in range(0, d.shape[1], gg.PHONEME_TILE)]


def test_cases_reach_the_paths_they_are_named_for():
    assert set(gc.CASES) < set(gg.CASES) and len(gc.CASES) == 11
    L = {n: case(n)[1].shape[1] for n in gg.CASES}
    D = {n: case(n)[0].shape[2] for n in gg.CASES}
    assert {1, 31, 33} <= set(L.values()), "one phoneme, a tile less one, a tile plus one"
    assert L["tile_plus_one 2x33x36"] == gg.PHONEME_TILE + 1 and L["three_chunks 2x513x32"] > 16 * gg.PHONEME_TILE
    assert D["four_channels 2x9x4"] == 4 and D["17_channel_tiles 1x9x520"] > 4 * gg.CHANNEL_PASS
    assert gg.CHANNEL_PASS < D["two_channel_passes 1x9x132"] < gg.CHANNEL_PASS + 32, "a second channel pass with one partial tile"
    assert any(d % 32 for d in D.values()) and any(d < 32 for d in D.values())
    # a band of several LDS chunks whose last is partial, and one of a single partial chunk
    spans = {n: [hi - lo for _, _, lo, hi, _ in tiles(n)] for n in gg.CASES}
    assert max(spans["long_durations 1x11x32"]) > 3 * gg.FRAME_CHUNK and max(spans["long_durations 1x11x32"]) % gg.FRAME_CHUNK
    assert max(spans["odd_L_partial_tile 2x7x24"]) < gg.FRAME_CHUNK and any(s % 2 for s in spans["odd_L_partial_tile 2x7x24"]), "an odd frame count: the padded pair"
    assert any(s == gg.FRAME_CHUNK for v in spans.values() for s in v) or any(s > gg.FRAME_CHUNK for v in spans.values() for s in v)
    # the band really cuts: tiles that start above frame 0 and tiles that end below lim
    t3 = tiles("three_chunks 2x513x32")
    assert any(lo > 0 for _, _, lo, hi, lim in t3) and any(hi < lim for _, _, lo, hi, lim in t3)
    # the long pause: the bands of utterance 0's two tiles are disjoint and leave live frames that no tile owns
    x, d, own_len, g, ref = case("long_pause 2x40x8")
    assert d[0, 31] + d[0, 32] > 2 * (2 * gg.REACH) - 1 and d[0, 31] > 204
    (b0, _, lo0, hi0, lim0), (_, _, lo1, hi1, _) = tiles("long_pause 2x40x8")[:2]
    assert b0 == 0 and lo0 == 0 and hi0 < lo1 and hi1 == lim0 == ref.T - 5
    between = ref.fwd.w[0, :, hi0:lo1]
    assert lo1 - hi0 > 40 and between.max() < 1e-24 and (between <= ref.fwd.bound_w[0, :, hi0:lo1]).all(), "between the bands a weight is below one fp32 denormal of e"
    # own_len of 0, negative and above T
    x, d, own_len, g, ref = case("forwards_dense 5x9x24")
    assert ref.lim == [ref.T, 0, ref.T - 33, 0, ref.T] and own_len[3] < 0 and own_len[4] > ref.T
    assert not ref.bound[1].any() and not ref.dx[1].any() and ref.bound[0].all()
    assert 0 in case("forwards_packed 5x9x24")[4].lim and 1 in case("forwards_packed 5x9x24")[4].lim
    x, d, own_len, g, ref = case("zero_utterance T=128 2x12x24")
    assert (d[1] == 0).all() and ref.bound[1].all(), "an utterance of zero durations still takes the gradient of frames 0 .. T - 1 in the plain form"


@pytest.mark.parametrize("name", list(gg.CASES))
def test_emulation_is_inside_the_bound_and_the_band_changes_no_bit(name):
    x, d, own_len, g, ref = case(name)
    worst = 0.0
    for label, ulp in (("expf -1 ulp", -1), ("expf exact", 0), ("expf +1 ulp", 1)):
        dx, used = gg.emulate(d, g, own_len, exp_ulp=ulp)
        s = gg.share(dx, ref)
        print(f"{name:32s} {label:12s} {s:.4f} of the bound")
        assert s <= 1.0, (name, label, s)
        if ulp == 0:
            worst = s
            full, used_full = gg.emulate(d, g, own_len, banded=False)
            assert full.tobytes() == dx.tobytes() and used_full.tobytes() == used.tobytes(), "a frame the band skips has the weight +0.0"
            w = gc.emulate(np.zeros(d.shape + (1,), np.float32), d)[1]
            for b, lim in enumerate(ref.lim):
                assert used[b, :, :lim].tobytes() == w[b, :, :lim].tobytes() and not used[b, :, lim:].any()
    assert worst <= 1.0   # (measured: at most 0.09 of the bound, at L = 256; 0.01 ... 0.05 elsewhere)


@pytest.mark.parametrize("mutant,name", [
    ("row_limit_off_by_one", "forwards_packed 5x9x24"), ("own_len_ignored", "forwards_dense 5x9x24"),
    ("last_frame_chunk_dropped", "long_durations 1x11x32"), ("band_of_30_frames", "long_pause 2x40x8"),
    ("no_1e-20", "zero_utterance T=128 2x12x24"), ("weights_untransposed", "odd_L_partial_tile 2x7x24"),
    ("last_channel_tile_zero", "two_channel_passes 1x9x132"), ("centre_without_half", "odd_L_partial_tile 2x7x24")])
def test_bound_rejects_mutant(mutant, name):
    x, d, own_len, g, ref = case(name)
    s = gg.share(gg.emulate(d, g, own_len, mutate=mutant)[0], ref)
    print(f"{mutant}: {s:.3g} of the bound on {name}")
    assert s > 1.0
    assert set(gg.MUTANTS) == {"row_limit_off_by_one", "own_len_ignored", "last_frame_chunk_dropped", "band_of_30_frames", "no_1e-20",
                               "weights_untransposed", "last_channel_tile_zero", "centre_without_half"}


def test_reference_restates_the_reference_modules_autograd():
    meta, z = load_golden("gaussian_grad_tiny")
    x, d, own_len, g, ref = case(meta["plain_case"])
    assert np.array_equal(z["plain_x"], x) and np.array_equal(z["plain_d"], d) and np.array_equal(z["plain_g"], g) and own_len is None
    assert np.abs(z["plain_w_f64"] - ref.fwd.w).max() <= 1e-14 and np.abs(z["plain_out_f64"] - ref.fwd.out).max() <= 1e-13
    assert np.abs(z["plain_dx_f64"] - ref.dx).max() <= 1e-13 * np.abs(ref.dx).max()
    # torch's own fp32 run of the module and the emulation: both inside the bound
    s32, semu = gg.share(z["plain_dx"], ref), gg.share(gg.emulate(d, g)[0], ref)
    print(f"torch fp32 autograd {s32:.3f}, emulation {semu:.3f} of the bound")
    assert s32 <= 1.0 and semu <= 1.0
    assert (meta["B"], meta["L"], meta["T"], meta["src_lens"], meta["mixes"]) == (2, 7, 20, [7, 4], ["pf", "fp"])
    assert z["duration"].sum(1).tolist() == [17, 11] and (z["duration"][1, 4:] == 0).all() and (z["duration"][0] == 0).any()
    assert all(np.array_equal(z[f"{m}_mel_len"], [17, 11]) for m in meta["mixes"])
    assert not any(k.startswith("w_") or "weight" in k for k in z.files)
    size = lambda n: os.path.getsize(os.path.join(ROOT, "tests", "golden", n))  # noqa: E731
    assert size("gaussian_grad_tiny.npz") < 0.7 * size("variance_adaptor_grad_tiny.npz")


# ---------------------------------------------------------------------------------------------------- the C side (no device work)
def test_workspace_query(lib):
    L_, so = lib
    assert so.ns_va_abi_version() == 1
    for B, L, T in ((1, 1, 1), (2, 7, 24), (16, 128, 1000), (8, 128, 4000), (3, 513, 5)):
        n = so.ns_va_gu_ws_bytes(B, L, T)
        fwd = (B * L * 4 + 15) // 16 * 16 + (B + B * L) * 4
        assert n % 256 == 0 and n >= max(fwd, B * T * 4) and n - 256 < max(fwd, B * T * 4), (B, L, T, n)


def test_every_refusal_precedes_the_first_hip_call(lib):
    L_, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    a, big = 0x100000, 1 << 40
    for args, msg in (((0, 7, 24), "B and L must be positive"), ((2, 0, 24), "B and L must be positive"), ((2, 7, 0), "T must be positive"),
                      ((2, 7, 1 << 20), "T must stay below 2^20"), ((65536, 7, 24), "B must stay below 65536"), ((1 << 12, 1 << 18, 24), "B * L * D must stay below 2^31"),
                      ((1 << 12, 7, 1 << 18), "B * T * D must stay below 2^31")):
        assert so.ns_va_gu_ws_bytes(*args) == 0 and msg in err(), (args, err())
    need = so.ns_va_gu_ws_bytes(2, 7, 24)
    fwd = lambda x=a, d=a, B=2, L=7, D=24, T=24, out=a, saved=a, mel_len=a, ws=a, n=big: so.ns_va_op_gu_fwd(  # noqa: E731
        P(x), P(d), B, L, D, T, P(out), P(saved), P(mel_len), P(ws), n, None)
    bwd = lambda g=a, saved=a, own=a, B=2, L=7, D=24, T=24, dx=a, w=0, ws=a, n=big, f=so.ns_va_op_gu_bwd: f(  # noqa: E731
        P(g), P(saved), P(own), B, L, D, T, P(dx), P(w), P(ws), n, None)
    calls = (
        (lambda: fwd(d=0), "null argument"), (lambda: fwd(saved=0), "null argument"), (lambda: fwd(mel_len=0), "null argument"),
        (lambda: fwd(ws=0), "null argument"), (lambda: fwd(x=0), "null argument"),
        (lambda: fwd(B=0), "B and L must be positive"), (lambda: fwd(L=-1), "B and L must be positive"), (lambda: fwd(T=0), "T must be positive"),
        (lambda: fwd(T=1 << 20), "T must stay below 2^20"), (lambda: fwd(D=22), "D must be a positive multiple of 4"), (lambda: fwd(D=0), "D must be a positive multiple of 4"),
        (lambda: fwd(B=1 << 10, L=1 << 10, D=1 << 11), "B * L * D must stay below 2^31"), (lambda: fwd(B=1 << 10, T=1 << 10, D=1 << 11), "B * T * D must stay below 2^31"),
        (lambda: fwd(x=a + 4), "x must be 16-byte aligned"), (lambda: fwd(out=a + 8), "out must be 16-byte aligned"), (lambda: fwd(saved=a + 4), "saved must be 16-byte aligned"),
        (lambda: fwd(d=a + 4), "duration must be 8-byte aligned"), (lambda: fwd(mel_len=a + 4), "mel_len must be 8-byte aligned"),
        (lambda: fwd(ws=a + 8), "the workspace must be 16-byte aligned"), (lambda: fwd(n=need - 1), "workspace too small"),
        (lambda: fwd(x=0, out=0, T=0, D=0), "D must be a positive multiple of 4"),   # the prepare-only form still checks what it reads
        (lambda: fwd(x=0, out=0, T=0, n=so.ns_va_gu_ws_bytes(2, 7, 1) - 1), "workspace too small"),
        (lambda: bwd(g=0), "null argument"), (lambda: bwd(saved=0), "null argument"), (lambda: bwd(dx=0), "null argument"), (lambda: bwd(ws=0), "null argument"),
        (lambda: bwd(B=0), "B and L must be positive"), (lambda: bwd(T=0), "T must be positive"), (lambda: bwd(T=1 << 20), "T must stay below 2^20"),
        (lambda: bwd(D=6), "D must be a positive multiple of 4"), (lambda: bwd(B=1 << 10, T=1 << 10, D=1 << 11), "B * T * D must stay below 2^31"),
        (lambda: bwd(B=1 << 10, L=1 << 11, T=1 << 10, D=4, w=a), "B * L * T must stay below 2^31"),
        (lambda: bwd(g=a + 4), "g must be 16-byte aligned"), (lambda: bwd(saved=a + 8), "saved must be 16-byte aligned"), (lambda: bwd(dx=a + 4), "d_x must be 16-byte aligned"),
        (lambda: bwd(w=a + 4), "w_out must be 16-byte aligned"), (lambda: bwd(own=a + 4), "own_len must be 8-byte aligned"),
        (lambda: bwd(ws=a + 4), "the workspace must be 16-byte aligned"), (lambda: bwd(n=need - 1), "workspace too small"),
        (lambda: bwd(n=need - 1, f=so.ns_va_op_gu_bwd_unbanded), "workspace too small"), (lambda: bwd(g=0, f=so.ns_va_op_gu_bwd_unbanded), "null argument"),
    )
    for i, (call, msg) in enumerate(calls):
        assert call() != 0 and msg in err() and so.ns_va_last_launches() == 0, (i, err())


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("gu_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("gaussgrad.hip", kernels=("k_gu_prepare", "k_gu_denominators", "k_gu_bwd"))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_the_key_chooses_the_regulator_and_changes_no_state_dict_key(lib):
    import torch

    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import adaptor, training

    assert pkg.GaussianUpsampling is adaptor.GaussianUpsampling and "GaussianUpsampling" in pkg.__all__
    pc = wl.preprocess_config("phoneme_level", "frame_level")
    hard, absent = wl.model_config("tiny"), wl.model_config("tiny")
    hard["length_regulator"] = "hard"
    gauss = wl.model_config("tiny+gaussian")
    assert gauss["length_regulator"] == "gaussian" and "length_regulator" not in absent
    mh, ma, mg = (adaptor.VarianceAdaptor(pc, c) for c in (hard, absent, gauss))
    assert type(mh.length_regulator) is type(ma.length_regulator) is adaptor.LengthRegulator
    assert type(mg.length_regulator) is adaptor.GaussianUpsampling and not list(mg.length_regulator.parameters()) and not mg.length_regulator.state_dict()
    assert list(mg.state_dict()) == list(mh.state_dict()) == list(ma.state_dict())
    assert mg.length_regulator in mg.hip_modules()
    for bad in ("Gaussian", "soft", None, 1):
        cfg = wl.model_config("tiny")
        cfg["length_regulator"] = bad
        with pytest.raises(ValueError, match="length_regulator"):
            adaptor.VarianceAdaptor(pc, cfg)
    # the whole trainable model: the same keys with and without the key, and the inference model takes them strictly
    th, tg = training.FastSpeech2Align(wl.preprocess_config(), hard), training.FastSpeech2Align(wl.preprocess_config(), gauss)
    assert type(tg.variance_adaptor.length_regulator) is adaptor.GaussianUpsampling and list(tg.state_dict()) == list(th.state_dict())
    x = torch.zeros(2, 5, 256)
    with pytest.raises(RuntimeError, match="no CPU path"):
        adaptor.GaussianUpsampling()(x, torch.ones(2, 5, dtype=torch.long), 9)
