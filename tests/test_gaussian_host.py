"""The Gaussian length regulator's yardstick, proved both ways without a GPU (tests/gaussian_cpu.py): the numpy-fp32 emulation of
k_gauss_upsample's arithmetic stays inside the elementwise bounds on every case the GPU test runs — with expf pushed by -1, 0 and +1
ulp and with the denominator summed left to right — and every mutant of the emulation leaves a bound on at least one case.  Also the
host side of the two test hooks (ns_op_gaussian_regulate, ns_aln_op_input): every refusal comes before any device work."""
import ctypes

import numpy as np
import pytest

from tests import gaussian_cpu as gc

_REF = {}


def case(name):
    """(x, d, own_len, Reference) of a case, built once"""
    if name not in _REF:
        x, d, own_len = gc.CASES[name]()
        _REF[name] = (x, d, own_len, gc.reference(x, d, own_len))
    return _REF[name]


def test_cases_cover_the_edges_they_are_named_for():
    T = {n: case(n)[3].T for n in gc.CASES}
    assert T["zero_utterance T=128 2x12x24"] % gc.FRAME_TILE == 0 and T["T=32k+1 3x10x40"] % gc.FRAME_TILE == 1
    L = {n: case(n)[1].shape[1] for n in gc.CASES}
    assert L["lds_chunk_edge 1x256x256"] == gc.LDS_CHUNK and L["padded_odd_tail 1x257x64"] == gc.LDS_CHUNK + 1
    assert L["three_chunks 2x513x32"] == 2 * gc.LDS_CHUNK + 1
    assert gc.CHANNEL_PASS < case("17_channel_tiles 1x9x520")[0].shape[2] < gc.CHANNEL_PASS + 32
    x, d, _, ref = case("long_durations 1x11x32")
    assert tuple(d[0]) == gc.LONG_ROW and ref.T == 771
    c, _ = gc.centres(d)
    a = 0.01 * (np.arange(ref.T)[None, :] - c[0].astype(np.float64)[:, None]) ** 2
    assert a[ref.w[0] > 1e-3].max() > 50, "weights above 1e-3 at exponent arguments past 50"
    x, d, _, ref = case("zero_utterance T=128 2x12x24")
    assert (d[1] == 0).all() and abs(ref.w[1, :, 0] - 1 / 12).max() < 1e-15 and ref.w[1, :, 127].max() < 1e-45
    assert 0 < ref.w[1, 0, 75] < 1e-4 < ref.w[1, 0, 65], "1e-20 takes over inside the row range"
    x, d, own, ref = case("forwards_dense 5x9x24")
    assert own == [ref.T, 0, ref.T - 33, -1, ref.T + 5]
    x, d, own, ref = case("forwards_packed 5x9x24")
    assert 0 in own and 1 in own and ref.T in own and any(ref.T - gc.PACK_GUARD <= n < ref.T for n in own)
    assert any(0 < n < ref.T - gc.PACK_GUARD for n in own), "one window that ends before the grid does"


@pytest.mark.parametrize("name", list(gc.CASES))
def test_emulation_is_inside_both_bounds(name):
    x, d, own_len, ref = case(name)
    for label, kw in (("expf -1 ulp", dict(exp_ulp=-1)), ("expf exact", {}), ("expf +1 ulp", dict(exp_ulp=1)), ("serial denominator", dict(denominator="serial"))):
        out, w, s = gc.emulate(x, d, own_len, **kw)
        sw, so = gc.shares(out, w, ref)
        print(f"{name:32s} {label:18s} {sw:.3f} of the weight bound, {so:.3f} of the output bound")
        assert sw <= 1.0 and so <= 1.0, (name, label, sw, so)
        assert np.array_equal(s.astype(np.float64), ref.s)


@pytest.mark.parametrize("mutant", gc.MUTANTS)
def test_bounds_reject_mutant(mutant):
    """each mutant leaves a bound on at least one case; a mutant no case catches means a case is missing"""
    for name in gc.CASES:
        x, d, own_len, ref = case(name)
        out, w, _ = gc.emulate(x, d, own_len, mutate=mutant)
        sw, so = gc.shares(out, w, ref)
        if sw > 1.0 or so > 1.0:
            print(f"{mutant}: caught by {name} at {sw:.3g} of the weight bound, {so:.3g} of the output bound")
            return
    pytest.fail(f"no case catches {mutant}")


def test_reference_restates_the_oracle():
    """the float64 reference against the project's fp32 restatement of GaussianUpsampling.forward (oracle/fs2_oracle.py), loosely: the
    formula, not the rounding"""
    import torch

    from oracle import fs2_oracle as orc

    x, d, _, ref = case("odd_L_partial_tile 2x7x24")
    out, s, w = orc.gaussian_upsampling(torch.from_numpy(x), torch.from_numpy(d), None)
    assert out.shape == ref.out.shape and w.shape == ref.w.shape
    assert np.abs(out.numpy() - ref.out).max() < 1e-5 and np.abs(w.numpy() - ref.w).max() < 1e-6
    assert np.array_equal(s.numpy().reshape(-1).astype(np.float64), ref.s)


def test_hooks_refuse_bad_arguments_before_any_device_work():
    from smart_nar_fast_tts_amd import _lib

    lib = _lib.load()
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: every call below is refused first)
    g = lib.ns_op_gaussian_regulate
    #          x    d    own  B  L  D   T   out  s    w    st   zero nz plan Mp att stream
    assert g(nul, one, one, 2, 9, 24, 40, one, one, nul, nul, nul, 0, nul, 0, 0, nul) != 0
    assert g(one, nul, one, 2, 9, 24, 40, one, one, nul, nul, nul, 0, nul, 0, 0, nul) != 0
    assert g(one, one, nul, 2, 9, 24, 40, one, one, nul, nul, nul, 0, nul, 0, 0, nul) != 0
    assert g(one, one, one, 2, 9, 24, 40, nul, one, nul, nul, nul, 0, nul, 0, 0, nul) != 0
    assert g(one, one, one, 2, 9, 24, 40, one, nul, nul, nul, nul, 0, nul, 0, 0, nul) != 0
    for shape in ((0, 9, 24, 40), (2, 0, 24, 40), (2, 9, 0, 40), (2, 9, 24, 0), (2, 9, 24, -3)):
        assert g(one, one, one, *shape, one, one, nul, nul, nul, 0, nul, 0, 0, nul) != 0
    assert g(one, one, one, 2, 9, 24, 40, one, one, nul, nul, one, 0, nul, 0, 0, nul) != 0     # zero without nzero
    assert g(one, one, one, 2, 9, 24, 40, one, one, nul, nul, nul, 4, nul, 0, 0, nul) != 0     # nzero without zero
    assert g(one, one, one, 2, 9, 24, 40, one, one, nul, nul, one, -1, nul, 0, 0, nul) != 0
    assert g(one, one, one, 2, 9, 24, 40, one, one, nul, nul, nul, 0, nul, 52, 4, nul) != 0    # Mp / att_wgs without a plan
    assert g(one, one, one, 2, 9, 24, 40, one, one, nul, nul, nul, 0, one, 81, 4, nul) != 0    # Mp > B * T
    assert g(one, one, one, 2, 9, 24, 40, one, one, nul, nul, nul, 0, one, 52, 0, nul) != 0
    assert g(one, one, one, 2, 9, 24, 40, one, one, nul, nul, nul, 0, one, 0, 4, nul) != 0
    assert g(one, one, one, 2, 9, 24, 40, one, one, one, nul, nul, 0, one, 52, 4, nul) != 0    # a weight tensor together with a plan
    assert b"weight tensor" in lib.ns_last_error()
    a = lib.ns_aln_op_input
    assert a(nul, one, 2, 5, 80, nul) != 0 and a(one, nul, 2, 5, 80, nul) != 0
    for shape in ((0, 5, 80), (2, 0, 80), (2, 5, 0), (2, 5, 6), (2, 5, 81)):
        assert a(one, one, *shape, nul) != 0
    assert a(ctypes.c_void_p(260), one, 2, 5, 80, nul) != 0 and a(one, ctypes.c_void_p(264), 2, 5, 80, nul) != 0   # not 16-byte aligned
