"""The yardstick of tests/test_gpu_predictor_grad.py proven on the CPU, the split plan of the weight gradient, and every refusal of
the ns_pg_* family (no GPU).

Found on the fixture (tests/golden/predictor_grad_tiny.npz, the reference's own VariancePredictor in train() at dropout 0): the float64
restatement agrees with the reference's float64 autograd to <= 1e-10 relative; in fp32 the restatement reproduces the reference BITWISE on
all 22 tensors where the fixture was written.  The assertion allows one fp32 ulp of the tensor's largest magnitude, because torch's CPU
matmul may split its sums differently with another thread count."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import lossgrad_cpu as lg
from tests import predictor_grad_cpu as pc
from tests.util import built_lib, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the (B, S, lens) cases of tests/test_gpu_predictor_grad.py (lens None: ragged, see its lens_of)
GPU_CASES = [(5, 1), (5, 3), (4, 33), (3, 343), (7, 911)]


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def _fixture(c):
    meta, z = load_golden("predictor_grad_tiny")
    w = {k: z[f"{c}_w_{k}"] for k in pc.NAMES[:10]}
    return meta, z, w, z[f"{c}_x"], z[f"{c}_g"], z[f"{c}_mask"]


# ---------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("c", ["a", "b"])
def test_restatement_reproduces_the_reference(c):
    meta, z, w, x, g, mask = _fixture(c)
    r64, f64 = pc.autograd_ref(x, w, mask, g, dtype=torch.float64)
    r32, f32 = pc.autograd_ref(x, w, mask, g, dtype=torch.float32)
    assert np.abs(f64["pred"].numpy() - z[f"{c}_pred_f64"]).max() <= 1e-10 * np.abs(z[f"{c}_pred_f64"]).max()
    for n in pc.NAMES:
        want64, want32 = z[f"{c}_d_{n}_f64"], z[f"{c}_d_{n}"]
        assert r64[n].shape == want64.shape
        assert np.abs(r64[n] - want64).max() <= 1e-10 * np.abs(want64).max(), n
        err = np.abs(r32[n].astype(np.float64) - want32.astype(np.float64)).max()
        print(f"{c} {n}: fp32 restatement vs reference {err:.3g} ({'bitwise' if err == 0 else 'ulp of max: %.3g' % lg.ulp32(np.abs(want32).max())})")
        assert err <= lg.ulp32(np.abs(want32).max()), n


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("c", ["a", "b"])
def test_closed_form_equals_float64_autograd(c, p):
    meta, z, w, x, g, mask = _fixture(c)
    F = w["b1"].shape[0]
    keeps = None
    if p > 0:
        rs = np.random.RandomState(7)
        keeps = (rs.rand(*x.shape[:2], F) >= p, rs.rand(*x.shape[:2], F) >= p)
    ref, fwd = pc.autograd_ref(x, w, mask, g, keeps, p, torch.float64)
    got = pc.closed_form(x, w, mask, g, (fwd["v1"], fwd["h1"], fwd["v2"]), keeps, p, torch.float64)
    for n in pc.NAMES:
        assert np.abs(got[n] - ref[n]).max() <= 1e-10 * max(np.abs(ref[n]).max(), 1e-300), n


@pytest.mark.parametrize("c", ["a", "b"])
def test_first_padded_row_gets_a_gradient(c):
    """the row at index lens[b] is padded, but the last valid row's conv1d_2 / conv1d_1 tap reads it: dh1 and dx are nonzero there, in
    the reference's autograd and in the closed form; the row behind it gets dh1 = 0"""
    meta, z, w, x, g, mask = _fixture(c)
    b, t = 2, meta["lens"][2]
    assert mask[b, t] and not mask[b, t - 1] and t + 1 < meta["S"]
    for dx in (z[f"{c}_d_dx"], z[f"{c}_d_dx_f64"]):
        assert np.abs(dx[b, t]).max() > 0
    _, fwd = pc.autograd_ref(x, w, mask, g, dtype=torch.float64)
    got = pc.closed_form(x, w, mask, g, (fwd["v1"], fwd["h1"], fwd["v2"]))
    assert np.abs(got["_dh1"][b, t]).max() > 0 and np.abs(got["dx"][b, t]).max() > 0
    assert np.abs(got["_dh1"][b, t + 1]).max() == 0


def _gated(x, w, mask, g, keeps, p, pad=None):
    """(saved activations of the fp32 forward, float64 closed form from them, the gates)"""
    fwd = pc.statement(x, w, mask, keeps, p, torch.float32)
    saved = tuple(fwd[k].detach() for k in ("v1", "h1", "v2"))
    g_fin = np.where(np.isfinite(g), g, 0.0).astype(np.float32) if mask is not None else g
    r64 = pc.closed_form(x, w, mask, g_fin, saved, keeps, p, torch.float64, pad=pad)
    r32 = pc.closed_form(x, w, mask, g_fin, saved, keeps, p, torch.float32, pad=pad)
    return saved, r64, r32, pc.gate(r32, r64)


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_gate_rejects_mutant(mutant):
    """each mutant, evaluated in float64 (its only error is the mutation), is outside the gate of at least one tensor; the fp32 closed
    form itself is inside every gate (share <= 0.5 by construction)"""
    B, S, Cin, F = 4, 9, 48, 32
    K, pad = (5, 1) if mutant == "dgrad_pad_not_flipped" else (3, None)
    w = pc.seeded_weights(Cin, F, K, seed=3)
    rs = np.random.RandomState(11)
    x = rs.standard_normal((B, S, Cin)).astype(np.float32)
    g = rs.standard_normal((B, S)).astype(np.float32)
    mask = pc.mask_of([9, 0, 5, 9], S)
    p = 0.5 if mutant == "keep_scale_dropped" else 0.0
    keeps = (rs.rand(B, S, F) >= p, rs.rand(B, S, F) >= p) if p > 0 else None
    if mutant == "mask_multiplied":
        g = g.copy()
        g[2, 7] = np.nan  # behind the mask
        assert mask[2, 7]
    saved, r64, r32, gates = _gated(x, w, mask, g, keeps, p, pad)
    good = pc.shares(r32, r64, gates)
    assert max(good.values()) <= 0.5 + 1e-12
    # the correct closed form is untouched by a NaN behind the mask
    clean = pc.closed_form(x, w, mask, g, saved, keeps, p, torch.float64, pad=pad)
    assert max(pc.shares(clean, r64, gates).values()) == 0.0
    bad = pc.shares(pc.closed_form(x, w, mask, g, saved, keeps, p, torch.float64, mutate=mutant, pad=pad), r64, gates)
    worst = max(bad, key=bad.get)
    print(f"{mutant}: worst share {bad[worst]:.3g} ({worst})")
    assert bad[worst] > 1.0
    expected = {"dgrad_without_tap_flip": "dx", "dgrad_pad_not_flipped": "dx", "wgrad_across_utterances": "w1", "d_ln_g_without_xhat": "g2",
                "db_over_valid_rows_only": "b1"}
    if mutant in expected:
        assert bad[expected[mutant]] > 1.0


def test_gate_of_an_all_zero_gradient_is_exact():
    z = {n: np.zeros(3) for n in pc.NAMES}
    gates = pc.gate(z, z)
    assert all(v < 1e-40 for v in gates.values())
    off = dict(z, w1=np.array([0.0, 1e-30, 0.0]))
    assert pc.shares(off, z, gates)["w1"] > 1.0 and pc.shares(z, z, gates)["w1"] == 0.0
    assert pc.shares(dict(z, b1=np.array([0.0, np.inf, 0.0])), z, gates)["b1"] == float("inf")


# ---------------------------------------------------------------------------------------------------- the split plan
def _plan(so, M, N, Cin, K):
    out = (C.c_int32 * 8)()
    assert so.ns_pg_plan_wgrad(M, N, Cin, K, out) == 0, so.ns_last_error()
    return list(out)


def _align(n):
    return (n + 255) & ~255


def expected_ws_bytes(so, B, S, Cin, F, K):
    """the carve of csrc/predgrad_api.hip restated: four packed weights, the larger partial area, the column partials, three [M, F]"""
    M = B * S
    n1, n2 = 4 * F * K * Cin, 4 * F * K * F
    part = 4 * max(_plan(so, M, F, Cin, K)[5], _plan(so, M, F, F, K)[5])
    cols = 8 * 2 * ((M + 63) // 64) * 5 * F
    return 2 * _align(n1) + 2 * _align(n2) + _align(part) + _align(cols) + 3 * _align(4 * M * F)


@pytest.mark.parametrize("Cin", [256, 512])
@pytest.mark.parametrize("K", [3, 5])
def test_plan_wgrad_covers_the_rows_once_and_sizes_the_workspace(lib, Cin, K):
    L, so = lib
    F = 256
    for B, S in GPU_CASES + [(16, 128), (16, 1000)]:
        M = B * S
        tn, tc, rows, ranges, tiles, floats, chunk, _ = _plan(so, M, F, Cin, K)
        assert (tn, tc) == (128, 128) and tiles == (F // 128) * -(-K * Cin // 128)
        assert rows % 16 == 0 and rows > 0 and chunk % 16 == 0
        cover = [(r * rows, min(M, (r + 1) * rows)) for r in range(ranges)]
        assert cover[0][0] == 0 and cover[-1][1] == M and all(a < b for a, b in cover)       # no empty range
        assert all(cover[i][1] == cover[i + 1][0] for i in range(ranges - 1))                   # exactly once
        assert floats == ranges * F * K * Cin
        assert _plan(so, M, F, Cin, K) == [tn, tc, rows, ranges, tiles, floats, chunk, 0]      # a pure function of its arguments
        s = L.NsPgShape(B, S, Cin, F, K)
        assert so.ns_pg_ws_bytes(C.byref(s)) == expected_ws_bytes(so, B, S, Cin, F, K)
        assert so.ns_pg_saved_bytes(C.byref(s)) == 3 * M * F * 4
        if M >= 1029:
            assert ranges >= 2 and M % rows != 0, (M, rows, ranges)
    assert _plan(so, 2048, F, Cin, K)[3] * _plan(so, 2048, F, Cin, K)[4] >= 200  # the grid fills the chip at M = 2048
    bad = (C.c_int32 * 8)()
    for args in ((0, 256, 256, 3), (64, 200, 256, 3), (64, 256, 6, 3), (64, 256, 256, 4)):
        assert so.ns_pg_plan_wgrad(*args, bad) != 0 and "refused" in so.ns_last_error().decode()
    assert so.ns_pg_plan_wgrad(64, 256, 256, 3, None) != 0 and "null argument" in so.ns_last_error().decode()


# ---------------------------------------------------------------------------------------------------- refusals (no device work)
def test_every_refusal_precedes_the_first_hip_call(lib):
    L, so = lib
    assert so.ns_pg_abi_version() == 1
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a)  # noqa: E731  (made-up device addresses: never dereferenced)
    ok_shape = dict(B=2, S=8, Cin=256, F=256, K=3)

    def weights(**over):
        w = L.NsPgWeights()
        for i, n in enumerate(L.PG_NAMES):
            setattr(w, n, over.get(n, 0x100000 + 0x10000 * i))
        return w

    def fwd(shape=None, w=None, x=0x900000, mask=None, k1=None, k2=None, p=0.0, pred=0xA00000, saved=0xB00000, ws=0xC00000, nbytes=1 << 40):
        s = L.NsPgShape(**dict(ok_shape, **(shape or {})))
        return so.ns_pg_forward(C.byref(s), C.byref(w or weights()), P(x), mask, P(k1) if k1 else None, P(k2) if k2 else None, p, P(pred),
                                P(saved), P(ws), nbytes, None)

    def bwd(shape=None, w=None, x=0x900000, k1=None, k2=None, p=0.0, saved=0xB00000, g=0xD00000, grads=None, ws=0xC00000, nbytes=1 << 40):
        s = L.NsPgShape(**dict(ok_shape, **(shape or {})))
        d = grads or L.NsPgGrads()
        return so.ns_pg_backward(C.byref(s), C.byref(w or weights()), P(x), None, P(k1) if k1 else None, P(k2) if k2 else None, p, P(saved) if saved else None,
                                 P(g) if g else None, C.byref(d), P(ws), nbytes, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(x=0), "null argument"), (dict(ws=0), "null argument"), (dict(x=0x900004), "16-byte aligned"),
                        (dict(shape=dict(K=4)), "K must be odd"), (dict(shape=dict(K=0)), "K must be odd"), (dict(shape=dict(F=128)), "F must be 256 or 512"),
                        (dict(shape=dict(Cin=260)), "Cin must be a multiple of 16"), (dict(shape=dict(B=0)), "must be positive"),
                        (dict(shape=dict(B=1 << 12, S=1 << 11)), "problem too large"), (dict(p=1.0), "p_drop must lie in [0, 1)"),
                        (dict(p=-0.1), "p_drop must lie in [0, 1)"), (dict(p=float("nan")), "p_drop must lie in [0, 1)"),
                        (dict(p=0.5), "needs both keep-masks"), (dict(p=0.5, k1=0xE00000), "needs both keep-masks"),
                        (dict(k1=0xE00000, k2=0xF00000), "although p_drop == 0"), (dict(p=0.5, k1=0xE00004, k2=0xF00000), "16-byte aligned"),
                        (dict(w=weights(w2=0)), "null weights->w2"), (dict(w=weights(ln1_g=0x100004)), "weights->ln1_g must be 16-byte aligned"),
                        (dict(nbytes=1024), "workspace too small")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
    assert fwd(pred=0) != 0 and "null argument" in err()
    assert bwd(saved=0) != 0 and "null argument" in err()
    assert bwd(g=0) != 0 and "null argument" in err()
    d = L.NsPgGrads()
    d.w1 = 0x1000004
    assert bwd(grads=d) != 0 and "every gradient must be 16-byte aligned" in err()
    assert bwd() == 0  # nothing wanted: nothing launched, no HIP call
    assert so.ns_pg_last_launches() == 0

    def wgrad(dz=0x100000, X=0x200000, B=2, S=8, N=256, Cin=256, K=3, dW=0x300000, db=0x400000, ws=0x500000, nbytes=1 << 40):
        return so.ns_pg_op_wgrad(P(dz), P(X), B, S, N, Cin, K, P(dW), P(db) if db else None, P(ws), nbytes, None)

    def dgrad(dz=0x100000, W=0x200000, B=2, S=8, N=256, Cin=256, K=3, dX=0x300000, ws=0x500000, nbytes=1 << 40):
        return so.ns_pg_op_dgrad(P(dz), P(W), B, S, N, Cin, K, P(dX), P(ws), nbytes, None)

    for call in (wgrad, dgrad):
        for kw, msg in ((dict(dz=0), "null argument"), (dict(ws=0), "null argument"), (dict(dz=0x100008), "16-byte aligned"), (dict(K=2), "K must be odd"),
                        (dict(N=384), "F must be 256 or 512"), (dict(Cin=6), "Cin must be a multiple of"), (dict(B=-1), "must be positive"),
                        (dict(B=1 << 12, S=1 << 11), "problem too large"), (dict(nbytes=64), "workspace too small")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
    assert dgrad(Cin=260) != 0 and "multiple of 16" in err()

    def row(tail=0, dy=0x100000, g=0x110000, v=0x200000, ln_g=0x210000, ln_b=0x220000, wlin=0x230000, keep=None, p=0.0, M=16, F=256, dz=0x300000,
            o=(0x310000, 0x320000, 0x330000, 0x340000, 0x350000), ws=0x500000, nbytes=1 << 40):
        a = [P(q) if q else None for q in (dy, g)] + [None] + [P(q) if q else None for q in (v, ln_g, ln_b, wlin)] + [P(keep) if keep else None, p, M, F,
                                                                                                                        P(dz) if dz else None]
        return so.ns_pg_op_row_backward(tail, *a, *[P(q) if q else None for q in o], P(ws), nbytes, None)

    for kw, msg in ((dict(v=0), "null argument"), (dict(dy=0), "null argument"), (dict(tail=1, g=0), "null argument"), (dict(tail=1, wlin=0), "null argument"),
                    (dict(F=128), "F must be 256 or 512"), (dict(M=0), "must be positive"), (dict(p=0.3), "needs both keep-masks"),
                    (dict(keep=0x600000), "although p_drop == 0"), (dict(v=0x200004), "16-byte aligned"), (dict(nbytes=8), "workspace too small")):
        assert row(**kw) != 0 and msg in err(), (kw, err())
    assert so.ns_pg_ws_bytes(None) == 0 and "null argument" in err()
    s = L.NsPgShape(2, 8, 256, 100, 3)
    assert so.ns_pg_ws_bytes(C.byref(s)) == 0 and "F must be 256 or 512" in err()
    assert so.ns_pg_saved_bytes(C.byref(s)) == 0 and "F must be 256 or 512" in err()


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("pg_host_only", lib[0].LIB_PATH, tmp_path)


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_module_has_the_reference_names_and_no_cpu_path(lib):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import predictor
    from tests.util import weights_for

    assert pkg.VariancePredictor is predictor.VariancePredictor
    cfg, sd = weights_for(dict(config="tiny", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25))
    m = predictor.VariancePredictor(wl.model_config("tiny"))
    assert [n for n, _ in m.named_parameters()] == list(predictor.PARAM_NAMES)
    for which in ("duration", "pitch", "energy"):
        prefix = f"variance_adaptor.{which}_predictor."
        sub = {k[len(prefix):]: torch.as_tensor(np.asarray(v)) for k, v in sd.items() if k.startswith(prefix)}
        assert set(sub) == set(predictor.PARAM_NAMES)
        m.load_state_dict(sub)  # strict: the checkpoint's subtree, unchanged
    assert m.training and m.dropout == wl.model_config("tiny")["variance_predictor"]["dropout"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 5, m.input_size), None)
    bad = wl.model_config("tiny")
    bad["variance_predictor"] = dict(bad["variance_predictor"], dropout=1.0)
    with pytest.raises(ValueError, match=r"dropout must lie in \[0, 1\)"):
        predictor.VariancePredictor(bad)
