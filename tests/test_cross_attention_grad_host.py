"""The yardstick of tests/test_gpu_cross_attention_grad.py proven on the CPU, and every refusal of the ns_xg_* family (no GPU).

On the fixture (tests/golden/cross_attention_grad_tiny.npz, the reference's own MultiHeadAttention in train() at dropout 0 called as
FFTBlock2.crs_attn calls it) the float64 restatement agrees with the reference's float64 autograd to <= 1e-10 relative; in fp32 the
assertion allows one fp32 ulp of the tensor's largest magnitude, because torch's CPU matmul may split its sums differently with another
thread count.  (d_bk is zero in exact arithmetic — the softmax does not see a key bias, with or without a gradient of the map — so its
fixture values are rounding noise; its 1e-10 and its ulp are taken relative to the other gradients' scale, as in
tests/test_attention_grad_host.py.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import cross_attention_grad_cpu as xc
from tests import lossgrad_cpu as lg
from tests.util import assert_no_spill, built_lib, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the case table of tests/test_gpu_cross_attention_grad.py
CONFIGS = [(256, 2), (256, 4), (512, 8)]
CASES = [(2, 1, 1, [1, 1]), (3, 33, 5, [5, 1, 4]), (2, 130, 37, [37, 32]), (2, 70, 131, [131, 97]), (3, 343, 40, [40, 9, 33])]
_cid = lambda c: f"{c[0]}x{c[1]}x{c[2]}"  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def _fixture(c):
    meta, z = load_golden("cross_attention_grad_tiny")
    w = {k: z[f"{c}_w_{k}"] for k in xc.NAMES[:10]}
    return meta, z, w, z[f"{c}_tgt"], z[f"{c}_src"], z[f"{c}_g"], meta["lens"], meta["configs"][c]


# ---------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("v", ["h0", "all"])
@pytest.mark.parametrize("c", ["a", "b"])
def test_restatement_reproduces_the_reference(c, v):
    meta, z, w, tgt, src, g, lens, H = _fixture(c)
    a = z[f"{c}_a_{v}"]
    if v == "h0":
        assert not a[:, 1:].any() and a[:, 0].all()
    else:
        assert a.all()
    assert g.all(axis=-1).all()
    r64, f64 = xc.autograd_ref(tgt, src, w, lens, H, g, a, dtype=torch.float64)
    r32, f32 = xc.autograd_ref(tgt, src, w, lens, H, g, a, dtype=torch.float32)
    for k in ("y", "attn"):
        want = z[f"{c}_{k}_f64"]
        assert f64[k].shape == want.shape
        assert np.abs(f64[k].numpy() - want).max() <= 1e-10 * np.abs(want).max()
        assert np.abs(f32[k].numpy().astype(np.float64) - z[f"{c}_{k}"]).max() <= lg.ulp32(np.abs(z[f"{c}_{k}"]).max())
    assert not z[f"{c}_attn"][np.broadcast_to(xc.key_mask(lens, meta["L"]).numpy()[:, None], z[f"{c}_attn"].shape)].any()
    scale = max(np.abs(z[f"{c}_{v}_d_{n}_f64"]).max() for n in xc.NAMES)
    for n in xc.NAMES:
        want64, want32 = z[f"{c}_{v}_d_{n}_f64"], z[f"{c}_{v}_d_{n}"]
        assert r64[n].shape == want64.shape
        assert np.abs(r64[n] - want64).max() <= 1e-10 * (scale if n == "bk" else np.abs(want64).max()), n
        err = np.abs(r32[n].astype(np.float64) - want32.astype(np.float64)).max()
        print(f"{c} {v} {n}: fp32 restatement vs reference {err:.3g}")
        assert err <= lg.ulp32(np.abs(z[f"{c}_{v}_d_bq"]).max() if n == "bk" else np.abs(want32).max()), n


@pytest.mark.parametrize("v", [None, "h0", "all"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("c", ["a", "b"])
def test_closed_form_equals_float64_autograd(c, p, v):
    meta, z, w, tgt, src, g, lens, H = _fixture(c)
    a = None if v is None else z[f"{c}_a_{v}"]
    keep = (np.random.RandomState(7).rand(*tgt.shape) >= p) if p > 0 else None
    ref, fwd = xc.autograd_ref(tgt, src, w, lens, H, g, a, keep, p, torch.float64)
    got = xc.closed_form(tgt, src, w, lens, H, g, a, tuple(fwd[k] for k in ("q", "kv", "ctx", "z", "attn")), keep, p, torch.float64)
    scale = max(np.abs(ref[n]).max() for n in xc.NAMES)
    for n in xc.NAMES:
        assert np.abs(got[n] - ref[n]).max() <= 1e-10 * (scale if n == "bk" else np.abs(ref[n]).max()), n
    # masked keys: dK and dV rows past lens[b] are exactly zero; sum_l dS = 0 makes d_bk rounding noise
    pad = np.arange(meta["L"])[None, :] >= np.asarray(lens)[:, None]
    assert not got["_dkv"][pad].any() and np.abs(got["_dq"]).max() > 0
    assert np.abs(got["bk"]).max() <= 1e-12 * scale


_BASE = {}


def _base(cfg, case, p=0.0):
    """(inputs, saved tensors of the fp32 forward, float64 and fp32 closed forms with a dense a, the gates), once per (config, case, p)"""
    key = (cfg, _cid(case), p)
    if key not in _BASE:
        d, H = cfg
        B, T, L, lens = case
        w = xc.seeded_weights(d, seed=100 + d + H)
        rs = np.random.RandomState(B * T + L + d)
        tgt = rs.standard_normal((B, T, d)).astype(np.float32)
        src = rs.standard_normal((B, L, d)).astype(np.float32)
        g = rs.standard_normal((B, T, d)).astype(np.float32)
        a = rs.standard_normal((B, H, T, L)).astype(np.float32)
        keep = (rs.rand(B, T, d) >= p) if p > 0 else None
        fwd = xc.statement(tgt, src, w, lens, H, keep, p, torch.float32)
        saved = tuple(fwd[k].detach() for k in ("q", "kv", "ctx", "z", "attn"))
        r64 = xc.closed_form(tgt, src, w, lens, H, g, a, saved, keep, p, torch.float64)
        r32 = xc.closed_form(tgt, src, w, lens, H, g, a, saved, keep, p, torch.float32)
        _BASE[key] = (w, tgt, src, g, a, keep, saved, r64, r32, xc.gate(r32, r64))
    return _BASE[key]


# With one key (L = 1) A = 1 and dS = A (dP - D) = 0 identically, so a mistake inside dS cannot show; what has no masked key cannot
# show a read at one.  Everything else must show at every case of the table.
_NEEDS_dS = {"AdA_missing_from_D", "dA_missing_from_dP", "c_applied_once", "dK_without_transpose", "heads_swapped_in_dA", "dbq_over_valid_rows_only"}
_EXPECTED = {"AdA_missing_from_D": "wq", "dA_missing_from_dP": "wq", "dA_read_at_masked_keys": "wq", "c_applied_once": "wk",
             "dK_without_transpose": "wk", "heads_swapped_in_dA": "wq", "V_branch_missing_from_dsrc": "dsrc", "residual_missing_from_dtgt": "dtgt",
             "dbq_over_valid_rows_only": "bq", "keep_scale_dropped": "wfc"}


@pytest.mark.parametrize("mutant", xc.MUTANTS)
def test_gate_rejects_mutant_on_the_gpu_case_table(mutant):
    """each mutant, evaluated in float64 (its only error is the mutation), is outside the gate of the tensor it damages at every case of
    the GPU test's table where it can show at all; the fp32 closed form itself is inside every gate (share <= 0.5 by construction), so
    the reference alone passes at those shapes"""
    cfg = CONFIGS[0]
    d, H = cfg
    p = 0.5 if mutant == "keep_scale_dropped" else 0.0
    shown = 0
    for case in CASES:
        B, T, L, lens = case
        w, tgt, src, g, a, keep, saved, r64, r32, gates = _base(cfg, case, p)
        good = xc.shares(r32, r64, gates)
        assert max(good.values()) <= 0.5 + 1e-12, (case, good)
        masked = np.broadcast_to(xc.key_mask(lens, L).numpy()[:, None], a.shape)
        if mutant in _NEEDS_dS and L == 1:
            continue
        if mutant == "dA_read_at_masked_keys":
            if not masked.any():
                continue
            a = a.copy()
            a[masked] = np.nan  # the closed form selects it away; the mutant reads it
            clean = xc.closed_form(tgt, src, w, lens, H, g, a, saved, keep, p, torch.float64)
            assert all(clean[n].tobytes() == r64[n].tobytes() for n in xc.NAMES)
        bad = xc.shares(xc.closed_form(tgt, src, w, lens, H, g, a, saved, keep, p, torch.float64, mutate=mutant), r64, gates)
        print(f"{mutant} {_cid(case)}: share of {_EXPECTED[mutant]} {bad[_EXPECTED[mutant]]:.3g}")
        assert bad[_EXPECTED[mutant]] > 1.0, (case, bad)
        shown += 1
    assert shown >= len(CASES) - 1


@pytest.mark.parametrize("cfg", CONFIGS[1:], ids=lambda c: f"d{c[0]}h{c[1]}")
def test_the_reference_passes_its_gate_at_the_other_configs(cfg):
    for case in CASES:
        *_, r64, r32, gates = _base(cfg, case)
        assert max(xc.shares(r32, r64, gates).values()) <= 0.5 + 1e-12


# ---------------------------------------------------------------------------------------------------- sizes and refusals (no device work)
def _align(n):
    return (n + 255) & ~255


def _planned(B, H, T, L):
    """the rule include/nar_fs2.h states"""
    wgs, nqt, n = ((L + 127) // 128) * H * B, (T + 31) // 32, 1
    while n < 8 and wgs * n < 256 and nqt // (2 * n) >= 4:
        n *= 2
    return n


def test_kv_splits_and_sizes(lib):
    L_, so = lib
    assert so.ns_xg_abi_version() == 1
    seen = set()
    for B in (1, 2, 3, 16, 64):
        for H, d in ((2, 256), (4, 256), (4, 512), (8, 512)):
            for T in (1, 33, 128, 129, 224, 225, 343, 1000, 1030):
                for L in (1, 5, 40, 128, 131, 300):
                    s = L_.NsXgShape(B, T, L, d, H)
                    n = so.ns_xg_kv_splits(C.byref(s))
                    assert n == so.ns_xg_kv_splits(C.byref(s)) == _planned(B, H, T, L), (B, H, T, L, n)
                    assert 1 <= n <= 8
                    if T <= 128:
                        assert n == 1
                    seen.add(n)
    assert seen == {1, 2, 4, 8}
    for case in CASES:  # the GPU test's last case is the one whose planned split is above 1
        for d, H in CONFIGS:
            n = so.ns_xg_kv_splits(C.byref(L_.NsXgShape(case[0], case[1], case[2], d, H)))
            assert (n > 1) == (case[1] == 343), (case, n)
    for B, T, L, d, H in ((2, 1, 1, 256, 2), (3, 343, 40, 512, 8), (16, 1000, 128, 256, 2)):
        s = L_.NsXgShape(B, T, L, d, H)
        MT, ML = B * T, B * L
        assert so.ns_xg_saved_bytes(C.byref(s)) == (3 * MT * d + 2 * ML * d) * 4
        pt, pl = (C.c_int32 * 8)(), (C.c_int32 * 8)()
        assert so.ns_pg_plan_wgrad(MT, d, d, 1, pt) == 0 and so.ns_pg_plan_wgrad(ML, d, d, 1, pl) == 0
        n = so.ns_xg_kv_splits(C.byref(s))
        want = (2 * _align(8 * d * d) + _align(8 * d) + 2 * _align(4 * d * d) + _align(4 * max(pt[5], pl[5]))
                + _align(8 * 2 * ((MT + 63) // 64) * 5 * d) + _align(8 * ((ML + 63) // 64) * 5 * d)
                + 4 * _align(4 * MT * d) + _align(8 * ML * d) + _align(4 * B * H * T) + (_align(n * 8 * ML * d) if n > 1 else 0))
        assert so.ns_xg_ws_bytes(C.byref(s)) == want


def test_every_refusal_precedes_the_first_hip_call(lib):
    L_, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    ok_shape = dict(B=2, T=8, L=5, d=256, H=2)

    def weights(**over):
        w = L_.NsXgWeights()
        for i, n in enumerate(L_.AG_NAMES):
            setattr(w, n, over.get(n, 0x100000 + 0x100000 * i))
        return w

    def fwd(shape=None, w=None, tgt=0x9000000, src=0x9800000, lens=0x9100000, keep=None, p=0.0, y=0xA000000, attn=0xA800000, saved=0xB000000,
            ws=0xC000000, nbytes=1 << 40):
        s = L_.NsXgShape(**dict(ok_shape, **(shape or {})))
        return so.ns_xg_forward(C.byref(s), C.byref(w or weights()), P(tgt), P(src), P(lens), P(keep), p, P(y), P(attn), P(saved), P(ws), nbytes, None)

    def bwd(shape=None, w=None, tgt=0x9000000, src=0x9800000, lens=0x9100000, keep=None, p=0.0, saved=0xB000000, attn=0xA800000, g=0xD000000,
            da=0xD800000, grads=None, ws=0xC000000, nbytes=1 << 40):
        s = L_.NsXgShape(**dict(ok_shape, **(shape or {})))
        d = grads or L_.NsXgGrads()
        return so.ns_xg_backward(C.byref(s), C.byref(w or weights()), P(tgt), P(src), P(lens), P(keep), p, P(saved), P(attn), P(g), P(da), C.byref(d),
                                 P(ws), nbytes, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(tgt=0), "null argument"), (dict(src=0), "null argument"), (dict(lens=0), "null argument"), (dict(attn=0), "null argument"),
                        (dict(ws=0), "null argument"), (dict(tgt=0x9000004), "16-byte aligned"), (dict(src=0x9800008), "16-byte aligned"),
                        (dict(attn=0xA800004), "16-byte aligned"), (dict(lens=0x9100004), "src_lens must be 8-byte aligned"),
                        (dict(shape=dict(d=128)), "d must be 256 or 512"), (dict(shape=dict(d=384)), "d must be 256 or 512"),
                        (dict(shape=dict(H=3)), "d must be a multiple of H"), (dict(shape=dict(H=0)), "d must be a multiple of H"),
                        (dict(shape=dict(H=1)), "d / H must be 64 or 128"), (dict(shape=dict(H=8)), "d / H must be 64 or 128"),
                        (dict(shape=dict(B=0)), "must be positive"), (dict(shape=dict(L=0)), "must be positive"), (dict(shape=dict(T=-1)), "must be positive"),
                        (dict(shape=dict(B=1 << 10, T=1 << 10, L=1 << 10)), "B * H * T * L must stay below 2^31"),
                        (dict(shape=dict(B=1 << 11, T=1, L=1 << 11)), "B * max(T, L) * 2d must stay below 2^31"),
                        (dict(p=1.0), "p_drop must lie in [0, 1)"), (dict(p=-0.1), "p_drop must lie in [0, 1)"),
                        (dict(p=float("nan")), "p_drop must lie in [0, 1)"), (dict(p=0.5), "needs a keep-mask"),
                        (dict(keep=0xE000000), "although p_drop == 0"), (dict(p=0.5, keep=0xE000004), "16-byte aligned"),
                        (dict(w=weights(wk=0)), "null weights->wk"), (dict(w=weights(ln_g=0x100004)), "weights->ln_g must be 16-byte aligned"),
                        (dict(nbytes=1024), "workspace too small")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
    assert fwd(saved=0, nbytes=64) != 0 and "workspace too small" in err()  # saved is nullable
    assert fwd(y=0) != 0 and "null argument" in err()
    assert fwd(y=0xA000004) != 0 and "16-byte aligned" in err()
    assert bwd(saved=0) != 0 and "null argument" in err()
    assert bwd(g=0) != 0 and "null argument" in err()
    assert bwd(g=0xD000004) != 0 and "16-byte aligned" in err()
    assert bwd(da=0xD800004) != 0 and "16-byte aligned" in err()
    d = L_.NsXgGrads()
    d.dtgt = 0x1000004
    assert bwd(grads=d) != 0 and "every gradient must be 16-byte aligned" in err()
    assert bwd() == 0 and so.ns_xg_last_launches() == 0  # nothing wanted: nothing launched, no HIP call
    assert bwd(da=0) == 0 and so.ns_xg_last_launches() == 0  # dA is nullable

    def op(q=0x100000, kv=0x200000, ctx=0x300000, attn=0x400000, dctx=0x500000, da=0x600000, lens=0x700000, B=2, T=8, L=5, d=256, H=2, ks=0,
           dq=0x800000, dkv=0x900000, ws=0xA00000, nbytes=1 << 40):
        return so.ns_xg_op_attention_backward(P(q), P(kv), P(ctx), P(attn), P(dctx), P(da), P(lens), B, T, L, d, H, ks, P(dq), P(dkv), P(ws), nbytes, None)

    for kw, msg in ((dict(q=0), "null argument"), (dict(attn=0), "null argument"), (dict(lens=0), "null argument"), (dict(dkv=0), "null argument"),
                    (dict(ws=0), "null argument"), (dict(kv=0x200008), "16-byte aligned"), (dict(da=0x600004), "16-byte aligned"),
                    (dict(lens=0x700004), "src_lens must be 8-byte aligned"), (dict(d=300), "d must be 256 or 512"), (dict(H=7), "d must be a multiple of H"),
                    (dict(H=8), "d / H must be 64 or 128"), (dict(T=0), "must be positive"), (dict(ks=-1), "kv_splits must lie in [0, 8]"),
                    (dict(ks=9), "kv_splits must lie in [0, 8]"), (dict(B=1 << 10, T=1 << 10, L=1 << 10), "problem too large"),
                    (dict(nbytes=16), "workspace too small"), (dict(ks=3, nbytes=256 + 2 * 2 * 5 * 512 * 4), "workspace too small")):
        assert op(**kw) != 0 and msg in err(), (kw, err())
    assert so.ns_xg_ws_bytes(None) == 0 and "null argument" in err()
    s = L_.NsXgShape(2, 8, 5, 100, 2)
    assert so.ns_xg_ws_bytes(C.byref(s)) == 0 and "d must be 256 or 512" in err()
    assert so.ns_xg_saved_bytes(C.byref(s)) == 0 and "d must be 256 or 512" in err()
    assert so.ns_xg_kv_splits(C.byref(s)) == 0 and "d must be 256 or 512" in err()


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("xg_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("xattngrad.hip", kernels=("k_xg_bwd_q<64>", "k_xg_bwd_q<128>", "k_xg_bwd_kv<64>", "k_xg_bwd_kv<128>", "k_xg_kv_reduce"))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_module_has_the_reference_names_and_refuses_what_it_cannot_do(lib):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import sublayers

    assert pkg.MultiHeadCrossAttention is sublayers.MultiHeadCrossAttention and "MultiHeadCrossAttention" in pkg.__all__
    cfg = wl.model_config("tiny")
    t = cfg["transformer"]
    d = t["decoder_hidden"]
    sd = wl.synth_aligner_state_dict(cfg, seed=0)
    prefixes = sorted({k[:k.index("crs_attn.") + len("crs_attn.")] for k in sd if ".crs_attn." in k})
    assert prefixes and all(p.startswith("mel_encoder.layer_stack.") for p in prefixes)
    sub = {k[len(prefixes[0]):]: torch.as_tensor(np.asarray(v)) for k, v in sd.items() if k.startswith(prefixes[0])}
    assert set(sub) == set(sublayers.PARAM_NAMES)
    dm = sub["w_qs.weight"].shape[1]
    H = 2 if dm == 256 else 4
    m = sublayers.MultiHeadCrossAttention(H, dm, dm // H, dm // H, dropout=0.1)
    assert sorted(n for n, _ in m.named_parameters()) == sorted(sublayers.PARAM_NAMES)
    m.load_state_dict(sub)  # strict: the checkpoint's subtree, unchanged
    assert m.training and d
    tgt, src = torch.zeros(2, 5, dm), torch.zeros(2, 3, dm)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(tgt, src, src)
    with pytest.raises(ValueError, match="k and v must be the same tensor"):
        m(tgt, src, src.clone())
    with pytest.raises(ValueError, match="d_k must equal d_v"):
        sublayers.MultiHeadCrossAttention(2, 256, 128, 64)
    with pytest.raises(ValueError, match="n_head \\* d_k must equal d_model"):
        sublayers.MultiHeadCrossAttention(2, 256, 64, 64)
    with pytest.raises(ValueError, match=r"dropout must lie in \[0, 1\)"):
        sublayers.MultiHeadCrossAttention(2, 256, 128, 128, dropout=1.0)
    with pytest.raises(ValueError, match="d_model must be 256 or 512 and d_k 64 or 128"):
        sublayers.MultiHeadCrossAttention(8, 256, 32, 32)
    with pytest.raises(ValueError, match="d_model must be 256 or 512"):
        sublayers.MultiHeadCrossAttention(2, 128, 64, 64)
    # the self-attention module still refuses cross-attention
    sa = sublayers.MultiHeadAttention(H, dm, dm // H, dm // H)
    with pytest.raises(NotImplementedError, match="self-attention only"):
        sa(tgt, src, src)
