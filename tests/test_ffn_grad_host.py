"""The yardstick of tests/test_gpu_ffn_grad.py proven on the CPU, and every refusal of the ns_fg_* family (no GPU).

On the fixture (tests/golden/ffn_grad_tiny.npz, the reference's own PositionwiseFeedForward and FFTBlock in train() at dropout 0) the
float64 restatement agrees with the reference's float64 autograd to <= 1e-12 relative, and the fp32 restatement stays within the
fixture's own fp32-vs-float64 distance of the fixture's fp32 values.  (In the block, d_bk is zero in exact arithmetic — the softmax does
not see a key bias — so its bounds are taken relative to the other gradients' scale, as tests/test_attention_grad_host.py does.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import attention_grad_cpu as ac
from tests import ffn_grad_cpu as fc
from tests.util import assert_no_spill, built_lib, expect_refusals, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((2, 1), (3, 5), (2, 33), (1, 65), (3, 130))  # the (B, S) table of tests/test_gpu_ffn_grad.py


@pytest.fixture(scope="module")
def lib():
    return built_lib()


def _fixture(c):
    meta, z = load_golden("ffn_grad_tiny")
    k1, k2 = meta["configs"][c]
    w = fc.seeded_weights(meta["d"], meta["d_hid"], k1, k2, meta["seeds"][c])
    return meta, z, w, z[f"{c}_x"], z[f"{c}_g"]


def _within(got, z, key, f64_scale=None):
    """the two bounds of a recorded tensor: fp32 within the fixture's own fp32-vs-float64 distance, float64 to 1e-12 relative"""
    want32, want64 = z[key].astype(np.float64), z[key + "_f64"]
    dist = np.abs(want32 - want64).max()
    err32 = np.abs(got[0].astype(np.float64) - want32).max()
    err64 = np.abs(got[1] - want64).max()
    print(f"{key}: fp32 {err32:.3g} (fixture's fp32-vs-float64 distance {dist:.3g}), float64 {err64:.3g}")
    assert got[0].shape == z[key].shape and err32 <= dist, key
    assert err64 <= 1e-12 * (np.abs(want64).max() if f64_scale is None else f64_scale), key


# ---------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("c", ["a", "b"])
def test_restatement_reproduces_the_reference(c):
    meta, z, w, x, g = _fixture(c)
    r64, f64 = fc.autograd_ref(x, w, g, dtype=torch.float64)
    r32, f32 = fc.autograd_ref(x, w, g, dtype=torch.float32)
    _within((f32["y"].numpy(), f64["y"].numpy()), z, f"{c}_y")
    for n in fc.NAMES:
        _within((r32[n], r64[n]), z, f"{c}_d_{n}")


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("c", ["a", "b"])
def test_closed_form_equals_float64_autograd(c, p):
    meta, z, w, x, g = _fixture(c)
    keep = (np.random.RandomState(7).rand(*x.shape) >= p) if p > 0 else None
    ref, fwd = fc.autograd_ref(x, w, g, keep, p, torch.float64)
    got = fc.closed_form(x, w, g, (fwd["h"], fwd["z"]), keep, p, torch.float64)
    for n in fc.NAMES:
        assert got[n].shape == ref[n].shape and np.abs(got[n] - ref[n]).max() <= 1e-12 * np.abs(ref[n]).max(), n
    assert not got["_dh"][fwd["h"].numpy() <= 0].any() and np.abs(got["_da"][fwd["h"].numpy() <= 0]).max() > 0


def _gated(x, w, g, keep, p):
    """(saved tensors of the fp32 forward, float64 closed form from them, fp32 closed form, the gates)"""
    fwd = fc.statement(x, w, keep, p, torch.float32)
    saved = (fwd["h"].detach(), fwd["z"].detach())
    r64 = fc.closed_form(x, w, g, saved, keep, p, torch.float64)
    r32 = fc.closed_form(x, w, g, saved, keep, p, torch.float32)
    return saved, r64, r32, fc.gate(r32, r64)


# (mutant, (B, S)) pairs on which the mutation changes nothing, and the case of the table that does catch it
BLIND = {
    ("dgrad_without_tap_flip", (2, 1)): (3, 5),      # S = 1: only the centre tap is in range, and it is its own mirror image
    ("wgrad_across_utterances", (1, 65)): (3, 130),  # B = 1: there is no neighbouring utterance to read
}
EXPECTED = {"relu_gate_dropped": "w1", "gate_from_preactivation_sign_of_da": "w1", "dgrad_without_tap_flip": "dx", "wgrad_across_utterances": "w1",
            "residual_dropped": "dx", "keep_scale_dropped": "w2", "db1_before_gate": "b1"}


@pytest.mark.parametrize("kernel", [(9, 1), (3, 3)], ids=lambda k: f"k{k[0]}{k[1]}")
@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_gate_rejects_mutant(mutant, kernel):
    """each mutant, evaluated in float64 (its only error is the mutation), is outside the gate of the tensor it damages on every case of
    the GPU test's table — but for the pairs of BLIND, where it is the identity; the fp32 closed form itself is inside every gate
    (share <= 0.5 by construction).  Run at p = 0.5 with a keep-mask, so that the dropout scale is in every case."""
    d, d_hid, p = 32, 64, 0.5
    w = fc.seeded_weights(d, d_hid, kernel[0], kernel[1], seed=3)
    for i, (B, S) in enumerate(CASES):
        rs = np.random.RandomState(11 + i)
        x = rs.standard_normal((B, S, d)).astype(np.float32)
        g = rs.standard_normal((B, S, d)).astype(np.float32)
        keep = rs.rand(B, S, d) >= p
        saved, r64, r32, gates = _gated(x, w, g, keep, p)
        good = fc.shares(r32, r64, gates)
        assert max(good.values()) <= 0.5 + 1e-12, ((B, S), good)
        bad = fc.shares(fc.closed_form(x, w, g, saved, keep, p, torch.float64, mutate=mutant), r64, gates)
        worst = max(bad, key=bad.get)
        print(f"{mutant} {kernel} {(B, S)}: worst share {bad[worst]:.3g} ({worst})")
        if (mutant, (B, S)) in BLIND:
            assert bad[worst] == 0.0 and BLIND[(mutant, (B, S))] in CASES and (mutant, BLIND[(mutant, (B, S))]) not in BLIND, bad
        else:
            assert bad[EXPECTED[mutant]] > 1.0, ((B, S), bad)


def test_fft_block_composite_reproduces_the_reference():
    meta, z = load_golden("ffn_grad_tiny")
    d, H, lens = meta["d"], meta["H"], meta["lens"]
    wa = ac.seeded_weights(d, meta["seeds"]["blk_attn"])
    wf = fc.seeded_weights(d, meta["d_hid"], meta["block_kernel"][0], meta["block_kernel"][1], meta["seeds"]["blk_ffn"])
    got = {}
    for dtype in (torch.float32, torch.float64):
        la = {k: v.clone().requires_grad_(True) for k, v in ac._w(wa, dtype).items()}
        la["x"] = torch.as_tensor(z["blk_x"]).to(dtype).clone().requires_grad_(True)
        lf = {k: v.clone().requires_grad_(True) for k, v in fc._w(wf, dtype).items()}
        y = fc.fft_block(None, None, None, lens, H, dtype=dtype, leaves=(la, lf))
        names = [f"a_{n}" for n in ac.NAMES[:10]] + [f"f_{n}" for n in fc.NAMES[:6]] + ["dx"]
        grads = torch.autograd.grad(y, [la[n] for n in ac.NAMES[:10]] + [lf[n] for n in fc.NAMES[:6]] + [la["x"]],
                                    grad_outputs=torch.as_tensor(z["blk_g"]).to(dtype))
        got[dtype] = dict(zip(names, (t.numpy() for t in grads)), y=y.detach().numpy())
    pad = np.arange(meta["S"])[None, :] >= np.asarray(lens)[:, None]
    assert not got[torch.float64]["y"][pad].any() and not z["blk_y"][pad].any()
    _within((got[torch.float32]["y"], got[torch.float64]["y"]), z, "blk_y")
    scale = max(np.abs(z[f"blk_d_{n}_f64"]).max() for n in names)
    for n in names:
        if n == "a_bk":  # zero up to rounding: relative to the gradients' common scale, in both precisions
            assert np.abs(got[torch.float64][n] - z["blk_d_a_bk_f64"]).max() <= 1e-12 * scale
            assert np.abs(got[torch.float32][n].astype(np.float64) - z["blk_d_a_bk"]).max() <= np.abs(z["blk_d_a_bq"].astype(np.float64) - z["blk_d_a_bq_f64"]).max()
            continue
        _within((got[torch.float32][n], got[torch.float64][n]), z, f"blk_d_{n}")


# ---------------------------------------------------------------------------------------------------- sizes and refusals (no device work)
def _align(n):
    return (n + 255) & ~255


def test_sizes_and_versions(lib):
    L, so = lib
    assert so.ns_fg_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    versions = dict(re.findall(r"^#define NS_(\w*?)_?ABI_VERSION (\d+)$", header, re.M))
    assert versions == {"": "6", "VOC": "1", "ALN": "1", "LOSS": "1", "MEL": "1", "GL": "1", "VT": "1", "OPT": "1", "LOSSG": "1", "PG": "1", "AG": "1",
                        "XG": "1", "PN": "1", "VA": "1", "FG": "1"}
    for fam, v in versions.items():
        assert getattr(so, f"ns_{fam.lower()}_abi_version" if fam else "ns_abi_version")() == int(v), fam
    for B, S, d, di, K1, K2 in ((2, 1, 256, 1024, 9, 1), (3, 343, 512, 2048, 9, 1), (16, 1000, 256, 1024, 9, 1), (2, 33, 256, 512, 3, 3)):
        s = L.NsFgShape(B, S, d, di, K1, K2)
        M, nblk = B * S, (B * S + 63) // 64
        assert so.ns_fg_saved_bytes(C.byref(s)) == M * (di + d) * 4
        p1, p2 = (C.c_int32 * 8)(), (C.c_int32 * 8)()
        assert so.ns_pg_plan_wgrad(M, di, d, K1, p1) == 0 and so.ns_pg_plan_wgrad(M, d, di, K2, p2) == 0
        want = (2 * (_align(4 * di * d * K1) + _align(4 * d * di * K2)) + _align(4 * max(p1[5], p2[5])) + _align(8 * nblk * 5 * d)
                + _align(8 * nblk * 5 * di) + 2 * _align(4 * M * d) + _align(4 * M * di))
        assert so.ns_fg_ws_bytes(C.byref(s)) == want
    # monotone in B, 0 on refused shapes
    last_ws = last_saved = 0
    for B in (1, 2, 3, 5, 8, 16, 33):
        s = L.NsFgShape(B, 77, 256, 1024, 9, 1)
        ws, saved = so.ns_fg_ws_bytes(C.byref(s)), so.ns_fg_saved_bytes(C.byref(s))
        assert ws > last_ws and saved > last_saved
        last_ws, last_saved = ws, saved
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    for bad, msg in ((dict(d=100), "d must be 256 or 512"), (dict(d_inner=0), "d_inner must be a positive multiple of 256"),
                     (dict(d_inner=384), "d_inner must be a positive multiple of 256"), (dict(K1=4), "K1 must be odd and positive"),
                     (dict(K2=0), "K2 must be odd and positive"), (dict(K2=-1), "K2 must be odd and positive"), (dict(B=0), "must be positive"),
                     (dict(S=-3), "must be positive"), (dict(B=1 << 11, S=1 << 10), "problem too large"),
                     (dict(d_inner=256 * 4097), "refuses this shape")):
        s = L.NsFgShape(**dict(dict(B=2, S=8, d=256, d_inner=1024, K1=9, K2=1), **bad))
        assert so.ns_fg_ws_bytes(C.byref(s)) == 0 and msg in err(), (bad, err())
        assert so.ns_fg_saved_bytes(C.byref(s)) == 0 and msg in err(), (bad, err())
    assert so.ns_fg_ws_bytes(None) == 0 and "null argument" in err()
    assert so.ns_fg_saved_bytes(None) == 0 and "null argument" in err()


def test_every_refusal_precedes_the_first_hip_call(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    ok_shape = dict(B=2, S=8, d=256, d_inner=1024, K1=9, K2=1)

    def weights(**over):
        w = L.NsFgWeights()
        for i, n in enumerate(L.FG_NAMES):
            setattr(w, n, over.get(n, 0x1000000 + 0x1000000 * i))
        return w

    def fwd(shape=None, w=None, x=0x9000000, keep=None, p=0.0, y=0xA000000, saved=0xB000000, ws=0xC000000, nbytes=1 << 40):
        s = L.NsFgShape(**dict(ok_shape, **(shape or {})))
        return so.ns_fg_forward(C.byref(s), C.byref(w or weights()), P(x), P(keep), p, P(y), P(saved), P(ws), nbytes, None)

    def bwd(shape=None, w=None, x=0x9000000, keep=None, p=0.0, saved=0xB000000, g=0xD000000, grads=None, ws=0xC000000, nbytes=1 << 40):
        s = L.NsFgShape(**dict(ok_shape, **(shape or {})))
        d = grads or L.NsFgGrads()
        return so.ns_fg_backward(C.byref(s), C.byref(w or weights()), P(x), P(keep), p, P(saved), P(g), C.byref(d), P(ws), nbytes, None)

    for call in (fwd, bwd):
        expect_refusals(err, call, ((dict(x=0), "null argument"), (dict(ws=0), "null argument"), (dict(x=0x9000004), "x must be 16-byte aligned"),
                        (dict(ws=0xC000008), "the workspace must be 16-byte aligned"), (dict(saved=0xB000004), "saved must be 16-byte aligned"),
                        (dict(shape=dict(d=128)), "d must be 256 or 512"), (dict(shape=dict(d=384)), "d must be 256 or 512"),
                        (dict(shape=dict(d_inner=0)), "d_inner must be a positive multiple of 256"),
                        (dict(shape=dict(d_inner=1000)), "d_inner must be a positive multiple of 256"),
                        (dict(shape=dict(d_inner=-256)), "d_inner must be a positive multiple of 256"),
                        (dict(shape=dict(K1=8)), "K1 must be odd and positive"), (dict(shape=dict(K1=0)), "K1 must be odd and positive"),
                        (dict(shape=dict(K2=2)), "K2 must be odd and positive"), (dict(shape=dict(K2=-3)), "K2 must be odd and positive"),
                        (dict(shape=dict(B=0)), "must be positive"), (dict(shape=dict(S=0)), "must be positive"),
                        (dict(shape=dict(B=1 << 11, S=1 << 10)), "B * S * d_inner must stay below 2^31"),
                        (dict(shape=dict(d_inner=256 * 4097)), "refuses this shape"),  # K2 * d_inner past the weight gradient's 2^20 columns
                        (dict(p=1.0), "p_drop must lie in [0, 1)"), (dict(p=-0.1), "p_drop must lie in [0, 1)"),
                        (dict(p=float("nan")), "p_drop must lie in [0, 1)"), (dict(p=0.5), "needs a keep-mask"),
                        (dict(keep=0xE000000), "although p_drop == 0"), (dict(p=0.5, keep=0xE000004), "16-byte aligned"),
                        (dict(w=weights(w2=0)), "null weights->w2"), (dict(w=weights(b1=0)), "null weights->b1"),
                        (dict(w=weights(ln_g=0x100004)), "weights->ln_g must be 16-byte aligned"), (dict(nbytes=1024), "workspace too small")))
    assert fwd(saved=0, nbytes=64) != 0 and "workspace too small" in err()  # saved is nullable in the forward
    assert fwd(y=0) != 0 and "null argument" in err()
    assert fwd(y=0xA000004) != 0 and "y must be 16-byte aligned" in err()
    assert bwd(saved=0) != 0 and "null argument" in err()
    assert bwd(g=0) != 0 and "null argument" in err()
    assert bwd(g=0xD000004) != 0 and "g must be 16-byte aligned" in err()
    for n in L.FG_NAMES + ("dx",):
        d = L.NsFgGrads()
        setattr(d, n, 0x1000004)
        assert bwd(grads=d) != 0 and "every gradient must be 16-byte aligned" in err(), n
    assert bwd() == 0 and so.ns_fg_last_launches() == 0  # nothing wanted: nothing launched, no HIP call

    def gate(da=0x100000, h=0x200000, M=16, di=1024, dh=0x300000, d_b1=0x400000, ws=0x500000, nbytes=1 << 40):
        return so.ns_fg_op_relu_gate(P(da), P(h), M, di, P(dh), P(d_b1), P(ws), nbytes, None)

    for kw, msg in ((dict(da=0), "null argument"), (dict(h=0), "null argument"), (dict(dh=0), "null argument"), (dict(ws=0), "null argument"),
                    (dict(M=0), "M must be positive"), (dict(di=0), "d_inner must be a positive multiple of 256"),
                    (dict(di=640 + 1), "d_inner must be a positive multiple of 256"), (dict(M=1 << 21), "problem too large"),
                    (dict(h=0x200004), "h must be 16-byte aligned"), (dict(d_b1=0x400008), "d_b1 must be 16-byte aligned"),
                    (dict(nbytes=8), "workspace too small")):
        assert gate(**kw) != 0 and msg in err(), (kw, err())


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("fg_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernel_does_not_spill():
    assert_no_spill("ffngrad.hip", kernels=("k_fg_relu_gate",))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_modules_have_the_reference_names_and_no_cpu_path(lib):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import sublayers
    from tests.util import weights_for

    assert pkg.PositionwiseFeedForward is sublayers.PositionwiseFeedForward and pkg.FFTBlock is sublayers.FFTBlock
    cfg, sd = weights_for(dict(config="tiny", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25))
    t = wl.model_config("tiny")["transformer"]
    d, H, di, ks = t["encoder_hidden"], t["encoder_head"], t["conv_filter_size"], t["conv_kernel_size"]
    f = sublayers.PositionwiseFeedForward(d, di, ks, dropout=t["encoder_dropout"])
    blk = sublayers.FFTBlock(d, H, d // H, d // H, di, ks, dropout=t["encoder_dropout"])
    assert sorted(n for n, _ in f.named_parameters()) == sorted(sublayers.FFN_PARAM_NAMES)
    assert sorted(n for n, _ in blk.named_parameters()) == sorted([f"slf_attn.{n}" for n in sublayers.PARAM_NAMES]
                                                                  + [f"pos_ffn.{n}" for n in sublayers.FFN_PARAM_NAMES])
    assert not list(f.named_buffers()) and not list(blk.named_buffers())
    n_loaded = 0
    for stack, key in (("encoder", "txt_encoder"), ("decoder", "mel_decoder")):
        if (t[f"{stack}_hidden"], t[f"{stack}_head"]) != (d, H):
            continue
        for i in range(t[f"{stack}_layer"]):
            prefix = f"{key}.layer_stack.{i}."
            sub = {k[len(prefix):]: torch.as_tensor(np.asarray(v)) for k, v in sd.items() if k.startswith(prefix)}
            ffn = {k[len("pos_ffn."):]: v for k, v in sub.items() if k.startswith("pos_ffn.")}
            if not ffn:
                continue
            assert set(ffn) == set(sublayers.FFN_PARAM_NAMES), (prefix, sorted(ffn))
            f.load_state_dict(ffn)  # strict: the checkpoint's subtree, unchanged
            blk.load_state_dict(sub)
            assert torch.equal(blk.pos_ffn.w_1.weight, f.w_1.weight) and tuple(f.w_1.weight.shape) == (di, d, ks[0])
            n_loaded += 1
    assert n_loaded == 2
    assert f.training and blk.training
    x = torch.zeros(2, 5, d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        blk(x)
    with pytest.raises(ValueError, match="d_in must be 256 or 512"):
        sublayers.PositionwiseFeedForward(128, 1024, (9, 1))
    with pytest.raises(ValueError, match="d_hid must be a positive multiple of 256"):
        sublayers.PositionwiseFeedForward(256, 1000, (9, 1))
    with pytest.raises(ValueError, match="kernel sizes must be odd"):
        sublayers.PositionwiseFeedForward(256, 1024, (8, 1))
    with pytest.raises(ValueError, match=r"dropout must lie in \[0, 1\)"):
        sublayers.PositionwiseFeedForward(256, 1024, (9, 1), dropout=1.0)
