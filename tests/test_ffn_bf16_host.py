"""The yardstick of tests/test_gpu_ffn_bf16.py proven on the CPU, the plan of the bf16 weight gradient, every refusal of the
ns_fg_*_bf16 entry points and the Python surface of the opt-in "bf16" feed-forward mode (no GPU).

The gate (tests/ffn_bf16_emu.py) is proven both ways on the GPU test's own table: torch's fp32 evaluation of the rounded operands is
inside it on every case, on random-sign and on same-sign operands, and each wrong variant, evaluated in float64 (its only error is the
mutation), is outside it on every case where it is not the identity; those cases are named in BLIND."""
import ctypes as C

import pytest
import torch

from tests import ffn_bf16_emu as E
from tests.util import assert_no_spill, built_lib, expect_refusals, run_c_caller

WEIGHTS = [(cfg, i) for cfg in E.CONFIGS for i in range(2)]
_wid = lambda cw: f"d{cw[0][0]}i{cw[0][1]}k{cw[0][2]}{cw[0][3]}-w{cw[1] + 1}"  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    return built_lib()


# ---------------------------------------------------------------------------------------------------- the gate, both ways
def _blind(mutant, B, S, KW):
    """the (mutant, case, weight) triples on which the mutation changes nothing, by rule"""
    pad, M = (KW - 1) // 2, B * S
    return {"drop_last_tap": KW > 1 and S <= pad,    # the last tap reads t + pad: outside every utterance
            "cross_utterance": B == 1 or KW == 1,     # no neighbouring utterance, or no tap that leaves the row
            "drop_second_kstep": M <= 16,             # the rows [16, 32) do not exist
            "no_tap_flip": KW == 1 or S == 1,         # one tap, or only the centre tap in range: its own mirror image
            }.get(mutant, False)


# the cases of the table each rule above names (B, S, KW) — written out, so that a change of the table or of a rule shows here
BLIND = {
    "drop_last_tap": {(2, 1, 9), (2, 1, 3)},
    "cross_utterance": {(1, 65, 9), (1, 65, 3), (1, 65, 1), (2, 1, 1), (3, 5, 1), (2, 33, 1), (3, 130, 1)},
    "drop_second_kstep": {(2, 1, 9), (2, 1, 3), (2, 1, 1), (3, 5, 9), (3, 5, 3), (3, 5, 1)},
    "no_tap_flip": {(2, 1, 9), (2, 1, 3), (2, 1, 1), (3, 5, 1), (2, 33, 1), (1, 65, 1), (3, 130, 1)},
}


def test_blind_cases_are_the_named_ones():
    for mutant, named in BLIND.items():
        ruled = {(B, S, KW) for cfg in E.CONFIGS for (_, _, KW) in E.weight_shapes(cfg) for (B, S) in E.CASES if _blind(mutant, B, S, KW)}
        assert ruled == named, (mutant, sorted(ruled ^ named))
        assert {(B, S, KW) for cfg in E.CONFIGS for (_, _, KW) in E.weight_shapes(cfg) for (B, S) in E.CASES} - ruled, mutant  # caught somewhere


@pytest.mark.parametrize("cw", WEIGHTS, ids=_wid)
def test_wgrad_gate_passes_fp32_and_rejects_mutants(cw, lib):
    cfg, i = cw
    N, Cin, KW = E.weight_shapes(cfg)[i]
    for ci, (B, S) in enumerate(E.CASES):
        M = B * S
        E.plan(lib[1], M, N, Cin, KW)  # rows per range <= 2816: the bound's own statement holds on this case
        for same_sign in (False, True):
            dz, x = E.operands(B, S, N, Cin, seed=1000 * ci + N + KW + same_sign, same_sign=same_sign)
            ref, unit = E.wgrad_emu(dz, x, KW), E.wgrad_unit(dz, x, KW)
            good = E.wgrad_check(E.wgrad_emu(dz, x, KW, dtype=torch.float32), dz, x, KW, ref=ref, unit=unit)
            print(f"{_wid(cw)} {(B, S)} same_sign={same_sign}: fp32 CPU {good.worst:.3g} of the bound")
            assert good.ok and good.worst <= 0.5, str(good)
            if same_sign:
                continue
            mutants = {
                "unrounded": dict(round_fn=E.exact),
                "truncated": dict(round_fn=E.bf_trunc),
                "drop_last_tap": dict(drop_tap=KW - 1),
                "cross_utterance": dict(cross_utterance=True),
                "drop_second_kstep": dict(drop_rows=(16, 32)),
                "drop_last_partial_stage": dict(drop_rows=E.last_partial_stage(M)),
            }
            assert mutants["drop_last_partial_stage"]["drop_rows"] is not None  # no case of the table has only full stages
            for name, kw in mutants.items():
                wrong = E.wgrad_emu(dz, x, KW, **kw)
                bad = E.wgrad_check(wrong, dz, x, KW, ref=ref, unit=unit)
                print(f"  {name}: {bad.worst:.3g}")
                if _blind(name, B, S, KW):
                    assert torch.equal(wrong, ref) and (B, S, KW) in BLIND[name], (name, (B, S), str(bad))
                else:
                    assert not bad.ok and (bad.worst > 1.0 or not bad.zeros_ok), (name, (B, S), str(bad))


@pytest.mark.parametrize("cw", WEIGHTS, ids=_wid)
def test_dgrad_gate_passes_fp32_and_rejects_mutants(cw):
    cfg, i = cw
    N, Cin, KW = E.weight_shapes(cfg)[i]
    w = (torch.randn(N, Cin, KW, generator=torch.Generator().manual_seed(N + KW)) / (Cin * KW) ** 0.5).float()
    for ci, (B, S) in enumerate(E.CASES):
        dz, resid = E.operands(B, S, N, Cin, seed=77 * ci + Cin + KW)
        fp32 = E.dgrad_emu(dz, w, resid, dtype=torch.float32)
        good = E.dgrad_check(fp32, dz, w, resid)
        print(f"{_wid(cw)} {(B, S)}: fp32 CPU {good.worst:.3g} of the bound")
        assert good.ok and good.worst <= 0.5, str(good)
        for name, kw in (("unrounded", dict(round_fn=E.exact)), ("truncated", dict(round_fn=E.bf_trunc)), ("no_tap_flip", dict(no_flip=True)),
                         ("resid_before_rounding", dict(resid_before_rounding=True))):
            wrong = E.dgrad_emu(dz, w, resid, **kw)
            bad = E.dgrad_check(wrong, dz, w, resid)
            print(f"  {name}: {bad.worst:.3g}")
            if _blind(name, B, S, KW):
                assert torch.equal(wrong, E.dgrad_emu(dz, w, resid)) and (B, S, KW) in BLIND[name], (name, (B, S), str(bad))
            else:
                assert not bad.ok and bad.worst > 1.0, (name, (B, S), str(bad))


def test_zero_elements_must_be_plus_zero():
    """S <= pad: the taps |j - pad| >= S are outside every utterance; the gate wants +0.0 there, bit for bit"""
    B, S, N, Cin, KW = 2, 2, 128, 32, 9
    dz, x = E.operands(B, S, N, Cin, seed=5)
    ref, unit = E.wgrad_emu(dz, x, KW), E.wgrad_unit(dz, x, KW)
    dead = unit == 0
    assert bool(dead[:, :, 0].all()) and bool(dead[:, :, 8].all()) and not bool(dead[:, :, 4].any()) and not bool(dead[:, :, 3].any())
    good = ref.float()
    assert E.wgrad_check(good, dz, x, KW, ref=ref, unit=unit).ok
    for wrong in (-0.0, 1e-30):
        bad = good.clone()
        bad[0, 0, 0] = wrong
        c = E.wgrad_check(bad, dz, x, KW, ref=ref, unit=unit)
        assert not c.ok and not c.zeros_ok, wrong


# ---------------------------------------------------------------------------------------------------- the plan
def test_plan_invariants_and_refusals(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    shapes = [(M, N, Cin, KW) for M in (1, 2, 15, 31, 32, 33, 64, 65, 66, 390, 2048, 2100, 16000, 40000)
              for (N, Cin, KW) in ((1024, 256, 9), (256, 1024, 1), (2048, 512, 9), (512, 256, 3), (128, 32, 1), (128, 2048, 5))]
    for M, N, Cin, KW in shapes:
        out, again = (C.c_int32 * 8)(), (C.c_int32 * 8)()
        assert so.ns_fg_plan_wgrad_bf16(M, N, Cin, KW, out) == 0, (M, N, Cin, KW, err())
        assert so.ns_fg_plan_wgrad_bf16(M, N, Cin, KW, again) == 0 and list(out) == list(again)  # a function of the shape alone
        tile_n, tile_c, rows, ranges, tiles, ws_floats, chunk, zero = out
        assert (tile_n, tile_c, zero) == (128, 128, 0) and chunk % 32 == 0
        assert rows > 0 and rows % 32 == 0, out[:]                                  # a multiple of the stage
        assert (ranges - 1) * rows < M <= ranges * rows, (M, rows, ranges)         # the ranges cover [0, M) exactly, none empty
        assert tiles == (N // 128) * ((KW * Cin + 127) // 128)
        assert 0 < ws_floats < 2 ** 31 and ws_floats == ranges * N * KW * Cin
        assert ranges == 1 or rows >= 64                                            # never shorter than two stages
    out = (C.c_int32 * 8)()
    for bad in ((0, 1024, 256, 9), (-5, 1024, 256, 9), (64, 1000, 256, 9), (64, 0, 256, 9), (64, 1024, 0, 9), (64, 1024, 48, 9),
                (64, 1024, 260, 9), (64, 1024, 16, 1), (64, 1024, 256, 8), (64, 1024, 256, 0), (64, 1024, 256 * 4097, 1),
                (1 << 22, 1024, 256, 1), (1 << 20, 128, 4096, 1), (1 << 21, 1024, 256, 9)):
        assert so.ns_fg_plan_wgrad_bf16(*bad, out) != 0 and "ns_fg_plan_wgrad_bf16: refused" in err(), bad
    assert so.ns_fg_plan_wgrad_bf16(64, 1024, 256, 9, None) != 0 and "null argument" in err()
    # what ns_pg_plan_wgrad refuses, this refuses; Cin % 32 on top
    for M, N, Cin, KW in ((64, 1000, 256, 9), (64, 1024, 256, 8), (0, 1024, 256, 9)):
        assert so.ns_pg_plan_wgrad(M, N, Cin, KW, out) != 0 and so.ns_fg_plan_wgrad_bf16(M, N, Cin, KW, out) != 0
    assert so.ns_pg_plan_wgrad(64, 1024, 48, 9, out) == 0 and so.ns_fg_plan_wgrad_bf16(64, 1024, 48, 9, out) != 0


# ---------------------------------------------------------------------------------------------------- sizes and refusals (no device work)
def _align(n):
    return (n + 255) & ~255


def test_sizes(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    for B, S, d, di, K1, K2 in ((2, 1, 256, 1024, 9, 1), (3, 343, 512, 2048, 9, 1), (16, 1000, 256, 1024, 9, 1), (2, 33, 256, 512, 3, 3)):
        s = L.NsFgShape(B, S, d, di, K1, K2)
        M, nblk = B * S, (B * S + 63) // 64
        p1, p2 = (C.c_int32 * 8)(), (C.c_int32 * 8)()
        assert so.ns_fg_plan_wgrad_bf16(M, di, d, K1, p1) == 0 and so.ns_fg_plan_wgrad_bf16(M, d, di, K2, p2) == 0
        want = (2 * (_align(2 * di * d * K1) + _align(2 * d * di * K2)) + _align(4 * max(p1[5], p2[5])) + _align(8 * nblk * 5 * d)
                + _align(8 * nblk * 5 * di) + 2 * _align(4 * M * d) + _align(4 * M * di))
        assert so.ns_fg_ws_bytes_bf16(C.byref(s)) == want  # bf16 planes where the fp32 workspace holds fp32 ones
        assert so.ns_fg_saved_bytes(C.byref(s)) == M * (di + d) * 4  # shared
        assert so.ns_fg_op_bf16_ws_bytes(B, S, di, d, K1) == _align(2 * di * d * K1) + _align(4 * p1[5])
    for bad, msg in ((dict(d=100), "d must be 256 or 512"), (dict(d_inner=384), "d_inner must be a positive multiple of 256"),
                     (dict(K1=4), "K1 must be odd and positive"), (dict(K2=0), "K2 must be odd and positive"), (dict(B=0), "must be positive"),
                     (dict(B=1 << 11, S=1 << 10), "problem too large"), (dict(d_inner=256 * 4097), "refuses this shape")):
        s = L.NsFgShape(**dict(dict(B=2, S=8, d=256, d_inner=1024, K1=9, K2=1), **bad))
        assert so.ns_fg_ws_bytes_bf16(C.byref(s)) == 0 and msg in err(), (bad, err())
    assert so.ns_fg_ws_bytes_bf16(None) == 0 and "null argument" in err()
    for bad, msg in ((dict(B=0), "must be positive"), (dict(N=100), "N must be a positive multiple of 32"), (dict(Cin=48), "Cin must be a positive multiple of 32"),
                     (dict(KW=2), "KW must be odd and positive"), (dict(B=1 << 12, S=1 << 10), "problem too large")):
        kw = dict(dict(B=2, S=8, N=1024, Cin=256, KW=9), **bad)
        assert so.ns_fg_op_bf16_ws_bytes(kw["B"], kw["S"], kw["N"], kw["Cin"], kw["KW"]) == 0 and msg in err(), (bad, err())


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
        return so.ns_fg_forward_bf16(C.byref(s), C.byref(w or weights()), P(x), P(keep), p, P(y), P(saved), P(ws), nbytes, None)

    def bwd(shape=None, w=None, x=0x9000000, keep=None, p=0.0, saved=0xB000000, g=0xD000000, grads=None, ws=0xC000000, nbytes=1 << 40):
        s = L.NsFgShape(**dict(ok_shape, **(shape or {})))
        d = grads or L.NsFgGrads()
        return so.ns_fg_backward_bf16(C.byref(s), C.byref(w or weights()), P(x), P(keep), p, P(saved), P(g), C.byref(d), P(ws), nbytes, None)

    # the table of tests/test_ffn_grad_host.py for the fp32 namesakes: the same refusals in the same words
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
                        (dict(shape=dict(d_inner=256 * 4097)), "refuses this shape"),
                        (dict(p=1.0), "p_drop must lie in [0, 1)"), (dict(p=-0.1), "p_drop must lie in [0, 1)"),
                        (dict(p=float("nan")), "p_drop must lie in [0, 1)"), (dict(p=0.5), "needs a keep-mask"),
                        (dict(keep=0xE000000), "although p_drop == 0"), (dict(p=0.5, keep=0xE000004), "16-byte aligned"),
                        (dict(w=weights(w2=0)), "null weights->w2"), (dict(w=weights(b1=0)), "null weights->b1"),
                        (dict(w=weights(ln_g=0x100004)), "weights->ln_g must be 16-byte aligned"), (dict(nbytes=1024), "workspace too small")))
    assert "ns_fg_backward_bf16: " in err()
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

    def wgrad(dz=0x100000, X=0x200000, B=2, S=8, N=1024, Cin=256, KW=9, dW=0x300000, ws=0x500000, nbytes=1 << 40):
        return so.ns_fg_op_wgrad_bf16(P(dz), P(X), B, S, N, Cin, KW, P(dW), P(ws), nbytes, None)

    expect_refusals(err, wgrad, ((dict(dz=0), "null argument"), (dict(X=0), "null argument"), (dict(dW=0), "null argument"), (dict(ws=0), "null argument"),
                    (dict(B=0), "must be positive"), (dict(S=-1), "must be positive"), (dict(N=100), "N must be a positive multiple of 32"),
                    (dict(N=160), "the weight gradient's plan refuses"), (dict(Cin=16), "Cin must be a positive multiple of 32"),
                    (dict(KW=4), "KW must be odd and positive"), (dict(B=1 << 12, S=1 << 10), "problem too large"),
                    (dict(dz=0x100004), "dz must be 16-byte aligned"), (dict(X=0x200008), "X must be 16-byte aligned"),
                    (dict(dW=0x300004), "dW must be 16-byte aligned"), (dict(ws=0x500004), "the workspace must be 16-byte aligned"),
                    (dict(nbytes=64), "workspace too small")))

    def conv(x=0x100000, W=0x200000, bias=0x210000, resid=0x220000, B=2, S=8, N=1024, Cin=256, KW=9, transposed=0, act=0, y=0x300000, ws=0x500000,
             nbytes=1 << 40):
        return so.ns_fg_op_conv_bf16(P(x), P(W), P(bias), P(resid), B, S, N, Cin, KW, transposed, act, P(y), P(ws), nbytes, None)

    for t in (0, 1):
        expect_refusals(err, conv, tuple((dict(kw, transposed=t), msg) for kw, msg in (
            (dict(x=0), "null argument"), (dict(W=0), "null argument"), (dict(y=0), "null argument"), (dict(ws=0), "null argument"),
            (dict(B=0), "must be positive"), (dict(N=48), "N must be a positive multiple of 32"), (dict(Cin=-32), "Cin must be a positive multiple of 32"),
            (dict(KW=0), "KW must be odd and positive"), (dict(B=1 << 12, S=1 << 10), "problem too large"), (dict(act=2), "act must be 0 (none) or 1 (ReLU)"),
            (dict(y=0x100000), "y must not be x or resid"), (dict(y=0x220000), "y must not be x or resid"),
            (dict(x=0x100004), "x must be 16-byte aligned"), (dict(W=0x200008), "W must be 16-byte aligned"), (dict(bias=0x210004), "bias must be 16-byte aligned"),
            (dict(resid=0x220004), "resid must be 16-byte aligned"), (dict(y=0x300004), "y must be 16-byte aligned"),
            (dict(ws=0x500008), "the workspace must be 16-byte aligned"), (dict(nbytes=64), "workspace too small"))))


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("fgb_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("ffngrad_bf16.hip", kernels=("k_fg_pack_bf16", "k_fg_wgrad_bf16"))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_matmul_mode_keeps_the_state_dict_and_set_ffn_matmul_counts(lib):
    import smart_nar_fast_tts_amd as pkg
    from smart_nar_fast_tts_amd import sublayers

    assert pkg.set_ffn_matmul is sublayers.set_ffn_matmul
    a = sublayers.PositionwiseFeedForward(256, 1024, (9, 1), dropout=0.2)
    b = sublayers.PositionwiseFeedForward(256, 1024, (9, 1), dropout=0.2, matmul="bf16")
    assert a.matmul == "fp32" and b.matmul == "bf16"
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) and sorted(b.state_dict()) == sorted(sublayers.FFN_PARAM_NAMES)
    assert not list(b.named_buffers()) and [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    b.load_state_dict(a.state_dict())  # strict
    assert b.WORKSPACES is not a.WORKSPACES and b.WORKSPACES.query == "ns_fg_ws_bytes_bf16" and a.WORKSPACES.query == "ns_fg_ws_bytes"
    assert sublayers.PositionwiseFeedForward.WORKSPACES.query == "ns_fg_ws_bytes"  # the class default is untouched
    for bad in ("fp16", "BF16", "", None, 16):
        with pytest.raises(ValueError, match="matmul must be 'fp32' or 'bf16'"):
            sublayers.PositionwiseFeedForward(256, 1024, (9, 1), matmul=bad)
    stack = torch.nn.ModuleList([sublayers.FFTBlock(256, 2, 128, 128, 1024, (9, 1)) for _ in range(3)])
    keys = list(stack.state_dict().keys())
    assert sublayers.set_ffn_matmul(stack, "bf16") == 3 and all(blk.pos_ffn.matmul == "bf16" for blk in stack)
    assert sublayers.set_ffn_matmul(stack[1], "fp32") == 1 and [blk.pos_ffn.matmul for blk in stack] == ["bf16", "fp32", "bf16"]
    assert sublayers.set_ffn_matmul(stack[0].pos_ffn, "fp32") == 1 and sublayers.set_ffn_matmul(stack[0].slf_attn, "bf16") == 0
    assert list(stack.state_dict().keys()) == keys
    with pytest.raises(ValueError, match="mode must be 'fp32' or 'bf16'"):
        sublayers.set_ffn_matmul(stack, "tf32")
    assert [blk.pos_ffn.matmul for blk in stack] == ["fp32", "fp32", "bf16"]  # a refused mode switched nothing
    with pytest.raises(RuntimeError, match="no CPU path"):
        b(torch.zeros(2, 5, 256))
