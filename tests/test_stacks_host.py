"""The yardstick of tests/test_gpu_stacks.py proven on the CPU, and every refusal of the ns_st_* family (no GPU).

On the fixture (tests/golden/stacks_tiny.npz, the reference's own TxtEncoder and MelDecoder at dropout 0) the float64 restatement
agrees with the reference's float64 autograd to <= 1e-12 relative, and the fp32 restatement stays inside the project gate
(tests/util.gate_value) taken from the fixture's own fp32 and float64 values.  (d_bk of an attention is zero in exact arithmetic — the
softmax does not see a key bias — so its bounds are taken from d_bq's, as tests/test_ffn_grad_host.py does.)

The table gradient's mutants.  The bound of the GPU test, 0.5 ulp32(|s|) + n_hits 2^-53 sum |g|, is the rounding of the exact sum plus
the error of n_hits float64 adds IN ANY ORDER, so ``descending_order`` cannot leave it: on every case but "order" it gives the very bits
of the ascending sum, and on "order" other bits that still lie inside the bound.  What catches it is the GPU test's second assertion,
bit-equality with ``stacks_cpu.embed_grad_ordered``, on "order"; this file proves both halves.  The other four mutants leave the bound
on the case CATCHER names, at every (D, n_vocab); BLIND lists the cases on which a mutant is the identity."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import stacks_cpu as sc
from tests.util import assert_no_spill, built_lib, expect_refusals, gate_value, load_golden, run_c_caller, share_of, weights_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return built_lib()


# ---------------------------------------------------------------------------------------------------- the stacks' yardstick
CASES = {  # case -> (encoder?, training, lens key, S key)
    "enc": (True, True, "lens", "S"), "enc_eval": (True, False, "lens", "S"), "dec": (False, True, "lens", "S"),
    "dec_eval": (False, False, "lens", "S"), "dec_trunc": (False, True, "lens_long", "S_long"), "dec_long_eval": (False, False, "lens_long", "S_long"),
}


@pytest.mark.parametrize("c", list(CASES))
def test_restatement_reproduces_the_reference(c):
    meta, z = load_golden("stacks_tiny")
    enc, training, lens_key, _ = CASES[c]
    w = sc.seeded_stack(meta["d"], meta["d_hid"], meta["kernel"], meta["n_layers"], meta["seeds"]["encoder" if enc else "decoder"],
                        n_vocab=meta["n_vocab"] if enc else None)
    inp, lens = z[f"{c}_in"], meta[lens_key]
    stored = sorted(k[len(c) + 3:] for k in z.files if k.startswith(f"{c}_d_") and not k.endswith("_f64"))
    got = {}
    for dtype in (torch.float32, torch.float64):
        if stored:
            got[dtype] = sc.autograd_ref(inp if enc else None, w, lens, meta["H"], z[f"{c}_g"], meta["max_seq_len"], training, dtype=dtype,
                                         x=None if enc else inp)
        else:
            with torch.no_grad():
                leaves = sc.leaves_of(w, dtype, None if enc else inp)
                got[dtype] = (sc.statement(inp if enc else None, leaves, lens, meta["H"], meta["max_seq_len"], training, dtype=dtype, encoder=enc)[0].numpy(), {})
    y32, y64 = got[torch.float32][0], got[torch.float64][0]
    assert y64.shape == z[f"{c}_y_f64"].shape
    pad = sc.pad_of([min(n, y64.shape[1]) for n in lens], y64.shape[1])
    assert not y64[pad].any() and not z[f"{c}_y"][pad].any()

    def check(key, a32, a64, gate_key=None, scale=None):
        want32, want64 = z[key], z[key + "_f64"]
        gate = gate_value(z[gate_key or key], z[(gate_key or key) + "_f64"])
        s32 = share_of(a32, want64, gate)[0]
        e64 = np.abs(a64 - want64).max()
        print(f"{key}: fp32 share of the gate {s32:.3g}, float64 {e64:.3g}")
        assert a32.shape == want32.shape and s32 <= 1.0, key
        assert e64 <= 1e-12 * (scale if scale is not None else np.abs(want64).max()), key

    check(f"{c}_y", y32, y64)
    if stored:
        scale = max(np.abs(z[f"{c}_d_{n}_f64"]).max() for n in stored)
        for n in stored:
            bk = n.endswith("_a_bk")  # zero up to rounding: bounds from d_bq, relative to the gradients' common scale
            check(f"{c}_d_{n}", got[torch.float32][1][n], got[torch.float64][1][n], f"{c}_d_{n[:-1]}q" if bk else None, scale if bk else None)
    if c == "enc":
        assert sorted(stored) == sorted(sc.grad_names(sc.leaves_of(w, torch.float32)))
        used = np.unique(inp[inp > 0])
        rest = np.setdiff1d(np.arange(meta["n_vocab"]), used)
        assert not z["enc_d_emb"][rest].any() and np.abs(z["enc_d_emb"][used]).min(axis=1).max() > 0
    if c == "dec_trunc":
        assert y64.shape[1] == meta["max_seq_len"] < inp.shape[1] and not got[torch.float64][1]["dx"][:, meta["max_seq_len"]:].any()
    if c == "dec_long_eval":
        assert y64.shape[1] == inp.shape[1] > meta["max_seq_len"]


def test_embed_grad64_is_the_backward_of_nn_embedding():
    for D, V in ((8, 5), (4, 361)):
        for case in ("M65", "ends", "one_id"):
            g, t = sc.embed_case(case, D, V)
            table = torch.zeros(V, D, dtype=torch.float64, requires_grad=True)
            torch.nn.functional.embedding(torch.from_numpy(t), table, padding_idx=0).backward(torch.from_numpy(g).double())
            want = table.grad.numpy()
            got = sc.embed_grad64(g, t, V)
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
            assert not got[0].any()


def test_mask_rows_is_masked_fill():
    rs = np.random.RandomState(0)
    x = rs.standard_normal((3, 7, 4)).astype(np.float32)
    pad = sc.pad_of([7, 0, 3], 7)
    x[pad] = np.nan
    want = torch.from_numpy(x).masked_fill(torch.from_numpy(pad).unsqueeze(-1), 0).numpy()
    assert np.array_equal(sc.mask_rows(x, pad).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the mutants of the table gradient
CATCHER = {"pad_row_summed": "ends", "last_of_group_dropped": "M64", "fp32_accumulation": "one_id", "oob_clamped": "oob", "descending_order": None}
BLIND = {  # the cases on which the mutation changes no bit, at every (D, n_vocab)
    "pad_row_summed": {"M1", "one_id", "order"},            # no PAD token among the rows
    "last_of_group_dropped": {"M1", "M63", "order"},        # no row 63 (mod 64), or a gradient row there that changes no bit of the sum
    "fp32_accumulation": {"M1", "order"},                   # one hit; sums that fp32 holds exactly
    "oob_clamped": {"M1", "M63", "M64", "M65", "M129", "one_id", "order", "ends"},   # no token outside [0, n_vocab)
    "descending_order": {"M1", "M63", "M64", "M65", "M129", "one_id", "ends", "oob", "nan"},  # <= 129 float64 adds, rounded to fp32: the same bits
}


def _outside(m, s, bound):
    with np.errstate(invalid="ignore"):
        return bool(np.any(~(np.abs(m.astype(np.float64) - s) <= bound)))  # (a NaN is outside)


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_bound_and_order_reject_the_mutants(mutant):
    identity = None
    for D, V in sc.EMBED_DIMS:
        same, caught = set(), set()
        for case in sc.EMBED_CASES:
            g, t = sc.embed_case(case, D, V)
            s, bound = sc.embed_grad64(g, t, V), sc.embed_grad_bound(g, t, V)
            good = sc.embed_grad_ordered(g, t, V)
            assert np.isfinite(s).all() and not _outside(good, s, bound), "the ascending float64 sum itself is inside the bound"
            m = sc.embed_grad_mutant(g, t, V, mutant)
            if np.array_equal(m.view(np.uint32), good.view(np.uint32)):
                same.add(case)
            elif _outside(m, s, bound):
                caught.add(case)
        print(f"{mutant} D {D} n_vocab {V}: identity on {sorted(same)}, outside the bound on {sorted(caught)}")
        identity = same if identity is None else identity & same
        if CATCHER[mutant] is None:
            # inside the bound everywhere (it holds for any order), yet other bits on "order": bit-equality with the ascending sum catches it
            assert not caught and "order" not in same
        else:
            assert CATCHER[mutant] in caught and CATCHER[mutant] not in BLIND[mutant]
    assert identity == BLIND[mutant], (sorted(identity), sorted(BLIND[mutant]))


def test_order_probe_tells_the_orders_apart():
    g, t = sc.embed_case("order", 256, 5)
    up, down = sc.embed_grad_ordered(g, t, 5), sc.embed_grad_mutant(g, t, 5, "descending_order")
    v = int(t[0])
    assert (up[v] == np.float32(1.0)).all() and (down[v] == np.float32(1.0) + np.float32(2.0 ** -23)).all()


# ---------------------------------------------------------------------------------------------------- versions and refusals (no device work)
def test_version(lib):
    L, so = lib
    assert so.ns_st_abi_version() == 1 and so.ns_st_last_launches() == 0
    header = open(os.path.join(ROOT, "include", "nar_fs2.h")).read()
    assert re.findall(r"^#define NS_ST_ABI_VERSION (\d+)\b", header, re.M) == ["1"]
    for name in ("ns_st_abi_version", "ns_st_last_launches", "ns_st_op_embed_pos", "ns_st_op_add_pos", "ns_st_op_embed_grad", "ns_st_op_row_mask"):
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\(", header), name


def test_every_refusal_precedes_the_first_hip_call(lib):
    L, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)

    def embed_pos(texts=0x1000000, emb=0x2000000, pos=0x3000000, B=2, S=8, D=256, V=361, out=0x4000000):
        return so.ns_st_op_embed_pos(P(texts), P(emb), P(pos), B, S, D, V, P(out), None)

    def add_pos(x=0x1000000, pos=0x3000000, B=2, S=8, D=256, out=0x4000000):
        return so.ns_st_op_add_pos(P(x), P(pos), B, S, D, P(out), None)

    def embed_grad(g=0x1000000, texts=0x2000000, M=16, D=256, V=361, d_table=0x4000000):
        return so.ns_st_op_embed_grad(P(g), P(texts), M, D, V, P(d_table), None)

    def row_mask(x=0x1000000, mask=0x2000001, lens=0, B=2, S=8, D=256, y=0x4000000):
        return so.ns_st_op_row_mask(P(x), P(mask), P(lens), B, S, D, P(y), None)

    shape = ((dict(B=0), "must be positive"), (dict(S=-2), "must be positive"), (dict(D=128), "D must be 256 or 512"), (dict(D=384), "D must be 256 or 512"),
             (dict(D=1024), "D must be 256 or 512"), (dict(B=1 << 11, S=1 << 12), "B * S * D must stay below 2^31"))
    vocab = ((dict(V=1), "n_vocab must be at least 2"), (dict(V=0), "n_vocab must be at least 2"), (dict(V=-5), "n_vocab must be at least 2"))
    expect_refusals(err, embed_pos, shape + vocab + (
        (dict(texts=0), "null argument"), (dict(emb=0), "null argument"), (dict(pos=0), "null argument"), (dict(out=0), "null argument"),
        (dict(texts=0x1000004), "texts must be 8-byte aligned"), (dict(emb=0x2000004), "emb must be 16-byte aligned"),
        (dict(pos=0x3000008), "pos must be 16-byte aligned"), (dict(out=0x400000c), "out must be 16-byte aligned")))
    expect_refusals(err, add_pos, shape + (
        (dict(x=0), "null argument"), (dict(pos=0), "null argument"), (dict(out=0), "null argument"), (dict(x=0x1000004), "x must be 16-byte aligned"),
        (dict(pos=0x3000008), "pos must be 16-byte aligned"), (dict(out=0x4000004), "out must be 16-byte aligned")))
    expect_refusals(err, embed_grad, vocab + (
        (dict(g=0), "null argument"), (dict(texts=0), "null argument"), (dict(d_table=0), "null argument"), (dict(M=0), "M must be positive"),
        (dict(M=-1), "M must be positive"), (dict(D=128), "D must be 256 or 512"), (dict(D=768), "D must be 256 or 512"),
        (dict(M=1 << 23), "must stay below 2^31"), (dict(M=1 << 22, D=512), "must stay below 2^31"), (dict(g=0x1000008), "g must be 16-byte aligned"),
        (dict(texts=0x2000004), "texts must be 8-byte aligned"), (dict(d_table=0x4000004), "d_table must be 16-byte aligned")))
    expect_refusals(err, row_mask, shape + (
        (dict(x=0), "null argument"), (dict(y=0), "null argument"), (dict(mask=0, lens=0), "neither mask nor lens given"),
        (dict(y=0x1000000), "out of place"), (dict(x=0x1000004), "x must be 16-byte aligned"), (dict(y=0x4000008), "y must be 16-byte aligned"),
        (dict(mask=0, lens=0x5000004), "lens must be 8-byte aligned")))
    assert so.ns_st_last_launches() == 0


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("st_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("stackgrad.hip", kernels=("k_st_embed_grad", "k_st_row_mask"))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_stacks_have_the_reference_names_and_no_cpu_path(lib):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import stacks

    assert pkg.TxtEncoder is stacks.TxtEncoder and pkg.MelDecoder is stacks.MelDecoder
    assert pkg.WordEmbedding is stacks.WordEmbedding and pkg.mask_rows is stacks.mask_rows
    meta, _ = load_golden("stacks_tiny")
    # the fixture's names, and its shapes with the fixture's widths (d 32, d_inner 64) replaced by ones the kernels are built for
    widths = {meta["d"]: 256, meta["d_hid"]: 512}
    t = dict(conv_filter_size=512, conv_kernel_size=meta["kernel"])
    for side in ("encoder", "decoder"):
        t.update({f"{side}_hidden": 256, f"{side}_head": meta["H"], f"{side}_layer": meta["n_layers"], f"{side}_dropout": 0.1})
    small = {"max_seq_len": meta["max_seq_len"], "transformer": t}
    for key, cls in (("txt_encoder", stacks.TxtEncoder), ("mel_decoder", stacks.MelDecoder)):
        m = cls(small)
        want = [(k, tuple(widths.get(n, n) for n in shape)) for k, shape in meta["state_dict"][key]]
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want, key
        assert [n for n, p in m.named_parameters() if not p.requires_grad] == ["position_enc"] and not list(m.named_buffers())
    # the checkpoint's slices load strictly, and position_enc holds the table's bits before and after
    cfg, sd = weights_for(dict(config="tiny", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25))
    for key, cls in (("txt_encoder", stacks.TxtEncoder), ("mel_decoder", stacks.MelDecoder)):
        m = cls(wl.model_config("tiny"))
        built = m.position_enc.detach().numpy().copy()
        assert built.tobytes() == np.asarray(sd[f"{key}.position_enc"]).tobytes()
        m.load_state_dict({k[len(key) + 1:]: torch.as_tensor(np.asarray(v)) for k, v in sd.items() if k.startswith(key + ".")})  # strict
        assert m.position_enc.detach().numpy().tobytes() == built.tobytes() and m.training
        if key == "txt_encoder":
            assert tuple(m.src_word_emb.weight.shape) == (wl.N_SYMBOLS + 1, 256)
            with pytest.raises(RuntimeError, match="no CPU path"):
                m(torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.bool))
        else:
            with pytest.raises(RuntimeError, match="no CPU path"):
                m(torch.zeros(2, 5, 256), torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        stacks.mask_rows(torch.zeros(2, 5, 256), mask=torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="d must be 256 or 512"):
        stacks.WordEmbedding(361, 128)
    with pytest.raises(ValueError, match="n_vocab must be at least 2"):
        stacks.WordEmbedding(1, 256)
    assert not stacks.WordEmbedding(5, 256).weight[0].any()
