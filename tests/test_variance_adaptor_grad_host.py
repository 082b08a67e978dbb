"""The yardstick of tests/test_gpu_variance_adaptor_grad.py proven on the CPU, the embedding gradient's plan, and every refusal of the
ns_va_* family (no GPU).

On the fixture (tests/golden/variance_adaptor_grad_tiny.npz: the reference's own VarianceAdaptor at d 32, filter 256, n_bins 8 in eval(),
teacher-forced, the four level mixes) the yardstick's autograd statement agrees with the reference's float64 run to <= 1e-10 relative
and its fp32 run is inside the gate; the written-out forward and backward agree with the float64 autograd to <= 1e-10; every mutant is
outside the gate of some tensor of some mix."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import variance_adaptor_grad_cpu as vc
from tests.util import assert_no_spill, built_lib, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return built_lib()


_FIX = {}


def _fixture(mix):
    """(meta, weights, inputs, the reference's float64 and fp32 tensors by FIXTURE_NAMES, the gates), once per mix"""
    if mix not in _FIX:
        meta, z = load_golden("variance_adaptor_grad_tiny")
        w = vc.synth_weights(meta["cfg"], meta["seeds"][0])
        ref64 = {k: z[f"{mix}_{k}_f64"] for k in vc.FIXTURE_NAMES}
        ref32 = {k: z[f"{mix}_{k}"] for k in vc.FIXTURE_NAMES}
        _FIX[mix] = (meta, z, w, vc.inputs_for(z, mix), ref64, ref32, vc.gate(ref32, ref64))
    return _FIX[mix]


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_the_fixture_holds_the_cases_it_must():
    meta, z, w, *_ = _fixture("pp")
    assert (meta["B"], meta["L"], meta["T"], meta["src_lens"]) == (3, 7, 12, [7, 4, 5]) and meta["cfg"] == vc.config(32, 256, 3, 8)
    assert not any(k.startswith("w_") or "weight" in k for k in z.files)  # no weights: both sides draw them from the seed
    d = z["duration"]
    assert d[0, 0] == 0 and (d[:, :4] == 0).any() and d.sum(1).tolist() == [14, 9, 6] and d.sum(1).max() > meta["T"] > d.sum(1).min()
    for s in ("pitch", "energy"):
        bins = w[f"{s}_bins"]
        for c in "pf":
            t = z[f"{s}_t_{c}"]
            assert (t < bins[0]).any() and (t > bins[-1]).any() and np.isin(t, bins).any(), (s, c)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "variance_adaptor_grad_tiny.npz")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "postnet_grad_tiny.npz"))


@pytest.mark.parametrize("mix", vc.MIXES)
def test_yardstick_reproduces_the_reference(mix):
    meta, z, w, inp, ref64, ref32, gates = _fixture(mix)
    r64 = vc.autograd_ref(inp, w, mix, torch.float64)
    r32 = vc.autograd_ref(inp, w, mix, torch.float32)
    for k in vc.FIXTURE_NAMES:
        want = ref64[k].reshape(r64[k].shape)  # (linear_layer.weight is [1, F] in the checkpoint)
        assert np.abs(r64[k] - want).max() <= 1e-10 * np.abs(want).max(), k
    assert np.array_equal(vc.masks(inp)[2], z[f"{mix}_mel_len"])
    sh = vc.shares(r32, ref64, gates)
    print(mix, "fp32 yardstick, worst share per class:", vc.classes(sh))
    assert max(sh.values()) <= 1.0, sh


@pytest.mark.parametrize("mix", vc.MIXES)
def test_written_out_forward_and_backward_equal_float64_autograd(mix):
    meta, z, w, inp, *_ = _fixture(mix)
    ref = vc.autograd_ref(inp, w, mix, torch.float64)
    got = vc.evaluate(inp, w, mix, torch.float64)
    for k in vc.NAMES:
        assert np.abs(got[k] - ref[k]).max() <= 1e-10 * np.abs(ref[k]).max(), k
    assert np.array_equal(got["mel_len"], z[f"{mix}_mel_len"])


def _mutant_share(mutant):
    worst = (0.0, None)
    for mix in vc.MIXES:
        meta, z, w, inp, ref64, ref32, gates = _fixture(mix)
        sh = vc.shares(vc.evaluate(inp, w, mix, torch.float64, mutate=mutant), ref64, gates)
        k = max(sh, key=sh.get)
        if sh[k] > worst[0]:
            worst = (sh[k], f"{mix}:{k}")
    return worst


@pytest.mark.parametrize("mutant", vc.MUTANTS)
def test_gate_rejects_mutant(mutant):
    """each mutant, evaluated in float64 (its only error is the mutation), is outside the gate of some tensor of some mix"""
    share, where = _mutant_share(mutant)
    print(f"{mutant}: share {share:.3g} at {where}")
    assert share > 1.0


def test_the_unmutated_forms_sit_far_inside_every_gate():
    for mix in vc.MIXES:
        meta, z, w, inp, ref64, ref32, gates = _fixture(mix)
        assert max(vc.shares(vc.evaluate(inp, w, mix, torch.float64), ref64, gates).values()) <= 1e-3


def test_gate_rules():
    ref64 = {"a": np.zeros(4), "b": np.array([1.0, -2.0])}
    ref32 = {"a": np.zeros(4, np.float32), "b": np.array([1.0, -2.0], np.float32) + np.float32(1e-6)}
    gates = vc.gate(ref32, ref64)
    assert 0 < gates["a"] < 1e-40  # an all-zero float64 tensor must be matched exactly
    assert vc.shares({"a": np.zeros(4), "b": ref64["b"]}, ref64, gates) == {"a": 0.0, "b": 0.0}
    assert vc.shares({"a": np.array([0, 0, 1e-30, 0]), "b": None}, ref64, gates)["a"] > 1.0
    assert vc.shares({"a": np.zeros(4), "b": np.array([np.nan, 0.0])}, ref64, gates)["b"] == float("inf")
    assert vc.classes({"dur.w1": 0.1, "dur.b2": 0.3, "y": 0.2}) == {"dur.*": 0.3, "y": 0.2}
    assert vc.order("pp") == ["pitch", "energy", "lr"] and vc.order("fp") == ["energy", "lr", "pitch"] and vc.order("ff") == ["lr", "pitch", "energy"]


def test_synth_weights_come_from_the_seed_alone():
    a, b = vc.synth_weights(vc.config(), 5), vc.synth_weights(vc.config(), 5)
    assert all(np.array_equal(a[k], b[k]) for k in ("pitch_emb", "energy_emb")) and np.array_equal(a["dur"]["w1"], b["dur"]["w1"])
    assert not np.array_equal(a["dur"]["w1"], a["pitch"]["w1"]) and not np.array_equal(a["pitch_emb"], vc.synth_weights(vc.config(), 6)["pitch_emb"])


# ---------------------------------------------------------------------------------------------------- the plan (no device work)
def test_plan_embed_sweep(lib):
    L_, so = lib
    assert so.ns_va_abi_version() == 1
    out = (C.c_int32 * 8)()
    for M in (1, 2, 74, 511, 512, 513, 650, 16160, 100000):
        for D in (4, 16, 36, 256, 260, 512):
            for n_bins in (2, 3, 8, 128, 129, 256, 257, 1024, 2048):
                assert so.ns_va_plan_embed(M, D, n_bins, out) == 0, (M, D, n_bins)
                blocks, rows, slab, n_slabs, lds, launches, threads, _ = out
                assert blocks >= 1 and launches == 2 and threads == 64 and slab in (4, 8, 16, 32, 64) and slab <= threads
                assert lds == n_bins * slab * 8 and lds <= 65536 and (slab == 64 or n_bins * slab * 2 * 8 > 65536)  # the widest slab that fits
                # every row in exactly one block, every column in exactly one slab
                assert (blocks - 1) * rows < M <= blocks * rows and (n_slabs - 1) * slab < D <= n_slabs * slab
                assert blocks == (M + 511) // 512  # a function of the shape alone
                assert so.ns_va_embed_ws_bytes(M, D, n_bins) == 8 * blocks * n_bins * D
    assert so.ns_va_plan_embed(650, 256, 256, out) == 0 and out[0] > 1
    assert so.ns_va_plan_embed(16160, 256, 256, out) == 0 and list(out)[:6] == [32, 512, 32, 8, 65536, 2]


def test_every_refusal_precedes_the_first_hip_call(lib):
    L_, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    a, big = 0x100000, 1 << 40
    out = (C.c_int32 * 8)()
    for args, msg in (((0, 256, 256), "M must be positive"), ((8, 254, 256), "D must be a positive multiple of 4"), ((8, 0, 256), "D must be a positive multiple of 4"),
                      ((8, 256, 1), "n_bins must be at least 2"), ((8, 256, 2049), "cannot hold this shape"), ((1 << 20, 1 << 11, 8), "M * D must stay below 2^31")):
        assert so.ns_va_plan_embed(*args, out) != 0 and msg in err() and list(out) == [0] * 8, (args, err())
        assert so.ns_va_embed_ws_bytes(*args) == 0 and msg in err()
        assert so.ns_va_op_embed_fwd(P(a), P(a), P(a), P(a), *args, P(a), P(a), None) != 0 and msg in err()
        assert so.ns_va_op_embed_bwd(P(a), P(a), *args, P(a), P(a), big, None) != 0 and msg in err()
    calls = (
        (lambda: so.ns_va_op_embed_fwd(None, P(a), P(a), P(a), 8, 256, 256, P(a), P(a), None), "null argument"),
        (lambda: so.ns_va_op_embed_fwd(P(a), P(a), P(a), P(a), 8, 256, 256, P(a), None, None), "null argument"),
        (lambda: so.ns_va_op_embed_fwd(P(a + 4), P(a), P(a), P(a), 8, 256, 256, P(a), P(a), None), "x must be 16-byte aligned"),
        (lambda: so.ns_va_op_embed_fwd(P(a), P(a + 2), P(a), P(a), 8, 256, 256, P(a), P(a), None), "target must be 4-byte aligned"),
        (lambda: so.ns_va_op_embed_fwd(P(a), P(a), P(a), P(a + 8), 8, 256, 256, P(a), P(a), None), "table must be 16-byte aligned"),
        (lambda: so.ns_va_op_embed_fwd(P(a), P(a), P(a), P(a), 8, 256, 256, P(a), P(a + 1), None), "idx must be 4-byte aligned"),
        (lambda: so.ns_va_op_embed_bwd(P(a), None, 8, 256, 256, P(a), P(a), big, None), "null argument"),
        (lambda: so.ns_va_op_embed_bwd(P(a), P(a), 8, 256, 256, P(a), None, big, None), "null argument"),
        (lambda: so.ns_va_op_embed_bwd(P(a + 8), P(a), 8, 256, 256, P(a), P(a), big, None), "g must be 16-byte aligned"),
        (lambda: so.ns_va_op_embed_bwd(P(a), P(a), 8, 256, 256, P(a), P(a + 8), big, None), "the workspace must be 16-byte aligned"),
        (lambda: so.ns_va_op_embed_bwd(P(a), P(a), 8, 256, 256, P(a), P(a), 8 * 256 * 256 - 1, None), "workspace too small"),
        (lambda: so.ns_va_op_embed_bwd(P(a), P(a), 650, 256, 256, P(a), P(a), 8 * 256 * 256, None), "workspace too small"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 2, 5, 256, 37, P(a), None, P(a), None), "null argument"),
        (lambda: so.ns_va_op_lr_fwd(P(a), None, 2, 5, 256, 37, None, P(a), P(a), None), "null argument"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 2, 5, 256, 37, P(a), P(a), None, None), "null argument"),
        (lambda: so.ns_va_op_lr_fwd(None, P(a), 2, 5, 256, 37, P(a), P(a), P(a), None), "null argument"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 0, 5, 256, 37, P(a), P(a), P(a), None), "B and L must be positive"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 2, 5, 256, 0, P(a), P(a), P(a), None), "T must be positive"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 2, 5, 250, 37, P(a), P(a), P(a), None), "D must be a positive multiple of 4"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 1 << 10, 1 << 10, 1 << 11, 37, P(a), P(a), P(a), None), "B * L * D must stay below 2^31"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 1 << 10, 5, 1 << 10, 1 << 11, P(a), P(a), P(a), None), "B * T * D must stay below 2^31"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a + 4), 2, 5, 256, 37, P(a), P(a), P(a), None), "duration must be 8-byte aligned"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 2, 5, 256, 37, P(a + 4), P(a), P(a), None), "out must be 16-byte aligned"),
        (lambda: so.ns_va_op_lr_fwd(P(a), P(a), 2, 5, 256, 37, P(a), P(a + 2), P(a), None), "cum must be 4-byte aligned"),
        (lambda: so.ns_va_op_lr_bwd(P(a), P(a), 2, 5, 256, 37, None, None), "null argument"),
        (lambda: so.ns_va_op_lr_bwd(P(a), P(a), 2, 5, 256, 0, P(a), None), "T must be positive"),
        (lambda: so.ns_va_op_lr_bwd(P(a), P(a), 2, 0, 256, 37, P(a), None), "B and L must be positive"),
        (lambda: so.ns_va_op_lr_bwd(P(a + 4), P(a), 2, 5, 256, 37, P(a), None), "g must be 16-byte aligned"),
        (lambda: so.ns_va_op_lr_bwd(P(a), P(a), 2, 5, 256, 37, P(a + 8), None), "d_x must be 16-byte aligned"),
    )
    for i, (call, msg) in enumerate(calls):
        assert call() != 0 and msg in err() and so.ns_va_last_launches() == 0, (i, err())


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("va_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("adaptorgrad.hip", kernels=("k_va_embed_fwd", "k_va_embed_bwd", "k_va_embed_finish", "k_va_duration_scan", "k_va_lr_bwd"))


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_module_has_the_reference_names_and_refuses_what_it_cannot_do(lib):
    import smart_nar_fast_tts_amd as pkg
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd import adaptor, predictor

    assert pkg.VarianceAdaptor is adaptor.VarianceAdaptor and pkg.VarianceEmbedding is adaptor.VarianceEmbedding
    assert pkg.LengthRegulator is adaptor.LengthRegulator and {"VarianceAdaptor", "VarianceEmbedding", "LengthRegulator"} <= set(pkg.__all__)
    mc = wl.model_config("tiny")
    m = adaptor.VarianceAdaptor(wl.preprocess_config("phoneme_level", "frame_level"), mc)
    keys = ["pitch_bins", "energy_bins", "pitch_embedding.weight", "energy_embedding.weight"] + [
        f"{p}_predictor.{k}" for p in ("duration", "pitch", "energy") for k in predictor.PARAM_NAMES]
    assert sorted(m.state_dict()) == sorted(keys)
    assert (m.pitch_feature_level, m.energy_feature_level) == ("phoneme_level", "frame_level")
    assert isinstance(m.pitch_bins, torch.nn.Parameter) and not m.pitch_bins.requires_grad and not m.energy_bins.requires_grad
    pb, eb = wl.variance_bins(mc)
    assert np.array_equal(m.pitch_bins.numpy(), pb) and np.array_equal(m.energy_bins.numpy(), eb)
    assert tuple(m.pitch_embedding.weight.shape) == (256, 256) and m.pitch_embedding.weight.requires_grad
    assert all(isinstance(getattr(m, f"{p}_predictor"), predictor.VariancePredictor) for p in ("duration", "pitch", "energy"))
    # a variance_adaptor.* slice of a checkpoint, reference-named, loads strictly
    full = wl.synth_state_dict(mc, seed=3)
    sd = {k[len("variance_adaptor."):]: torch.from_numpy(np.asarray(v)) for k, v in full.items() if k.startswith("variance_adaptor.")}
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    x = torch.zeros(2, 5, 256)
    with pytest.raises(NotImplementedError, match="FastSpeech2Align"):
        m(x, None)
    with pytest.raises(NotImplementedError, match="FastSpeech2Align"):
        m(x, None, None, None, torch.zeros(2, 5), torch.zeros(2, 9), None)
    with pytest.raises(NotImplementedError, match="controls"):
        m(x, None, None, 9, torch.zeros(2, 5), torch.zeros(2, 9), torch.ones(2, 5, dtype=torch.long), p_control=1.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, None, None, 9, torch.zeros(2, 5), torch.zeros(2, 9), torch.ones(2, 5, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU path"):
        adaptor.LengthRegulator()(x, torch.ones(2, 5, dtype=torch.long), 9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        adaptor.VarianceEmbedding(8, 256)(x, torch.zeros(2, 5), torch.zeros(7))
    with pytest.raises(ValueError, match="D must be a positive multiple of 4"):
        adaptor.VarianceEmbedding(8, 30)
    with pytest.raises(ValueError, match="n_bins must be at least 2"):
        adaptor.VarianceEmbedding(1, 32)
    with pytest.raises(ValueError, match="cannot hold this shape"):
        adaptor.VarianceEmbedding(4096, 32)
    with pytest.raises(ValueError, match="feature must be one of"):
        adaptor.VarianceAdaptor({"preprocessing": {"pitch": {"feature": "word_level"}, "energy": {"feature": "frame_level"}}}, mc)
