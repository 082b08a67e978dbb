"""The yardstick of tests/test_gpu_postnet_grad.py proven on the CPU, and every refusal of the ns_pn_* family (no GPU).

On the fixture (tests/golden/postnet_grad_tiny.npz, the reference's own PostNet(16, 32, 5, 3) in train() with recorded keep-masks at
p = 0.5, and in eval()) the yardstick's autograd statement agrees with the reference's float64 run to <= 1e-10 relative and its fp32 run
is inside the gate; the written-out forward and backward agree with the float64 autograd to <= 1e-10; every mutant is outside the gate.
(In train() every d_bias is zero in exact arithmetic — the batch mean removes the bias — so its fixture values are rounding noise; its
1e-10 is taken relative to the other gradients' scale, as tests/test_cross_attention_grad_host.py does for d_bk.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import postnet_grad_cpu as pc
from tests.util import assert_no_spill, built_lib, load_golden, run_c_caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return built_lib()


_FIX = {}


def _fixture(mode):
    """(meta, inputs, the reference's float64 and fp32 tensors by all_names, the gates), once per mode"""
    if mode not in _FIX:
        meta, z = load_golden("postnet_grad_tiny")
        n = meta["n"]
        w = {k[2:]: z[k] for k in z.files if k.startswith("w_")}
        train = mode == "train"
        keeps, p = ([z[f"keep{i}"] for i in range(n)], meta["p"]) if train else (None, 0.0)
        ref64 = {k: z[f"{mode}_d_{k}_f64"] for k in pc.grad_names(n)}
        ref32 = {k: z[f"{mode}_d_{k}"] for k in pc.grad_names(n)}
        ref64["y"], ref32["y"] = z[f"{mode}_y_f64"], z[f"{mode}_y"]
        for k in pc.buffer_names(n):  # eval() leaves the buffers as they were
            ref64[k] = z[f"train_{k}_f64"] if train else w[k].astype(np.float64)
            ref32[k] = z[f"train_{k}"] if train else w[k]
        _FIX[mode] = (meta, z, w, z["x"], z["g"], keeps, p, train, ref64, ref32, pc.gate(ref32, ref64))
    return _FIX[mode]


# ---------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_yardstick_reproduces_the_reference(mode):
    meta, z, w, x, g, keeps, p, train, ref64, ref32, gates = _fixture(mode)
    n = meta["n"]
    assert (meta["n_mel"], meta["emb"], meta["K"], n, meta["B"], meta["T"]) == (16, 32, 5, 3, 3, 7)
    assert all(0 < z[f"keep{i}"].mean() < 1 for i in range(n)) and g.all()
    r64, _ = pc.autograd_ref(x, w, g, keeps, p, train, torch.float64)
    r32, _ = pc.autograd_ref(x, w, g, keeps, p, train, torch.float32)
    scale = max(np.abs(ref64[k]).max() for k in pc.grad_names(n))
    for k in pc.all_names(n):
        assert r64[k].shape == ref64[k].shape, k
        noise = train and k[0] == "b" and k[1:].isdigit()
        assert np.abs(r64[k] - ref64[k]).max() <= 1e-10 * (scale if noise else np.abs(ref64[k]).max()), k
        if noise:
            assert np.abs(ref64[k]).max() <= 1e-12 * scale and np.abs(ref32[k]).max() <= 1e-5 * scale, k
    sh = pc.shares(r32, ref64, gates)
    print(mode, "fp32 yardstick, worst share per class:", pc.classes(sh))
    assert max(sh.values()) <= 1.0, sh
    if train:
        for i in range(n):
            assert int(z[f"train_nbt{i}"]) == int(z[f"train_nbt{i}_f64"]) == int(w[f"nbt{i}"]) + 1
            assert np.abs(ref64[f"rm{i}"] - w[f"rm{i}"]).max() > 1e-3 and np.abs(ref64[f"rv{i}"] - w[f"rv{i}"]).max() > 1e-3


@pytest.mark.parametrize("mode,p", [("train", 0.5), ("train", 0.0), ("eval", 0.0)])
def test_written_out_forward_and_backward_equal_float64_autograd(mode, p):
    meta, z, w, x, g, keeps, _, train, *_ = _fixture(mode)
    keeps = keeps if p > 0 else None
    ref, saved = pc.autograd_ref(x, w, g, keeps, p, train, torch.float64)
    got = pc.evaluate(x, w, g, keeps, p, train, torch.float64)
    n = meta["n"]
    scale = max(np.abs(ref[k]).max() for k in pc.grad_names(n))
    for k in pc.all_names(n):
        noise = train and k[0] == "b" and k[1:].isdigit()
        assert np.abs(got[k] - ref[k]).max() <= 1e-10 * (scale if noise else np.abs(ref[k]).max()), k
    _, sv = pc.forward_form(x, w, keeps, p, train, torch.float64)
    for i in range(n):
        assert np.abs(sv["u"][i].numpy() - saved["u"][i].numpy()).max() <= 1e-12
        assert np.abs(sv["h"][i].numpy() - saved["h"][i].numpy()).max() <= 1e-12


def _mutant_share(mutant):
    mode = "eval" if mutant == "eval_backward_with_batch_terms" else "train"
    meta, z, w, x, g, keeps, p, train, ref64, ref32, gates = _fixture(mode)
    bad = pc.evaluate(x, w, g, keeps, p, train, torch.float64, mutate=mutant, lens=meta["lens"])
    sh = pc.shares(bad, ref64, gates)
    worst = max(sh, key=sh.get)
    return sh[worst], worst


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_gate_rejects_mutant(mutant):
    """each mutant, evaluated in float64 (its only error is the mutation), is outside the gate of some tensor of the fixture"""
    share, where = _mutant_share(mutant)
    print(f"{mutant}: share {share:.3g} at {where}")
    assert share > 1.0


def test_the_smallest_mutant_share_is_at_least_10():
    """the condition the fixture's seeds were chosen for (tests/golden/make_golden_postnet_grad.py); the unmutated float64 forms sit
    far inside every gate"""
    got = {m: _mutant_share(m)[0] for m in pc.MUTANTS}
    smallest = min(got, key=got.get)
    print(f"smallest mutant share: {got[smallest]:.3g} ({smallest})")
    assert got[smallest] >= 10.0, got
    for mode in ("train", "eval"):
        meta, z, w, x, g, keeps, p, train, ref64, ref32, gates = _fixture(mode)
        assert max(pc.shares(pc.evaluate(x, w, g, keeps, p, train, torch.float64), ref64, gates).values()) <= 1e-3


def test_gate_rules():
    ref64 = {"a": np.zeros(4), "b": np.array([1.0, -2.0])}
    ref32 = {"a": np.zeros(4, np.float32), "b": np.array([1.0, -2.0], np.float32) + np.float32(1e-6)}
    gates = pc.gate(ref32, ref64)
    assert 0 < gates["a"] < 1e-40  # an all-zero float64 tensor must be matched exactly
    assert pc.shares({"a": np.zeros(4), "b": ref64["b"]}, ref64, gates) == {"a": 0.0, "b": 0.0}
    assert pc.shares({"a": np.array([0, 0, 1e-30, 0]), "b": None}, ref64, gates)["a"] > 1.0
    assert pc.shares({"a": np.zeros(4), "b": np.array([np.nan, 0.0])}, ref64, gates)["b"] == float("inf")
    assert pc.classes({"w0": 0.1, "w2": 0.3, "g1": 0.2, "rm0": 0.4, "dx": 0.5, "y": 0.6}) == {"w": 0.3, "gamma": 0.2, "running_mean": 0.4, "dx": 0.5, "y": 0.6}


# ---------------------------------------------------------------------------------------------------- sizes and refusals (no device work)
def _align(n):
    return (n + 255) & ~255


def test_sizes(lib):
    L_, so = lib
    assert so.ns_pn_abi_version() == 1
    for B, T, n_mel, emb, K, n in ((2, 37, 80, 512, 5, 3), (5, 130, 80, 512, 5, 5), (5, 130, 16, 256, 5, 3), (16, 1010, 80, 512, 5, 5), (2, 1, 80, 512, 5, 2)):
        s = L_.NsPnShape(B, T, n_mel, emb, K, n)
        M = B * T
        assert so.ns_pn_saved_bytes(C.byref(s)) == 4 * M * (2 * (n - 1) * emb + n_mel) + 16 * n * emb
        chans = [n_mel] + [emb] * (n - 1) + [n_mel]
        plan, pmax = (C.c_int32 * 8)(), 0
        for i in range(n):
            assert so.ns_pg_plan_wgrad(M, 128 if i == n - 1 else emb, chans[i], K, plan) == 0
            pmax = max(pmax, plan[5])
        nblk = (M + 31) // 32
        want = (2 * sum(_align(4 * chans[i + 1] * K * chans[i]) for i in range(n)) + _align(4 * pmax) + _align(4 * 128 * emb * K)
                + _align(8 * nblk * 2 * emb) + sum(_align(8 * nblk * chans[i + 1]) for i in range(n)) + _align(16 * emb) + _align(16 * n * emb)
                + 2 * _align(4 * M * emb))
        assert so.ns_pn_ws_bytes(C.byref(s)) == want


def test_every_refusal_precedes_the_first_hip_call(lib):
    L_, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731  (made-up device addresses: never dereferenced)
    ok_shape = dict(B=2, T=8, n_mel=80, emb=512, K=5, n=3)

    def weights(**over):
        w, names = L_.NsPnWeights(), L_.PN_PARAMS + L_.PN_BUFFERS  # over: gamma1 = layer[1].gamma
        for i in range(len(w.layer)):
            for j, name in enumerate(names):
                setattr(w.layer[i], name, over.get(f"{name}{i}", 0x100000 + 0x10000 * (i * len(names) + j)))
        return w

    def keeps(*addr):
        return (C.c_void_p * 5)(*addr)

    def fwd(shape=None, w=None, training=1, x=0x9000000, keep=None, p=0.0, y=0xA000000, saved=0xB000000, ws=0xC000000, nbytes=1 << 40):
        s = L_.NsPnShape(**dict(ok_shape, **(shape or {})))
        return so.ns_pn_forward(C.byref(s), C.byref(w or weights()), training, P(x), keep, p, P(y), P(saved), P(ws), nbytes, None)

    def bwd(shape=None, w=None, training=1, x=0x9000000, keep=None, p=0.0, saved=0xB000000, g=0xD000000, grads=None, ws=0xC000000, nbytes=1 << 40):
        s = L_.NsPnShape(**dict(ok_shape, **(shape or {})))
        d = grads or L_.NsPnGrads()
        return so.ns_pn_backward(C.byref(s), C.byref(w or weights()), training, P(x), keep, p, P(saved), P(g), C.byref(d), P(ws), nbytes, None)

    three = keeps(0xE000000, 0xE100000, 0xE200000)
    for call in (fwd, bwd):
        for kw, msg in ((dict(x=0), "null argument"), (dict(ws=0), "null argument"), (dict(x=0x9000004), "16-byte aligned"), (dict(ws=0xC000008), "16-byte aligned"),
                        (dict(saved=0xB000004), "16-byte aligned"),
                        (dict(shape=dict(emb=128)), "emb must be 256 or 512"), (dict(shape=dict(emb=384)), "emb must be 256 or 512"),
                        (dict(shape=dict(n_mel=72)), "n_mel must be a multiple of 16 in [16, 128]"), (dict(shape=dict(n_mel=0)), "n_mel must be a multiple of 16"),
                        (dict(shape=dict(n_mel=144)), "n_mel must be a multiple of 16 in [16, 128]"),
                        (dict(shape=dict(K=4)), "K must be odd and at most 9"), (dict(shape=dict(K=11)), "K must be odd and at most 9"),
                        (dict(shape=dict(K=0)), "K must be odd and at most 9"),
                        (dict(shape=dict(n=1)), "n must lie in [2, 5]"), (dict(shape=dict(n=6)), "n must lie in [2, 5]"),
                        (dict(shape=dict(B=0)), "must be positive"), (dict(shape=dict(T=-1)), "must be positive"),
                        (dict(shape=dict(B=1 << 11, T=1 << 11)), "B * T * emb must stay below 2^31"),
                        (dict(shape=dict(B=1, T=1)), "training needs more than one row"),
                        (dict(p=1.0), "p_drop must lie in [0, 1)"), (dict(p=-0.1), "p_drop must lie in [0, 1)"), (dict(p=float("nan")), "p_drop must lie in [0, 1)"),
                        (dict(p=0.5), "needs all n keep-masks"), (dict(p=0.5, keep=keeps(0xE000000, 0xE100000, 0)), "needs all n keep-masks"),
                        (dict(keep=three), "although p_drop == 0"), (dict(keep=keeps(0, 0xE100000, 0)), "although p_drop == 0"),
                        (dict(p=0.5, keep=keeps(0xE000000, 0xE100004, 0xE200000)), "keep-masks must be 16-byte aligned"),
                        (dict(w=weights(gamma1=0)), "null weights->layer[1].gamma"), (dict(w=weights(running_var2=0)), "null weights->layer[2].running_var"),
                        (dict(w=weights(w0=0x100004)), "weights->layer[0].w must be 16-byte aligned"),
                        (dict(w=weights(num_batches_tracked0=0x100004)), "weights->layer[0].num_batches_tracked must be 8-byte aligned"),
                        (dict(nbytes=1024), "workspace too small")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
    # layers past n are ignored; M == 1 is legal in eval
    assert fwd(w=weights(w3=0, gamma4=0, running_mean3=4), nbytes=64) != 0 and "workspace too small" in err()
    assert fwd(shape=dict(B=1, T=1), training=0, nbytes=64) != 0 and "workspace too small" in err()
    assert fwd(saved=0, nbytes=64) != 0 and "workspace too small" in err()  # saved is nullable
    assert fwd(y=0) != 0 and "null argument" in err()
    assert fwd(y=0xA000004) != 0 and "16-byte aligned" in err()
    assert bwd(saved=0) != 0 and "null argument" in err()
    assert bwd(g=0) != 0 and "null argument" in err()
    assert bwd(g=0xD000004) != 0 and "16-byte aligned" in err()
    d = L_.NsPnGrads()
    d.layer[1].gamma = 0x1000004
    assert bwd(grads=d) != 0 and "every gradient must be 16-byte aligned" in err()
    assert bwd() == 0 and so.ns_pn_last_launches() == 0  # nothing wanted: nothing launched, no HIP call
    assert bwd(p=0.5, keep=three) == 0 and so.ns_pn_last_launches() == 0

    assert so.ns_pn_ws_bytes(None) == 0 and "null argument" in err()
    s = L_.NsPnShape(2, 8, 80, 300, 5, 3)
    assert so.ns_pn_ws_bytes(C.byref(s)) == 0 and "emb must be 256 or 512" in err()
    assert so.ns_pn_saved_bytes(C.byref(s)) == 0 and "emb must be 256 or 512" in err()


def test_the_single_kernel_entries_refuse_before_any_hip_call(lib):
    L_, so = lib
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    P = lambda a: C.c_void_p(a) if a else None  # noqa: E731
    a, big = 0x100000, 1 << 30
    calls = (
        (lambda: so.ns_pn_op_stats(P(a), 8, 80, 1, None, None, None, None, P(a), big, None), "null argument"),
        (lambda: so.ns_pn_op_stats(None, 8, 80, 1, None, None, None, P(a), P(a), big, None), "null argument"),
        (lambda: so.ns_pn_op_stats(None, 8, 80, 0, None, None, None, P(a), None, 0, None), "null argument"),
        (lambda: so.ns_pn_op_stats(P(a), 8, 80, 1, P(a), None, None, P(a), P(a), big, None), "the three buffers come together"),
        (lambda: so.ns_pn_op_stats(P(a), 8, 72, 1, None, None, None, P(a), P(a), big, None), "C must be a multiple of 16 up to 512"),
        (lambda: so.ns_pn_op_stats(P(a), 8, 528, 1, None, None, None, P(a), P(a), big, None), "C must be a multiple of 16 up to 512"),
        (lambda: so.ns_pn_op_stats(P(a), 0, 80, 1, None, None, None, P(a), P(a), big, None), "M must be positive"),
        (lambda: so.ns_pn_op_stats(P(a), 1, 80, 1, None, None, None, P(a), P(a), big, None), "training needs more than one row"),
        (lambda: so.ns_pn_op_stats(P(a + 4), 8, 80, 1, None, None, None, P(a), P(a), big, None), "16-byte aligned"),
        (lambda: so.ns_pn_op_stats(P(a), 8, 80, 1, P(a), P(a), P(a + 4), P(a), P(a), big, None), "num_batches_tracked must be 8-byte aligned"),
        (lambda: so.ns_pn_op_stats(P(a), 8, 80, 1, None, None, None, P(a), P(a), 16, None), "workspace too small"),
        (lambda: so.ns_pn_op_apply(P(a), P(a), P(a), None, None, 0.0, 0, 8, 80, P(a), None), "null argument"),
        (lambda: so.ns_pn_op_apply(P(a), P(a), P(a), P(a), None, 0.5, 0, 8, 80, P(a), None), "needs a keep-mask"),
        (lambda: so.ns_pn_op_apply(P(a), P(a), P(a), P(a), P(a), 0.0, 0, 8, 80, P(a), None), "although p_drop == 0"),
        (lambda: so.ns_pn_op_apply(P(a), P(a), P(a), P(a), None, 0.0, 0, 8, 80, P(a + 8), None), "16-byte aligned"),
        (lambda: so.ns_pn_op_bwd_reduce(P(a), P(a), None, P(a), None, 0.0, 0, 8, 80, P(a), P(a), P(a), P(a), big, None), "null argument"),
        (lambda: so.ns_pn_op_bwd_reduce(P(a), P(a), None, P(a), None, 0.0, 1, 8, 80, P(a), P(a), P(a), P(a), 16, None), "workspace too small"),
        (lambda: so.ns_pn_op_bwd_reduce(P(a), P(a), P(a), P(a), None, 0.0, 0, 8, 40, P(a), P(a), P(a), P(a), big, None), "C must be a multiple of 16"),
        (lambda: so.ns_pn_op_bwd_apply(P(a), P(a), P(a), P(a), P(a), None, None, 0.0, 0, 8, 80, 80, P(a), None, None, 0, None), "null argument"),
        (lambda: so.ns_pn_op_bwd_apply(P(a), P(a), P(a), P(a), P(a), P(a), None, 0.0, 0, 8, 80, 96, P(a), None, None, 0, None), "ldz must be C, or 128"),
        (lambda: so.ns_pn_op_bwd_apply(P(a), P(a), P(a), P(a), P(a), P(a), None, 0.0, 0, 8, 256, 128, P(a), None, None, 0, None), "ldz must be C, or 128"),
        (lambda: so.ns_pn_op_bwd_apply(P(a), P(a), P(a), P(a), P(a), P(a), None, 0.0, 0, 8, 80, 128, P(a), P(a), P(a), 16, None), "workspace too small"),
        (lambda: so.ns_pn_op_wgrad_narrow(P(a), P(a), 2, 8, 80, 512, 5, None, P(a), big, None), "null argument"),
        (lambda: so.ns_pn_op_wgrad_narrow(P(a), P(a), 2, 8, 128, 512, 5, P(a), P(a), big, None), "N must be a multiple of 16 below 128"),
        (lambda: so.ns_pn_op_wgrad_narrow(P(a), P(a), 2, 8, 80, 510, 5, P(a), P(a), big, None), "Cin must be a multiple of 4"),
        (lambda: so.ns_pn_op_wgrad_narrow(P(a), P(a), 2, 8, 80, 512, 4, P(a), P(a), big, None), "K must be odd"),
        (lambda: so.ns_pn_op_wgrad_narrow(P(a), P(a), 2, 8, 80, 512, 5, P(a), P(a), 1024, None), "workspace too small"),
    )
    for i, (call, msg) in enumerate(calls):
        assert call() != 0 and msg in err(), (i, err())


def test_header_is_plain_c_and_validation_works_from_c(lib, tmp_path):
    run_c_caller("pn_host_only", lib[0].LIB_PATH, tmp_path)


def test_the_new_kernels_do_not_spill():
    assert_no_spill("postnetgrad.hip", kernels=("k_pn_stats", "k_pn_finish", "k_pn_apply", "k_pn_bwd_reduce", "k_pn_bwd_apply", "k_pn_bias_finish", "k_pn_copy"))


# ---------------------------------------------------------------------------------------------------- the Python surface
REF_KEYS = [f"convolutions.{i}.{s}" for i in range(5)
            for s in ("0.conv.weight", "0.conv.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var", "1.num_batches_tracked")]


def test_module_has_the_reference_names_and_refuses_what_it_cannot_do(lib):
    import smart_nar_fast_tts_amd as pkg
    from smart_nar_fast_tts_amd import postnet

    assert pkg.PostNet is postnet.PostNet and "PostNet" in pkg.__all__
    m = postnet.PostNet()
    assert (m.n_mel, m.emb, m.kernel, m.n, m.dropout) == (80, 512, 5, 5, 0.5) and m.training
    assert sorted(m.state_dict()) == sorted(REF_KEYS)
    assert list(m.PARAM_NAMES) == [k for k in REF_KEYS if "running" not in k and "tracked" not in k]
    assert [tuple(p.shape) for p in m.ordered_parameters()][:8] == [(512, 80, 5), (512,), (512,), (512,), (512, 512, 5), (512,), (512,), (512,)]
    assert tuple(m.convolutions[4][0].conv.weight.shape) == (80, 512, 5) and tuple(m.convolutions[4][1].running_var.shape) == (80,)
    # a postnet.* slice of a checkpoint, reference-named, loads strictly; what is saved afterwards carries the same keys and values
    rs = np.random.RandomState(0)
    sd = {}
    for k, v in m.state_dict().items():
        sd["postnet." + k] = torch.tensor(7) if k.endswith("tracked") else torch.from_numpy(rs.standard_normal(tuple(v.shape)).astype(np.float32))
    sd["mel_linear.weight"] = torch.zeros(80, 256)
    res = m.load_state_dict({k[len("postnet."):]: v for k, v in sd.items() if k.startswith("postnet.")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = m.state_dict()
    assert all(torch.equal(out[k[len("postnet."):]], v) for k, v in sd.items() if k.startswith("postnet."))
    assert out["convolutions.2.1.num_batches_tracked"].dtype == torch.int64
    small = postnet.PostNet(16, 256, 3, 2, dropout=0.0)
    assert sorted(small.state_dict()) == sorted(k for k in REF_KEYS if int(k.split(".")[1]) < 2) and small.dropout == 0.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 5, 80))
    with pytest.raises(ValueError, match="postnet_embedding_dim must be 256 or 512"):
        postnet.PostNet(80, 384)
    with pytest.raises(ValueError, match=r"n_mel_channels must be a multiple of 16 in \[16, 128\]"):
        postnet.PostNet(72)
    with pytest.raises(ValueError, match=r"n_mel_channels must be a multiple of 16 in \[16, 128\]"):
        postnet.PostNet(144)
    with pytest.raises(ValueError, match="postnet_kernel_size must be odd and at most 9"):
        postnet.PostNet(80, 512, 4)
    with pytest.raises(ValueError, match="postnet_kernel_size must be odd and at most 9"):
        postnet.PostNet(80, 512, 11)
    with pytest.raises(ValueError, match=r"postnet_n_convolutions must lie in \[2, 5\]"):
        postnet.PostNet(80, 512, 5, 1)
    with pytest.raises(ValueError, match=r"postnet_n_convolutions must lie in \[2, 5\]"):
        postnet.PostNet(80, 512, 5, 6)
    with pytest.raises(ValueError, match=r"dropout must lie in \[0, 1\)"):
        postnet.PostNet(dropout=1.0)
