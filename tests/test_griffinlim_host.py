"""CPU-only checks of the Griffin-Lim mel-to-wave path: the closed-form inverse basis and window_sumsquare against the reference's
stored values, the float64 restatement (tests/griffinlim_cpu.py) against the reference's stored fp32 outputs inside the derived
gates, the mutants, and the host side of the ns_gl_* C ABI and of audio.STFT / griffin_lim / mel_to_wave."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import griffinlim_cpu as gc  # noqa: E402
import melfront_cpu as mc  # noqa: E402
from smart_nar_fast_tts_amd import audio as A  # noqa: E402
from tests.util import built_lib  # noqa: E402

CONFIGS = {"tiny": gc.TINY, "ljspeech": gc.LJSPEECH}


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in CONFIGS:
        z = np.load(os.path.join(HERE, "golden", f"griffinlim_{name}.npz"))
        out[name] = (json.loads(str(z["meta"])), z)
    return out


@pytest.fixture(scope="module")
def refs(golden):
    """per config and fixture mel: float64 (mag, g_mag, {n_iters: (wave, gate)}), computed once"""
    out = {}
    for name, (meta, z) in golden.items():
        out[name] = []
        for i in range(meta["n_mels"]):
            mag, g_mag = gc.mel_to_mag(z[f"mel{i}"].T, z["mel_basis"])
            out[name].append((mag, g_mag, {n: gc.griffin_lim(mag, z[f"angles{i}"], n, CONFIGS[name]) for n in (0, 2)}))
    return out


@pytest.fixture(scope="module")
def lib():
    return built_lib()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_closed_form_inverse_basis_against_the_reference_buffer(golden, name):
    meta, z = golden[name]
    cfg = CONFIGS[name]
    assert meta["config"] == cfg
    fl, hop, win = gc.dims(cfg)
    ib = A.stft_inverse_basis(fl, hop, win)
    assert ib.shape == (fl + 2, 1, fl) and ib.dtype == np.float32
    assert meta["inverse_basis_max_diff"] <= 1e-16
    tol = max(meta["inverse_basis_max_diff"], 1e-30) * 1.0000001
    assert np.abs(ib[z["basis_rows"], 0, :].astype(np.float64) - z["inverse_basis_rows"]).max() <= tol
    assert abs(float(ib.astype(np.float64).sum()) - meta["inverse_basis_sum"]) <= tol * ib.size
    assert abs(float(np.abs(ib.astype(np.float64)).sum()) - meta["inverse_basis_abs_sum"]) <= tol * ib.size
    cut = fl // 2 + 1
    assert not ib[cut, 0].any() and not ib[cut + fl // 2, 0].any(), "the imaginary rows of bins 0 and N/2 are exactly zero"
    # it inverts the forward basis where the window allows: sum over hops of (forward . inverse) windows = identity is checked end to
    # end by the restatement below; here the un-windowed pair: inverse^T forward = I / scale
    four = np.fft.fft(np.eye(fl))
    F = np.vstack([four[:cut].real, four[:cut].imag])
    raw = A.stft_inverse_basis(fl, hop, fl)[:, 0, :].astype(np.float64) / np.maximum(A.hann_periodic(fl).astype(np.float32), 1e-30)
    assert np.abs((raw.T @ F)[1:, 1:] * (fl / hop) - np.eye(fl)[1:, 1:]).max() < 1e-4  # column 0 of the window is 0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_window_sumsquare_bit_for_bit(golden, name):
    meta, z = golden[name]
    fl, hop, win = gc.dims(CONFIGS[name])
    ws_ref = z["window_sum0"]
    T = (len(ws_ref) - fl) // hop + 1
    assert T == z["mag0"].shape[0]
    ws = A.window_sumsquare(T, hop, win, fl)
    assert ws.dtype == np.float32 and ws.tobytes() == ws_ref.tobytes()
    assert ws[0] == 0 and ws[fl // 2] > 0.5 * ws[len(ws) // 2] and ws[hop] < ws[len(ws) // 2], "the ends are partial sums"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_fp32_values_lie_inside_the_gates(golden, refs, name):
    meta, z = golden[name]
    for i, (mag, g_mag, waves) in enumerate(refs[name]):
        sh = {"mag": gc.share(z[f"mag{i}"], mag, g_mag)}
        for n, (y, g) in waves.items():
            # BLAS may order a float64 sum differently on another machine: the stored float64 values agree far inside the gate
            assert gc.share(z[f"wave{i}_it{n}_f64"], y, 1e-6 * g + 1e-300) <= 1.0, "the float64 restatement moved"
            sh[f"it{n}"] = gc.share(z[f"wave{i}_it{n}"], y, g)
        print(f"{name} mel {i}: reference fp32 shares of the gates {sh}")
        assert max(sh.values()) <= 1.0


def _mutant_share(name, mutant, z, refs, i=0):
    cfg = CONFIGS[name]
    mag, g_mag, waves = refs[name][i]
    ang = z[f"angles{i}"]
    if mutant in gc.MEL_MUTANTS:
        m, _ = gc.mel_to_mag(z[f"mel{i}"].T, z["mel_basis"], mutant)
        T = z[f"mel{i}"].shape[1]
        return gc.share(gc.pad_rows(m, T), gc.pad_rows(mag, T), gc.pad_rows(g_mag, T))
    if mutant in gc.INVERSE_MUTANTS:
        # the mel basis gives bins 0 and N/2 no weight, so the fixture's own magnitudes are zero there: the operator is fed
        # magnitudes with both bins raised to the mean level (the "dc_nyquist_2N" mutant is invisible otherwise)
        m = mag.copy()
        m[:, [0, -1]] = mag.mean()
        X, gX = gc.recombine(m, ang)
        y, _ = gc.inverse(X, gX, cfg, mutant)
        return gc.share(y, *gc.inverse(X, gX, cfg))
    if mutant in gc.STEP_MUTANTS:
        y0, g0 = waves[0]
        want, g = gc.step(y0, g0, mag, cfg)
        got, _ = gc.step(y0, g0, mag, cfg, mutant)
        return gc.share(got, want, g)
    if mutant in gc.REPHASE_MUTANTS:
        Y, _ = gc.spectrum(waves[0][0], None, cfg)
        Y = Y.copy()
        Y[1, :] = 0.0                      # an exactly silent frame
        Y[:, [5, Y.shape[1] // 2 + 5]] = 0.0  # bin 5 exactly zero in every frame
        want, g = gc.rephase(Y, None, mag)
        got, _ = gc.rephase(Y, None, mag, mutant)
        return gc.share(got, want, g)
    # a loop-wiring mutant: the two-iteration gate is the sum of everything before it and too loose to see it, so the loop is held
    # to what the GPU test holds it to — result k is one step of result k - 1, inside the gate of that ONE step on an exact input
    # (iterations 2 and 3: the stale mutant's first iteration repeats the start, so its second is still a true step of its first)
    y2, _ = gc.griffin_lim(mag, ang, 2, cfg, mutant, with_gate=False)
    y3, _ = gc.griffin_lim(mag, ang, 3, cfg, mutant, with_gate=False)
    return gc.share(y3, *gc.step(y2, None, mag, cfg))


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("mutant", gc.MUTANTS)
def test_every_mutant_leaves_its_gate(golden, refs, name, mutant):
    meta, z = golden[name]
    worst = _mutant_share(name, mutant, z, refs)
    print(f"{name} {mutant}: share {worst:.3g}")
    assert worst > 1.0, f"{mutant} stays inside the gate"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_spectral_convergence_allowance_separates_the_mutants(golden, refs, name):
    """the 60-iteration check compares spectral convergence; its allowance is 8 |SC_np32 - SC_64| from the fixture's meta.  Every loop
    mutant's SC shift is recorded here; the allowance must be at least ten times below the smallest of them."""
    meta, z = golden[name]
    cfg, sc = CONFIGS[name], meta["sc"]
    mag, _, _ = refs[name][0]
    allowance = 8 * abs(sc["sc_np32"] - sc["sc_f64"])
    assert abs(sc["sc_reference"] - sc["sc_f64"]) <= allowance, "the reference's own fp32 run sits inside the allowance"
    shifts = {}
    for mutant in gc.INVERSE_MUTANTS + gc.STEP_MUTANTS + gc.REPHASE_MUTANTS + gc.LOOP_MUTANTS:
        y, _ = gc.griffin_lim(mag, z["angles0"], sc["iters"], cfg, mutant, with_gate=False)
        shifts[mutant] = abs(gc.spectral_convergence(y, mag, cfg) - sc["sc_f64"])
    for mutant in ("scaling_1", "pinv_mel"):  # a wrong magnitude drives the loop; its result is held against the TRUE magnitude
        m, _ = gc.mel_to_mag(z["mel0"].T, z["mel_basis"], mutant)
        y, _ = gc.griffin_lim(m, z["angles0"], sc["iters"], cfg, with_gate=False)
        shifts[mutant] = abs(gc.spectral_convergence(y, mag, cfg) - sc["sc_f64"])
    # "last_frame_kept" has no SC shift to record: its wave is one hop longer, so |STFT(y)| and mag differ in shape; the GPU tests
    # hold wave_lens and the zero row at the dropped frame exactly
    print(f"{name}: allowance {allowance:.3g}, mutant SC shifts {({k: float(f'{v:.3g}') for k, v in shifts.items()})}")
    # an equivalent mutant inside the loop: no bin of any frame of the fixture's trajectory is exactly zero, so the rule for Y = 0 is
    # never consulted; the rephase operator's own test (crafted exact zeros) carries it
    assert shifts.pop("rephase_zero_at_zero") == 0.0
    # an equivalent mutant on magnitudes that come from a mel: the mel basis gives bins 0 and N/2 no weight, so their magnitudes are
    # exactly zero and their weight in the inverse basis multiplies zeros; the inverse operator's own test carries it
    assert not mag[:, [0, -1]].any() and shifts.pop("dc_nyquist_2N") == 0.0
    assert 10 * allowance <= min(shifts.values()), shifts


# ---- the host side of the C ABI -----------------------------------------------------------------------------------------------
def _create(so, **over):
    kw = dict(filter_length=1024, hop_length=256, win_length=1024, n_mel=80, scaling=1000.0)
    kw.update(over)
    h = C.c_void_p()
    rc = so.ns_gl_create(C.byref(A.gl_config_struct(kw["filter_length"], kw["hop_length"], kw["win_length"], kw["n_mel"], kw["scaling"])), C.byref(h))
    return rc, h


def test_create_refusals_and_sizes(lib):
    L, so = lib
    assert so.ns_gl_abi_version() == 1 and so.ns_mel_abi_version() == 1
    for over, msg in ((dict(filter_length=1000), "multiple of hop_length"), (dict(hop_length=80, filter_length=320), "multiple of 32"),
                      (dict(win_length=1025), "win_length"), (dict(n_mel=82), "multiple of 4"), (dict(filter_length=8192), "outside the range"),
                      (dict(scaling=0.0), "spec_from_mel_scaling")):
        rc, h = _create(so, **over)
        assert rc != 0 and msg in so.ns_last_error().decode(), (over, so.ns_last_error())
    rc, h = _create(so)
    assert rc == 0
    r256 = lambda n: (4 * n + 255) // 256 * 256  # noqa: E731
    assert so.ns_gl_arena_bytes(h) == 2 * r256(1024 * 1024) + r256(80 * 513) + r256(2 * 1024)
    prev_b = 0
    for B in (1, 2, 3, 16):
        prev_t = 0
        for T in (1, 2, 7, 24, 25, 1000):
            b = so.ns_gl_ws_bytes(h, B, T)
            assert b >= prev_t and b >= so.ns_gl_ws_bytes(h, max(B - 1, 1), T) and b >= 4 * B * T * (2 * 1024 + 513 + 256)
            prev_t = b
        assert prev_t >= prev_b
        prev_b = prev_t
    so.ns_gl_destroy(h)


def test_weight_keys_and_finalize_refusals(lib):
    L, so = lib
    rc, h = _create(so, filter_length=256, hop_length=32, win_length=192, n_mel=16)
    assert rc == 0

    def chk(name, shape):
        return so.ns_gl_check_weight(h, name.encode(), (C.c_int64 * len(shape))(*shape), len(shape))

    def setw(name, arr):
        return so.ns_gl_set_weight(h, name.encode(), C.c_void_p(arr.ctypes.data), (C.c_int64 * arr.ndim)(*arr.shape), arr.ndim)

    assert chk("stft_fn.forward_basis", (258, 1, 256)) == 0 and chk("stft_fn.inverse_basis", (258, 1, 256)) == 0 and chk("mel_basis", (16, 129)) == 0
    assert chk("stft_fn.inverse_basis", (258, 256)) != 0 and "rank mismatch" in so.ns_last_error().decode()
    assert chk("mel_basis", (16, 128)) != 0 and "size mismatch" in so.ns_last_error().decode()
    assert chk("window", (256,)) != 0 and "unexpected key" in so.ns_last_error().decode()
    assert so.ns_gl_finalize_weights(h, None) != 0 and "no arena" in so.ns_last_error().decode()
    # a host buffer stands in for the arena: finalize checks the keys before it touches the device
    arena = np.zeros(so.ns_gl_arena_bytes(h) + 256, np.uint8)
    base = (arena.ctypes.data + 255) & ~255
    assert so.ns_gl_bind_arena(h, C.c_void_p(base), so.ns_gl_arena_bytes(h)) == 0
    assert so.ns_gl_bind_arena(h, C.c_void_p(base + 4), so.ns_gl_arena_bytes(h)) != 0 and "aligned" in so.ns_last_error().decode()
    assert setw("stft_fn.forward_basis", A.stft_forward_basis(256, 192)) == 0
    assert so.ns_gl_finalize_weights(h, None) != 0
    err = so.ns_last_error().decode()
    assert "missing keys" in err and "stft_fn.inverse_basis" in err and "mel_basis" not in err, err
    bad = A.stft_inverse_basis(256, 32, 192).copy()
    bad[129, 0, 7] = 1e-3
    assert setw("stft_fn.inverse_basis", bad) == 0
    assert so.ns_gl_finalize_weights(h, None) != 0 and "not the inverse of a real DFT basis" in so.ns_last_error().decode()
    so.ns_gl_destroy(h)


def test_python_surface_without_a_gpu(lib):
    import torch

    st = A.STFT(256, 32, 192)
    assert list(st.state_dict()) == ["forward_basis", "inverse_basis"]
    assert tuple(st.forward_basis.shape) == tuple(st.inverse_basis.shape) == (258, 1, 256)
    assert np.array_equal(st.inverse_basis.numpy(), A.stft_inverse_basis(256, 32, 192))
    st.load_state_dict({"inverse_basis": np.zeros((258, 1, 256), np.float32)})
    assert not st.inverse_basis.numpy().any()
    with pytest.raises(RuntimeError, match="size mismatch"):
        st.load_state_dict({"inverse_basis": np.zeros((258, 1, 255), np.float32)})
    with pytest.raises(RuntimeError, match="unexpected key"):
        st.load_state_dict({"mel_basis": np.zeros((16, 129), np.float32)})
    with pytest.raises(ValueError, match="hann"):
        A.STFT(256, 32, 192, window="hamming")
    with pytest.raises(RuntimeError, match="multiple of 32"):
        A.STFT(320, 80, 320)
    taco = A.TacotronSTFT(256, 32, 192, 16, 16000, 0, 8000)
    assert set(taco.state_dict()) == {"stft_fn.forward_basis", "mel_basis"}
    fn = taco.stft_fn
    assert isinstance(fn, A.STFT) and fn is taco.stft_fn and (fn.filter_length, fn.hop_length, fn.win_length, fn.n_mel_channels) == (256, 32, 192, 16)
    assert set(taco.state_dict()) == {"stft_fn.forward_basis", "mel_basis"}
    assert np.array_equal(fn.forward_basis.numpy(), taco.forward_basis.numpy())
    # CPU tensors, wrong dtypes, wrong shapes, too-short host lengths
    mag, ph = torch.zeros(2, 129, 9), torch.zeros(2, 129, 9)
    with pytest.raises(RuntimeError, match="cuda"):
        st.inverse(mag, ph)
    with pytest.raises(RuntimeError, match="cuda"):
        st.transform(torch.zeros(1, 1000))
    with pytest.raises(ValueError, match="float32"):
        st.transform(torch.zeros(1, 1000, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        A.griffin_lim(mag.double(), st)
    with pytest.raises(RuntimeError, match="cuda"):
        A.griffin_lim(mag, st)
    with pytest.raises(RuntimeError, match="cuda"):
        A.mel_to_wave(torch.zeros(1, 16, 12), taco)
    with pytest.raises(ValueError, match="dimensions"):
        A.mel_to_wave(torch.zeros(16, 12), taco)
    dev = torch.device("cpu")
    assert A._as_long_lens([9, 6], 2, 9, dev, 256, 32, 0, "lens").tolist() == [9, 6]
    for lens, drop, msg in (([9, 5], 0, "too short"), ([9, 6], 1, "too short"), ([10, 9], 0, "exceeds"), ([9.0, 9.0], 0, "integers"), ([9], 0, "shape")):
        with pytest.raises(ValueError, match=msg):  # 32 * (5 - 1) = 128 = filter_length / 2 is refused, 32 * 5 is not
            A._as_long_lens(lens, 2, 9, dev, 256, 32, drop, "lens")
    import smart_nar_fast_tts_amd as pkg

    assert pkg.STFT is A.STFT and pkg.griffin_lim is A.griffin_lim and pkg.mel_to_wave is A.mel_to_wave and pkg.inv_mel_spec is A.inv_mel_spec
    # the start of the loop is the reference's draw
    np.random.seed(5)
    want = np.angle(np.exp(2j * np.pi * np.random.rand(1, 129, 4))).astype(np.float32)
    np.random.seed(5)
    assert np.array_equal(A.random_angles((1, 129, 4)), want)
