"""CPU-only checks of the wave-to-mel front end: the two bases, the stored reference values against the derived gates
(tests/melfront_cpu.py), the hop-row and band-form identities, the mutants, and the host side of the ns_mel_* C ABI."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import melfront_cpu as mc  # noqa: E402
from smart_nar_fast_tts_amd import audio as A  # noqa: E402
from tests.util import built_lib  # noqa: E402

CONFIGS = {"tiny": mc.TINY, "ljspeech": mc.LJSPEECH}


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in CONFIGS:
        z = np.load(os.path.join(HERE, "golden", f"melfront_{name}.npz"))
        out[name] = (json.loads(str(z["meta"])), z)
    return out


@pytest.fixture(scope="module")
def refs(golden):
    """reference64 of every fixture wave, computed once"""
    return {name: [mc.reference64(z[f"wave{i}"], CONFIGS[name]) for i in range(meta["n_waves"])] for name, (meta, z) in golden.items()}


@pytest.fixture(scope="module")
def lib():
    return built_lib()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_basis_equals_the_reference_buffer(golden, name):
    meta, z = golden[name]
    cfg = CONFIGS[name]
    assert meta["config"] == cfg
    fb = A.stft_forward_basis(cfg["filter_length"], cfg["win_length"])
    assert fb.shape == (cfg["filter_length"] + 2, 1, cfg["filter_length"]) and fb.dtype == np.float32
    rows = z["basis_rows"]
    assert np.array_equal(fb[rows, 0, :].view(np.uint32), z["forward_basis_rows"].view(np.uint32))
    assert float(fb.astype(np.float64).sum()) == meta["forward_basis_sum"]
    assert float(np.abs(fb.astype(np.float64)).sum()) == meta["forward_basis_abs_sum"]
    cut = cfg["filter_length"] // 2 + 1
    assert not fb[cut, 0].any() and np.abs(fb[cut + cfg["filter_length"] // 2, 0]).max() <= 1e-6
    assert np.array_equal(A.slaney_mel_basis(cfg["sampling_rate"], cfg["filter_length"], cfg["n_mel_channels"], cfg["mel_fmin"], cfg["mel_fmax"]), z["mel_basis"])


@pytest.mark.parametrize("win", [192, 1024, 7])
def test_hann_window_equals_scipy(win):
    from scipy.signal import get_window

    assert np.array_equal(A.hann_periodic(win).astype(np.float32), get_window("hann", win, fftbins=True).astype(np.float32))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_slaney_bank_properties(name):
    cfg = CONFIGS[name]
    fl, n_mel, sr = cfg["filter_length"], cfg["n_mel_channels"], cfg["sampling_rate"]
    mb = A.slaney_mel_basis(sr, fl, n_mel, cfg["mel_fmin"], cfg["mel_fmax"]).astype(np.float64)
    edges = A.mel_band_edges(n_mel, cfg["mel_fmin"], cfg["mel_fmax"])
    freqs = np.linspace(0, sr / 2, fl // 2 + 1)
    assert mb.shape == (n_mel, fl // 2 + 1) and (mb >= 0).all()
    assert (np.diff(edges) > 0).all() and edges[0] == cfg["mel_fmin"] and abs(edges[-1] - cfg["mel_fmax"]) < 1e-9
    centres = []
    for m in range(n_mel):
        nz = np.nonzero(mb[m])[0]
        if len(nz) == 0:
            continue  # a filter narrower than the bin spacing (low bands of a short transform)
        assert (np.diff(nz) == 1).all(), "one contiguous band"
        assert freqs[nz[0]] > edges[m] and freqs[nz[-1]] < edges[m + 2], "inside its own edges"
        peak = int(np.argmax(mb[m]))
        assert (np.diff(mb[m, nz[0]:peak + 1]) >= 0).all() and (np.diff(mb[m, peak:nz[-1] + 1]) <= 0).all(), "a triangle"
        centres.append(freqs[peak])
        # area normalisation: height 2 / (f_{m+2} - f_m) at the centre, i.e. sampled triangle values x (f_{m+2} - f_m) / 2 <= 1
        tri = mb[m] * (edges[m + 2] - edges[m]) / 2.0
        assert tri.max() <= 1.0 + 1e-6
        k = nz[len(nz) // 2]
        want = min((freqs[k] - edges[m]) / (edges[m + 1] - edges[m]), (edges[m + 2] - freqs[k]) / (edges[m + 2] - edges[m + 1]))
        assert abs(tri[k] - want) < 1e-6
    assert (np.diff(centres) >= 0).all(), "bands rise in frequency"
    assert ((mb > 0).sum(0) <= 2).all(), "each bin touches at most two filters"
    # Slaney's scale: linear below 1 kHz, 27 log steps per factor 6.4 above
    assert abs(float(A.hz_to_mel(1000.0)) - 15.0) < 1e-12 and abs(float(A.hz_to_mel(6400.0)) - 42.0) < 1e-9
    assert np.allclose(A.mel_to_hz(A.hz_to_mel(np.array([0.0, 440.0, 1000.0, 7999.0]))), [0.0, 440.0, 1000.0, 7999.0], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_fp32_values_lie_inside_the_gates(golden, refs, name):
    meta, z = golden[name]
    for i, r in enumerate(refs[name]):
        assert np.array_equal(r[0], z[f"mel{i}_f64"]) and np.array_equal(r[1], z[f"energy{i}_f64"]), "the float64 restatement moved"
        sh = mc.shares(z[f"mel{i}"], z[f"energy{i}"], r)
        print(f"{name} wave {i}: reference fp32 shares of the gates {sh}")
        assert sh["mel"] <= 1.0 and sh["energy"] <= 1.0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hop_row_route_equals_framed_route(golden, name):
    meta, z = golden[name]
    cfg = CONFIGS[name]
    for n in (cfg["filter_length"] // 2 + 1, 700 if name == "ljspeech" else 300, None):
        w = z["wave0"] if n is None else z["wave0"][:n]
        y, Aabs = mc.spectrum64(w, cfg)
        y2 = mc.spectrum64_hop_rows(w, cfg)
        assert y.shape == y2.shape == (len(w) // cfg["hop_length"] + 1, cfg["filter_length"] + 2)
        assert np.abs(y - y2).max() <= 1e-12 * max(1.0, Aabs.max())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_band_form_equals_dense_product(golden, name):
    meta, z = golden[name]
    cfg = CONFIGS[name]
    mb = z["mel_basis"]
    y, _ = mc.spectrum64(z["wave1"], cfg)
    cut = y.shape[1] // 2
    mag = np.sqrt(y[:, :cut] ** 2 + y[:, cut:] ** 2)
    bands = mc.band_form(mb)
    assert sum(len(w) for _, w in bands) < mb.size // 8
    for m, (k0, w) in enumerate(bands):
        acc_b = np.zeros(len(mag))
        for i in range(len(w)):
            acc_b = acc_b + float(w[i]) * mag[:, k0 + i]
        acc_d = np.zeros(len(mag))
        for k in range(mb.shape[1]):
            acc_d = acc_d + float(mb[m, k]) * mag[:, k]  # the terms outside the band add exact zeros
        assert np.array_equal(acc_b, acc_d)
    # a dense row with an interior zero keeps it
    dense = np.array([[0.0, 0.5, 0.0, 0.25, 0.0]], np.float32)
    assert mc.band_form(dense)[0][0] == 1 and list(mc.band_form(dense)[0][1]) == [0.5, 0.0, 0.25]


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("mutant", mc.MUTANTS)
def test_every_mutant_leaves_the_gate(golden, refs, name, mutant):
    meta, z = golden[name]
    cfg = CONFIGS[name]
    if mutant == "window_not_centred" and cfg["win_length"] == cfg["filter_length"]:
        # an equivalent mutant here: there is nothing to centre when the window fills the frame; the tiny configuration carries it
        assert np.array_equal(mc.bases(cfg, mutant)[0], mc.bases(cfg)[0])
        return
    worst = 0.0
    for i, r in enumerate(refs[name]):
        mel, energy, _, _ = mc.reference64(z[f"wave{i}"], cfg, mutant=mutant)
        sh = mc.shares(mel, energy, r)
        worst = max(worst, sh["mel"], sh["energy"])
    print(f"{name} {mutant}: worst share {worst:.3g}")
    assert worst > 1.0, f"{mutant} stays inside the gate: the fixture waves are too tame"


# ---- the host side of the C ABI ---------------------------------------------------------------------------------------------
def _create(L, so, **over):
    kw = dict(filter_length=1024, hop_length=256, win_length=1024, n_mel=80)
    kw.update(over)
    h = C.c_void_p()
    rc = so.ns_mel_create(C.byref(A.config_struct(kw["filter_length"], kw["hop_length"], kw["win_length"], kw["n_mel"], kw.get("clip_val", 1e-5))), C.byref(h))
    return rc, h


def test_create_refusals_and_sizes(lib):
    L, so = lib
    assert so.ns_mel_abi_version() == 1
    for over, msg in ((dict(filter_length=1000), "multiple of hop_length"), (dict(hop_length=64 + 16, filter_length=320), "multiple of 32"),
                      (dict(win_length=1025), "win_length"), (dict(n_mel=82), "multiple of 4"),
                      (dict(filter_length=8192), "outside the range"), (dict(clip_val=0.0), "clip_val")):
        rc, h = _create(L, so, **over)
        assert rc != 0 and msg in so.ns_last_error().decode(), (over, so.ns_last_error())
    rc, h = _create(L, so)
    assert rc == 0
    # packed basis + band table + room for a dense mel matrix, every tensor at a 256-byte step
    r256 = lambda n: (4 * n + 255) // 256 * 256  # noqa: E731
    assert so.ns_mel_arena_bytes(h) == r256(1024 * 1024) + r256(3 * 80) + r256(80 * 513)
    prev = 0
    for B, n in ((1, 0), (1, 513), (1, 5000), (2, 5000), (2, 5001), (3, 256000), (16, 256000)):
        b = so.ns_mel_ws_bytes(h, B, n)
        assert b >= prev and b >= 4 * B * (n // 256 + 4) * (256 + 1024)
        prev = b
    assert [so.ns_mel_frames(n, 256) for n in (0, 255, 256, 513, 5000, -1)] == [1, 1, 2, 3, 20, 0] and so.ns_mel_frames(100, 0) == 0
    so.ns_mel_destroy(h)


def test_weight_keys(lib):
    L, so = lib
    rc, h = _create(L, so, filter_length=256, hop_length=32, win_length=192, n_mel=16)
    assert rc == 0

    def chk(name, shape):
        return so.ns_mel_check_weight(h, name.encode(), (C.c_int64 * len(shape))(*shape), len(shape))

    def setw(name, arr):
        return so.ns_mel_set_weight(h, name.encode(), C.c_void_p(arr.ctypes.data), (C.c_int64 * arr.ndim)(*arr.shape), arr.ndim)

    assert chk("stft_fn.forward_basis", (258, 1, 256)) == 0 and chk("mel_basis", (16, 129)) == 0
    assert chk("stft_fn.inverse_basis", (258, 1, 256)) == 0, "accepted and ignored"
    assert chk("stft_fn.forward_basis", (258, 256)) != 0 and "rank mismatch" in so.ns_last_error().decode()
    assert chk("mel_basis", (16, 128)) != 0 and "size mismatch" in so.ns_last_error().decode()
    assert chk("window", (256,)) != 0 and "unexpected key" in so.ns_last_error().decode()
    fb = A.stft_forward_basis(256, 192)
    assert setw("stft_fn.forward_basis", fb) == 0 and setw("stft_fn.inverse_basis", fb) == 0
    # finalize: host-side checks come first (no arena, then missing keys)
    assert so.ns_mel_finalize_weights(h, None) != 0 and "no arena" in so.ns_last_error().decode()
    so.ns_mel_destroy(h)


def test_python_surface_without_a_gpu(lib):
    import torch

    st = A.TacotronSTFT(256, 32, 192, 16, 16000, 0, 8000)
    assert st.frames(1559) == 49 and tuple(st.mel_basis.shape) == (16, 129) and tuple(st.forward_basis.shape) == (258, 1, 256)
    assert set(st.state_dict()) == {"stft_fn.forward_basis", "mel_basis"}
    st.load_state_dict({"mel_basis": np.ones((16, 129), np.float32), "stft_fn.inverse_basis": np.zeros((258, 1, 256), np.float32)})
    assert float(st.mel_basis.sum()) == 16 * 129
    with pytest.raises(RuntimeError, match="size mismatch"):
        st.load_state_dict({"mel_basis": np.ones((16, 128), np.float32)})
    with pytest.raises(RuntimeError, match="unexpected key"):
        st.load_state_dict({"window": np.ones(4, np.float32)})
    with pytest.raises(RuntimeError, match="cuda"):
        st.mel_spectrogram(torch.zeros(1, 1000))
    with pytest.raises(ValueError, match="float32"):
        st.mel_spectrogram(torch.zeros(1, 1000, dtype=torch.float64))
    with pytest.raises(ValueError, match="batch of waves"):
        st.mel_spectrogram(torch.zeros(1000))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        A.TacotronSTFT(320, 80, 320, 16, 16000, 0, 8000)
    cfg = {"preprocessing": {"stft": {"filter_length": 1024, "hop_length": 256, "win_length": 1024}, "mel": {"n_mel_channels": 80, "mel_fmin": 0, "mel_fmax": 8000},
                             "audio": {"sampling_rate": 22050}}}
    assert A.TacotronSTFT.from_config(cfg).filter_length == 1024
    import smart_nar_fast_tts_amd as pkg

    assert pkg.TacotronSTFT is A.TacotronSTFT and pkg.get_mel_from_wav is A.get_mel_from_wav
