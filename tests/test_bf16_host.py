"""CPU-only checks of the opt-in "bf16" precision mode (ns_config.matmul_bf16x3 == 2, model_config["matmul"] = "bf16"):
the configuration is accepted, the arena grows by exactly the rounded bf16 weight planes, and the new kernels keep the
register budget.  No compute calls."""
import ctypes as C
import os

import pytest

from tests.util import assert_no_spill, built_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return built_lib()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date


def _cfg(name="tiny", **over):
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import config_struct

    c = config_struct(wl.preprocess_config(), wl.model_config(name))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _arena_bytes(so, cfg):
    h = C.c_void_p()
    assert so.ns_create(C.byref(cfg), C.byref(h)) == 0, so.ns_last_error()
    try:
        return so.ns_arena_bytes(h)
    finally:
        so.ns_destroy(h)


def _plane_bytes(n_out, kw, cin):
    """one bf16 plane [n_out][kw][cin rounded up to 32] as the arena takes it: 2-byte elements in whole floats, 64-float blocks"""
    cinp = (cin + 31) // 32 * 32
    floats = (n_out * kw * cinp + 1) // 2
    return ((floats + 63) // 64 * 64) * 4


def test_create_accepts_the_bf16_mode_and_rejects_unknown_modes(lib):
    L, so = lib
    h = C.c_void_p()
    for mode in (0, 1, 2):
        assert so.ns_create(C.byref(_cfg(matmul_bf16x3=mode)), C.byref(h)) == 0, (mode, so.ns_last_error())
        so.ns_destroy(h)
    for mode in (3, -1):
        assert so.ns_create(C.byref(_cfg(matmul_bf16x3=mode)), C.byref(h)) != 0, mode
        assert "matmul_bf16x3" in so.ns_last_error().decode()


@pytest.mark.parametrize("name", ["tiny", "ljspeech", "d512"])
def test_bf16_arena_is_the_fp32_arena_plus_the_planes(lib, name):
    """Decoder QKV / fc / w_1 / w_2, mel_linear and all five PostNet convolutions get one bf16 plane each; nothing else moves
    (the fp32 copies stay for state_dict() and the arena broadcast)."""
    import smart_nar_fast_tts_amd.workload as wl

    L, so = lib
    mc = wl.model_config(name)
    c = _cfg(name)
    d, di = c.d_dec, c.d_inner
    planes = 0
    for _ in range(c.n_dec_layer):
        planes += _plane_bytes(3 * d, 1, d) + _plane_bytes(d, 1, d) + _plane_bytes(di, c.ffn_k1, d) + _plane_bytes(d, c.ffn_k2, di)
    planes += _plane_bytes(c.n_mel, 1, d)
    for i in range(c.postnet_n):
        cin = c.n_mel if i == 0 else c.postnet_dim
        cout = c.n_mel if i == c.postnet_n - 1 else c.postnet_dim
        planes += _plane_bytes(cout, c.postnet_k, cin)
    fp32 = _arena_bytes(so, _cfg(name))
    bf16 = _arena_bytes(so, _cfg(name, matmul_bf16x3=2))
    assert bf16 - fp32 == planes, (name, bf16 - fp32, planes)
    assert mc["transformer"]["decoder_layer"] == c.n_dec_layer


def test_model_config_key_maps_to_mode_2():
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import config_struct

    for key, mode in (("fp32", 0), ("bf16x3", 1), ("bf16", 2)):
        assert config_struct(wl.preprocess_config(), dict(wl.model_config("tiny"), matmul=key)).matmul_bf16x3 == mode
    with pytest.raises(KeyError):
        config_struct(wl.preprocess_config(), dict(wl.model_config("tiny"), matmul="fp16"))


def test_dtype_casts_still_raise_and_name_the_mode():
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    m = FastSpeech2Align(wl.preprocess_config(), wl.model_config("tiny"))
    for cast in (m.half, m.bfloat16, m.double):
        with pytest.raises(NotImplementedError, match="'bf16'"):
            cast()


@pytest.mark.parametrize("src", ["gemm_bf16.hip", "attention.hip"])
def test_bf16_kernels_do_not_spill(src):
    """The register gate of the fp32 sources (tests/test_cabi_and_host.py) over the bf16 GEMM tiles and the attention
    variants: no VGPR / SGPR spill, no scratch."""
    if src == "gemm_bf16.hip":
        stdout = assert_no_spill(src)
        assert stdout.count("k_conv_gemm_bf16<") >= 5, stdout
    else:
        assert_no_spill(src, kernels=("k_attention<64, true>", "k_attention_strip<64, true>"))
