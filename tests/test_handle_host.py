"""CPU-only checks of ``_handle.NativeHandle`` over each of the five C-ABI handle families: create, check_weight and arena_bytes run
without a device.  The text ``check_weight`` returns must be the library's own: what the direct ``ns_*_check_weight`` +
``ns_last_error()`` pair gives for the same key and shape."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402


def _family(prefix):
    """(config struct, an accepted key with its shape) — the smallest configs the other host tests build."""
    from smart_nar_fast_tts_amd import audio, model, vocoder

    if prefix in ("ns", "ns_aln"):
        cfg = model.config_struct(wl.preprocess_config(), wl.model_config("tiny"))
        return cfg, ("mel_linear.bias", (80,)) if prefix == "ns" else ("mel_encoder.prenet.w_2.bias", (256,))
    if prefix == "ns_voc":
        return vocoder.config_struct(wl.hifigan_config("v1")), ("conv_post.bias", (1,))
    if prefix == "ns_mel":
        return audio.config_struct(256, 32, 192, 16), ("mel_basis", (16, 129))
    return audio.gl_config_struct(256, 32, 192, 16), ("mel_basis", (16, 129))


def _direct(lib, prefix, h, key, a):
    """The library's answer without the class: rc of ``{prefix}_check_weight`` and, when refused, ``ns_last_error()``."""
    rc = getattr(lib, prefix + "_check_weight")(h, key.encode(), (C.c_int64 * a.ndim)(*a.shape), a.ndim)
    return "" if rc == 0 else lib.ns_last_error().decode()


@pytest.mark.parametrize("prefix", ["ns", "ns_aln", "ns_voc", "ns_mel", "ns_gl"])
def test_native_handle_life_cycle_on_the_host(prefix):
    from smart_nar_fast_tts_amd import _lib
    from smart_nar_fast_tts_amd._handle import NativeHandle, host_f32

    lib = _lib.load()
    cfg, (key, shape) = _family(prefix)
    h = NativeHandle(prefix, cfg, "test")
    assert h and isinstance(h._as_parameter_, C.c_void_p)
    good = host_f32(np.zeros(shape, np.float64))
    assert good.dtype == np.float32 and good.flags.c_contiguous
    assert h.check_weight(key, good) == "" and _direct(lib, prefix, h, key, good) == ""
    for k, a in (("not.a.key", good), (key, np.zeros(tuple(shape) + (3,), np.float32))):
        text = h.check_weight(k, a)
        assert text and text == _direct(lib, prefix, h, k, a)
    assert getattr(lib, prefix + "_arena_bytes")(h) > 0  # the instance is the handle argument
    h.close()
    assert not h
    h.close()
    assert not h
