"""CPU-only checks of the HiFi-GAN vocoder's host side (smart_nar_fast_tts_amd.vocoder, include/nar_fs2.h ns_voc_*): the
weight-norm fold, config validation, state-dict rejection, the workspace formula, the int16 cast / trim of vocoder_infer and the
register gate of csrc/vocoder.hip.  The GPU side is tests/test_gpu_vocoder.py."""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import smart_nar_fast_tts_amd.workload as wl  # noqa: E402
from tests import hifigan_cpu  # noqa: E402
from tests.util import assert_no_spill  # noqa: E402

pytestmark = pytest.mark.filterwarnings("ignore::FutureWarning")


@pytest.fixture(scope="module")
def V():
    from smart_nar_fast_tts_amd import vocoder

    return vocoder


@pytest.fixture(scope="module")
def h():
    return wl.hifigan_config("v1")


@pytest.fixture(scope="module")
def sd(h):
    return wl.synth_vocoder_state_dict(h, seed=0)


def test_weight_norm_fold_is_bit_identical_to_remove_weight_norm(V, h, sd):
    ref = hifigan_cpu.folded(h, sd).state_dict()
    n = 0
    for k in sd:
        if k.endswith(".weight_g"):
            p = k[: -len("_g")]
            got = V.fold_weight_norm(sd[k], sd[p + "_v"])
            assert got.dtype == torch.float32 and torch.equal(got, ref[p]), p
            n += 1
    assert n == 1 + 4 + 4 * 3 * 3 * 2 + 1  # conv_pre, ups, resblock convs, conv_post
    # the fold is not the identity: g was drawn away from ||v||
    assert not torch.equal(ref["ups.0.weight"], torch.from_numpy(sd["ups.0.weight_v"]))


def test_synthetic_weights_are_in_checkpoint_form(h, sd):
    assert all(k.endswith((".weight_g", ".weight_v", ".bias")) for k in sd)
    assert sd["ups.0.weight_v"].shape == (512, 256, 16) and sd["ups.0.weight_g"].shape == (512, 1, 1)
    assert sd["resblocks.11.convs1.2.weight_g"].shape == (32, 1, 1)
    assert sd["conv_post.weight_v"].shape == (1, 32, 7)
    again = wl.synth_vocoder_state_dict(h, seed=0)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)


@pytest.mark.parametrize("edit, msg", [
    (lambda c: c.update(resblock="2"), "resblock"),
    (lambda c: c.update(upsample_kernel_sizes=[16, 15, 4, 4]), "2 * rate"),
    (lambda c: c.update(upsample_rates=[8, 8, 3, 2], upsample_kernel_sizes=[16, 16, 6, 4]), "even"),
    (lambda c: c.update(resblock_kernel_sizes=[3, 8, 11]), "odd"),
    (lambda c: c.update(upsample_initial_channel=128), "multiple of 32"),
    (lambda c: c.update(num_mels=81), "n_mel"),
])
def test_config_validation_rejects(V, h, edit, msg):
    bad = copy.deepcopy(h)
    edit(bad)
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        V.Generator(bad)


def test_config_validation_host_side(V, h):
    bad = copy.deepcopy(h)
    bad["resblock_dilation_sizes"] = [[1, 3], [1, 3], [1, 3]]  # ResBlock2's shape
    with pytest.raises(ValueError, match="three dilations"):
        V.Generator(bad)
    assert V.Generator(h).hop == 256


def test_state_dict_rejection_leaves_loaded_weights(V, h, sd):
    g = V.Generator(h)
    if torch.cuda.is_available():  # (upload needs a device; the validation under test does not)
        g.to("cuda")
    g.load_state_dict(sd)
    before = {k: v.copy() for k, v in g._sd.items()}
    unknown = dict(sd)
    unknown["resblocks.12.convs1.0.bias"] = np.zeros(32, np.float32)
    with pytest.raises(RuntimeError, match="unexpected key 'resblocks.12.convs1.0.bias'"):
        g.load_state_dict(unknown)
    shape = dict(sd)
    shape["ups.1.weight_v"] = np.zeros((256, 128, 15), np.float32)
    shape["ups.1.weight_g"] = np.ones((256, 1, 1), np.float32)
    with pytest.raises(RuntimeError, match="size mismatch for 'ups.1.weight'"):
        g.load_state_dict(shape)
    missing = {k: v for k, v in sd.items() if not k.startswith("conv_post.")}
    with pytest.raises(RuntimeError, match="missing key.*conv_post.weight"):
        g.load_state_dict(missing)
    half = dict(sd)
    del half["conv_pre.weight_v"]
    with pytest.raises(RuntimeError, match="conv_pre.weight_g"):
        g.load_state_dict(half)
    assert set(g._sd) == set(before) and all(np.array_equal(g._sd[k], before[k]) for k in before)
    # plain (already folded) weights are accepted too
    plain = {k: v for k, v in hifigan_cpu.folded(h, sd).state_dict().items()}
    g.load_state_dict(plain)
    assert all(np.array_equal(g._sd[k], before[k]) for k in before)


def test_ws_bytes_formula(V, h):
    g = V.Generator(h)

    def formula(B, T):
        c0, s, a = h["upsample_initial_channel"], 1, T * max(h["num_mels"], h["upsample_initial_channel"])
        for i, u in enumerate(h["upsample_rates"]):
            s *= u
            a = max(a, T * s * (c0 >> (i + 1)))
        per = (B * a + 63) // 64 * 64
        return 4 * per * 4

    for B, T in ((1, 1), (3, 33), (16, 1013), (5, 7)):
        assert g.ws_bytes(B, T) == formula(B, T), (B, T)
    assert g.ws_bytes(0, 5) == 0
    lib = g._lib
    assert lib.ns_voc_abi_version() == 1
    assert lib.ns_abi_version() == 6  # the acoustic model's contract is unchanged


def _cast_trim_expected(wavs, max_wav, lengths):
    out = []
    for i, row in enumerate(wavs):
        n = len(row) if lengths is None else lengths[i]
        out.append(np.array([int(np.float32(v) * np.float32(max_wav)) for v in row[:n]], dtype=np.int16))
    return out


def test_vocoder_infer_cast_and_trim(V):
    rs = np.random.RandomState(3)
    w = rs.uniform(-0.999, 0.999, size=(3, 512)).astype(np.float32)
    w[0, :4] = [0.5 / 32768, -0.5 / 32768, 1.5 / 32768, -1.5 / 32768]  # truncation toward zero, both signs
    pc = {"preprocessing": {"audio": {"max_wav_value": 32768.0}, "stft": {"hop_length": 256}}}
    lengths = [512, 256, 1]
    got = V.wav_cast_trim(torch.from_numpy(w), pc, lengths)
    exp = _cast_trim_expected(w, 32768.0, lengths)
    assert [g.dtype for g in got] == [np.int16] * 3
    assert all(np.array_equal(a, b) for a, b in zip(got, exp))
    assert list(got[0][:4]) == [0, 0, 1, -1]
    full = V.wav_cast_trim(torch.from_numpy(w), pc, None)
    assert [len(x) for x in full] == [512] * 3
    assert V.hop_length(pc) == 256


def test_get_vocoder_rejects_melgan(V):
    with pytest.raises(NotImplementedError, match="MelGAN"):
        V.get_vocoder({"vocoder": {"model": "MelGAN", "speaker": "LJSpeech"}}, "cuda")


def test_vocoder_kernels_do_not_spill():
    stdout = assert_no_spill("vocoder.hip", kernels=("k_voc_post", "k_voc_transpose"))
    assert stdout.count("k_voc_gemm<") == 3, stdout
