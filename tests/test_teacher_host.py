"""Teacher-forced forward, everything that needs no GPU: the torch-CPU restatement (tests/teacher_cpu.py) against the fixtures
captured from the imported reference (tests/golden/make_golden_teacher.py), the numpy statement of the target scan on hand-made
rows, and the new C-ABI symbols' declarations."""
import os
import re

import numpy as np
import pytest
import torch

from smart_nar_fast_tts_amd import _lib
from tests import aligner_cpu as ac
from tests import teacher_cpu as tc
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("teacher_tiny", "teacher_tiny_phoneme_level", "teacher_T_above_1000")
FLOATS = ("output", "postnet_output", "p_predictions", "e_predictions", "log_d_predictions")


def restated(name, dtype):
    meta, z = load_golden(name)
    cfg, sd = ac.fixture_weights(meta)
    w = ac.to_torch_weights(sd, dtype)
    pitch, energy = tc.fixture_levels(meta)
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    with torch.no_grad():
        out = tc.forward(w, cfg, t("texts"), t("src_lens"), t("mels").to(dtype), t("mel_lens"), t("p_targets").to(dtype), t("e_targets").to(dtype),
                         pitch_level=pitch, energy_level=energy,
                         d_targets=None if dtype == torch.float32 else t("d_targets"))  # (the maker forces float64's durations too)
    return meta, z, out


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    """fp32 against the reference's fp32 and float64 against its .double() evaluation.  Integers and masks exact — d_targets computed
    by the restatement's own fp32 alignment, exact where the fixture's seed met the maker's gap bar and under the rule of
    test_durations where none in range(32) did (teacher_T_above_1000: best ratio 382; its smallest gap, 8.4e-4, still forces every
    frame to agree) —; floats within the rule the maker recorded in meta["restatement_max_abs"] (2e-5, what the aligner restatement
    is held to in tests/test_aligner_host.py: torch's own kernels on the same operands — bit for bit on the machine that wrote the
    fixtures — but another thread count or instruction set may sum in another order)."""
    for dtype, suffix in ((torch.float32, ""), (torch.float64, "_f64")):
        meta, z, out = restated(name, dtype)
        rows = slice(None) if meta["rows"] is None else np.asarray(meta["rows"])
        assert out[5] is out[11] and out[11].dtype == torch.int64
        assert tc.check_durations(out[10][-1].numpy(), out[11].numpy(), meta, z) == 0
        assert np.array_equal(out[9].numpy(), z["out_mel_lens"]) and np.array_equal(z["out_mel_lens"], z["d_targets"].sum(axis=1))
        assert np.array_equal(out[6].numpy(), z["src_masks"]) and np.array_equal(out[7].numpy(), z["mel_masks"])
        # the mask the HIP path returns (t >= sum of the durations) is the reference's on these inputs (src_lens >= 1, mel_lens <= T)
        assert np.array_equal(np.arange(meta["T"])[None, :] >= z["out_mel_lens"][:, None], z["mel_masks"])
        for i, key in enumerate(FLOATS):
            if key + suffix not in z:
                continue
            got = out[i].numpy()
            got = got[:, rows] if key in ("output", "postnet_output") else got
            e = float(np.abs(got - z[key + suffix]).max())
            print(f"{name} {dtype} {key}: max-abs {e:.3e}")
            assert e <= meta["restatement_max_abs"], (name, dtype, key, e)
        if meta["rows"] is None:
            for i, a in enumerate(out[10]):
                e = float(np.abs(a.numpy() - z[f"attn{i}{suffix}"]).max())
                assert e <= meta["restatement_max_abs"], (name, dtype, i, e)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_gap_bar(name):
    """What the maker recorded: the float64 top-two gap against 1000 x the fp32-vs-float64 distance of the head-summed last map, and
    that the float64 map's own durations are the fp32 evaluation's."""
    meta, z = load_golden(name)
    assert meta["exact_durations"] == (meta["min_top2_gap_f64"] >= meta["gap_factor"] * meta["head_sum_dist_fp32_f64"])
    assert meta["gap_factor"] == 1000.0
    if meta["exact_durations"]:
        assert np.array_equal(z["d_targets"], z["d_targets_f64map"]) and meta["frames_differing_fp32_f64"] == 0
    else:  # the maker asserted the reference's own fp32 evaluation against the fallback's cap
        assert meta["frames_differing_fp32_f64"] <= 0.01 * z["argmax_f64"].size
    assert z["argmax_f64"].shape == z["top2_gap_f64"].shape == (int(z["mel_lens"].sum()),)
    assert abs(float(z["top2_gap_f64"].min()) - meta["min_top2_gap_f64"]) <= 1e-12
    assert (z["d_targets"] >= 0).all() and np.array_equal(z["d_targets"].sum(axis=1), z["mel_lens"])


def test_target_scan_statement():
    """tests/teacher_cpu.target_scan on hand-made rows: zeros, a negative entry (clamped in the sums, kept in dur_keep), a short
    utterance and a bad token id."""
    d = np.array([[2, 0, 3, 0], [1, -4, 5, 0], [0, 0, 0, 0]], dtype=np.int64)
    texts = np.array([[1, 2, 3, 4], [5, 6, 0, 0], [7, 99, 1, 1]])
    cum, keep, mask, lens = tc.target_scan(d, [4, 2, 4], texts, n_vocab=50)
    assert cum.dtype == np.int32 and keep.dtype == np.float32 and lens.dtype == np.int64
    assert cum.tolist() == [[2, 2, 5, 5], [1, 1, 6, 6], [0, 0, 0, 0]]
    assert keep.tolist() == [[2, 0, 3, 0], [1, -4, 5, 0], [0, 0, 0, 0]]
    assert mask.tolist() == [[False] * 4, [False, False, True, True], [False] * 4]
    assert lens.tolist() == [5, 6, -1]
    assert tc.target_scan(d, [4, 2, 4])[3].tolist() == [5, 6, 0]
    # the expansion those sums describe is LengthRegulator.expand's (model/modules.py:221-223)
    for b in range(3):
        idx = np.repeat(np.arange(4), np.maximum(d[b], 0))
        assert [int(np.searchsorted(cum[b], t, side="right")) for t in range(len(idx))] == idx.tolist()


def test_symbols_declared():
    """Additions only: both new entries are in the header, carry argtypes whose count matches the declaration, and the ABI versions
    stay where they were."""
    with open(os.path.join(ROOT, "include", "nar_fs2.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("ns_forward_durations_teacher", "ns_op_duration_target_scan"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_args, (name, len(args), n_args)
        assert getattr(lib, name).argtypes == args
    assert "#define NS_ABI_VERSION 6" in header and "#define NS_ALN_ABI_VERSION 1" in header
    assert lib.ns_abi_version() == 6 and lib.ns_aln_abi_version() == 1


def test_forward_still_refuses_mel_lens_and_points_to_the_new_method():
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    m = FastSpeech2Align(wl.preprocess_config(), wl.model_config("tiny"))
    assert callable(m.forward_teacher_forced)
    with pytest.raises(NotImplementedError, match="forward_teacher_forced"):
        m.forward(None, None, None, 3, mels=None, mel_lens=[3])
    with pytest.raises(RuntimeError, match=r"no aligner weights"):
        m.forward_teacher_forced(None, None, None, 3, None, None)
