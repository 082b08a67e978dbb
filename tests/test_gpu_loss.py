"""Validation loss on the GPU (csrc/loss.hip through loss.FastSpeech2Loss): the stored reference values, seeded random tuples
against the float64 restatement (tests/loss_cpu.py) within the derived gate, NaN poison behind every mask, bitwise determinism,
empty selections, the chain behind forward_teacher_forced() with evaluate(), and the refusals."""
import numpy as np
import pytest
import torch

import smart_nar_fast_tts_amd.workload as wl
from tests import loss_cpu as lc
from tests.util import load_golden

pytestmark = pytest.mark.gpu


def _loss(level):
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss

    return FastSpeech2Loss(wl.preprocess_config(level, level), wl.model_config("tiny"))


def _cuda(x):
    if torch.is_tensor(x):
        return x.cuda()
    return [a.cuda() for a in x] if isinstance(x, (list, tuple)) else x


def _upload(inputs, predictions):
    return tuple(_cuda(x) for x in inputs), tuple(_cuda(x) for x in predictions)


def _run(loss, inputs, predictions):
    out = loss(inputs, predictions)
    assert len(out) == 7 and all(o.dim() == 0 and o.dtype == torch.float32 and o.is_cuda for o in out)
    assert all(o._base is out[0]._base for o in out) and tuple(out[0]._base.shape) == (7,)
    return out[0]._base.cpu().numpy()


def _inside(got, want, gate, what):
    share = lc.shares(got, want, gate)
    print(what, "share of the gate:", dict(zip(lc.NAMES, share.round(4))))
    assert (share <= 1.0).all(), (what, dict(zip(lc.NAMES, share)), got, want)


@pytest.mark.parametrize("name,source", [("loss_tiny", "teacher_tiny"), ("loss_tiny_phoneme_level", "teacher_tiny_phoneme_level")])
def test_fixtures(name, source):
    meta, z = load_golden(name)
    ms, zs = load_golden(source)
    i64, p64 = lc.fixture_case(zs, ms, "_f64")
    gate = lc.gates(i64, p64, ms["pitch"], ms["energy"])
    got = _run(_loss(ms["pitch"]), *_upload(*lc.fixture_case(zs, ms, "")))
    _inside(got, z["values_f64"], gate, name)


@pytest.mark.parametrize("level", lc.LEVELS)
@pytest.mark.parametrize("name", list(lc.CASES))
def test_random_tuples(name, level):
    inputs, predictions, want, gate = lc.case(name, level)
    _inside(_run(_loss(level), *_upload(inputs, predictions)), want, gate, f"{name} {level}")


@pytest.mark.parametrize("level", lc.LEVELS)
def test_poison_behind_every_mask(level):
    inputs, predictions, _, _ = lc.case("unaligned_prime_T_empty_utterances", level)
    loss = _loss(level)
    clean = _run(loss, *_upload(inputs, predictions))
    dirty = _run(loss, *_upload(*lc.poison(inputs, predictions, level, level)))
    assert np.isfinite(clean).all()
    assert clean.tobytes() == dirty.tobytes(), (clean, dirty)


def test_determinism():
    inputs, predictions, _, _ = lc.case("L_past_two_strips_H4_longer_targets", "frame_level")
    gi, gp = _upload(inputs, predictions)
    loss = _loss("frame_level")
    first = _run(loss, gi, gp)
    assert _run(loss, gi, gp).tobytes() == first.tobytes()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = loss(gi, gp)
    side.synchronize()
    assert second[0]._base.cpu().numpy().tobytes() == first.tobytes()
    for w in loss._ws.values():
        w.fill_(0xFF)  # every float64 and int64 word of every slot: NaN / -1
    assert _run(loss, gi, gp).tobytes() == first.tobytes()


def test_empty_selection():
    inputs, predictions = lc.random_case(3, 9, 33, 2, mel_lens=[0, 0, 0], seed=5)
    got = _run(_loss("frame_level"), *_upload(inputs, predictions))
    assert np.isnan(got[[0, 1, 2, 3, 4, 6]]).all() and np.isfinite(got[5]), got
    want = lc.loss(inputs, predictions, "frame_level", "frame_level")
    assert abs(got[5] - want[5]) <= lc.gates(inputs, predictions, "frame_level", "frame_level")[5]


def _teacher_model(meta):
    from smart_nar_fast_tts_amd.model import FastSpeech2Align

    cfg = wl.model_config(meta["config"])
    sd = wl.synth_state_dict(cfg, seed=meta["weight_seed"], frames_per_phoneme=meta["frames_per_phoneme"])
    sd.update(wl.synth_aligner_state_dict(cfg, seed=meta["aligner_seed"]))
    m = FastSpeech2Align(wl.preprocess_config(meta["pitch"], meta["energy"]), cfg).to("cuda:0").eval()
    m.load_state_dict(sd)
    return m


def test_end_to_end_and_evaluate():
    from smart_nar_fast_tts_amd.loss import FastSpeech2Loss, evaluate

    meta, z = load_golden("teacher_tiny")
    dev = lambda k: torch.from_numpy(np.asarray(z[k])).cuda()  # noqa: E731
    batch = (["a", "b"], ["", ""], torch.zeros(2, dtype=torch.long).cuda(), dev("texts"), dev("src_lens"), meta["L"], dev("mels"), dev("mel_lens"),
             meta["T"], dev("p_targets"), dev("e_targets"))
    level = meta["pitch"]
    results = {}
    m = _teacher_model(meta)
    loss = FastSpeech2Loss(m.preprocess_config, m.model_config)
    for outputs in ("views", "separate"):
        m.outputs = outputs  # (model_config["outputs"]: read at every forward)
        out = m.forward_teacher_forced(*batch[2:])
        results[outputs] = _run(loss, batch, out)
        if outputs == "views":
            host_in = tuple(x.cpu() if torch.is_tensor(x) else x for x in batch)
            host_out = tuple([a.cpu() for a in x] if isinstance(x, list) else (x.cpu() if torch.is_tensor(x) else x) for x in out)
            want = lc.loss(host_in, host_out, level, level)
            _inside(results[outputs], want, lc.gates(host_in, host_out, level, level), "teacher-forced tuple")
            means = np.array(evaluate(m, [batch, batch], loss))
            rel = np.abs(means - results[outputs].astype(np.float64)) / np.abs(results[outputs])
            print("evaluate() against one batch, relative:", rel)
            assert (rel <= 1e-6).all(), rel
    assert results["views"].tobytes() == results["separate"].tobytes()


def test_error_paths():
    inputs, predictions, _, _ = lc.case("exact_tiles", "frame_level")
    gi, gp = _upload(inputs, predictions)
    loss = _loss("frame_level")
    swap = lambda t, i, v: t[:i] + (v,) + t[i + 1:]  # noqa: E731
    with pytest.raises(ValueError, match=r"layers 0-3 \(model/loss.py:233-236\); got 2 map"):
        loss(gi, swap(gp, 10, gp[10][:2]))
    with pytest.raises(ValueError, match="mel_predictions must be float32"):
        loss(gi, swap(gp, 0, gp[0].double()))
    with pytest.raises(ValueError, match="mel_targets must be float32"):
        loss(swap(gi, 6, gi[6].half()), gp)
    with pytest.raises(ValueError, match=r"mel_targets must have shape \(2, >= 256, 80\)"):
        loss(swap(gi, 6, gi[6][:, :200]), gp)
    with pytest.raises(ValueError, match=r"pitch_targets must have shape \(2, 256\)"):
        loss(swap(gi, 9, gi[9][:, :64]), gp)
    with pytest.raises(ValueError, match=r"duration_targets must have shape \(2, >= 64\)"):
        loss(gi, swap(gp, 11, gp[11][:, :60]))
    with pytest.raises(ValueError, match=r"attn\[3\] must have shape"):
        loss(gi, swap(gp, 10, gp[10][:3] + [gp[10][3][:, :1]]))
    with pytest.raises(RuntimeError, match="postnet_mel_predictions must live on the MI355X"):
        loss(gi, swap(gp, 1, predictions[1]))
    with pytest.raises(NotImplementedError, match=r"requires_grad: training is out of scope for this path \(SURVEY.md §2\); only eval\(\) is supported"):
        loss(gi, swap(gp, 0, gp[0].clone().requires_grad_(True)))
    with pytest.raises(NotImplementedError, match="training is out of scope"):
        loss.train()
    # non-contiguous inputs are accepted: a transposed-storage mel, and host-side lengths
    odd = swap(gp, 0, gp[0].transpose(1, 2).contiguous().transpose(1, 2))
    host_lens = swap(swap(gi, 4, inputs[4].numpy()), 7, inputs[7].tolist())
    assert _run(loss, host_lens, odd).tobytes() == _run(loss, gi, gp).tobytes()
