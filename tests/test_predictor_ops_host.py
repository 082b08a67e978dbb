"""The gates of tests/test_gpu_predictor_ops.py proven on the CPU, both ways, and the table of its cases checked against the dispatch
itself (no GPU).

A VariancePredictor forward is two launches (csrc/api.hip predictor_conv1 / predictor_tail, ops.predictor_conv1 / ops.predictor_tail):

1. h = layer_norm_1(relu(conv1d_1(x))): the LayerNorm row epilogue with KW = 3, ReLU in front and no residual.  Gate:
   tests/bf16_emu.py gemm_ln_check(act="relu", resid=None) at FP32_REL — the propagated GEMM bound holds behind a 1-Lipschitz ReLU.
2. pred = masked_fill(layer_norm_2(relu(conv1d_2(h))) . wlin + blin) [* control without a target], then the embedding add.
   The first-order bound  sum_n |wlin_n| (LayerNorm bound)_n + FP32_REL (sum_n |y_n wlin_n| + |blin|)  (bf16_emu.pred_tail_ref) has
   the right shape and is far too loose: it is 4e-3 ... 6e-3 of |pred|, so a row off by 2^-12 would pass.  The gate is PRED_TIGHT x
   that bound, PRED_TIGHT = 8 x the largest share of the bound torch's fp32 CPU evaluation of the same tail reaches over every
   PRED_CASES row and both embedding predictors, rounded up to one significant digit.  The 8 is for the GPU summing the same fp32
   expression in another order (chunks of 64 products on the matrix cores, a wave-shuffle tree for the dot): noise of the same
   size, not the same bits.  Measured against the CPU fp32 evaluation and float64 only, never against a kernel.

   Measured (test_pred_tight_is_eight_times_the_fp32_share with NS_PRED_ALL_CASES=1, run with -s): CPU fp32 shares of the bound,
   pitch / energy, per case: tiny 3 x 33 1.70e-4 / 1.71e-4, ljspeech 3 x 343 2.13e-4 / 2.30e-4, tiny 3 x 701 2.65e-4 / 2.39e-4,
   ljspeech 3 x 1031 2.93e-4 / 2.64e-4, tiny 7 x 911 2.73e-4 / 2.57e-4, ljspeech 7 x 1171 2.67e-4 / 2.73e-4, tiny 7 x 2341 3.09e-4 /
   2.84e-4, ljspeech 7 x 3511 2.82e-4 / 3.02e-4, tiny512 3 x 33 1.99e-4 / 1.97e-4, d512 3 x 343 2.49e-4 / 2.29e-4, tiny512 7 x 911
   2.51e-4 / 2.79e-4, tiny 5 x 1 9.3e-5 / 1.32e-4, tiny 5 x 3 1.02e-4 / 1.88e-4, ljspeech 4 x 33 (a length of 0) 1.46e-4 / 2.31e-4.
   Largest 3.09e-4; 8 x = 2.47e-3 -> PRED_TIGHT = 3e-3 (fp32 on the CPU then sits at 0.03 ... 0.10 of the gate).
   Mutants, each evaluated in float64 (factor = worst error / gate; > 1 fails), smallest ... largest over the 99-, 1029- and
   6377-row cases and both predictors: one (channel, tap) of conv1d_2 dropped 1.0e4 ... 3.3e4; the neighbouring utterance's row for
   zero padding and ReLU omitted 3.9e4 ... 1.6e5; one wlin element dropped 248 ... 2.7e4; blin omitted 5.0e4 ... 9.1e4; ln_2 gamma /
   beta of columns 7 and 8 swapped 1.1e3 ... 8.6e3; the row with the largest |pred| off by 2^-12 44.9 ... 70.4; the mask one row
   late infinite (a padded row must be exactly zero), one row early 6.8e4 ... 2.1e5; control applied although a target is given
   9.2e4 ... 2.0e5, not applied without one 7.6e4 ... 2.9e5.  Stage 1 (3 x 33, tiny and tiny512): fp32 on the CPU 0.0052 ... 0.0075
   of its bound; ReLU omitted 6.5e3 ... 1.0e4, neighbour's row 8.6e3 ... 1.0e4, a dropped (channel, tap) 673 ... 881, LayerNorm
   columns swapped 509 ... 834 x.
   On the MI355X (profiles/predictor_ops.md, 48 cases): stage 1 at most 0.0064 of its bound (fp32 on the CPU 0.0101); pred of the
   pitch / energy predictors at most 1.93e-4 of the first-order bound = 0.064 of the gate (fp32 on the CPU 2.82e-4), of the
   duration predictor 5.41e-4 = 0.18 of the gate (fp32 on the CPU 3.77e-4).

The embedding needs no tolerance: x_out must be the bits of fp32 (x_in + emb[idx]) + pos[t] with idx = bucketize of the STORED pred
(or of the target), padded rows included (the add is unmasked).  embed_ref states that on the CPU; the precondition test asserts
that the synthetic weights spread the predictions over the buckets (a seed change that collapses them fails here)."""
import numpy as np
import pytest
import torch

import tests.test_fp32_ops_host as T
from tests import bf16_emu as E
from tests.util import weights_for

REL = E.FP32_REL
PRED_TIGHT = 3e-3
METAS = {
    "tiny": dict(config="tiny", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25),
    "tiny512": dict(config="tiny512", weight_seed=0, frames_per_phoneme=4.0, dur_weight_scale=0.25),
    "ljspeech": dict(config="ljspeech", weight_seed=0, frames_per_phoneme=8.0, dur_weight_scale=0.25),
    "d512": dict(config="d512", weight_seed=0, frames_per_phoneme=8.0, dur_weight_scale=0.25),
}
F = 256  # variance_predictor.filter_size of every config
_f = T._f

# (config, B, S, lens (None: T._lens), row_epilogue, form of conv1d_1's launches, form of conv1d_2's).  The eight forms the two
# contractions take (full-row heights 32 / 48 / 80 / 112, the four ticketed rungs), tiny / ljspeech alternating as LN_CASES does;
# 3 x 33, 3 x 343 and 7 x 911 again on the 512-wide configs (conv1d_1 reads 512 channels; the embedding / position add walks a
# 512-wide row); the two-launch form; utterances shorter than the kernel's reach; an utterance of length 0.  Every M leaves a
# partial last row tile, lens are ragged, B >= 3; S > 1000 (the last three full-row cases) crosses the position-table switch.
_T1 = dict(ticket=1)
_RUNGS = {33: _f(32, 32, ks=8, **_T1), 343: _f(32, 64, ks=4, **_T1), 701: _f(48, 64, ks=4, mf=16, **_T1), 1031: _f(32, 128, ks=2, **_T1)}
_ROWS = {911: _f(32, 256, rowepi=1), 1171: _f(48, 256, mf=16, rowepi=1), 2341: _f(80, 256, mf=16, rowepi=1), 3511: _f(112, 256, mf=16, rowepi=1)}
PRED_CASES = (
    [(("tiny", "ljspeech")[i % 2], 3, S, None, "fused", [f], [f]) for i, (S, f) in enumerate(_RUNGS.items())]
    + [(("tiny", "ljspeech")[i % 2], 7, S, None, "fused", [f], [f]) for i, (S, f) in enumerate(_ROWS.items())]
    + [("tiny512", 3, 33, None, "fused", [_RUNGS[33]], [_RUNGS[33]]), ("d512", 3, 343, None, "fused", [_RUNGS[343]], [_RUNGS[343]]),
       ("tiny512", 7, 911, None, "fused", [_ROWS[911]], [_ROWS[911]])]
    + [("tiny", 3, 33, None, "two_launch", [_f(32, 32, ks=8)], [_f(32, 32, ks=8)]),
       ("ljspeech", 3, 1031, None, "two_launch", [_f(32, 128, ks=2)], [_f(32, 128, ks=2)])]
    + [("tiny", 5, 1, [1, 1, 1, 1, 1], "fused", [_RUNGS[33]], [_RUNGS[33]]), ("tiny", 5, 3, [3, 2, 1, 3, 3], "fused", [_RUNGS[33]], [_RUNGS[33]])]
    + [("ljspeech", 4, 33, [33, 0, 20, 33], "fused", [_RUNGS[33]], [_RUNGS[33]])]
)
CONTROLS = (1.0, 0.5, 1.7)


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}" + ("-lens" + "_".join(map(str, c[3])) if c[3] else "") + ("-two_launch" if c[4] != "fused" else "")


def lens_of(case):
    return list(case[3]) if case[3] is not None else T._lens(case[1], case[2])


def by_config(cases):
    return sorted(cases, key=lambda c: ["tiny", "tiny512", "ljspeech", "d512"].index(c[0]))


# ---------------------------------------------------------------------------------------------------- weights, inputs, references
_W = {}


def pred_weights(config, which):
    """the predictor's tensors from the seeded checkpoint: conv1d_1 / layer_norm_1 / conv1d_2 / layer_norm_2 / linear_layer, and
    (pitch, energy) the bin edges and the embedding table; mel_decoder.position_enc for the cached position rows"""
    if (config, which) not in _W:
        if not any(k[0] == config for k in _W):
            _W.clear()
        cfg, sd = weights_for(METAS[config])
        t = lambda k: torch.as_tensor(np.asarray(sd[k]))  # noqa: E731
        p = f"variance_adaptor.{which}_predictor."
        w = dict(w1=t(p + "conv_layer.conv1d_1.conv.weight"), b1=t(p + "conv_layer.conv1d_1.conv.bias"),
                 g1=t(p + "conv_layer.layer_norm_1.weight"), be1=t(p + "conv_layer.layer_norm_1.bias"),
                 w2=t(p + "conv_layer.conv1d_2.conv.weight"), b2=t(p + "conv_layer.conv1d_2.conv.bias"),
                 g2=t(p + "conv_layer.layer_norm_2.weight"), be2=t(p + "conv_layer.layer_norm_2.bias"),
                 wlin=t(p + "linear_layer.weight").reshape(-1), blin=t(p + "linear_layer.bias").reshape(()),
                 pos=t("mel_decoder.position_enc")[0], max_seq_len=cfg["max_seq_len"])
        if which != "duration":
            w.update(bins=t(f"variance_adaptor.{which}_bins"), emb=t(f"variance_adaptor.{which}_embedding.weight"))
        _W[(config, which)] = w
    return _W[(config, which)]


def x_of(B, S, C, seed):
    """N(0, 1) rows, the last utterance a copy of the first (its outputs must carry the first's bits)"""
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal((B, S, C)).astype(np.float32))
    assert bool((x != 0).any(dim=-1).all())
    x[B - 1] = x[0]
    return x


def stage1(x, w, dtype=torch.float64):
    return E.layernorm_emu(E.gemm_emu(x, w["w1"], w["b1"], act="relu", dtype=dtype, round_fn=E.exact), w["g1"], w["be1"], dtype=dtype)


def stage1_check(got, x, w):
    return E.gemm_ln_check(got, x, w["w1"], w["b1"], None, w["g1"], w["be1"], rel=REL, round_fn=E.exact, act="relu")


def tail_ref(h, w, lens, control=1.0, target_given=False):
    return E.pred_tail_ref(h, w["w2"], w["b2"], w["g2"], w["be2"], w["wlin"], w["blin"], lens, control, target_given)


def tail_fp32(h, w, lens, control=1.0, target_given=False):
    return E.pred_tail_fp32(h, w["w2"], w["b2"], w["g2"], w["be2"], w["wlin"], w["blin"], lens, control, target_given)


def targets_of(bins, B, S, seed):
    """[B, S] fp32 targets: every bin edge, its fp32 neighbours on both sides, values beyond both ends, NaN and both infinities,
    -0.0, then values drawn over (and a little beyond) the bins' range; shuffled so that every row tile meets some of each"""
    b = bins.numpy()
    inf = np.float32(np.inf)
    special = np.concatenate([b, np.nextafter(b, -inf), np.nextafter(b, inf), [b[0] - 1, b[-1] + 1, b[0] * 0, -0.0, np.nan, inf, -inf]]).astype(np.float32)
    rs = np.random.RandomState(seed)
    n = B * S
    span = float(b[-1] - b[0])
    rest = rs.uniform(b[0] - 0.05 * span, b[-1] + 0.05 * span, size=max(n - special.size, 0)).astype(np.float32)
    t = np.concatenate([special, rest])
    if n < special.size:  # (the short cases: a rotating window of the special values)
        t = special[(np.arange(n) * 97 + seed) % special.size]
    else:
        rs.shuffle(t)
    return torch.from_numpy(t[:n].reshape(B, S).copy())


def embed_ref(x_in, values, bins, emb, pos=None):
    """fp32 (x_in + emb[bucketize(values)]) + pos[t], in that order, on every row (the add is unmasked)"""
    idx = torch.bucketize(values.float(), bins)
    out = x_in + emb[idx]
    return out if pos is None else out + pos[None, :x_in.shape[1]]


# ---------------------------------------------------------------------------------------------------- the coverage table
@pytest.mark.parametrize("case", PRED_CASES, ids=case_id)
def test_pred_cases_take_their_forms(case):
    config, B, S, lens, mode, forms1, forms2 = case
    M, d = B * S, T.D_MODEL[config]
    epi = 0 if mode == "two_launch" else T.ln_epi(M)
    assert (d, F, 3) in T.PRED_SHAPES and (F, F, 3) in T.PRED_SHAPES
    L1, L2 = T.launches(M, (d, F, 3), epi), T.launches(M, (F, F, 3), epi)
    moved = "a threshold of the dispatch moved: pick a size that takes this form again"
    assert [l[:7] for l in L1] == forms1 and [l[:7] for l in L2] == forms2, moved
    assert all(f in T.FORMS for f in forms1 + forms2)
    ln = lens_of(case)
    assert len(ln) == B >= 3 and max(ln) == S and min(ln) >= 0
    if lens is None:
        assert len(set(ln)) == B and M % forms2[0][0] != 0, "ragged lengths and a partial last row tile"


def test_pred_cases_cover_every_form_and_path():
    fused = [c for c in PRED_CASES if c[4] == "fused"]
    for stage in (5, 6):
        seen = {f for c in fused if T.D_MODEL[c[0]] == 256 for f in c[stage]}
        assert seen == set(_RUNGS.values()) | set(_ROWS.values())  # the eight forms of the issue's table
    # exactly what the dispatch can reach for these two shapes under a row epilogue (a ninth form would need a case)
    reach = {f for f, shapes in T.scan().items() if set(shapes) & set(T.PRED_SHAPES)}
    assert reach == set(_RUNGS.values()) | set(_ROWS.values()), sorted(reach)
    wide = [c for c in fused if T.D_MODEL[c[0]] == 512]
    assert {(c[1], c[2]) for c in wide} == {(3, 33), (3, 343), (7, 911)} and {c[0] for c in wide} == {"tiny512", "d512"}
    assert {(c[1], c[2]) for c in PRED_CASES if c[4] == "two_launch"} == {(3, 33), (3, 1031)}
    assert {(c[1], c[2]) for c in PRED_CASES if c[2] < 3 + 1 and c[1] == 5} == {(5, 1), (5, 3)}
    assert any(0 in lens_of(c) for c in PRED_CASES)
    assert sum(1 for c in fused if c[2] > 1000 and T.ln_epi(c[1] * c[2]) == 1) == 3  # add_pos past max_seq_len on the full-row tile
    assert any(c[2] > 1000 and T.ln_epi(c[1] * c[2]) == 2 for c in fused)            # ... and on the ticketed ladder
    assert max(c[1] * c[2] for c in PRED_CASES) == 24577


# ---------------------------------------------------------------------------------------------------- stage 1: the gate both ways
@pytest.mark.parametrize("config", ["tiny", "tiny512"])
def test_stage1_gate_passes_fp32_and_rejects_wrong_variants(config):
    """layer_norm_1(relu(conv1d_1(x))) at FP32_REL, no residual: torch's fp32 CPU evaluation is inside (0.01 ... 0.02 of the bound);
    ReLU omitted, the neighbouring utterance's row for zero padding, a dropped (channel, tap) and a swapped LayerNorm column are not"""
    B, S = 3, 33
    w = pred_weights(config, "pitch")
    x = x_of(B, S, w["w1"].shape[1], seed=B * S)
    good = stage1_check(stage1(x, w, torch.float32), x, w)
    print(f"\nstage 1 {config}: fp32 CPU {good.worst:.3g} x bound")
    assert good.ok and good.worst < 0.1, str(good)
    ln = lambda z: E.layernorm_emu(z, w["g1"], w["be1"])  # noqa: E731
    wd = w["w1"].clone()
    wd[:, 5, 0] = 0
    g2, b2 = w["g1"].clone(), w["be1"].clone()
    g2[[7, 8]], b2[[7, 8]] = g2[[8, 7]], b2[[8, 7]]
    mutants = {
        "ReLU omitted": ln(E.conv_rows(x, w["w1"], w["b1"])),
        "neighbour's row for zero": ln(E.conv_rows(x, w["w1"], w["b1"], cross_utterance=True).relu()),
        "one (c, tap) dropped": ln(E.conv_rows(x, wd, w["b1"]).relu()),
        "ln_1 columns 7 / 8 swapped": E.layernorm_emu(E.conv_rows(x, w["w1"], w["b1"]).relu(), g2, b2),
    }
    for name, y in mutants.items():
        bad = stage1_check(y, x, w)
        print(f"  {name}: {bad.worst:.3g} x bound")
        assert not bad.ok and bad.worst > 100, (name, str(bad))


# ---------------------------------------------------------------------------------------------------- stage 2: the gate both ways
def _tail64(h, w, lens, control=1.0, target_given=False, cross=False, relu=True, mask_shift=0):
    """the float64 tail with switches for the WRONG variants (its only error is the mutation)"""
    z = E.conv_rows(h, w["w2"], w["b2"], cross_utterance=cross)
    y = E.layernorm_emu(z.relu() if relu else z, w["g2"], w["be2"])
    pred = y @ w["wlin"].double() + w["blin"].double()
    valid = torch.arange(h.shape[1])[None, :] < (torch.as_tensor(lens) + mask_shift)[:, None]
    return torch.where(valid, pred, torch.zeros((), dtype=torch.float64)) * (1.0 if target_given else control)


def _mutants(h, w, lens, ref):
    w2 = dict(w, w2=w["w2"].clone())
    w2["w2"][:, F // 3, 0] = 0
    wl = dict(w, wlin=w["wlin"].clone())
    wl["wlin"][F // 2] = 0
    sw = dict(w, g2=w["g2"].clone(), be2=w["be2"].clone())
    sw["g2"][[7, 8]], sw["be2"][[7, 8]] = w["g2"][[8, 7]], w["be2"][[8, 7]]
    row = ref.clone()
    i = int(ref.abs().argmax())
    row.view(-1)[i] *= 1 + 2.0 ** -12
    out = {
        "one (c, tap) of conv1d_2 dropped": _tail64(h, w2, lens),
        "neighbour's row for zero": _tail64(h, w, lens, cross=True),
        "ReLU omitted": _tail64(h, w, lens, relu=False),
        "one wlin element dropped": _tail64(h, wl, lens),
        "blin omitted": _tail64(h, dict(w, blin=torch.zeros(())), lens),
        "ln_2 columns 7 / 8 swapped": _tail64(h, sw, lens),
        "largest |pred| row off by 2^-12": row,
        "mask one row late": _tail64(h, w, lens, mask_shift=1),
        "mask one row early": _tail64(h, w, lens, mask_shift=-1),
    }
    return out


GATE_CASES = [c for c in PRED_CASES if c[4] == "fused" and c[3] is None and T.D_MODEL[c[0]] == 256 and c[2] in (33, 343, 911)]
_DATA = {}


def case_data(case, which):
    """(x, lens, fp32 CPU h, float64 pred at control 1, its first-order bound, fp32 CPU pred): computed once per (case, predictor)"""
    key = (case_id(case), which)
    if key not in _DATA:
        config, B, S = case[:3]
        w = pred_weights(config, which)
        x = x_of(B, S, w["w1"].shape[1], seed=B * S + len(which))
        lens = lens_of(case)
        h = stage1(x, w, torch.float32)
        ref, bound = tail_ref(h, w, lens)
        if len(_DATA) > 6:
            _DATA.clear()
        _DATA[key] = (x, lens, h, ref, bound, tail_fp32(h, w, lens))
    return _DATA[key]


@pytest.mark.parametrize("which", ["pitch", "energy"])
@pytest.mark.parametrize("case", by_config(GATE_CASES), ids=case_id)
def test_pred_gate_passes_fp32_and_rejects_wrong_variants(case, which):
    w = pred_weights(case[0], which)
    x, lens, h, ref, bound, p32 = case_data(case, which)
    good = E.pred_check(p32, ref, bound, PRED_TIGHT)
    live = bound > 0
    print(f"\npred {case_id(case)} {which}: fp32 CPU {good.worst * PRED_TIGHT:.3g} of the first-order bound = {good.worst:.3g} x gate; "
          f"bound / |pred| median {float((bound[live] / ref[live].abs().clamp_min(1e-30)).median()):.2e}")
    assert good.ok and good.worst <= 1 / 8, str(good)
    assert torch.equal(_tail64(h, w, lens), ref)
    for name, y in _mutants(h, w, lens, ref).items():
        bad = E.pred_check(y, ref, bound, PRED_TIGHT)
        print(f"  {name}: {bad.worst:.3g} x gate")
        assert not bad.ok and bad.worst > 1, (name, str(bad))
    # control: applied without a target, not applied with one
    for c in CONTROLS[1:]:
        for given in (False, True):
            r, bd = tail_ref(h, w, lens, c, given)
            assert E.pred_check(tail_fp32(h, w, lens, c, given), r, bd, PRED_TIGHT).ok
            wrong = E.pred_check(_tail64(h, w, lens, c, not given), r, bd, PRED_TIGHT)
            print(f"  control {c} {'applied although a target is given' if given else 'not applied without a target'}: {wrong.worst:.3g} x gate")
            assert not wrong.ok and wrong.worst > 100
    # masked rows: bitwise +0.0 in the float64 reference and in the fp32 evaluation, at every control
    dead = ~(torch.arange(case[2])[None, :] < torch.tensor(lens)[:, None])
    assert bool(dead.any())
    for c in CONTROLS:
        z = tail_fp32(h, w, lens, c)[dead]
        assert bool((z.view(torch.int32) == 0).all())
    neg = p32.clone()
    neg[dead] = -0.0
    assert E.pred_check(neg, ref, bound, PRED_TIGHT).ok  # (the gate cannot see the sign of a zero: the GPU test compares the bits)


def _tight_from(share):
    """8 x share rounded UP to one significant digit"""
    v = 8 * share
    e = np.floor(np.log10(v))
    return float(np.ceil(v / 10 ** e - 1e-9) * 10 ** e)


def test_pred_tight_is_eight_times_the_fp32_share():
    """PRED_TIGHT restated from its definition on the cases of up to 6377 rows (largest share 2.93e-4); with NS_PRED_ALL_CASES=1 on
    every case (largest 3.09e-4, recorded in the module docstring): the same constant either way"""
    import os

    cases = [c for c in PRED_CASES if c[4] == "fused" and (os.environ.get("NS_PRED_ALL_CASES") or c[1] * c[2] <= 6377)]
    worst = 0.0
    for case in by_config(cases):
        for which in ("pitch", "energy"):
            x, lens, h, ref, bound, p32 = case_data(case, which)
            share = E.pred_check(p32, ref, bound, 1.0).worst
            print(f"\nfp32 CPU share {case_id(case)} {which}: {share:.3g}", end="")
            worst = max(worst, share)
    print(f"\nlargest {worst:.3g} -> PRED_TIGHT {_tight_from(worst):g}")
    assert _tight_from(worst) == PRED_TIGHT


# ---------------------------------------------------------------------------------------------------- input preconditions
@pytest.mark.parametrize("case", by_config([c for c in PRED_CASES if c[4] == "fused" and c[1] * c[2] >= 99 and c[1] * c[2] <= 6377]), ids=case_id)
def test_predictions_spread_over_the_buckets(case):
    """what the embedding check relies on: at control 1 the float64 predictions of the synthetic weights on N(0, 1) rows reach many
    buckets and both end buckets (at least 40 distinct below 1000 rows, 150 from 1000 rows), counted with every row valid"""
    for which in ("pitch", "energy"):
        w = pred_weights(case[0], which)
        x, lens, h, ref, bound, p32 = case_data(case, which)
        full, _ = tail_ref(h, w, [case[2]] * case[1])  # every row valid (a padded row predicts 0: the bottom bucket)
        idx = torch.bucketize(full.float(), w["bins"])
        n = int(idx.unique().numel())
        ends = [float((idx == e).double().mean()) for e in (0, w["bins"].numel())]
        print(f"\n{case_id(case)} {which}: {n} distinct buckets, end buckets {ends[0]:.3f} / {ends[1]:.3f} of the rows", end="")
        assert n >= (40 if case[1] * case[2] < 1000 else 150) and min(ends) > 0


def test_embed_ref_and_targets():
    """the targets hold every edge, its neighbours, both ends beyond, NaN and the infinities; bucketize puts them where
    model/modules.py's torch.bucketize does; the sum is (x + emb) + pos in that order"""
    w = pred_weights("tiny", "pitch")
    bins = w["bins"]
    t = targets_of(bins, 3, 343, seed=1)
    flat = t.reshape(-1)
    for v in (bins, torch.nextafter(bins, torch.tensor(np.inf)), torch.nextafter(bins, torch.tensor(-np.inf))):
        assert bool(torch.isin(v, flat).all())
    assert bool(torch.isnan(flat).any()) and bool((flat == np.inf).any()) and bool((flat == -np.inf).any())
    assert bool((flat < bins[0]).any()) and bool((flat > bins[-1]).any())
    idx = torch.bucketize(flat, bins)
    assert int(idx.min()) == 0 and int(idx.max()) == bins.numel() and idx.unique().numel() == bins.numel() + 1
    assert bool((idx[torch.isnan(flat)] == bins.numel()).all())
    small = targets_of(bins, 5, 1, seed=2)
    assert small.shape == (5, 1)
    x = x_of(3, 343, 256, seed=3)
    a = embed_ref(x, t, bins, w["emb"], w["pos"])
    assert torch.equal(a[1, 5], (x[1, 5] + w["emb"][idx.reshape(3, 343)[1, 5]]) + w["pos"][5])
    assert not torch.equal(a, x + (w["emb"][idx.reshape(3, 343)] + w["pos"][None, :343]))  # the other order is other bits


# ---------------------------------------------------------------------------------------------------- refusals (no device work)
def test_predictor_ops_refuse_bad_arguments_before_any_device_work():
    """unknown prefix, null arguments and an embedding on the duration predictor are refused on a machine without a GPU, on a
    handle whose weights were never loaded: nothing was looked up on, copied to or launched on a device"""
    import ctypes as C

    import smart_nar_fast_tts_amd._lib as L
    import smart_nar_fast_tts_amd.workload as wl
    from smart_nar_fast_tts_amd.model import config_struct

    so = L.load()
    h = C.c_void_p()
    assert so.ns_create(C.byref(config_struct(wl.preprocess_config(), wl.model_config("tiny"))), C.byref(h)) == 0
    buf = (C.c_float * 1024)()
    lens = (C.c_int64 * 1)(1)
    p = C.cast(buf, C.c_void_p)
    lp = C.cast(lens, C.c_void_p)
    err = lambda: so.ns_last_error().decode()  # noqa: E731
    pitch, dur = b"variance_adaptor.pitch_predictor", b"variance_adaptor.duration_predictor"
    try:
        assert so.ns_op_predictor_conv1(None, pitch, p, 1, 1, p, p, 4096, None) != 0 and "null model" in err()
        assert so.ns_op_predictor_conv1(h, b"variance_adaptor.pitch", p, 1, 1, p, p, 4096, None) != 0 and "unknown predictor prefix" in err()
        assert so.ns_op_predictor_conv1(h, None, p, 1, 1, p, p, 4096, None) != 0 and "unknown predictor prefix" in err()
        for args in ((None, 1, 1, p, p), (p, 1, 1, None, p), (p, 1, 1, p, None)):
            assert so.ns_op_predictor_conv1(h, pitch, *args, 4096, None) != 0 and "null argument" in err()
        assert so.ns_op_predictor_conv1(h, pitch, p, 1, 1, p, p, 4096, None) != 0 and "weights not loaded" in err()

        def tail(prefix, hid=p, ln=lp, target=None, x_in=None, add_pos=0, pred=p, x_out=None, ws=p, m=h):
            return so.ns_op_predictor_tail(m, prefix, hid, ln, 1, 1, 1.0, target, x_in, add_pos, pred, x_out, ws, 4096, None)

        assert tail(pitch, m=None) != 0 and "null model" in err()
        assert tail(b"variance_adaptor.pitch_predictor.conv_layer") != 0 and "unknown predictor prefix" in err()
        for kw in (dict(hid=None), dict(ln=None), dict(pred=None), dict(ws=None)):
            assert tail(pitch, **kw) != 0 and "null argument" in err(), kw
        for kw in (dict(x_in=p, x_out=p), dict(x_out=p), dict(add_pos=1)):
            assert tail(dur, **kw) != 0 and "duration predictor has no embedding" in err(), kw
        assert tail(pitch, x_in=p) != 0 and "x_in without x_out" in err()
        assert tail(pitch, x_out=p) != 0 and "without x_in" in err()
        assert tail(pitch, add_pos=1) != 0 and "without x_in" in err()
        for prefix, kw in ((pitch, dict(x_in=p, x_out=p, add_pos=1, target=p)), (dur, {}), (b"variance_adaptor.energy_predictor", dict(x_in=p, x_out=p))):
            assert tail(prefix, **kw) != 0 and "weights not loaded" in err()
    finally:
        so.ns_destroy(h)
