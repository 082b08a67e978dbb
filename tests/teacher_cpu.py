"""Torch-CPU restatement of the reference's teacher-forced branch — ``FastSpeech2Align.forward`` with ``mel_lens`` given, in
``eval()`` (model/fastspeech2_align.py:44-100, model/modules.py:102-159 with ``duration_target``) — in the dtype of the weights it is
given (fp32 or float64).  Built from ``oracle.fs2_oracle``'s functions and ``tests/aligner_cpu.py``; the reference's undefined
``_calculate_duration`` (:57) is the duration rule of DESIGN.md §12 (``aligner_cpu.durations``).  Written from the reference's
behaviour, with line citations; no reference text is copied."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import fs2_oracle as orc
from tests import aligner_cpu as ac

NAMES = ("output", "postnet_output", "p_predictions", "e_predictions", "log_d_predictions", "d_rounded", "src_masks", "mel_masks",
         "src_lens", "mel_lens", "tgt_alignment", "d_targets")


def forward(w, model_cfg, texts, src_lens, mels, mel_lens, p_targets=None, e_targets=None, p_control=1.0, e_control=1.0,
            pitch_level="frame_level", energy_level="frame_level", d_targets=None):
    """The 12-tuple in the reference's order (NAMES).  ``d_targets`` (int64 [B,L], optional) overrides the durations computed from
    the alignment, so that two evaluations can be made to differ in arithmetic only.  Slot 7 is the reference's own mask, built
    from the INPUT ``mel_lens`` (fastspeech2_align.py:47-51); slot 9 is the length regulator's count (modules.py:129)."""
    t = model_cfg["transformer"]
    msl = model_cfg["max_seq_len"]
    L, T = texts.shape[1], mels.shape[1]
    src_masks = orc.get_mask_from_lengths(src_lens, L)
    mel_masks = orc.get_mask_from_lengths(mel_lens, T)
    x = orc.txt_encoder(w, texts, src_masks, t["encoder_head"], msl)
    # :56-58 — the MelEncoder sees the encoder output itself, before any variance embedding is added to it
    _, alignment = ac.mel_encoder(w, x, mels, src_masks, mel_masks, t["decoder_head"], msl)
    if d_targets is None:
        d_targets = torch.from_numpy(ac.durations(alignment[-1].numpy(), src_lens.numpy(), mel_lens.numpy()))
    log_d = orc.variance_predictor(w, "variance_adaptor.duration_predictor", x, src_masks)  # modules.py:116: computed all the same
    if pitch_level == "phoneme_level":
        p_pred, emb = orc.variance_embedding(w, "pitch", x, src_masks, p_control, p_targets)
        x = x + emb
    if energy_level == "phoneme_level":
        e_pred, emb = orc.variance_embedding(w, "energy", x, src_masks, e_control, e_targets)
        x = x + emb
    x, out_lens = orc.length_regulate(x, d_targets, T)  # modules.py:128-130; max_len = max_mel_len = T
    if pitch_level == "frame_level":
        p_pred, emb = orc.variance_embedding(w, "pitch", x, mel_masks, p_control, p_targets)
        x = x + emb
    if energy_level == "frame_level":
        e_pred, emb = orc.variance_embedding(w, "energy", x, mel_masks, e_control, e_targets)
        x = x + emb
    x = orc.mel_decoder(w, x, mel_masks, t["decoder_head"], msl)
    mel = F.linear(x, w["mel_linear.weight"], w["mel_linear.bias"])
    post = orc.postnet(w, mel) + mel
    return (mel, post, p_pred, e_pred, log_d, d_targets, src_masks, mel_masks, src_lens, out_lens, alignment, d_targets)


def target_scan(d_targets, src_lens, texts=None, n_vocab=0):
    """numpy statement of the phase-1 tail of the teacher-forced forward (include/nar_fs2.h ns_op_duration_target_scan): from int64
    durations [B,L] -> (cum int32 — inclusive prefix sums of max(d, 0), model/modules.py:221-223 —, dur_keep float32 = d, src_mask
    = l >= src_len, mel_lens int64 = the totals, or -1 for an utterance that holds a token id outside [0, n_vocab))."""
    d = np.asarray(d_targets, dtype=np.int64)
    B, L = d.shape
    cum = np.cumsum(np.maximum(d, 0), axis=1)
    mel_lens = cum[:, -1].astype(np.int64) if L else np.zeros(B, dtype=np.int64)
    if texts is not None:
        tx = np.asarray(texts)
        mel_lens = np.where(((tx < 0) | (tx >= n_vocab)).any(axis=1), -1, mel_lens).astype(np.int64)
    src_mask = np.arange(L)[None, :] >= np.asarray(src_lens)[:, None]
    return cum.astype(np.int32), d.astype(np.float32), src_mask, mel_lens


def fixture_levels(meta):
    return meta.get("pitch", "frame_level"), meta.get("energy", "frame_level")


def check_durations(attn_last, d_targets, meta, z):
    """d_targets of an evaluation whose last-layer alignment is ``attn_last`` (numpy [B,H,T,L]) against the fixture.  A fixture whose
    aligner seed met the maker's bar (meta["exact_durations"]: the smallest float64 top-two gap is >= 1000 x the fp32-vs-float64
    distance of the head-summed map) demands exact equality.  Otherwise the rule of test_durations (tests/test_gpu_aligner.py): a
    frame's argmax may differ from float64's only where the float64 top-two gap is below 1e-6, at most 1 % of the frames may —
    and when none does, the durations are the fixture's.  Returns the number of differing frames."""
    d_targets = np.asarray(d_targets)
    if meta["exact_durations"]:
        assert np.array_equal(d_targets, z["d_targets"])
        return 0
    sl, ml = z["src_lens"], z["mel_lens"]
    a = ac.head_sum(np.asarray(attn_last))
    idx = np.concatenate([a[b, :ml[b], :sl[b]].argmax(axis=1) for b in range(a.shape[0])])
    bad = idx != z["argmax_f64"]
    assert (z["top2_gap_f64"][bad] < 1e-6).all(), "an argmax differs from float64's where the float64 row has a clear peak"
    assert bad.sum() <= 0.01 * bad.size
    if not bad.any():
        assert np.array_equal(d_targets, z["d_targets"])
    return int(bad.sum())
