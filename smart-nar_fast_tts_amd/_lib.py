"""ctypes binding of ``csrc/libnarfs2.so`` (C-ABI: ``include/nar_fs2.h``).

There is no CPU fallback: if the library is missing or a symbol is absent the
import fails loudly.  ``torch`` is imported first on purpose — it brings its own
``libamdhip64.so.7`` and the library must bind to that same HIP runtime so that
torch's device pointers and streams are valid in our launches.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL: one HIP runtime per process)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnarfs2.so")


class NsConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_vocab", "max_seq_len", "d_enc", "n_enc_layer", "n_enc_head", "d_dec", "n_dec_layer", "n_dec_head",
        "d_inner", "ffn_k1", "ffn_k2", "vp_filter", "vp_kernel", "n_bins", "n_mel",
        "postnet_dim", "postnet_k", "postnet_n", "pitch_frame_level", "energy_frame_level", "length_regulator",
        "matmul_bf16x3", "row_epilogue", "phase1_packing")]


class NsLossArgs(C.Structure):
    """``ns_loss_args`` (include/nar_fs2.h): sizes, the two feature levels, the two strides, then the device pointers."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "L", "T", "H", "n_mel", "pitch_frame_level", "energy_frame_level")]
                + [(n, C.c_int64) for n in ("mel_targets_stride", "d_targets_stride")]
                + [(n, C.c_void_p) for n in ("mel", "postnet", "mel_targets", "mel_masks", "pitch", "pitch_targets", "energy", "energy_targets",
                                             "log_d", "d_targets", "src_masks", "src_lens", "mel_lens")]
                + [("attn", C.c_void_p * 4)])


class NsLossgGrads(C.Structure):
    """``ns_lossg_grads`` (include/nar_fs2.h): the nine nullable outputs of ``ns_lossg_backward``."""
    _fields_ = [(n, C.c_void_p) for n in ("mel", "postnet", "pitch", "energy", "log_d")] + [("attn", C.c_void_p * 4)]


class NsVtState(C.Structure):
    """``ns_vt_state`` (include/nar_fs2.h): index 0 pitch, 1 energy."""
    _fields_ = [(n, C.c_double * 2) for n in ("count", "mean", "m2", "min", "max")]


class NsVtArgs(C.Structure):
    """``ns_vt_args`` (include/nar_fs2.h): sizes, the feature levels and normalization flags, the stride, then the device pointers."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "L", "T", "pitch_frame_level", "energy_frame_level", "pitch_normalization", "energy_normalization")]
                + [("durations_stride", C.c_int64)]
                + [(n, C.c_void_p) for n in ("pitch", "energy", "durations", "src_lens", "pitch_targets", "energy_targets", "frame_lens", "valid")])


class NsOptTensor(C.Structure):
    """``ns_opt_tensor`` (include/nar_fs2.h): one row of the chunk table."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("numel", C.c_int64), ("state_offset", C.c_int64), ("lag", C.c_int32), ("chunk_begin", C.c_int32)]


class NsOptPlan(C.Structure):
    """``ns_opt_plan`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int64) for n in ("n_tensors", "n_chunks", "table_bytes", "ws_bytes", "state_floats")]


class NsOptRecord(C.Structure):
    """``ns_opt_record`` (include/nar_fs2.h)."""
    _fields_ = [("norm64", C.c_double), ("total_norm", C.c_float), ("clip_coef", C.c_float)]


class NsOptHyper(C.Structure):
    """``ns_opt_hyper`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + [("global_step", C.c_int64), ("fuse_clip", C.c_int32), ("zero_grads", C.c_int32)]


class NsPgShape(C.Structure):
    """``ns_pg_shape`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "S", "Cin", "F", "K")]


PG_NAMES = ("w1", "b1", "ln1_g", "ln1_b", "w2", "b2", "ln2_g", "ln2_b", "wlin", "blin")


class NsPgWeights(C.Structure):
    """``ns_pg_weights`` (include/nar_fs2.h): the ten parameters in checkpoint layout."""
    _fields_ = [(n, C.c_void_p) for n in PG_NAMES]


class NsPgGrads(C.Structure):
    """``ns_pg_grads`` (include/nar_fs2.h): the ten parameter gradients and ``dx``, each nullable."""
    _fields_ = [(n, C.c_void_p) for n in PG_NAMES + ("dx",)]


class NsAgShape(C.Structure):
    """``ns_ag_shape`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "S", "d", "H")]


AG_NAMES = ("wq", "bq", "wk", "bk", "wv", "bv", "wfc", "bfc", "ln_g", "ln_b")


class NsAgWeights(C.Structure):
    """``ns_ag_weights`` (include/nar_fs2.h): the ten parameters in checkpoint layout."""
    _fields_ = [(n, C.c_void_p) for n in AG_NAMES]


class NsAgGrads(C.Structure):
    """``ns_ag_grads`` (include/nar_fs2.h): the ten parameter gradients and ``dx``, each nullable."""
    _fields_ = [(n, C.c_void_p) for n in AG_NAMES + ("dx",)]


class NsXgShape(C.Structure):
    """``ns_xg_shape`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "L", "d", "H")]


class NsXgWeights(C.Structure):
    """``ns_xg_weights`` (include/nar_fs2.h): the ten parameters in checkpoint layout, named as ``ns_ag_weights``."""
    _fields_ = [(n, C.c_void_p) for n in AG_NAMES]


class NsXgGrads(C.Structure):
    """``ns_xg_grads`` (include/nar_fs2.h): the ten parameter gradients, ``dtgt`` and ``dsrc``, each nullable."""
    _fields_ = [(n, C.c_void_p) for n in AG_NAMES + ("dtgt", "dsrc")]


class NsPnShape(C.Structure):
    """``ns_pn_shape`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "n_mel", "emb", "K", "n")]


PN_MAX_LAYERS = 5
PN_PARAMS = ("w", "b", "gamma", "beta")                                   # per layer, the order of ns_pn_layer_grads
PN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")       # what follows them in ns_pn_layer


class NsPnWeights(C.Structure):
    """``ns_pn_weights`` (include/nar_fs2.h): five ``ns_pn_layer`` blocks, flattened as ``w0, b0, gamma0, ..., num_batches_tracked4``."""
    _fields_ = [(f"{n}{i}", C.c_void_p) for i in range(PN_MAX_LAYERS) for n in PN_PARAMS + PN_BUFFERS]


class NsPnGrads(C.Structure):
    """``ns_pn_grads`` (include/nar_fs2.h): five ``ns_pn_layer_grads`` blocks flattened the same way, then ``dx``; each nullable."""
    _fields_ = [(f"{n}{i}", C.c_void_p) for i in range(PN_MAX_LAYERS) for n in PN_PARAMS] + [("dx", C.c_void_p)]


class NsFgShape(C.Structure):
    """``ns_fg_shape`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "S", "d", "d_inner", "K1", "K2")]


FG_NAMES = ("w1", "b1", "w2", "b2", "ln_g", "ln_b")


class NsFgWeights(C.Structure):
    """``ns_fg_weights`` (include/nar_fs2.h): the six parameters in checkpoint layout."""
    _fields_ = [(n, C.c_void_p) for n in FG_NAMES]


class NsFgGrads(C.Structure):
    """``ns_fg_grads`` (include/nar_fs2.h): the six parameter gradients and ``dx``, each nullable."""
    _fields_ = [(n, C.c_void_p) for n in FG_NAMES + ("dx",)]


class NsMeShape(C.Structure):
    """``ns_me_shape`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "n_mel", "d")]


ME_NAMES = ("w1", "b1", "w2", "b2")


class NsMeWeights(C.Structure):
    """``ns_me_weights`` (include/nar_fs2.h): the Prenet's four parameters in checkpoint layout."""
    _fields_ = [(n, C.c_void_p) for n in ME_NAMES]


class NsMeGrads(C.Structure):
    """``ns_me_grads`` (include/nar_fs2.h): ``dmels`` and the four parameter gradients, each nullable."""
    _fields_ = [(n, C.c_void_p) for n in ("dmels",) + ME_NAMES]


class NsMhShape(C.Structure):
    """``ns_mh_shape`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "d", "n_mel")]


MH_NAMES = ("w", "b")


class NsMhWeights(C.Structure):
    """``ns_mh_weights`` (include/nar_fs2.h): ``mel_linear``'s two parameters in checkpoint layout."""
    _fields_ = [(n, C.c_void_p) for n in MH_NAMES]


class NsMhGrads(C.Structure):
    """``ns_mh_grads`` (include/nar_fs2.h): ``dx`` and the two parameter gradients, each nullable."""
    _fields_ = [(n, C.c_void_p) for n in ("dx",) + MH_NAMES]


class NsKmMask(C.Structure):
    """``ns_km_mask`` (include/nar_fs2.h): one mask of a keep-mask draw."""
    _fields_ = [("n", C.c_uint64), ("stream", C.c_uint32), ("thr", C.c_uint32)]


class NsMelConfig(C.Structure):
    """``ns_mel_config`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("filter_length", "hop_length", "win_length", "n_mel")] + [("clip_val", C.c_float)]


class NsGlConfig(C.Structure):
    """``ns_gl_config`` (include/nar_fs2.h)."""
    _fields_ = [(n, C.c_int32) for n in ("filter_length", "hop_length", "win_length", "n_mel")] + [("spec_from_mel_scaling", C.c_float)]


_P, _I, _F, _Z, _S = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_char_p


def _handle_family(prefix: str, config_ptr) -> dict:
    """The life cycle every native handle has (csrc/host_core.h; driven by _handle.NativeHandle); ``config_ptr`` is what
    ``{prefix}_create`` takes for its config struct."""
    return {
        f"{prefix}_abi_version": (_I, []),
        f"{prefix}_create": (_I, [config_ptr, C.POINTER(_P)]),
        f"{prefix}_destroy": (None, [_P]),
        f"{prefix}_arena_bytes": (_Z, [_P]),
        f"{prefix}_bind_arena": (_I, [_P, _P, _Z]),
        f"{prefix}_set_weight": (_I, [_P, _S, _P, C.POINTER(C.c_int64), _I]),
        f"{prefix}_check_weight": (_I, [_P, _S, C.POINTER(C.c_int64), _I]),
        f"{prefix}_finalize_weights": (_I, [_P, _P]),
    }


# name -> (restype, argtypes); must list every symbol include/nar_fs2.h declares
SIGNATURES = {
    "ns_last_error": (C.c_char_p, []),
    **_handle_family("ns", C.POINTER(NsConfig)),
    "ns_adopt_arena": (_I, [_P]),
    "ns_encoder_ws_bytes": (_Z, [_P, _I, _I]),
    "ns_decoder_ws_bytes": (_Z, [_P, _I, _I, _I]),
    "ns_forward_durations": (_I, [_P, _P, _P, _I, _I, _F, _F, _F, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ns_forward_durations_packed": (_I, [_P, _P, _P, _P, _I, _I, _F, _F, _F, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ns_forward_durations_teacher": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _Z, _P, _Z, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ns_last_phase1_rows": (C.c_int64, [_P]),
    "ns_upload_lengths": (_I, [_P, _I, _P, _P]),
    "ns_forward_mel": (_I, [_P, _I, _I, _I, _P, _F, _F, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P, _P]),
    "ns_forward_mel_packed": (_I, [_P, _I, _I, _I, _P, _P, _F, _F, _P, _P, _P, _P, _Z, _P, _P, _P, _P, _P, _P, _P]),

    "ns_last_phase2_rows": (C.c_int64, [_P]),
    "ns_plan_gemm": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "ns_plan_gemm_launches": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "ns_plan_row_tile": (_I, [_I, _I]),
    "ns_plan_row_tile_k": (_I, [_I, _I, _I]),
    "ns_acc_chunk": (_I, []),
    "ns_plan_attention_split": (_I, [_I, _I, _I, _I]),
    "ns_op_ws_bytes": (_Z, [_P, _I, _I]),
    "ns_op_mask_from_lengths": (_I, [_P, _I, _I, _P, _P]),
    "ns_op_sinusoid_table": (_I, [_I, _I, _P, _P]),
    "ns_op_txt_encoder": (_I, [_P, _P, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_multi_head_attention": (_I, [_P, _S, _P, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_positionwise_ffn": (_I, [_P, _S, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_fft_block": (_I, [_P, _S, _P, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_variance_predictor": (_I, [_P, _S, _P, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_predictor_conv1": (_I, [_P, _S, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_predictor_tail": (_I, [_P, _S, _P, _P, _I, _I, _F, _P, _P, _I, _P, _P, _P, _Z, _P]),
    "ns_op_duration_round": (_I, [_P, _I, _F, _P, _P]),
    "ns_op_duration_scan": (_I, [_P, _I, _I, _P, _P, _P]),
    "ns_op_duration_target_scan": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "ns_op_length_regulate": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "ns_op_variance_embedding": (_I, [_P, _I, _P, _P, _I, _I, _F, _P, _P, _P, _P, _Z, _P]),
    "ns_op_bucketize": (_I, [_P, _I, _P, _I, _P, _P]),
    "ns_op_gaussian_upsampling": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "ns_op_mel_decoder": (_I, [_P, _P, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_mel_linear": (_I, [_P, _P, _I, _I, _P, _P]),
    "ns_op_postnet": (_I, [_P, _P, _I, _I, _P, _P, _Z, _P]),
    "ns_op_ffn_conv1": (_I, [_P, _S, _P, _I, _I, _P, _P]),
    "ns_op_attention_core": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "ns_op_attention_core_mode": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _Z, _P, _I]),
    "ns_op_attention_carve": (_I, [_I, _I, _I, _Z, _I, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "ns_plan_attention_dense": (_I, [_I, _I, _I, _I, _Z, _I, C.POINTER(C.c_int32)]),
    "ns_op_gemm": (_I, [_P, _S, _P, _I, _I, _P, _P]),
    "ns_plan_gemm_bf16": (_I, [_I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ns_plan_gemm_bf16_ln": (_I, [_I, _I, _I, _I]),
    "ns_plan_gemm_b3": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "ns_op_attention_scratch_bytes": (_Z, [_I, _I, _I, _I]),
    # packed-row test hooks: (plan, B, S, Mp, att_wgs) after the tensors
    "ns_op_pack_plan": (_I, [_P, _P, _I, _I, _I, _I, _P, _Z, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "ns_op_gemm_packed": (_I, [_P, _S, _P, _P, _I, _I, _I, _I, _P, _P]),
    "ns_op_attention_core_packed": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P, _I]),
    "ns_op_attention_packed_carve": (_I, [_I, _I, _I, _Z, _I, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "ns_plan_attention_packed": (_I, [_I, _I, _I, _I, _I, _I, _Z, _I, C.POINTER(C.c_int32)]),
    "ns_plan_attention_split_packed": (_I, [_I, _I, _I, _I, _I]),
    "ns_op_block_packed": (_I, [_P, _I, _S, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "ns_op_length_regulate_packed": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "ns_op_gaussian_regulate": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P]),
    "ns_op_embed_pos_packed": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "ns_op_add_pos_packed": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "ns_op_pack_vector": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "ns_op_unpack_rows": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "ns_op_unpack_phase1": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "ns_op_unpack_outputs": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ns_profile_enable": (_I, [_P, _I]),
    "ns_profile_read": (_I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "ns_profile_read_slot": (_I, [_P, _I, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    # HiFi-GAN vocoder (vocoder.py; the config pointer is a vocoder.NsVocConfig)
    **_handle_family("ns_voc", _P),
    "ns_voc_set_matmul": (_I, [_P, _I]),
    "ns_voc_ws_bytes": (_Z, [_P, _I, _I]),
    "ns_voc_forward": (_I, [_P, _P, _I, _I, _I, _P, _P, _Z, _P]),
    "ns_voc_op_conv": (_I, [_P, _S, _P, _I, _I, _P, _P]),
    "ns_voc_op_conv_form": (_I, [_P, _S, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ns_voc_op_upsample": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "ns_voc_op_stage_ws_bytes": (_Z, [_P, _I, _I, _I]),
    "ns_voc_op_stage": (_I, [_P, _I, _P, _I, _I, _P, _P, _Z, _P]),
    # reference-mel aligner (model.FastSpeech2Align.align; the config pointer is the model's NsConfig)
    **_handle_family("ns_aln", C.POINTER(NsConfig)),
    "ns_aln_ws_bytes": (_Z, [_P, _I, _I, _I]),
    "ns_aln_forward": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "ns_aln_op_cross_attention": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "ns_aln_op_input": (_I, [_P, _P, _I, _I, _I, _P]),
    "ns_aln_op_durations": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    # validation loss (loss.FastSpeech2Loss; handle-less)
    "ns_loss_abi_version": (_I, []),
    "ns_loss_ws_bytes": (_Z, [_I, _I, _I]),
    "ns_loss_forward": (_I, [C.POINTER(NsLossArgs), _P, _Z, _P, _P]),
    # wave-to-mel front end (audio.TacotronSTFT)
    **_handle_family("ns_mel", C.POINTER(NsMelConfig)),
    "ns_mel_frames": (C.c_int64, [C.c_int64, C.c_int32]),
    "ns_mel_ws_bytes": (_Z, [_P, _I, C.c_int64]),
    "ns_mel_forward": (_I, [_P, _P, C.c_int64, _P, _I, C.c_int64, _I, _P, _P, _P, _P, _Z, _P]),
    "ns_mel_op_frame_rows": (_I, [_P, _P, C.c_int64, _P, _I, C.c_int64, _I, _P, _P, _P]),
    "ns_mel_op_stft": (_I, [_P, _P, _I, _I, _P, _P]),
    "ns_mel_op_project": (_I, [_P, _P, _P, _I, _I, C.c_int64, _I, _P, _P, _P]),
    # Griffin-Lim mel-to-wave (audio.STFT, audio.griffin_lim, audio.mel_to_wave)
    **_handle_family("ns_gl", C.POINTER(NsGlConfig)),
    "ns_gl_ws_bytes": (_Z, [_P, _I, _I]),
    "ns_gl_forward": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, C.c_int64, _P, _P, _Z, _P]),
    "ns_gl_forward_mag": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, C.c_int64, _P, _P, _Z, _P]),
    "ns_gl_transform": (_I, [_P, _P, C.c_int64, _P, _I, C.c_int64, _I, _P, _P, _P, _Z, _P]),
    "ns_gl_op_mel_to_mag": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "ns_gl_op_recombine": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "ns_gl_op_rephase": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "ns_gl_op_inverse": (_I, [_P, _P, _P, _I, _I, _P, C.c_int64, _P, _P, _Z, _P]),
    "ns_gl_op_frame_rows": (_I, [_P, _P, C.c_int64, _P, _I, C.c_int64, _I, _P, _P]),
    "ns_gl_op_step": (_I, [_P, _P, _P, _I, _I, _P, C.c_int64, _P, _P, _Z, _P]),
    # variance targets and dataset statistics (targets.VarianceTargets; handle-less)
    "ns_vt_abi_version": (_I, []),
    "ns_vt_ws_bytes": (_Z, [_I, _I, _I]),
    "ns_vt_state_init": (_I, [_P, _P]),
    "ns_vt_targets": (_I, [C.POINTER(NsVtArgs), _P, _Z, _P]),
    "ns_vt_fit": (_I, [C.POINTER(NsVtArgs), _P, _P, _Z, _P]),
    "ns_vt_normalize": (_I, [C.POINTER(NsVtArgs), _P, _P, _Z, _P]),
    # clip_grad_norm_ + Adam + zero_grad (optim.Adam, optim.ScheduledOptim; handle-less)
    "ns_opt_abi_version": (_I, []),
    "ns_opt_plan_sizes": (_I, [C.POINTER(C.c_int64), _I, C.POINTER(NsOptPlan)]),
    "ns_opt_build_table": (_I, [C.POINTER(C.c_int64), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32), _I, _P, _Z]),
    "ns_opt_grad_norm": (_I, [C.POINTER(NsOptPlan), _P, _Z, _F, _P, _Z, _P, _P]),
    "ns_opt_scale_grads": (_I, [C.POINTER(NsOptPlan), _P, _Z, _P, _P]),
    "ns_opt_adam_step": (_I, [C.POINTER(NsOptPlan), _P, _Z, C.POINTER(NsOptHyper), _P, _P, C.c_int64, _P, _P]),
    "ns_opt_zero_grads": (_I, [C.POINTER(NsOptPlan), _P, _Z, _P]),
    # training loss: value with the record of its counts, and the backward (loss.FastSpeech2TrainingLoss; handle-less)
    "ns_lossg_abi_version": (_I, []),
    "ns_lossg_record_bytes": (_Z, []),
    "ns_lossg_forward": (_I, [C.POINTER(NsLossArgs), _P, _Z, _P, _P, _P]),
    "ns_lossg_backward": (_I, [C.POINTER(NsLossArgs), _P, _P, C.POINTER(NsLossgGrads), _P]),
    # VariancePredictor training forward and backward (predictor.VariancePredictor; handle-less)
    "ns_pg_abi_version": (_I, []),
    "ns_pg_plan_wgrad": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "ns_pg_ws_bytes": (_Z, [C.POINTER(NsPgShape)]),
    "ns_pg_saved_bytes": (_Z, [C.POINTER(NsPgShape)]),
    "ns_pg_last_launches": (_I, []),
    "ns_pg_forward": (_I, [C.POINTER(NsPgShape), C.POINTER(NsPgWeights), _P, _P, _P, _P, _F, _P, _P, _P, _Z, _P]),
    "ns_pg_backward": (_I, [C.POINTER(NsPgShape), C.POINTER(NsPgWeights), _P, _P, _P, _P, _F, _P, _P, C.POINTER(NsPgGrads), _P, _Z, _P]),
    "ns_pg_op_wgrad": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "ns_pg_op_dgrad": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "ns_pg_op_row_backward": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    # MultiHeadAttention (self-attention) training forward and backward (sublayers.MultiHeadAttention; handle-less)
    "ns_ag_abi_version": (_I, []),
    "ns_ag_ws_bytes": (_Z, [C.POINTER(NsAgShape)]),
    "ns_ag_saved_bytes": (_Z, [C.POINTER(NsAgShape)]),
    "ns_ag_last_launches": (_I, []),
    "ns_ag_forward": (_I, [C.POINTER(NsAgShape), C.POINTER(NsAgWeights), _P, _P, _P, _F, _P, _P, _P, _Z, _P]),
    "ns_ag_backward": (_I, [C.POINTER(NsAgShape), C.POINTER(NsAgWeights), _P, _P, _P, _F, _P, _P, C.POINTER(NsAgGrads), _P, _Z, _P]),
    "ns_ag_op_lse": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "ns_ag_op_attention_backward": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "ns_ag_op_row_backward": (_I, [_P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P, _Z, _P]),
    # MultiHeadAttention as cross-attention, training forward and backward (sublayers.MultiHeadCrossAttention; handle-less)
    "ns_xg_abi_version": (_I, []),
    "ns_xg_ws_bytes": (_Z, [C.POINTER(NsXgShape)]),
    "ns_xg_saved_bytes": (_Z, [C.POINTER(NsXgShape)]),
    "ns_xg_kv_splits": (_I, [C.POINTER(NsXgShape)]),
    "ns_xg_last_launches": (_I, []),
    "ns_xg_forward": (_I, [C.POINTER(NsXgShape), C.POINTER(NsXgWeights), _P, _P, _P, _P, _F, _P, _P, _P, _P, _Z, _P]),
    "ns_xg_backward": (_I, [C.POINTER(NsXgShape), C.POINTER(NsXgWeights), _P, _P, _P, _P, _F, _P, _P, _P, _P, C.POINTER(NsXgGrads), _P, _Z, _P]),
    "ns_xg_op_attention_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    # PostNet with train-mode BatchNorm, training forward and backward (postnet.PostNet; handle-less)
    "ns_pn_abi_version": (_I, []),
    "ns_pn_ws_bytes": (_Z, [C.POINTER(NsPnShape)]),
    "ns_pn_saved_bytes": (_Z, [C.POINTER(NsPnShape)]),
    "ns_pn_last_launches": (_I, []),
    "ns_pn_forward": (_I, [C.POINTER(NsPnShape), C.POINTER(NsPnWeights), _I, _P, C.POINTER(_P), _F, _P, _P, _P, _Z, _P]),
    "ns_pn_backward": (_I, [C.POINTER(NsPnShape), C.POINTER(NsPnWeights), _I, _P, C.POINTER(_P), _F, _P, _P, C.POINTER(NsPnGrads), _P, _Z, _P]),
    "ns_pn_op_stats": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    "ns_pn_op_apply": (_I, [_P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P]),
    "ns_pn_op_bwd_reduce": (_I, [_P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "ns_pn_op_bwd_apply": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "ns_pn_op_wgrad_narrow": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    # VarianceAdaptor: variance embedding and length regulator, forward and backward (adaptor.py; handle-less)
    "ns_va_abi_version": (_I, []),
    "ns_va_last_launches": (_I, []),
    "ns_va_plan_embed": (_I, [_I, _I, _I, C.POINTER(C.c_int32)]),
    "ns_va_embed_ws_bytes": (_Z, [_I, _I, _I]),
    "ns_va_op_embed_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "ns_va_op_embed_bwd": (_I, [_P, _P, _I, _I, _I, _P, _P, _Z, _P]),
    "ns_va_op_lr_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "ns_va_op_lr_bwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    # PositionwiseFeedForward training forward and backward (sublayers.PositionwiseFeedForward; handle-less)
    "ns_fg_abi_version": (_I, []),
    "ns_fg_ws_bytes": (_Z, [C.POINTER(NsFgShape)]),
    "ns_fg_saved_bytes": (_Z, [C.POINTER(NsFgShape)]),
    "ns_fg_last_launches": (_I, []),
    "ns_fg_forward": (_I, [C.POINTER(NsFgShape), C.POINTER(NsFgWeights), _P, _P, _F, _P, _P, _P, _Z, _P]),
    "ns_fg_backward": (_I, [C.POINTER(NsFgShape), C.POINTER(NsFgWeights), _P, _P, _F, _P, _P, C.POINTER(NsFgGrads), _P, _Z, _P]),
    "ns_fg_op_relu_gate": (_I, [_P, _P, _I, _I, _P, _P, _P, _Z, _P]),
    # what the TxtEncoder / MelDecoder training stacks add to their FFT blocks (stacks.py; handle-less, no workspace)
    "ns_st_abi_version": (_I, []),
    "ns_st_last_launches": (_I, []),
    "ns_st_op_embed_pos": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "ns_st_op_add_pos": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "ns_st_op_embed_grad": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "ns_st_op_row_mask": (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    # MelEncoder: the Prenet and the position add, training forward and backward (sublayers.Prenet; handle-less)
    "ns_me_abi_version": (_I, []),
    "ns_me_ws_bytes": (_Z, [C.POINTER(NsMeShape)]),
    "ns_me_saved_bytes": (_Z, [C.POINTER(NsMeShape)]),
    "ns_me_last_launches": (_I, []),
    "ns_me_forward": (_I, [C.POINTER(NsMeShape), C.POINTER(NsMeWeights), _P, _P, _P, _F, _P, _P, _P, _Z, _P]),
    "ns_me_backward": (_I, [C.POINTER(NsMeShape), C.POINTER(NsMeWeights), _P, _F, _P, _P, C.POINTER(NsMeGrads), _P, _Z, _P]),
    "ns_me_op_drop_pos": (_I, [_P, _P, _P, _F, _I, _I, _I, _P, _P]),
    "ns_me_op_drop_relu_gate": (_I, [_P, _P, _P, _F, _I, _I, _P, _P, _P, _Z, _P]),
    # mel head: mel_linear and the PostNet residual, training forward and backward (sublayers.MelLinear, training.add_residual; handle-less)
    "ns_mh_abi_version": (_I, []),
    "ns_mh_ws_bytes": (_Z, [C.POINTER(NsMhShape)]),
    "ns_mh_last_launches": (_I, []),
    "ns_mh_forward": (_I, [C.POINTER(NsMhShape), C.POINTER(NsMhWeights), _P, _P, _P, _Z, _P]),
    "ns_mh_backward": (_I, [C.POINTER(NsMhShape), C.POINTER(NsMhWeights), _P, _P, C.POINTER(NsMhGrads), _P, _Z, _P]),
    "ns_mh_op_pad_colsum": (_I, [_P, _I, _I, _P, _P, _P, _Z, _P]),
    "ns_mh_op_residual": (_I, [_P, _P, _I, _I, _P, _P]),
    # dropout keep-masks from a counter-based generator, one launch per draw (dropout.KeepMaskRNG; handle-less)
    "ns_km_abi_version": (_I, []),
    "ns_km_last_launches": (_I, []),
    "ns_km_threshold": (_I, [C.c_double, C.POINTER(C.c_uint32)]),
    "ns_km_table_bytes": (_Z, [_I]),
    "ns_km_plan": (_I, [C.POINTER(NsKmMask), _I, _P, _Z, C.POINTER(C.c_uint64)]),
    "ns_km_draw": (_I, [_P, _I, C.c_uint64, C.c_uint64, _P, _Z, _P]),
    "ns_km_op_philox": (_I, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "ns_km_host_draw": (_I, [_P, _I, C.c_uint64, C.c_uint64, _P, _Z]),
}
KM_MAX_MASKS, KM_GRID_CAP, KM_TABLE_ROW_BYTES = 1024, 2048, 32  # include/nar_fs2.h NS_KM_*

STATUS_TRUNCATED, STATUS_BAD_TOKEN = 1, 2  # include/nar_fs2.h NS_STATUS_*

_lib = None


def load():
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().ns_last_error()
        raise RuntimeError(f"{what}: {msg.decode() if msg else 'error'} (rc={rc})")


def ptr(t) -> C.c_void_p:
    """Device (or host) pointer of a contiguous tensor; None -> NULL."""
    if t is None:
        return C.c_void_p(0)
    assert t.is_contiguous(), "tensor must be contiguous"
    return C.c_void_p(t.data_ptr())


def stream_ptr(device=None) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
