/*
 * nar_fs2.h — C ABI of the MI355X-native FastSpeech2 inference forward.
 *
 * The reference (SMART-TTS/SMART-NAR_Fast_TTS) has no FFI / plugin layer: its
 * boundary for this path is the Python class FastSpeech2Align
 * (model/fastspeech2_align.py:13-100).  This header is the C-ABI a binding for
 * that class sits on: plain pointers and sizes, an explicit hipStream_t passed
 * as void*, int status returns (0 = ok; the Python side raises RuntimeError
 * with ns_last_error()).  The library allocates NO device memory: weights live
 * in a caller-provided arena and every call takes a caller-provided workspace
 * (PyTorch is only the allocator / stream owner on the Python side).
 *
 * THREADING.  One ns_model serves ONE host thread at a time: the model carries per-call state — the measurement slots of
 * ns_profile_enable and the row counts ns_last_phase1_rows / ns_last_phase2_rows report — that a forward writes while it
 * enqueues its launches (everything else a forward needs, the packed-row context included, lives in the caller's
 * workspaces).  Calls on the same model from two host threads must be serialised by the caller; different models (one per
 * thread, or one per process as bench.py does per GPU) are independent, and one thread may drive several HIP streams
 * with one model as long as each stream has its own workspaces.  ns_last_error() is per thread.  This matches the
 * reference's caller: single-threaded, synchronous, one module instance (synthesize.py:59-76).
 *
 * All tensors are dense row-major float32 unless stated; token ids and lengths
 * are int64 (what torch.long hands over); masks are uint8 with 1 = padding
 * (utils/tools.py:89-97: True = padding).
 */
#ifndef NAR_FS2_H
#define NAR_FS2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's contract, returned by ns_abi_version(): 6 = ns_plan_row_tile_k, ns_acc_chunk, ns_abi_version;
 * 5 = ns_plan_gemm writes out[8] (round 5; unversioned then). */
#define NS_ABI_VERSION 6

typedef struct ns_model ns_model;

/* Mirrors the keys FastSpeech2Align.__init__ reads from model.yaml / preprocess.yaml
 * (model/fastspeech2_align.py:16-28, model/modules.py:20-77, transformer/Models.py:36-71,176-210)
 * plus the sizes the reference hard-codes (PostNet 80/512/k5/x5: transformer/Layers.py:112-118). */
typedef struct ns_config {
  int32_t n_vocab;          /* len(symbols)+1 = 361, transformer/Models.py:40 */
  int32_t max_seq_len;      /* 1000 */
  int32_t d_enc, n_enc_layer, n_enc_head;
  int32_t d_dec, n_dec_layer, n_dec_head;
  int32_t d_inner;          /* conv_filter_size 1024 */
  int32_t ffn_k1, ffn_k2;   /* conv_kernel_size [9, 1] */
  int32_t vp_filter, vp_kernel; /* variance_predictor 256 / 3 */
  int32_t n_bins;           /* 256 */
  int32_t n_mel;            /* 80 */
  int32_t postnet_dim, postnet_k, postnet_n; /* 512, 5, 5 */
  int32_t pitch_frame_level, energy_frame_level; /* 1 = frame_level (shipped config), 0 = phoneme_level */
  int32_t length_regulator; /* 0 = LengthRegulator (what the reference wires, model/modules.py:22); 1 = EXTENSION: the
                               reference's unused GaussianUpsampling (model/modules.py:162-192) in its place */
  int32_t matmul_bf16x3;    /* 0 = every contraction on the fp32 matrix cores (the default, the reference's arithmetic);
                               1 = OPT-IN: the decoder stack's projections / FFN convolutions and the PostNet 512->512
                               convolutions (downstream of every discrete duration / bucket decision; only launches large
                               enough to fill the chip with 64..256-row tiles, smaller ones stay fp32) run from an exact
                               3-way bf16 split of both operands on the bf16 matrix cores, 6 products, fp32 accumulation:
                               fp32-sized error, different bits, ~1.6x faster on those layers (csrc/gemm_bf16x3.hip).
                               "fp32-sized" is held per launch form against float64, on random-sign and on same-sign
                               operands: |y - f64| <= 4e-6 * (conv(|x|, |w|) + |bias|) (tests/test_gpu_bf16x3_ops.py);
                               2 = OPT-IN "bf16": every contraction from the decoder input through the PostNet output
                               (decoder QKV, Q K^T, P V, fc, FFN w_1 / w_2, mel_linear, all five PostNet convolutions) takes
                               both operands rounded to bf16 (nearest even) and accumulates in fp32 on the bf16 matrix cores,
                               at every launch size; bias, activations, residuals, LayerNorm, softmax stay fp32.  Everything
                               upstream (encoder, durations, length regulator, pitch / energy) is the exact fp32 path, so
                               durations, frame counts, masks and predictions are bit-identical to mode 0; mel deviates from
                               the fp32 reference by ~1e-2 max / ~1e-3 mean (csrc/gemm_bf16.hip, csrc/attention.hip).
                               Adds one bf16 plane per covered weight to the arena.  Any other value is rejected. */
  int32_t row_epilogue;     /* 0 = the default: on small grids LayerNorm / the predictor tail / attention's key-range merge run as
                               TICKETED last-arriver epilogues inside the producing launch (csrc/gemm_conv.hip TICKET,
                               csrc/attention.hip); 1 = "two_launch": the same row functions as separate launches, no ticket is
                               ever drawn.  Same bits either way — the switch exists so that tests can A/B the ticket protocol
                               (tests/test_gpu_stress.py).  The full-row tile of large launches needs no ticket and is not affected */
  int32_t phase1_packing;   /* ns_forward_durations_packed: 0 = auto — pack the phoneme rows when >= 10 % of the [B, L] grid is padding AND the
                               smaller row count gives the fullest CU fewer rows of the phase's dominant launch (a whole round of its 32-row
                               K-split tile less, or one round of the 48-row form instead of two of the 32-row one); 1 = pack whenever >= 10 % is padding (tests exercise the path on small shapes);
                               2 = never */
} ns_config;

/* ---- lifetime ------------------------------------------------------------------------------ */
const char* ns_last_error(void);
int ns_create(const ns_config* cfg, ns_model** out);
void ns_destroy(ns_model* m);

/* Bytes of device memory the prepared weights need; the caller allocates it (torch.empty) and binds it.
 * The arena is position independent (offsets only), so rank 0 can fill it and RCCL-broadcast the bytes. */
size_t ns_arena_bytes(const ns_model* m);
int ns_bind_arena(ns_model* m, void* dev_arena, size_t bytes);

/* load_state_dict(): one call per state-dict entry, reference key names and torch-native layouts
 * (Linear [out,in], Conv1d [out,in,k]; utils/model.py:21-22).  `host` is HOST memory.  Unknown
 * "mel_encoder.*" keys and "*.num_batches_tracked" are accepted and ignored (returns 0);
 * any other unknown key or a shape mismatch is an error. */
int ns_set_weight(ns_model* m, const char* name, const float* host, const int64_t* shape, int ndim);
/* The same key / rank / shape validation WITHOUT touching the model (nothing staged, a loaded model stays loaded):
 * load_state_dict() checks every entry with this first, so that a rejected state dict leaves the previous weights in use
 * (nn.Module.load_state_dict raises before/without corrupting the module, utils/model.py:21-22). */
int ns_check_weight(ns_model* m, const char* name, const int64_t* shape, int ndim);
/* After the last ns_set_weight: repack (conv [out,in,k] -> [out,k,in]; fused QKV), fold eval-mode
 * BatchNorm into the PostNet convs, upload into the arena.  Fails if an inference key is missing.
 * Success releases the staged host copies: a second call without staging every key again returns non-zero
 * ("missing keys: ...") and leaves the model ready on the arena it already has. */
int ns_finalize_weights(ns_model* m, void* stream);
/* Non-root ranks: arena bytes arrived by broadcast; mark the model ready without ns_set_weight. */
int ns_adopt_arena(ns_model* m);

/* ---- the forward: model/fastspeech2_align.py:30-100, inference branch -------------------------- */
size_t ns_encoder_ws_bytes(const ns_model* m, int B, int L);
size_t ns_decoder_ws_bytes(const ns_model* m, int B, int L, int T);

/* Phase 1: get_mask_from_lengths + TxtEncoder + duration predictor + rounding + duration scan.
 * Writes log_d [B,L], d_rounded [B,L] (float32, may hold -0.0), src_mask [B,L], mel_lens [B] (int64).
 * The encoder output and the duration prefix sums stay in ws_enc for phase 2.
 * mel_lens_host (nullable): device-visible HOST memory (hipHostMalloc / a pinned torch tensor), [B] int64; the kernel that
 * produces mel_lens writes a second copy there, so the caller's read needs only a stream synchronisation, no D2H copy.
 * A token id outside [0, n_vocab) (nn.Embedding raises IndexError, transformer/Models.py:89) is reported as
 * mel_lens[b] = -1 for its utterance; the kernels read embedding row 0 for it, nothing out of bounds.
 * The caller reads mel_lens back (the one unavoidable device->host read: the output tensors are
 * shaped by max(mel_lens), model/modules.py:136-137) and allocates the phase-2 outputs. */
/* phoneme_level pitch / energy (preprocess.yaml `feature`, model/modules.py:117-126) are predicted here, on the
 * encoder output: p_control / e_control / p_targets / e_targets / p_pred / e_pred ([B,L]) are used by THIS call for a
 * phoneme_level feature and by ns_forward_mel ([B,T]) for a frame_level one; pass NULL where not applicable. */
int ns_forward_durations(ns_model* m, const int64_t* texts, const int64_t* src_lens, int B, int L,
                         float d_control, float p_control, float e_control, const float* p_targets, const float* e_targets,
                         void* ws_enc, size_t ws_enc_bytes,
                         float* log_d, float* d_rounded, uint8_t* src_mask, int64_t* mel_lens, float* p_pred, float* e_pred,
                         int64_t* mel_lens_host, void* stream);
/* The same with the HOST copy of src_lens (what a caller that builds its batches on the host has anyway: dataset.py:182-191,
 * utils/tools.py:254-264): ragged phoneme counts then run phase 1 on PACKED phoneme rows — utterance b keeps
 * min(src_lens[b] + 2, L) rows instead of L (transformer/Models.py:73-100 computes, then zeroes, every padded phoneme) — when that
 * saves >= 10 % of the rows and both variance features are frame_level.  Same outputs, padded like the reference's; values agree
 * with ns_forward_durations to fp32 summation order (another row count picks other tiles on the small-grid ladder).
 * ns_last_phase1_rows: the row count the most recent phase 1 ran on (B*L, or the packed rows). */
int ns_forward_durations_packed(ns_model* m, const int64_t* texts, const int64_t* src_lens, const int64_t* src_lens_host, int B, int L,
                                float d_control, float p_control, float e_control, const float* p_targets, const float* e_targets,
                                void* ws_enc, size_t ws_enc_bytes,
                                float* log_d, float* d_rounded, uint8_t* src_mask, int64_t* mel_lens, float* p_pred, float* e_pred,
                                int64_t* mel_lens_host, void* stream);
int64_t ns_last_phase1_rows(const ns_model* m);
/* Phase 1 of the TEACHER-FORCED branch (model/fastspeech2_align.py:44,53-58,70-80 with mel_lens given; model/modules.py:128-130):
 * the recording's own alignment drives the length regulator.  In this order, on `stream`:
 *   1. TxtEncoder -> enc_out in ws_enc                                                (fastspeech2_align.py:53)
 *   2. ns_aln_forward(aln, enc_out, src_lens, mels, mel_lens_in, ...) -> tgt_output [B,T,d], attn_all_layers [n_layer,B,H,T,L],
 *      d_targets [B,L] int64 — the duration rule stated with ns_aln_forward below, the stand-in for the reference's undefined
 *      _calculate_duration                                                            (fastspeech2_align.py:56-58)
 *   3. duration predictor -> log_d [B,L] (still computed, model/modules.py:116)
 *   4. phoneme_level pitch / energy, which add their embeddings into enc_out IN PLACE (model/modules.py:117-126): the aligner
 *      must have read enc_out before this step — fastspeech2_align.py:53-56 hands it the encoder's output itself
 *   5. one launch: src_mask, and from d_targets what ns_forward_mel reads out of ws_enc — the prefix sums of max(d, 0)
 *      (model/modules.py:221-223), the float copy of d — and mel_lens[b] = sum_i max(d_targets[b,i], 0), or -1 for a token id outside
 *      [0, n_vocab) exactly as ns_forward_durations reports it.
 * The text encoder runs once.  Always exact fp32, whatever ns_config.matmul_bf16x3 says.  T = mels' frame axis is known up front, so
 * ns_forward_mel(m, B, L, T, mel_lens, ...) can be enqueued right behind this call with no host read; sum d <= T, so its
 * NS_STATUS_TRUNCATED bit is never set.  T == 0: no aligner launch, d_targets = 0 (mels, mel_lens_in, tgt_output, attn_all_layers and
 * ws_aln may be NULL then).  Dense [B,L] grid only: packed phase-1 rows (ns_forward_durations_packed) are out of scope for this
 * path.  There is no d_rounded output: the reference returns duration_target in that slot (model/modules.py:130), i.e. d_targets.
 * ws_enc >= ns_encoder_ws_bytes(m, B, L), ws_aln >= ns_aln_ws_bytes(aln, B, L, T), both 256-byte aligned; mels 16-byte aligned.
 * `aln` must have been created from the same ns_config as `m` (ns_aln_create). */
typedef struct ns_aligner ns_aligner;
int ns_forward_durations_teacher(ns_model* m, ns_aligner* aln, const int64_t* texts, const int64_t* src_lens, const float* mels,
                                 const int64_t* mel_lens_in, int B, int L, int T, float p_control, float e_control,
                                 const float* p_targets, const float* e_targets, void* ws_enc, size_t ws_enc_bytes, void* ws_aln,
                                 size_t ws_aln_bytes, float* log_d, uint8_t* src_mask, int64_t* mel_lens, float* p_pred, float* e_pred,
                                 float* tgt_output, float* attn_all_layers, int64_t* d_targets, void* stream);
/* Helper for callers whose lengths live on the host: dev[i] = host[i] (int64) on `stream`, the values riding in a kernel's
 * argument block — one ~3 us launch, no copy command (a pinned-staging async copy of these 128 bytes costs a forward ~35 us of
 * blit + stream dependency, a pageable copy ~80 us).  host is read before the call returns. */
int ns_upload_lengths(const int64_t* host, int n, int64_t* dev, void* stream);

/* Phase 2: LengthRegulator + frame-level pitch/energy + MelDecoder + mel_linear + PostNet (+ residual).
 * T is max(mel_lens), or a caller-chosen capacity (max_mel_len, model/modules.py:128-131,204-213 semantics: the mel axis is
 * padded and masked to it).  mel_lens stays on the device: a caller that fixes T up front can enqueue this call right
 * behind ns_forward_durations with NO host read in between (capacity mode).
 * Writes mel [B,T,n_mel], postnet_mel [B,T,n_mel], p_pred [B,T], e_pred [B,T], mel_mask [B,T] and
 * status [B] (int32, device or pinned host memory, REQUIRED): per utterance a bit set of
 *   NS_STATUS_TRUNCATED  mel_lens[b] > T: the frames past T were cut off (the rest of the row is still well defined)
 *   NS_STATUS_BAD_TOKEN  phase 1 reported a token id outside [0, n_vocab) for this utterance (mel_lens[b] = -1)
 * so that neither condition can pass silently when the caller never reads mel_lens before this call. */
#define NS_STATUS_TRUNCATED 1
#define NS_STATUS_BAD_TOKEN 2
/* p_targets / e_targets ([B,T], nullable): forward()'s p_targets / e_targets — when given, the embedding is
 * taken from bucketize(target) and the prediction is returned unscaled (model/modules.py:82-84,93-95). */
int ns_forward_mel(ns_model* m, int B, int L, int T, const int64_t* mel_lens, float p_control, float e_control,
                   const float* p_targets, const float* e_targets, const void* ws_enc, void* ws_dec, size_t ws_dec_bytes,
                   float* mel, float* postnet_mel, float* p_pred, float* e_pred, uint8_t* mel_mask, int32_t* status, void* stream);

/* Phase 2 on PACKED rows, for variable-length batches.  The reference computes every frame of the padded [B, T] grid and then
 * zeroes or ignores the frames past each utterance's length (transformer/Layers.py:43,46, model/modules.py:283-284); this
 * entry point keeps, per utterance, only a window of min(mel_lens[b] + 20, T) frames, lays the windows end to end and runs the
 * same kernels on sum(windows) rows instead of B*T.  Same arguments, same padded outputs: valid frames are computed by the
 * same arithmetic (they differ from ns_forward_mel's only by fp32 summation order where a launch picks another tile shape for
 * the smaller problem), padded frames are rebuilt — mel = the mel_linear bias, predictions 0, PostNet frames within 10 of an
 * utterance's end computed, all others constants of the weights (the PostNet has no mask between its layers).
 * mel_lens_host: the caller's HOST copy of mel_lens (what ns_forward_durations wrote to its mel_lens_host): the row count of
 * the launches comes from it, so this is the synchronous path's entry point.  The call falls back to the dense grid by
 * itself when packing does not apply (bf16x3 mode) or saves less than 10 % of the rows (20 % on grids of up to 20 000 rows, where the grid is one full round of the tallest tile). */
int ns_forward_mel_packed(ns_model* m, int B, int L, int T, const int64_t* mel_lens, const int64_t* mel_lens_host,
                          float p_control, float e_control, const float* p_targets, const float* e_targets, const void* ws_enc,
                          void* ws_dec, size_t ws_dec_bytes, float* mel, float* postnet_mel, float* p_pred, float* e_pred,
                          uint8_t* mel_mask, int32_t* status, void* stream);
/* Activation rows phase 2 of the most recent ns_forward_mel / ns_forward_mel_packed call on this model ran on: B*T on the
 * dense grid, the sum of the windows when packed (measurement / tests). */
int64_t ns_last_phase2_rows(const ns_model* m);

/* ---- per-operator entry points (the rows of SURVEY.md §8a; used by the parity tests and by bench.py's
 *      dominant-kernel timing).  `prefix` is the reference module path, e.g.
 *      "mel_decoder.layer_stack.0.slf_attn".  lens[b] = valid length of utterance b (keys/rows >= it are padding). */
size_t ns_op_ws_bytes(const ns_model* m, int B, int S);
/* a1  utils/tools.py:89-97 */
int ns_op_mask_from_lengths(const int64_t* lens, int B, int max_len, uint8_t* mask, void* stream);
/* a2  transformer/Models.py:10-30 */
int ns_op_sinusoid_table(int n_position, int d_hid, float* out, void* stream);
/* a3  transformer/Models.py:73-100 */
int ns_op_txt_encoder(ns_model* m, const int64_t* texts, const int64_t* lens, int B, int L, float* out, void* ws, size_t ws_bytes, void* stream);
/* a4+a5  transformer/SubLayers.py:29-59, transformer/Modules.py:14-25 */
int ns_op_multi_head_attention(ns_model* m, const char* prefix, const float* x, const int64_t* lens, int B, int S, float* out, void* ws, size_t ws_bytes, void* stream);
/* a6  transformer/SubLayers.py:87-95 */
int ns_op_positionwise_ffn(ns_model* m, const char* prefix, const float* x, int B, int S, float* out, void* ws, size_t ws_bytes, void* stream);
/* a7  transformer/Layers.py:39-48 */
int ns_op_fft_block(ns_model* m, const char* prefix, const float* x, const int64_t* lens, int B, int S, float* out, void* ws, size_t ws_bytes, void* stream);
/* a8  model/modules.py:278-286 */
int ns_op_variance_predictor(ns_model* m, const char* prefix, const float* x, const int64_t* lens, int B, int S, float* out, void* ws, size_t ws_bytes, void* stream);
/* a8 as its two launches, for tests that hold one contraction plus its row epilogue to a reference.  Both choose the full-row
 * tile / the ticketed ladder / the two-launch form exactly as the forward does (row count and the model's row_epilogue setting).
 * ns_op_predictor_conv1: h [B*S, filter] = layer_norm_1(relu(conv1d_1(x))), x [B*S, d].
 * ns_op_predictor_tail: from a hidden tensor h [B*S, filter] the caller supplies, pred [B*S] = masked_fill(linear(layer_norm_2(
 * relu(conv1d_2(h))))) (* control when target is NULL).  With x_in [B*S, d] (pitch / energy predictors only; the duration predictor
 * refuses it) x_out = x_in + embedding[bucketize(target ? target : pred)] (unmasked), and with add_pos != 0 also + the decoder
 * position row of each frame (the cached table up to max_seq_len, the regenerated one beyond: what the last frame-level embedding
 * of the forward adds).  x_out / add_pos need x_in.  Unknown prefixes and null arguments are refused before any device work. */
int ns_op_predictor_conv1(ns_model* m, const char* prefix, const float* x, int B, int S, float* h, void* ws, size_t ws_bytes, void* stream);
int ns_op_predictor_tail(ns_model* m, const char* prefix, const float* h, const int64_t* lens, int B, int S, float control,
                         const float* target /* nullable */, const float* x_in /* nullable: no embedding */, int add_pos, float* pred,
                         float* x_out /* with x_in */, void* ws, size_t ws_bytes, void* stream);
/* a9  model/modules.py:132-135 */
int ns_op_duration_round(const float* log_d, int n, float d_control, float* d_rounded, void* stream);
/* a10 model/modules.py:201-230 + utils/tools.py:288-306: step 1 prefix sums + mel_lens, step 2 gather to [B,T,D] */
int ns_op_duration_scan(const float* d_rounded, int B, int L, int32_t* cum, int64_t* mel_lens, void* stream);
/* a10 with GIVEN durations (model/modules.py:128-130, the teacher-forced branch; step 5 of ns_forward_durations_teacher alone):
 * d_targets [B,L] int64 -> cum [B,L] int32 inclusive prefix sums of max(d, 0) (:221-223), dur_keep [B,L] = (float)d, src_mask [B,L]
 * = l >= src_lens[b] (utils/tools.py:89-97), mel_lens[b] = the total — or -1 when texts (nullable: no check) holds an id outside
 * [0, n_vocab) in utterance b.  One launch, one workgroup per utterance. */
int ns_op_duration_target_scan(const int64_t* d_targets, const int64_t* src_lens, const int64_t* texts /* nullable */, int n_vocab, int B, int L,
                               int32_t* cum, float* dur_keep, uint8_t* src_mask, int64_t* mel_lens, void* stream);
int ns_op_length_regulate(const float* x, const int32_t* cum, int B, int L, int D, int T, float* out, void* stream);
/* a11 model/modules.py:80-100,139-149: which = 0 pitch, 1 energy; x_out = x + embedding[bucketize(pred*control)] (unmasked add) */
int ns_op_variance_embedding(ns_model* m, int which, const float* x, const int64_t* lens, int B, int S, float control, const float* target /* nullable */, float* pred, float* x_out, void* ws, size_t ws_bytes, void* stream);
/* a11 torch.bucketize(values, bins, right=False) as called at model/modules.py:86-88,97-99 (the same device routine
 * the fused ns_op_variance_embedding kernel uses); idx[i] in [0, n_edges] */
int ns_op_bucketize(const float* values, int n, const float* bins, int n_edges, int64_t* idx, void* stream);
/* a12 model/modules.py:166-192 (dead code in the reference forward): out [B,T_out,D] (rows >= T zero),
 * w [B,L,T] (may be NULL), s: B*(L+1) floats — s[0..B) = sum of durations, the rest is scratch for the Gaussian centres */
int ns_op_gaussian_upsampling(const float* x, const float* durations, int B, int L, int D, int T, int T_out, float* out, float* s, float* w, void* stream);
/* a13 transformer/Models.py:212-244 */
int ns_op_mel_decoder(ns_model* m, const float* x, const int64_t* lens, int B, int T, float* out, void* ws, size_t ws_bytes, void* stream);
/* a14 model/fastspeech2_align.py:24-27,83 */
int ns_op_mel_linear(ns_model* m, const float* x, int B, int T, float* out, void* stream);
/* a15 transformer/Layers.py:169-177 (returns postnet(x) WITHOUT the residual, like PostNet.forward) */
int ns_op_postnet(ns_model* m, const float* mel, int B, int T, float* out, void* ws, size_t ws_bytes, void* stream);

/* bench.py's roofline leg: launches only the dominant kernel (the FFN k=9 Conv1D-as-GEMM of `prefix`.w_1,
 * bias+ReLU epilogue) on [B,S,d] -> [B,S,d_inner]; flops = 2*B*S*k*d*d_inner. */
int ns_op_ffn_conv1(ns_model* m, const char* prefix, const float* x, int B, int S, float* hidden, void* stream);
/* a5 alone (transformer/Modules.py:14-25 on already projected heads): qkv [B*S, 3*H*dk] with columns [0,d) = Q,
 * [d,2d) = K, [2d,3d) = V (head h at h*dk inside each), out [B*S, H*dk] = merged heads of
 * softmax(Q K^T / sqrt(dk) + (-inf at keys >= lens[b])) V.  dk in {32, 64, 128}. */
/* scratch (nullable): device memory for the split-key path the kernel takes when a launch has few workgroups
 * (single-utterance latency); 8 * (B*S*H*dk + 2*B*S*H) floats always suffice. */
int ns_op_attention_core(const float* qkv, const int64_t* lens, int B, int S, int H, int dk, float* out, void* scratch,
                         size_t scratch_bytes, void* stream);
/* The same with flags chosen by the caller.  Bit 0: 0 is ns_op_attention_core, 1 the "bf16" mode's attention (Q K^T and P V from
 * operands rounded to bf16, fp32 softmax: the kernels a bf16 model's decoder layers run) — a caller that passed bf16 = 0 / 1 here
 * keeps its meaning.  Bit 1: withhold the ticket block the op carves from the end of `scratch` (split strips then merge their key
 * ranges by a k_attention_merge launch instead of by the last arriver).  Any other bit is refused. */
int ns_op_attention_core_mode(const float* qkv, const int64_t* lens, int B, int S, int H, int dk, float* out, void* scratch,
                              size_t scratch_bytes, void* stream, int flags);
/* host only: what ns_op_attention_core[_mode] makes of a scratch of scratch_bytes under `flags` (the op carves by this very
 * function): the floats left to the split-key partials, and whether a ticket block was taken from the end */
int ns_op_attention_carve(int B, int S, int H, size_t scratch_bytes, int flags, size_t* partial_floats, int32_t* has_tickets);
/* host only: what the dense (grid) attention launch of this shape does, answered by the function the launch dispatches on
 * (csrc/attention.hip attention_plan_dense).  out = {kernel: 0 k_attention_strip / 1 k_attention, key-range workgroups per 32-query
 * strip / per 128-query tile, merge: 0 none / 1 by the last arriver of a strip's workgroups (tickets) / 2 by a k_attention_merge
 * launch, 32-key tiles per wave of a strip / per key range of k_attention for an utterance of S keys}.  scratch_floats: floats of
 * scratch left to the partials (0 = none); has_tickets: a ticket block is handed over.  Follows NS_PLAN.  Bad shapes (B, S, H <= 0,
 * dk not 32 / 64 / 128, S * 3 * H * dk * 4 >= 2^31) and a null out are refused before anything else.  An addition: NS_ABI_VERSION
 * is unchanged. */
int ns_plan_attention_dense(int B, int S, int H, int dk, size_t scratch_floats, int has_tickets, int32_t out[4]);
/* One named contraction alone, for tests: x [B*S, Cin] -> out [B*S, N] on the dense grid (zero padding per utterance of S rows),
 * in the model's precision mode and through the forward's own dispatch, with bias and the layer's activation (ReLU for w_1, tanh
 * for every PostNet layer but the last) and neither residual nor LayerNorm.  name: "<layer prefix>.slf_attn.qkv" (N = 3 d: Q | K |
 * V), "<layer prefix>.slf_attn.fc", "<layer prefix>.pos_ffn.w_1", "<layer prefix>.pos_ffn.w_2", "mel_linear",
 * "postnet.convolutions.<i>" (BatchNorm folded); any other name is an error. */
int ns_op_gemm(ns_model* m, const char* name, const float* x, int B, int S, float* out, void* stream);

/* Introspection of the step-aware launch plan (csrc/gemm_conv.hip plan_rows, csrc/attention.hip plan_key_split); host-side, no GPU
 * needed.  ns_plan_gemm: how a plain Conv1D-as-GEMM of M rows, N output channels, kernel size KW over Cin input channels
 * (transformer/SubLayers.py:87-95 over an arbitrary B*T) is launched: out = {BM, BN, rows} of the main launch, {BM, BN, rows} of
 * the remainder launch (zeros: a single launch), the edge of the MFMA tile the launch(es) are built from — 32, or 16 for the 16-row
 * family whose tile HEIGHT (any multiple of 16) is chosen for the row count — and the cost model's estimate in microseconds.
 * Returns 1 when the planner covers the shape, 0 when it is left to the small-grid K-split ladder (few tiles) or the
 * narrow-channel rules (then out is zeroed).  All rows of one GEMM are summed in one order: a cut is only ever made between tiles
 * of the 32-row family, which share it, so it never shows in the bits.
 * ns_plan_row_tile: height of the full-row tile (GEMM + LayerNorm / predictor-tail epilogue, N = 256 or 512 = one activation
 * row) for M rows: 32, or 48 / 80 / 112 (16-row family) when that gives the fullest CU fewer rows; 0 for other widths.
 * ns_plan_attention_split: key ranges per 128-query tile of a dense attention launch (1 = none; 16 = the small-grid paths' own
 * sizing, the value the workspace is reserved for). */
int ns_plan_gemm(int M, int N, int Cin, int KW, int32_t out[8]);
/* Every launch the fp32 Conv1D-as-GEMM dispatch (csrc/gemm_conv.hip launch_conv_gemm) makes for M rows, N output channels, kernel
 * size KW over Cin input channels, answered by the dispatch itself with launching switched off — the planner's range, the small-grid
 * K-split ladder, the narrow-output (N = 80) and Cin = 80 rules and the row-epilogue launches alike.  epi: 0 = plain GEMM, 1 = GEMM +
 * LayerNorm on the full-row tile, 2 = GEMM + LayerNorm on the ticketed ladder (which of the two a model takes for a shape is its own
 * rule: full-row from ceil(M / 32) >= 200 row tiles, ticketed below).  Returns the number of launches, 0, 1 or 2 (0: the dispatch
 * refuses the shape; 2: main + remainder of a cut plan), and writes per launch {BM, BN, BK, KS, MF, ROWEPI, TICKET, rows}: tile rows
 * and columns, K step, in-workgroup K groups, MFMA tile edge (32 / 16), 1 for a full-row tile, ticketed row width / 256 (0 = not
 * ticketed), rows of the launch; unused entries are zero.  Host-side, no GPU needed; follows NS_PLAN and the other A/B switches. */
int ns_plan_gemm_launches(int M, int N, int Cin, int KW, int epi, int32_t out[2][8]);
int ns_plan_row_tile(int M, int N);            /* = ns_plan_row_tile_k(M, N, N): the attention output projection's contraction */
int ns_plan_row_tile_k(int M, int N, int K);   /* contraction length K = KW * Cin: K > 256 keeps to the heights with chunked accumulation */
/* k values per accumulation chunk of the long contractions (K > 256; csrc/gemm_conv.hip ACC2): partial sums of this many
 * products are formed from zero and then added to the running total, so that the matrix cores round against short sums.
 * 64 by default; NS_ACC_CHUNK in the environment (a multiple of 64, or 0 = one sequential sum per output: A/B runs). */
int ns_acc_chunk(void);
/* Version of this header's contract (NS_ABI_VERSION below): bumped whenever a signature, an output-array length or a struct
 * layout changes, so that a caller built against an older header can refuse to run instead of overrunning a buffer
 * (round 5 grew ns_plan_gemm's out[6] to out[8]). */
int ns_abi_version(void);
int ns_plan_attention_split(int B, int S, int H, int dk);
/* the tile (rows x columns: 256x256, 128x256, 64x128 or 64x64) a plain "bf16"-mode GEMM of M rows and N output channels is
 * launched with (csrc/gemm_bf16.hip conv_gemm_bf16_plan; every tile gives the same bits).  Host-side, no GPU needed. */
int ns_plan_gemm_bf16(int M, int N, int32_t* bm, int32_t* bn);
/* 1 when the "bf16"-mode GEMM + LayerNorm of M rows, N columns takes the 64 x 256 full-row LayerNorm tile, 0 when it runs the
 * plain GEMM followed by the row kernel (same bits either way). */
int ns_plan_gemm_bf16_ln(int M, int N, int Cin, int KW);
/* What a "bf16x3"-mode model does with a GEMM of M rows, N output channels, kernel size KW over Cin input channels whose weight
 * has the three bf16 planes (csrc/gemm_bf16x3.hip; answered by the functions the launch path itself calls).  epi 0: the plain
 * GEMM; epi 1: GEMM + LayerNorm.  Returns the number of bf16x3 launches, 1 or 0 (0: the exact-fp32 kernels take the launch — a
 * plain GEMM with fewer than 200 tiles of 128 x 256, a LayerNorm GEMM below the full-row thresholds, a shape the kernel does not
 * cover, or any other epi) and writes out = {BM, BN, ROWEPI, workgroups}: the 128 x 256 or 256 x 256 plain tile (256 rows once
 * that still gives 240 workgroups), or for epi 1 at N = 256 the 64 x 256 full-row tile with the LayerNorm epilogue (ROWEPI = 1;
 * from 200 such tiles).  epi 1 with ROWEPI = 0 is the two-launch form for widths the full-row tile does not cover (N = 512): the
 * plain bf16x3 GEMM described, followed by the LayerNorm row kernel.  out is zeroed when 0 is returned and may be NULL.
 * Host-side, no GPU needed. */
int ns_plan_gemm_b3(int M, int N, int Cin, int KW, int epi, int32_t out[4]);
/* bytes of scratch with which ns_op_attention_core[_mode] splits its keys exactly as a model's own attention of this shape
 * does (the partials its workspace reserves plus the op's ticket block); 0 = pass no scratch. */
size_t ns_op_attention_scratch_bytes(int B, int S, int H, int dk);

/* ---- Test hooks: one stage alone on PACKED rows (the default layout of ns_forward_mel_packed / ns_forward_durations_packed:
 * utterance b owns the Mp-row matrix's rows [off[b], off[b] + win[b]), win[b] = min(max(len[b], 0) + guard, S)).  Each entry goes
 * through the function the forwards call with a packed context; additions only, NS_ABI_VERSION is unchanged.  Every entry refuses
 * null or inconsistent arguments before any device work.
 *
 * ns_op_pack_plan: Mp = sum of the windows and att_wgs = sum of ceil(win / 128) * H, computed on the host from lens_host by the
 * forwards' own helpers; with lens_dev and plan_dev (both or neither) also the device plan, plan_ints >= 4 B + 4 + 3 Mp ints laid
 * out as  off [B+1] | win [B], 1 unused | att_off [B+1] | att_order [B], 1 unused | row_b [Mp] | row_t [Mp] | row_w [Mp]
 * (att_order: utterances by descending window, ties by index; att_off: exclusive scan of ceil(win / 128) * H in that order).
 * guard: 20 for frame rows, 2 for phoneme rows.  Every other entry takes the same (plan_dev, B, S, Mp, att_wgs). */
int ns_op_pack_plan(const int64_t* lens_dev, const int64_t* lens_host, int B, int S, int H, int guard, int32_t* plan_dev, size_t plan_ints,
                    int32_t* Mp, int32_t* att_wgs, void* stream);
/* ns_op_gemm on packed rows: x_p [Mp, Cin] -> out_p [Mp, N], zero padding at each window's own edges, the model's precision mode */
int ns_op_gemm_packed(ns_model* m, const char* name, const float* x_p, const int32_t* plan_dev, int B, int S, int Mp, int att_wgs, float* out_p,
                      void* stream);
/* ns_op_attention_core_mode on packed rows: qkv_p [Mp, 3 H dk] -> out_p [Mp, H dk]; keys of utterance b are its rows
 * t < min(lens[b], win[b]).  flags: bit 0 = the bf16 mode's kernels, bit 1 = withhold the ticket block carved from the end of
 * `scratch` (the strip form then merges its key ranges by a launch of its own). */
int ns_op_attention_core_packed(const float* qkv_p, const int64_t* lens, const int32_t* plan_dev, int B, int S, int Mp, int att_wgs, int H, int dk,
                                float* out_p, void* scratch /* nullable */, size_t scratch_bytes, void* stream, int flags);
/* host only: what ns_op_attention_core_packed makes of a scratch of scratch_bytes under `flags` (the op carves by this very function):
 * the floats left to the split-key partials, and whether a ticket block was taken from the end */
int ns_op_attention_packed_carve(int B, int S, int H, size_t scratch_bytes, int flags, size_t* partial_floats, int32_t* has_tickets);
/* host only: what the packed attention launch of this shape does, answered by the function the launch dispatches on.
 * out = {form: 0 strip kernel / 1 flat work list, key ranges per strip / per work-list workgroup, merge launch 0 / 1,
 * 32-key tiles per range of a window of S}.  scratch_floats: floats of scratch left to the partials (0 = none). */
int ns_plan_attention_packed(int B, int S, int H, int dk, int att_wgs, int Mp, size_t scratch_floats, int has_tickets, int32_t out[4]);
/* host only: the key ranges whose partials ns_op_block_packed and the packed forwards reserve on these rows (before the workspace's
 * size limits them): scratch for that many makes ns_op_attention_core_packed split as the block's own attention does */
int ns_plan_attention_split_packed(int att_wgs, int S, int H, int dk, int Mp);
/* which: 0 = ns_op_positionwise_ffn, 1 = ns_op_multi_head_attention, 2 = ns_op_fft_block on the packed rows of layer `prefix`
 * (the FFTBlock's own prefix for all three).  mask_rows != 0 zeroes the rows at t >= lens[b] (always for which = 2).  ws:
 * ns_op_ws_bytes(m, B, S) bytes. */
int ns_op_block_packed(ns_model* m, int which, const char* prefix, const float* x_p, const int64_t* lens /* nullable for an unmasked ffn */,
                       const int32_t* plan_dev, int B, int S, int Mp, int att_wgs, int mask_rows, float* out_p, void* ws, size_t ws_bytes,
                       void* stream);
/* The packed data movement, each launch alone.  ns_op_length_regulate_packed and ns_op_embed_pos_packed write row maps themselves
 * (the former builds the whole plan with guard 20; the latter needs off / win of a plan built before).  status nullable.
 * ns_op_unpack_outputs: mel_bias [n_mel], post_const [11, n_mel]; p_p / p_pred, e_p / e_pred and mel_mask are nullable. */
int ns_op_length_regulate_packed(const float* x, const int32_t* cum, const int64_t* mel_lens, int B, int L, int D, int T, int Mp, int H,
                                 float* out_p, int32_t* status, int32_t* plan_dev, size_t plan_ints, void* stream);
/* The Gaussian length regulator alone in the form ns_forward_mel / ns_forward_mel_packed launch it (T_out = T): own_len [B] int64 (frames
 * at or past it are zeros), status [B] (nullable) = (own_len > T) | 2 (own_len < 0), zero / nzero (nullable together: words zeroed by
 * the launch), plan_dev (nullable: null with Mp = att_wgs = 0 is the dense grid, out [B, T, D]; else out [Mp, D] on the rows of a plan
 * built by ns_op_pack_plan with guard 20).  s: B (L + 1) floats of scratch.  w [B, L, T] is nullable on the dense grid (the forwards
 * pass null) and refused with a plan. */
int ns_op_gaussian_regulate(const float* x, const float* durations, const int64_t* own_len, int B, int L, int D, int T, float* out, float* s,
                            float* w, int32_t* status, int32_t* zero, int nzero, const int32_t* plan_dev, int Mp, int att_wgs, void* stream);
int ns_op_embed_pos_packed(const int64_t* texts, const float* emb, const float* pos, const int32_t* plan_dev, int B, int L, int Mp, int att_wgs, int D,
                           int n_vocab, float* out_p, void* stream);
int ns_op_add_pos_packed(const float* x_p, const float* pos, const int32_t* plan_dev, int B, int S, int Mp, int att_wgs, int D, float* out_p,
                         void* stream);
int ns_op_pack_vector(const float* src, const int32_t* plan_dev, int B, int S, int Mp, int att_wgs, float* dst_p, void* stream);
int ns_op_unpack_rows(const float* src_p, const int64_t* lens /* nullable */, const int32_t* plan_dev, int B, int S, int Mp, int att_wgs, int D,
                      float* dst, void* stream);
int ns_op_unpack_phase1(const float* rows_p, const float* vec_p, const int64_t* lens, const int32_t* plan_dev, int B, int S, int Mp, int att_wgs,
                        int D, float* rows, float* vec, void* stream);
int ns_op_unpack_outputs(const int32_t* plan_dev, int B, int T, int Mp, int att_wgs, int n_mel, const int64_t* mel_lens, const float* mel_p,
                         const float* post_p, const float* p_p, const float* e_p, const float* mel_bias, const float* post_const, float* mel,
                         float* post, float* p_pred, float* e_pred, uint8_t* mel_mask, void* stream);

/* Measurement hook for bench.py's roofline legs: while enabled, the launches of the three heaviest kernels inside
 * ns_forward_mel carry hipEvents ON THEIR OWN DISPATCH PACKETS (hipExtLaunchKernel start / stop events: the kernel's begin and
 * end timestamps, no marker packet on the stream; a timed launch still costs the stream ~5 us, so bench.py times slot 0 inside
 * its timed region and the other two in a separate pass), one slot each:
 *   slot 0  the FFT blocks' k=9 Conv1D-as-GEMM (PositionwiseFeedForward.w_1, transformer/SubLayers.py:70-75; the dominant
 *           kernel): flops = 2*rows*k*d*d_inner per launch
 *   slot 1  the fused attention (transformer/Modules.py:14-25): flops = 4*rows*T*d per launch
 *   slot 2  the PostNet's 512->512 k=5 convolutions (transformer/Layers.py:120-152): flops = 2*rows*k*512*512 per launch
 * ns_profile_read_slot waits for the slot's events and returns the summed kernel time, the summed algorithmic flops and
 * the launch count, then resets the slot.  ns_profile_read is slot 0. */
#define NS_PROFILE_SLOTS 3
#define NS_PROFILE_OFF 0
#define NS_PROFILE_ALL 1
#define NS_PROFILE_SLOT(i) (2 << (i)) /* OR several together to time exactly those slots */
#define NS_PROFILE_KEEP 0x10000        /* OR into `on`: keep the events recorded so far (bench.py times every 5th forward of its
                                          timed region: NS_PROFILE_KEEP | NS_PROFILE_SLOT(0) on those, NS_PROFILE_KEEP alone between) */
int ns_profile_enable(ns_model* m, int on);
int ns_profile_read(ns_model* m, double* total_ms, double* total_flops, int64_t* launches);
int ns_profile_read_slot(ns_model* m, int slot, double* total_ms, double* total_flops, int64_t* launches);

/* ==== HiFi-GAN vocoder (the reference's inference tail: utils/model.py:38-88, utils/tools.py:189-199) ==========================
 * A separate handle with its own weights and arena; nothing above changes.  The generator (hifigan.Generator, resblock "1"):
 *   x = conv_pre(mel)                              Conv1d(n_mel, C0, 7, padding 3)
 *   for i < n_up:  x = ups[i](lrelu(x, 0.1))       ConvTranspose1d(C0 >> i, C0 >> (i+1), up_kernels[i], up_rates[i], padding (k-u)/2)
 *                  x = (rb[n_rb i](x) + ... + rb[n_rb i + n_rb - 1](x)) / n_rb     (summed left to right)
 *   wav = tanh(conv_post(lrelu(x, 0.01)))          Conv1d(C0 >> n_up, 1, 7, padding 3)
 * ResBlock1(ch, k, d[0..2]): for each d: x = c2(lrelu(c1(lrelu(x, 0.1)), 0.1)) + x, c1 = Conv1d(ch, ch, k, dilation d, "same"),
 * c2 = Conv1d(ch, ch, k, "same").  Every convolution has a bias.  Weights are plain `weight` tensors (weight norm already folded:
 * torch._weight_norm(weight_v, weight_g, 0), which is what remove_weight_norm() leaves), torch-native layouts — Conv1d
 * [Cout, Cin, k], ConvTranspose1d [Cin, Cout, k] — under the reference's module paths: conv_pre, ups.{i},
 * resblocks.{n_rb i + j}.convs{1,2}.{n}, conv_post.  The library allocates no device memory here either. */
#define NS_VOC_ABI_VERSION 1
typedef struct ns_vocoder ns_vocoder;
typedef struct ns_voc_config {
  int32_t n_mel;             /* num_mels: 80 */
  int32_t initial_channel;   /* upsample_initial_channel: 512 */
  int32_t n_up;              /* len(upsample_rates), 1..4 */
  int32_t up_rates[4];       /* [8, 8, 2, 2]: even */
  int32_t up_kernels[4];     /* [16, 16, 4, 4]: 2 * rate */
  int32_t n_rb;              /* len(resblock_kernel_sizes), 1..4 */
  int32_t rb_kernels[4];     /* [3, 7, 11]: odd */
  int32_t rb_dilations[4][4];/* [[1, 3, 5]] * 3: three dilations per resblock (ResBlock1), entry 3 must be 0 */
  int32_t resblock;          /* 1 ("1"): ResBlock2 is not supported */
} ns_voc_config;
int ns_voc_abi_version(void);
/* Rejects (nonzero, ns_last_error) anything but resblock 1, k = 2u with u even, odd resblock kernels, channel counts C0 >> i
 * that are multiples of 32 (i = 1 .. n_up) and n_mel a multiple of 16. */
int ns_voc_create(const ns_voc_config* cfg, ns_vocoder** out);
void ns_voc_destroy(ns_vocoder* v);
/* Matmul mode of the GEMM layers (every upsampler and every resblock convs1 / convs2), valid only between ns_voc_create and
 * ns_voc_bind_arena (fails after that, and for any mode but 0 and 1):
 *   0  fp32 (the default when this is never called);
 *   1  bf16, opt-in: the input leaky ReLU in fp32, then the activation rounded to bf16 (round to nearest even, a NaN stays a
 *      NaN); the folded weights rounded to bf16 (RNE) once, at ns_voc_finalize_weights; products accumulated in fp32, every
 *      output element one fp32 sum in a fixed k order whatever the batch or tile.  Bias, activations after the GEMM, the
 *      residual, the multi-receptive-field sum / mean, every stored tensor, conv_pre and conv_post stay fp32.
 * ns_voc_ws_bytes is the same in both modes. */
int ns_voc_set_matmul(ns_vocoder* v, int mode);
/* mode 0: the fp32 image, every tensor at a 256-byte aligned offset.  mode 1: the same image plus one bf16 plane per GEMM weight,
 *   arena_bytes(1) = arena_bytes(0) + sum over W in {ups.{i}.weight, resblocks.{r}.convs{1,2}.{n}.weight} of
 *                    roundup(2 * numel(W), 256). */
size_t ns_voc_arena_bytes(const ns_vocoder* v);
int ns_voc_bind_arena(ns_vocoder* v, void* dev_arena, size_t bytes);  /* 256-byte aligned */
/* host float32 `weight` / `bias`; unknown keys and shape mismatches are errors.  check: the same validation, no side effect. */
int ns_voc_set_weight(ns_vocoder* v, const char* name, const float* host, const int64_t* shape, int ndim);
int ns_voc_check_weight(ns_vocoder* v, const char* name, const int64_t* shape, int ndim);
/* repack (Conv1d -> [Cout][k][Cin]; ConvTranspose1d -> the polyphase [u Cout][2 Cin]) and upload; fails if a key is missing */
int ns_voc_finalize_weights(ns_vocoder* v, void* stream);
/* Workspace of ns_voc_forward: four buffers of B * A floats, each rounded up to 256 bytes, where
 * A = max(T * n_mel, T * C0, max_i T * (u_0 ... u_i) * (C0 >> (i+1))). */
size_t ns_voc_ws_bytes(const ns_vocoder* v, int B, int T);
/* wav [B, T * prod(up_rates)] (the memory of the reference's [B, 1, T * hop]) from the padded mel grid.
 * mel_layout 0: mel is [B, n_mel, T] contiguous (what Generator.forward takes); 1: mel is [B, T, n_mel] contiguous, i.e. the caller
 * holds a transpose(1, 2) view of the forward's postnet_output — consumed in place, 16-byte aligned. */
#define NS_VOC_MEL_CHANNEL_MAJOR 0
#define NS_VOC_MEL_TIME_MAJOR 1
int ns_voc_forward(ns_vocoder* v, const float* mel, int mel_layout, int B, int T, float* wav, void* ws, size_t ws_bytes, void* stream);
/* ---- per-operator entry points (tests), time-major [B, S, C] activations ----
 * conv:     name = "resblocks.{r}.convs{1,2}.{n}": out = conv(lrelu(x, 0.1)) + bias, [B, S, ch] -> [B, S, ch];
 *           "conv_pre": out = conv(x) + bias, [B, S, n_mel] -> [B, S, C0];
 *           "conv_post": out = tanh(conv(lrelu(x, 0.01)) + bias), [B, S, C_last] -> [B, S].
 * conv_form: one resblock launch in any form the stage gives it, name = "resblocks.{r}.convs{1,2}.{n}" only:
 *           v = conv(in_act ? lrelu(x, 0.1) : x) + bias;  if out_act: v = lrelu(v, 0.1);  if resid: v = v + resid;
 *           mrf 0: y = v;  1: y = y + v;  2: y = (y + v) / n_rb   (y is read and rewritten when mrf != 0)
 *           The stage launches c1 as (in_act 1, out_act 1), c2 as (in_act 0, resid = the pair's input), the last c2 of resblock
 *           j of a stage with mrf 0 / 1 / 2 for j = 0 / between / n_rb - 1.  x, resid, y: [B, S, ch]; resid may be NULL; x 16-byte
 *           aligned.  A bad name, a null x or y, an mrf outside {0, 1, 2} or a misaligned x fails before any HIP call.
 * upsample: out = ups[i](lrelu(x, 0.1)), [B, S, 2 ch] -> [B, S u, ch]
 * stage:    upsample i followed by its n_rb resblocks and their mean, [B, S, 2 ch] -> [B, S u, ch]; ws >= ns_voc_op_stage_ws_bytes */
int ns_voc_op_conv(ns_vocoder* v, const char* name, const float* x, int B, int S, float* out, void* stream);
int ns_voc_op_conv_form(ns_vocoder* v, const char* name, const float* x, const float* resid, float* y, int B, int S, int in_act,
                        int out_act, int mrf, void* stream);
int ns_voc_op_upsample(ns_vocoder* v, int i, const float* x, int B, int S, float* out, void* stream);
size_t ns_voc_op_stage_ws_bytes(const ns_vocoder* v, int i, int B, int S);
int ns_voc_op_stage(ns_vocoder* v, int i, const float* x, int B, int S, float* out, void* ws, size_t ws_bytes, void* stream);

/* ==== Reference-mel aligner (the reference's MelEncoder: transformer/Models.py:103-173, called at model/fastspeech2_align.py:56) ===
 * A separate handle with its own weights, arena and workspace; nothing above changes (NS_ABI_VERSION stays as it is).  From the text
 * encoder's output src_output [B, L, d] and a recording's mel frames mels [B, T, 80] it computes what
 *   mel_encoder(src_output, mels, src_masks, mel_masks)
 * returns in eval():
 *   x = relu(w_2(relu(w_1(mels with frame 0 := zeros)))) + position rows           Prenet, transformer/Layers.py:11-26; Models.py:145-164
 *   per layer (FFTBlock2, transformer/Layers.py:51-70):
 *     attn = softmax(w_qs(x) w_ks(src)^T / sqrt(dk) + (-inf at keys l >= src_lens[b]))   every query row, padded ones included
 *     x = masked_fill(LayerNorm(fc(attn w_vs(src)) + x));  x = masked_fill(LayerNorm(w_2(relu(w_1(x))) + x))   rows t >= mel_lens[b] := 0
 * tgt_output [B, T, d] and the attention maps of every layer, attn_all_layers [n_layer, B, H, T, L] (the reference's list of
 * [B, H, T, L] tensors, transformer/SubLayers.py:48-49).  Masked keys hold exactly 0; an utterance with src_lens[b] == 0 is NaN (torch's
 * softmax over a row of -inf) and so is nothing else.  Always exact fp32, whatever ns_config.matmul_bf16x3 says: the product is a
 * discrete decision.  Exists only for d_enc == d_dec == 256 (Prenet is hard-coded 80 -> 256 -> 256 and w_ks / w_vs take d_model
 * inputs) with d_dec / n_dec_head in {64, 128}; ns_aln_create refuses anything else.
 * EXTENSION beyond the reference (whose own duration extraction, _calculate_duration, is undefined: fastspeech2_align.py:57):
 *   a[t, l] = sum over heads h (in head order, fp32) of attn_all_layers[n_layer - 1][b, h, t, l]
 *   durations[b, i] = #{ t < mel_lens[b] : argmax over l < src_lens[b] of a[t, l] == i }, ties to the lowest l
 * int64 [B, L]; 0 for i >= src_lens[b]; the whole row 0 when src_lens[b] or mel_lens[b] is 0, else sum_i durations[b, i] =
 * min(mel_lens[b], T). */
#define NS_ALN_ABI_VERSION 1
int ns_aln_abi_version(void);
/* reads d_enc, d_dec, n_dec_layer, n_dec_head, d_inner, ffn_k1, ffn_k2, n_mel, max_seq_len, row_epilogue of the model's config
 * (transformer/Models.py:106-138) */
int ns_aln_create(const ns_config* cfg, ns_aligner** out);
void ns_aln_destroy(ns_aligner* a);
/* 4 * (sum of numel over every mel_encoder.* tensor, position_enc [1, max_seq_len + 1, d] included): packing keeps every element
 * (w_ks | w_vs fused to [2d, d], Conv1d [out, in, k] -> [out, k, in]) and every tensor's size is a multiple of 256 bytes. */
size_t ns_aln_arena_bytes(const ns_aligner* a);
int ns_aln_bind_arena(ns_aligner* a, void* dev_arena, size_t bytes);  /* 256-byte aligned */
/* host float32, reference key names ("mel_encoder.prenet.w_1.weight", "mel_encoder.layer_stack.{i}.crs_attn.w_qs.weight", ...) and
 * torch-native layouts; unknown keys and shape mismatches are errors.  "mel_encoder.position_enc" is optional (regenerated).
 * check: the same validation, no side effect. */
int ns_aln_set_weight(ns_aligner* a, const char* name, const float* host, const int64_t* shape, int ndim);
int ns_aln_check_weight(ns_aligner* a, const char* name, const int64_t* shape, int ndim);
int ns_aln_finalize_weights(ns_aligner* a, void* stream);
/* Workspace of ns_aln_forward; monotone in B, L and T. */
size_t ns_aln_ws_bytes(const ns_aligner* a, int B, int L, int T);
/* src_output [B, L, d] (ns_op_txt_encoder's output), mels [B, T, 80] (read only), src_lens / mel_lens [B] int64 on the device;
 * writes tgt_output [B, T, d], attn_all_layers [n_layer, B, H, T, L], durations [B, L] int64.  16-byte aligned float pointers. */
int ns_aln_forward(ns_aligner* a, const float* src_output, const int64_t* src_lens, const float* mels, const int64_t* mel_lens,
                   int B, int L, int T, float* tgt_output, float* attn_all_layers, int64_t* durations, void* ws, size_t ws_bytes,
                   void* stream);
/* ---- per-operator entry points (tests) ----
 * cross attention alone (transformer/Modules.py:14-25 on projected heads): q [B*T, H*dk], kv [B*L, 2*H*dk] (K | V, head h at h*dk
 * inside each) -> ctx [B*T, H*dk] (merged heads), attn [B, H, T, L]; dk in {64, 128}.
 * durations: the extension above applied to one [B, H, T, L] map.
 * input: x [B, T, C] = mels with frame 0 of every utterance replaced by zeros (transformer/Models.py:145-146); C % 4 == 0, both
 * pointers 16-byte aligned (additive: NS_ALN_ABI_VERSION is unchanged). */
int ns_aln_op_input(const float* mels, float* x, int B, int T, int C, void* stream);
int ns_aln_op_cross_attention(const float* q, const float* kv, const int64_t* src_lens, int B, int T, int L, int H, int dk,
                              float* ctx, float* attn, void* stream);
int ns_aln_op_durations(const float* attn_last, const int64_t* src_lens, const int64_t* mel_lens, int B, int H, int T, int L,
                        int64_t* out, void* stream);

/* ==== Validation loss (the reference's FastSpeech2Loss.forward, model/loss.py:149-250, in eval(): the forward VALUE only) ==========
 * A handle-less family: the loss has no weights.  Nothing above changes (NS_ABI_VERSION, NS_VOC_ABI_VERSION and NS_ALN_ABI_VERSION
 * stay as they are).  From the reference's 12-tuple of a teacher-forced batch (ns_forward_durations_teacher + ns_forward_mel) and the
 * batch's targets it computes, in two launches on `stream`, with no host read and no float atomic:
 *   mel, postnet   mean |pred - mel_targets[:, :T]| over the n_mel columns of the frames with mel_masks == 0     model/loss.py:189-191,219-227
 *   pitch, energy  mean (pred - target)^2 over the frames with mel_masks == 0 (frame_level) or the phonemes with
 *                  src_masks == 0 (phoneme_level)                                                                  model/loss.py:199-211,229-230
 *   duration       mean (log_d - log((float)d_targets[:, :L] + 1))^2 over the phonemes with src_masks == 0       model/loss.py:190,213-217,231
 *   attn           sum over k = 0..3 of 10 * mean over {t < olen_b, l < ilen_b} of W[b,t,l] * attn[k][b, 0, t, l],
 *                  W = 1 - exp(-((l / ilen_b - t / olen_b)^2) / (2 * 0.2^2)) in fp32, ilen = src_lens, olen = the
 *                  batch's INPUT mel_lens; head 0 only, layers 0-3 hard-coded                                     model/loss.py:60-65,104-108,144-146,233-236
 *   total          mel + postnet + duration + pitch + energy + attn, in fp32                                     model/loss.py:238-240
 * A masked-out element is selected away, never multiplied by zero: padded positions may hold NaN (an utterance with src_lens == 0)
 * and do not reach the sums.  An empty selection gives NaN (torch.mean of nothing), and the total is then NaN.  Equal inputs give
 * equal bits: the summation order is a function of the shapes alone.
 * DEVIATION: the reference fails on a broadcast when T != max(mel_lens) or L != max(src_lens) (model/loss.py:60, 69-71); here ilen is
 * clamped to [0, L] and olen to [0, T], and the selected region is what _make_masks would give if the shapes agreed. */
#define NS_LOSS_ABI_VERSION 1
int ns_loss_abi_version(void);
typedef struct ns_loss_args {
  int32_t B, L, T, H, n_mel;                          /* attn[k] is [B, H, T, L]; n_mel a multiple of 4 */
  int32_t pitch_frame_level, energy_frame_level;      /* preprocessing.{pitch,energy}.feature == "frame_level" (model/loss.py:154-159) */
  int64_t mel_targets_stride;                         /* floats between utterances of mel_targets: T' * n_mel with T' >= T (model/loss.py:191) */
  int64_t d_targets_stride;                           /* elements between rows of d_targets: L' >= L (model/loss.py:214-216) */
  const float* mel;                                   /* predictions[0]  [B, T, n_mel]                          model/loss.py:175,219 */
  const float* postnet;                               /* predictions[1]  [B, T, n_mel]                          model/loss.py:176,220 */
  const float* mel_targets;                           /* inputs[6]       [B, T', n_mel]                         model/loss.py:168,191,224 */
  const uint8_t* mel_masks;                           /* predictions[7]  [B, T] bool, nonzero = padded          model/loss.py:182,189 */
  const float* pitch;                                 /* predictions[2]  [B, T] or [B, L]                       model/loss.py:177,199-204 */
  const float* pitch_targets;                         /* inputs[9]       same shape                             model/loss.py:171 */
  const float* energy;                                /* predictions[3]  [B, T] or [B, L]                       model/loss.py:178,206-211 */
  const float* energy_targets;                        /* inputs[10]      same shape                             model/loss.py:172 */
  const float* log_d;                                 /* predictions[4]  [B, L]                                 model/loss.py:179,213 */
  const int64_t* d_targets;                           /* predictions[11] [B, L'] int64                          model/loss.py:186,190 */
  const uint8_t* src_masks;                           /* predictions[6]  [B, L] bool, nonzero = padded          model/loss.py:181,188 */
  const int64_t* src_lens;                            /* inputs[4]       [B] int64                              model/loss.py:166,233 */
  const int64_t* mel_lens;                            /* inputs[7]       [B] int64 — NOT predictions[9]         model/loss.py:169,233 */
  const float* attn[4];                               /* predictions[10][0..3], read in place at head 0         model/loss.py:233-236 */
} ns_loss_args;
/* Bytes of the partial-sum workspace of ns_loss_forward (one 64-byte slot per workgroup); positive, monotone in B, L and T.  The
 * workspace needs no initialisation. */
size_t ns_loss_ws_bytes(int B, int L, int T);
/* Every pointer in `a` is a device pointer; mel, postnet and mel_targets 16-byte aligned, ws 16-byte aligned; out7 <- total, mel,
 * postnet, pitch, energy, duration, attn (the reference's return order, model/loss.py:242-250) as 7 device floats.  Validation
 * happens before any HIP call: null pointers (of the tensors the shape makes non-empty), negative sizes, n_mel not a multiple of 4,
 * strides below the tensor's own extent and ws_bytes < ns_loss_ws_bytes(B, L, T) return nonzero with ns_last_error().  B == 0,
 * L == 0 or T == 0 is legal and yields NaNs. */
int ns_loss_forward(const ns_loss_args* a, void* ws, size_t ws_bytes, float* out7, void* stream);

/* ==== Wave-to-mel front end (the reference's TacotronSTFT.mel_spectrogram + Audio.tools.get_mel_from_wav: audio/stft.py:52-81,
 * 159-178, audio/tools.py:8-15, audio/audio_processing.py:85-91) ===============================================================
 * A separate handle with its own weights, arena and workspace; nothing above changes (every other ABI version stays as it is).  For a
 * batch of variable-length waves wav [B, ld_wav] (utterance b holds n_b = clamp(wav_lens[b], 0, n_max) samples) it computes, in three
 * launches on `stream`, with no host read and no device allocation:
 *   x = clip(wav, -1, 1), reflect-padded by filter_length / 2 on both sides (torch's "reflect": the edge sample is not repeated)
 *   frame t = x[t hop .. t hop + filter_length), spectrum = frame . forward_basis rows           F.conv1d(stride = hop), stft.py:67-72
 *   mag_k = sqrtf(re_k^2 + im_k^2), k = 0 .. filter_length / 2                                   stft.py:78
 *   energy[b, t] = sqrtf(sum_k mag_k^2)                                                          torch.norm, stft.py:176
 *   mel[b, t, m] = (float)log((double)max(sum_k mel_basis[m, k] mag_k, clip_val))                stft.py:174-175, audio_processing.py:91
 * mel is TIME-major [B, T, n_mel] (the layout ns_aln_forward and ns_forward_durations_teacher take), energy [B, T].  Frames
 * t >= mel_lens[b] = n_b / hop + 1 hold zeros in both (what pad_2D / pad_1D give a collated batch); mel_lens_out[b] is that count, not
 * clamped to T.  An utterance with n_b <= filter_length / 2 (which the reference's reflect pad refuses) has ZERO frames.  Samples at
 * and beyond n_b are never read; a NaN sample stays a NaN and reaches exactly the frames whose window covers it.  Equal inputs give
 * equal bits, and replicas of one utterance inside a batch are bit-identical: every reduction order is a function of the shapes alone.
 * The STFT is one fp32 Conv1D-as-GEMM over the padded wave cut into rows of hop samples (Cin = hop, KW = filter_length / hop, pad 0);
 * the imaginary basis rows of bins 0 and filter_length / 2 are identically zero and are dropped, which leaves filter_length columns.
 * The mel basis is consumed in band form (per filter: first to last non-zero bin), summed in bin order; any dense matrix is legal.
 * DEVIATION: the reference asserts min >= -1 and max <= 1 (a host read, stft.py:169-170); here the samples are clipped instead, the
 * identity on everything the assertion lets through (and what get_mel_from_wav does ahead of the call, tools.py:9). */
#define NS_MEL_ABI_VERSION 1
typedef struct ns_melfront ns_melfront;
typedef struct ns_mel_config {
  int32_t filter_length, hop_length, win_length, n_mel;   /* 1024, 256, 1024, 80 */
  float clip_val;                                         /* dynamic_range_compression's clip_val: 1e-5 */
} ns_mel_config;
int ns_mel_abi_version(void);
/* Rejects (nonzero, ns_last_error): filter_length % hop_length != 0, hop_length % 32 != 0, win_length > filter_length (or < 1),
 * n_mel % 4 != 0, and a filter_length outside what the GEMM dispatch accepts for N = KW * Cin = filter_length (and above 4096, the
 * magnitude row a workgroup stages on chip). */
int ns_mel_create(const ns_mel_config* cfg, ns_melfront** out);
void ns_mel_destroy(ns_melfront* h);
size_t ns_mel_arena_bytes(const ns_melfront* h);
int ns_mel_bind_arena(ns_melfront* h, void* dev_arena, size_t bytes);  /* 256-byte aligned */
/* host float32, the reference module's buffer names and torch-native shapes: "stft_fn.forward_basis" [filter_length + 2, 1,
 * filter_length], "mel_basis" [n_mel, filter_length / 2 + 1]; "stft_fn.inverse_basis" is accepted and ignored.  finalize refuses a
 * forward_basis whose imaginary rows of bins 0 or filter_length / 2 hold an entry of magnitude above 1e-6 (not a real DFT basis). */
int ns_mel_set_weight(ns_melfront* h, const char* name, const float* host, const int64_t* shape, int ndim);
int ns_mel_check_weight(ns_melfront* h, const char* name, const int64_t* shape, int ndim);
int ns_mel_finalize_weights(ns_melfront* h, void* stream);
/* frames of a wave of n samples: n / hop + 1 (0 for n < 0 or hop < 1) */
int64_t ns_mel_frames(int64_t n, int32_t hop);
/* Workspace of ns_mel_forward for B waves of at most n_max samples (hop rows + packed spectrum); monotone in B and n_max.  Needs no
 * initialisation: every word that is read is written first. */
size_t ns_mel_ws_bytes(const ns_melfront* h, int B, int64_t n_max);
/* wav [B, ld_wav] fp32 (ld_wav >= n_max), wav_lens [B] int64, both on the device; T >= 1 is the caller's choice: frames beyond it
 * are dropped, frames up to it zero-filled.  Writes mel [B, T, n_mel], energy [B, T], mel_lens_out [B] int64. */
int ns_mel_forward(ns_melfront* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int T, float* mel,
                   float* energy, int64_t* mel_lens_out, void* ws, size_t ws_bytes, void* stream);
/* ---- per-operator entry points (tests); S = Tc + filter_length / hop - 1 hop rows per utterance for Tc computed frames ----
 * frame_rows: rows [B, S, hop] from the waves (mel_lens_out nullable)
 * stft:       rows [B, S, hop] -> packed spectrum [B * S, filter_length]: column 0 = re_0, 1 = re_{filter_length/2}, 2k = re_k,
 *             2k + 1 = im_k; rows t >= Tc of an utterance are computed from partial taps and mean nothing
 * project:    packed spectrum -> mel [B, T, n_mel], energy [B, T] */
int ns_mel_op_frame_rows(ns_melfront* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int S,
                         float* rows, int64_t* mel_lens_out, void* stream);
int ns_mel_op_stft(ns_melfront* h, const float* rows, int B, int S, float* spec, void* stream);
int ns_mel_op_project(ns_melfront* h, const float* spec, const int64_t* wav_lens, int B, int S, int64_t n_max, int T, float* mel,
                      float* energy, void* stream);

/* ================================================================================================================================
 * Griffin-Lim mel-to-wave: the other half of the reference's audio/ package — inv_mel_spec (audio/tools.py:18-34), griffin_lim
 * (audio/audio_processing.py:66-82), STFT.inverse and STFT.transform (audio/stft.py:52-122), window_sumsquare
 * (audio/audio_processing.py:7-63).  It needs no trained weights.  A separate handle over the same three buffers as ns_mel_*; all
 * three are used here.  Per utterance, with N = filter_length, Tg_b frames and n_b = hop (Tg_b - 1) samples:
 *   mag[t, k]  = scaling * sum_m expf(mel[t, m]) mel_basis[m, k], t < Tg_b = mel_lens[b] - 1        tools.py:20-25,28 (the last frame is dropped;
 *                m ascending; the TRANSPOSE of mel_basis, not a pseudo-inverse: what the reference does)
 *   X          = (mag cos(angles), mag sin(angles)) in the packed layout of ns_mel_op_stft          stft.py:84-86
 *   frames     = X . inverse_basis rows (one fp32 GEMM, K = N = filter_length per frame)            F.conv_transpose1d, stft.py:88-93
 *   y[s]       = (N / hop) * (sum_t frames[t, s + N/2 - t hop]) / window_sum_b[s + N/2]             stft.py:95-120
 *                where window_sum_b > FLT_MIN; t ascending (at most N / hop terms); window_sum_b is rebuilt per sample with the
 *                reference's arithmetic: an fp32 accumulator, each += adds a float64 squared-window value and rounds once
 *   iteration:   signal -> reflect-padded hop rows WITHOUT a clip -> forward STFT GEMM -> X = mag * Y / |Y| per bin -> inverse
 *                (audio_processing.py:79-81; mag * Y / |Y| is mag (cos, sin)(atan2(im, re)) without the angle: (mag, 0) where Y = 0,
 *                +-mag at bins 0 and N/2, a NaN in either component makes both outputs of its bin NaN; the loop evaluates no atan2f, cosf or sinf)
 * No host read, no device allocation, no atomics: equal inputs give equal bits and replicas of an utterance inside a batch are
 * bit-identical.  Frame counts are device int64 [B], CLAMPED to [0, frames of the call] rather than validated; an utterance with
 * n_b <= filter_length / 2 (which the reference's reflect pad refuses) gives a zero wave of length 0.  Samples at and beyond n_b and
 * rows at and beyond Tg_b are written as zeros.
 * DEVIATIONS: the two imaginary columns of bins 0 and N/2 are dropped (their inverse_basis rows are zero up to the 1e-18 noise of
 * the reference's pinv; finalize refuses anything above 1e-9), and tools.py:28 reads `_stft._stft_fn`, an attribute that does not
 * exist: the evident intent `stft_fn` is what is implemented. */
#define NS_GL_ABI_VERSION 1
typedef struct ns_gl ns_gl;
typedef struct ns_gl_config {
  int32_t filter_length, hop_length, win_length, n_mel;   /* 1024, 256, 1024, 80 */
  float spec_from_mel_scaling;                            /* the reference's literal 1000, tools.py:22 */
} ns_gl_config;
int ns_gl_abi_version(void);
/* The constraints of ns_mel_create (filter_length % hop_length, hop_length % 32, win_length, n_mel % 4, the GEMM's range for
 * N = K = filter_length <= 4096); spec_from_mel_scaling > 0. */
int ns_gl_create(const ns_gl_config* cfg, ns_gl** out);
void ns_gl_destroy(ns_gl* h);
size_t ns_gl_arena_bytes(const ns_gl* h);
int ns_gl_bind_arena(ns_gl* h, void* dev_arena, size_t bytes);  /* 256-byte aligned */
/* host float32, the reference module's buffer names and torch-native shapes: "stft_fn.forward_basis" and "stft_fn.inverse_basis"
 * [filter_length + 2, 1, filter_length] (stft.py:49-50), "mel_basis" [n_mel, filter_length / 2 + 1] (stft.py:149).  mel_basis is
 * optional (a bare STFT has none): without it ns_gl_forward and ns_gl_op_mel_to_mag refuse.  finalize refuses a missing basis. */
int ns_gl_set_weight(ns_gl* h, const char* name, const float* host, const int64_t* shape, int ndim);
int ns_gl_check_weight(ns_gl* h, const char* name, const int64_t* shape, int ndim);
int ns_gl_finalize_weights(ns_gl* h, void* stream);
/* Workspace for B utterances of at most T_max frames (mel or magnitude frames); monotone in both.  Needs no initialisation: every
 * word that is read is written first. */
size_t ns_gl_ws_bytes(const ns_gl* h, int B, int T_max);
/* inv_mel_spec's batched core (tools.py:18-29): mel [B, T, n_mel] log-mel, TIME-major; mel_lens [B] int64; angles [B, T - 1,
 * filter_length / 2 + 1] (the start of audio_processing.py:74, time-major); n_iters >= 0 (0 = the initial inverse alone).  Writes
 * wave [B, ld_wave] (ld_wave % 4 == 0, >= hop (T - 2); 16-byte aligned) and wave_lens_out [B] = n_b. */
int ns_gl_forward(ns_gl* h, const float* mel, const int64_t* mel_lens, int B, int T, const float* angles, int n_iters, float* wave,
                  int64_t ld_wave, int64_t* wave_lens_out, void* ws, size_t ws_bytes, void* stream);
/* griffin_lim (audio_processing.py:66-82) from magnitudes mag [B, Tg, filter_length / 2 + 1], frame_lens [B] int64 */
int ns_gl_forward_mag(ns_gl* h, const float* mag, const int64_t* frame_lens, int B, int Tg, const float* angles, int n_iters, float* wave,
                      int64_t ld_wave, int64_t* wave_lens_out, void* ws, size_t ws_bytes, void* stream);
/* STFT.transform (stft.py:52-81) for users of the class: wav [B, ld_wav] -> magnitude, phase [B, T, filter_length / 2 + 1] =
 * sqrtf(re^2 + im^2), atan2f(im, re); no clip; the length rules of ns_mel_forward.  Never called by the loop. */
int ns_gl_transform(ns_gl* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int T, float* magnitude,
                    float* phase, void* ws, size_t ws_bytes, void* stream);
/* ---- per-operator entry points (tests); frame_lens [B] int64 are magnitude frame counts, X / Y packed rows of filter_length ----
 * mel_to_mag: tools.py:20-25,28 -> mag [B, T - 1, filter_length / 2 + 1]
 * recombine:  stft.py:84-86 -> X [B * Tg, filter_length]
 * rephase:    stft.py:79 + 84-86 from the packed spectrum Y [B * S, filter_length] (S >= Tg rows per utterance) -> X
 * inverse:    stft.py:88-120 from X -> wave, wave_lens_out
 * frame_rows: stft.py:58-65, ns_mel_op_frame_rows without the clip
 * step:       audio_processing.py:80-81, one iteration in place on wave (wave_lens_out is rewritten from frame_lens first) */
int ns_gl_op_mel_to_mag(ns_gl* h, const float* mel, const int64_t* mel_lens, int B, int T, float* mag, void* stream);
int ns_gl_op_recombine(ns_gl* h, const float* mag, const float* angles, const int64_t* frame_lens, int B, int Tg, float* X, void* stream);
int ns_gl_op_rephase(ns_gl* h, const float* Y, const float* mag, const int64_t* frame_lens, int B, int Tg, int S, float* X, void* stream);
int ns_gl_op_inverse(ns_gl* h, const float* X, const int64_t* frame_lens, int B, int Tg, float* wave, int64_t ld_wave,
                     int64_t* wave_lens_out, void* ws, size_t ws_bytes, void* stream);
int ns_gl_op_frame_rows(ns_gl* h, const float* wav, int64_t ld_wav, const int64_t* wav_lens, int B, int64_t n_max, int S, float* rows,
                        void* stream);
int ns_gl_op_step(ns_gl* h, const float* mag, const int64_t* frame_lens, int B, int Tg, float* wave, int64_t ld_wave,
                  int64_t* wave_lens_out, void* ws, size_t ws_bytes, void* stream);

/* ==== Pitch / energy variance targets and dataset statistics (the tail of the reference's Preprocessor.process_utterance and its
 * build_from_path / remove_outlier / normalize: preprocessor/preprocessor.py:188-227, 61-133, 289-310) ==========================
 * Handle-less like ns_loss_*: no weights, caller-owned workspace and state, one stream, no host read, no device allocation, no float
 * atomic; nothing above changes (every other ABI version stays as it is).  Frame-level f0 is an INPUT: pitch extraction, resampling,
 * TextGrid parsing and file I/O stay outside.  Per utterance b, with Ls = clamp(src_lens[b], 0, L) and d_i = durations[b, i]:
 *   n_b = min(T, sum_{i < Ls} max(d_i, 0))  -> frame_lens[b]                                      preprocessor.py:188,194-195
 *   valid[b] = more than one frame t < n_b has pitch != 0; an invalid utterance gets all-zero targets     preprocessor.py:189-190
 *   frame_level feature: the values at t < n_b, zeros behind (frame-level pitch is NOT interpolated)      preprocessor.py:197,218
 *   phoneme_level pitch: the contour interpolated linearly over unvoiced frames in float64 — slope * (t - x0) + y0 with
 *     slope = (y1 - y0) / (x1 - x0) between voiced neighbours x0 < t < x1, the first / last voiced value outside them — then
 *     the float64 mean over frames [c_i - d_i, c_i) within [0, n_b), c the inclusive prefix sum; 0 where d_i <= 0 or the
 *     intersection is empty; rounded once to fp32; zeros at i >= Ls                                       preprocessor.py:199-216
 *   phoneme_level energy: the same mean without the interpolation                                         preprocessor.py:219-227
 * Padded input positions (frames >= n_b, phonemes >= Ls) are selected away, never multiplied: they may hold NaN.  Every word of
 * every output is written.  Equal inputs give equal bits: every reduction order is a function of the shapes alone.
 * DEVIATION: the reference averages IN PLACE (pitch[i] = np.mean(pitch[pos:pos+d]), preprocessor.py:208-216, 219-227): with zero
 * durations early in an utterance (sum_{j<i} d_j < i for a phoneme with d_i > 0) it reads values it has already overwritten, and
 * it raises IndexError once i >= sum(d).  Here every mean is over the ORIGINAL frames — the function the loop intends; the two are
 * identical on every utterance with sum_{j<i} d_j >= i for all i with d_i > 0 and sum(d) >= Ls. */
#define NS_VT_ABI_VERSION 1
#define NS_VT_SORT_CAPACITY 8192 /* values of one (utterance, feature) that ns_vt_fit can sort in LDS */
int ns_vt_abi_version(void);
/* Device memory, 80 bytes, 8-byte aligned: the running statistics of the outlier-filtered RAW targets (float64 count / mean / M2,
 * index 0 pitch, 1 energy) and the extrema of the NORMALISED targets.  ns_vt_state_init writes count = mean = M2 = 0,
 * min = DBL_MAX, max = -DBL_MAX (preprocessor.py:61-62, 300-301) on `stream`. */
typedef struct ns_vt_state {
  double count[2], mean[2], m2[2], min[2], max[2];
} ns_vt_state;
typedef struct ns_vt_args {
  int32_t B, L, T;
  int32_t pitch_frame_level, energy_frame_level;      /* preprocessing.{pitch,energy}.feature == "frame_level" (preprocessor.py:33-38) */
  int32_t pitch_normalization, energy_normalization;  /* preprocessing.{pitch,energy}.normalization (preprocessor.py:40-41,93-105) */
  int64_t durations_stride;                           /* elements between rows of durations: L' >= L */
  const float* pitch;                                 /* [B, T] frame f0, 0 = unvoiced; ns_vt_targets only      preprocessor.py:181-188 */
  const float* energy;                                /* [B, T] frame energy; ns_vt_targets only                preprocessor.py:193-195 */
  const int64_t* durations;                           /* [B, L'] int64; ns_vt_targets only                      preprocessor.py:163,188 */
  const int64_t* src_lens;                            /* [B] int64 */
  float* pitch_targets;                               /* [B, T] or [B, L]: written by targets, read by fit, rewritten by normalize */
  float* energy_targets;                              /* [B, T] or [B, L] */
  int64_t* frame_lens;                                /* [B]: written by targets, read by fit and normalize */
  uint8_t* valid;                                     /* [B]: written by targets, read by fit; normalize accepts NULL = all valid */
} ns_vt_args;
/* Bytes of the workspace any of the three calls below needs at (B, L, T); positive, monotone.  Needs no initialisation. */
size_t ns_vt_ws_bytes(int B, int L, int T);
int ns_vt_state_init(ns_vt_state* state, void* stream);
/* pitch, energy, durations -> pitch_targets, energy_targets, frame_lens, valid (raw, not normalised).  One launch, one workgroup per
 * (utterance, feature).  Validation happens before any HIP call: null pointers (of what the shape makes non-empty), negative sizes,
 * durations_stride < L and ws_bytes < ns_vt_ws_bytes(B, L, T) return nonzero with ns_last_error().  B, L or T == 0 is legal. */
int ns_vt_targets(const ns_vt_args* a, void* ws, size_t ws_bytes, void* stream);
/* remove_outlier + StandardScaler.partial_fit (preprocessor.py:84-87, 289-297) of one batch of raw targets: per (valid utterance,
 * feature) its n = src_lens[b] (phoneme_level; the zeros of d_i = 0 phonemes included) or frame_lens[b] values are sorted in LDS,
 * p25 / p75 are numpy's default linear percentile at q / 100 * (n - 1) in float64, the values with lower < v < upper (strict),
 * lower = p25 - 1.5 (p75 - p25), upper = p75 + 1.5 (p75 - p25), give (count, mean, M2) in float64 in the utterance's workspace slot;
 * a second one-workgroup launch merges the slots in utterance order into `state` (Chan's update).  n = 0 and n = 1 contribute
 * nothing.  The sorted dimension (T at frame_level, L at phoneme_level) above NS_VT_SORT_CAPACITY is refused here, on the host. */
int ns_vt_fit(const ns_vt_args* a, ns_vt_state* state, void* ws, size_t ws_bytes, void* stream);
/* y = (float)(((double)x - mean) / std) in place on the selected positions (valid utterance, position < n), padding stays 0;
 * mean / std = sqrt(M2 / count) from `state` (StandardScaler.mean_ / scale_, the population std; 0 / 1 when the feature's
 * normalization flag is off, when nothing was fitted, or std == 0), and the min / max of the float64 quotients over ALL selected
 * positions — not the outlier-filtered ones — folded into `state` by per-workgroup slots and a fixed-order merge
 * (preprocessor.py:93-112, 299-310).  A NULL `valid` takes every utterance as valid: the zero rows of one that ns_vt_targets dropped
 * become -mean / std at positions < n and enter min / max, so pass the flag unless the batch holds no dropped utterance. */
int ns_vt_normalize(const ns_vt_args* a, ns_vt_state* state, void* ws, size_t ws_bytes, void* stream);

/* ==== The optimiser half of the training step: clip_grad_norm_, ScheduledOptim.step_and_update_lr's Adam.step() and zero_grad()
 * (train.py:91-95; model/optimizer.py:10-15,24,28) =================================================================================
 * Handle-less like ns_loss_* and ns_vt_*: the chunk table, the workspace, the two state arenas and the norm record are caller-owned;
 * one stream, no device allocation, no host read, no float atomic; nothing above changes (every other ABI version stays as it is).
 * The Noam warm-up / anneal schedule (optimizer.py:33-51) is host arithmetic: lr is an argument.  fp32 parameters only, one group,
 * no amsgrad, no maximize.  Per element, in the order of torch/optim/adam.py _single_tensor_adam (non-capturable branch), with
 * t = global_step - lag[tensor] the tensor's own step count and every product rounded before it is added:
 *   g' = g * clip_coef                        (fuse_clip; the coefficient is read from the device record)      train.py:91
 *   g' = g' + weight_decay * p                (weight_decay != 0)                                              optimizer.py:14
 *   m  = m + (1 - beta1) * (g' - m)           exp_avg.lerp_                                                    optimizer.py:24
 *   v  = v * beta2 + ((1 - beta2) * g') * g'  exp_avg_sq.mul_().addcmul_()
 *   p  = p - ((lr / (1 - beta1^t)) * m) / (sqrtf(v) / sqrt(1 - beta2^t) + eps)     true division, float64 bias corrections
 *   g  = 0                                    (zero_grads)                                                     train.py:95
 * The parameter list is cut into chunks of NS_OPT_CHUNK elements, tensor i owning max(1, ceil(numel_i / NS_OPT_CHUNK)) of them; a
 * workgroup finds a chunk's tensor from the per-tensor prefix `chunk_begin`, so no launch depends on the number of tensors.  p, g, m
 * and v move as 16-byte vectors where the tensor's pointer is 16-byte aligned and element by element otherwise (the same elements
 * per thread either way: alignment changes no bit).  Equal inputs give equal bits: the norm's reduction order is a function of the
 * sizes alone. */
#define NS_OPT_ABI_VERSION 1
#define NS_OPT_CHUNK 4096
int ns_opt_abi_version(void);
/* One row of the chunk table (40 bytes).  Built on the host by ns_opt_build_table, uploaded by the caller. */
typedef struct ns_opt_tensor {
  float* param;           /* device, 4-byte aligned; a view such as base[1:] is fine */
  float* grad;            /* device; NULL = skipped, as torch skips p.grad is None (no norm share, no update, no step) */
  int64_t numel;
  int64_t state_offset;   /* floats into exp_avg / exp_avg_sq; every tensor is padded to a multiple of 4 */
  int32_t lag;            /* global_step - lag is this tensor's `step` (torch keeps it per parameter); lag < global_step */
  int32_t chunk_begin;    /* chunks of the tensors in front */
} ns_opt_tensor;
typedef struct ns_opt_plan {
  int64_t n_tensors, n_chunks;
  int64_t table_bytes;    /* n_tensors rows */
  int64_t ws_bytes;       /* one float64 slot per chunk; needs no initialisation */
  int64_t state_floats;   /* of EACH of exp_avg and exp_avg_sq; zero them before the first step */
} ns_opt_plan;
/* Device memory, 16 bytes, 8-byte aligned, written by ns_opt_grad_norm: the float64 2-norm of all gradients, its fp32 rounding (what
 * clip_grad_norm_ returns) and min(1, max_norm / (total_norm + 1e-6)) evaluated in fp32 as torch evaluates it (a NaN norm gives a
 * NaN coefficient). */
typedef struct ns_opt_record {
  double norm64;
  float total_norm, clip_coef;
} ns_opt_record;
typedef struct ns_opt_hyper {
  double lr, beta1, beta2, eps, weight_decay;   /* param_groups[0] of torch.optim.Adam (optimizer.py:10-15,50-51) */
  int64_t global_step;                          /* >= 1: the number of this step */
  int32_t fuse_clip;                            /* multiply g by the record's clip_coef first (train.py:91) */
  int32_t zero_grads;                           /* write g = 0 behind the update (train.py:95) */
} ns_opt_hyper;
/* Host only.  Sizes for n_tensors >= 1 tensors of numels[i] >= 0 elements: all positive, monotone in every size. */
int ns_opt_plan_sizes(const int64_t* numels, int n_tensors, ns_opt_plan* out);
/* Host only.  Writes plan.n_tensors rows into table_host (8-byte aligned, >= plan.table_bytes); lags NULL = all zero.  A tensor of
 * zero elements is stored as skipped. */
int ns_opt_build_table(const int64_t* numels, float* const* params, float* const* grads, const int32_t* lags, int n_tensors,
                       void* table_host, size_t table_bytes);
/* The four launching calls take the planner's output and the DEVICE copy of the table.  Before any HIP call they return nonzero with
 * ns_last_error() on null pointers, a plan that ns_opt_plan_sizes cannot have produced (n_tensors == 0 included), a table, workspace
 * or arena smaller than the plan says, negative sizes, betas outside [0, 1), eps < 0, lr < 0, weight_decay < 0, global_step < 1.
 * nn.utils.clip_grad_norm_ (train.py:91), first half: two launches; writes `record`. */
int ns_opt_grad_norm(const ns_opt_plan* plan, const void* table, size_t table_bytes, float max_norm, void* ws, size_t ws_bytes,
                     ns_opt_record* record, void* stream);
/* clip_grad_norm_, second half: g *= record->clip_coef in place, also when the coefficient is 1 (as torch does).  One launch. */
int ns_opt_scale_grads(const ns_opt_plan* plan, const void* table, size_t table_bytes, const ns_opt_record* record, void* stream);
/* optimizer.step() (optimizer.py:24), one launch.  exp_avg / exp_avg_sq: 16-byte aligned arenas of state_floats floats each.  record
 * may be NULL unless hyper->fuse_clip.  With fuse_clip the result is bitwise that of ns_opt_scale_grads followed by this call
 * without it (the gradients themselves stay unscaled). */
int ns_opt_adam_step(const ns_opt_plan* plan, const void* table, size_t table_bytes, const ns_opt_hyper* hyper, float* exp_avg,
                     float* exp_avg_sq, int64_t state_floats, const ns_opt_record* record, void* stream);
/* optimizer.zero_grad() with set_to_none=False (optimizer.py:28, the torch default of the reference's day).  One launch. */
int ns_opt_zero_grads(const ns_opt_plan* plan, const void* table, size_t table_bytes, void* stream);

/* ==== Training loss: the value AND the backward of the reference's FastSpeech2Loss (train.py:83-88, model/loss.py:149-250) ==========
 * Handle-less like ns_loss_*, whose argument block it shares; nothing above changes (NS_LOSS_ABI_VERSION and every other ABI version
 * stay as they are).  The forward is ns_loss_forward — the same two launches, the same seven bits — which also leaves the three counts
 * its means divide by in a small caller-owned device record.  The backward is one launch: for grad_output g (7 device floats, in the
 * order of out7) it writes the gradient of sum_i g[i] * out7[i] with respect to each prediction, contiguous and shaped like it:
 *   d_mel, d_postnet   (g[0] + g[i]) / (n_mel * n_frames) * sign(pred - target) on the frames with mel_masks == 0, sign(0) = 0
 *   d_pitch, d_energy  2 * (g[0] + g[i]) / count * (pred - target) on the unmasked frames (frame_level) or phonemes (phoneme_level)
 *   d_log_d            2 * (g[0] + g[5]) / n_phonemes * (log_d - log((float)d_targets + 1.0f)) on the phonemes with src_masks == 0; the
 *                      logarithm of that fp32 argument is taken in float64 and rounded to fp32 once
 *   d_attn[k]          10 * (g[0] + g[6]) / n_attn * W[b, t, l] on head 0 at t < olen_b, l < ilen_b — the same for k = 0..3
 * and +0.0f everywhere else, all of heads >= 1 included.  A masked-out element is selected away, never multiplied by zero: it is not
 * read, so NaN behind a mask does not reach a gradient, and a part with an empty selection (value NaN) has an all-zero gradient, as
 * masked_select's backward gives.  Targets, masks and lengths get no gradient.  g and the record are read on the device; the
 * coefficients are formed in float64 and rounded once.  No atomic, no workspace, no host read; equal inputs give equal bits. */
#define NS_LOSSG_ABI_VERSION 1
#define NS_LOSSG_RECORD_BYTES 32   /* int64 n_frames, n_phonemes, n_attn, 0; device memory, 8-byte aligned, written by ns_lossg_forward */
int ns_lossg_abi_version(void);
size_t ns_lossg_record_bytes(void);
/* The nine outputs of ns_lossg_backward: device pointers, 16-byte aligned, each as large as its prediction.  NULL = not wanted: that
 * tensor is neither computed nor written, and a segment of the work list none of whose tensors is wanted launches no workgroup. */
typedef struct ns_lossg_grads {
  float* mel;                                         /* [B, T, n_mel] */
  float* postnet;                                     /* [B, T, n_mel] */
  float* pitch;                                       /* [B, T] or [B, L] */
  float* energy;                                      /* [B, T] or [B, L] */
  float* log_d;                                       /* [B, L] */
  float* attn[4];                                     /* [B, H, T, L] each: every head is written, heads >= 1 with zeros */
} ns_lossg_grads;
/* ns_loss_forward with the record: the same validation, the same two launches, out7 bit for bit; `record` (NS_LOSSG_RECORD_BYTES,
 * 8-byte aligned) is written by the second launch.  The record, not the workspace, carries the counts to the backward, so later loss
 * calls that reuse the workspace do not disturb it. */
int ns_lossg_forward(const ns_loss_args* a, void* ws, size_t ws_bytes, float* out7, void* record, void* stream);
/* One launch on `stream`.  `a` as given to ns_lossg_forward (validated the same way, and B * H * T < 2^31), `record` as it wrote it,
 * g7 = 7 device floats, 4-byte aligned.  Returns nonzero with ns_last_error(), before any HIP call, on a null a / record / g7 / grads
 * and on an output that is not 16-byte aligned.  With every output NULL nothing is launched. */
int ns_lossg_backward(const ns_loss_args* a, const void* record, const float* g7, const ns_lossg_grads* grads, void* stream);

/* ==== VariancePredictor: a training forward and its backward (model/modules.py:233-286) ===========================================
 * Handle-less; nothing above changes (every other ABI version stays as it is).  The module is
 *   conv1d_1 -> ReLU -> layer_norm_1 -> dropout_1 -> conv1d_2 -> ReLU -> layer_norm_2 -> dropout_2 -> Linear(F, 1) -> masked_fill
 * on M = B * S rows of Cin channels, F filters, K taps ("same" padding (K - 1) / 2).  The weights are LIVE device tensors in checkpoint
 * (torch) layout, read afresh by every call; dropout is given as two uint8 keep-masks [M, F] (1 = kept) and p_drop, the kept values
 * scaled by 1 / (1 - p_drop).  Exact fp32 on the fp32 matrix cores; column sums in float64, rounded once.  No atomic, no host read;
 * equal inputs give equal bits (the split of the weight gradient's contraction is a function of the shape alone: ns_pg_plan_wgrad). */
#define NS_PG_ABI_VERSION 1
int ns_pg_abi_version(void);
typedef struct ns_pg_shape { int32_t B, S, Cin, F, K; } ns_pg_shape;
/* Device pointers, 16-byte aligned, fp32, checkpoint layout. */
typedef struct ns_pg_weights {
  const float* w1;     /* [F, Cin, K] conv_layer.conv1d_1.conv.weight */
  const float* b1;     /* [F] */
  const float* ln1_g;  /* [F] conv_layer.layer_norm_1.weight */
  const float* ln1_b;  /* [F] */
  const float* w2;     /* [F, F, K] conv_layer.conv1d_2.conv.weight */
  const float* b2;     /* [F] */
  const float* ln2_g;  /* [F] */
  const float* ln2_b;  /* [F] */
  const float* wlin;   /* [1, F] linear_layer.weight */
  const float* blin;   /* [1] linear_layer.bias */
} ns_pg_weights;
/* The outputs of ns_pg_backward: the same ten, shaped alike, and dx [B, S, Cin].  16-byte aligned.  NULL = not wanted: neither
 * computed nor written, and a launch none of whose outputs is wanted is not made. */
typedef struct ns_pg_grads {
  float *w1, *b1, *ln1_g, *ln1_b, *w2, *b2, *ln2_g, *ln2_b, *wlin, *blin, *dx;
} ns_pg_grads;
/* Host only.  The split of the weight gradient dW[n][c][j] = sum_m dz[m, n] X[m + j - pad, c] (N x KW*Cin outputs, M contracted):
 * out = {tile rows (n), tile columns (j*Cin + c), rows of m per range, ranges, tiles, workspace floats (< 2^31), accumulation chunk
 * (rows of m; 0 = one sequential sum), 0}.  Range r contracts rows [r * rows, min(M, (r + 1) * rows)) and
 * writes its partial tile to the workspace; a second pass sums the ranges in ascending order in float64.  Returns 0, or nonzero with
 * ns_last_error() for a shape the kernels refuse. */
int ns_pg_plan_wgrad(int M, int N, int Cin, int KW, int32_t out[8]);
/* Bytes of the workspace of every ns_pg_* call of this shape (0 and ns_last_error() for a refused shape), and of `saved`
 * (v1 = relu(conv1d_1), h1 = dropout_1(layer_norm_1(v1)), v2 = relu(conv1d_2): 3 * M * F floats). */
size_t ns_pg_ws_bytes(const ns_pg_shape* shape);
size_t ns_pg_saved_bytes(const ns_pg_shape* shape);
/* Kernel launches the calling thread's last ns_pg_* call enqueued. */
int ns_pg_last_launches(void);
/* Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a pointer that is not
 * 16-byte aligned, K even or <= 0, F not 256 or 512, Cin not a multiple of 4 (forward, backward and dgrad: of 16), B * S * max(F, Cin)
 * >= 2^31, p_drop outside [0, 1), keep-masks without p_drop > 0 or p_drop > 0 without them, a workspace smaller than ns_pg_ws_bytes.
 * pred [B, S] = mask ? +0.0 : h2 . wlin + blin.  mask: uint8 [B * S], 1 = padded, nullable.  saved: ns_pg_saved_bytes, or NULL
 * (nothing kept: the no_grad forward).  Five launches. */
int ns_pg_forward(const ns_pg_shape* shape, const ns_pg_weights* weights, const float* x, const uint8_t* mask, const uint8_t* keep1,
                  const uint8_t* keep2, float p_drop, float* pred, void* saved, void* ws, size_t ws_bytes, void* stream);
/* The gradient of sum_m g[m] pred[m] with respect to every non-NULL member of grads, from `saved` as ns_pg_forward wrote it for the
 * same arguments.  dp = mask ? +0.0 : g is a selection: a NaN in g behind the mask reaches nothing.  Up to ten launches. */
int ns_pg_backward(const ns_pg_shape* shape, const ns_pg_weights* weights, const float* x, const uint8_t* mask, const uint8_t* keep1,
                   const uint8_t* keep2, float p_drop, const void* saved, const float* g, const ns_pg_grads* grads, void* ws,
                   size_t ws_bytes, void* stream);
/* Each kernel alone.  dW [N, Cin, KW] (torch layout) and db [N] (nullable) from dz [B*S, N] and X [B*S, Cin]; a tap outside the
 * utterance's [0, S) rows reads as zero. */
int ns_pg_op_wgrad(const float* dz, const float* X, int B, int S, int N, int Cin, int KW, float* dW, float* db, void* ws, size_t ws_bytes,
                   void* stream);
/* dX [B*S, Cin] = sum_j sum_n dz[m - j + pad, n] W[n][c][j] from W [N, Cin, KW] in torch layout: the pack kernel, then the forward's
 * Conv1D-as-GEMM on the transposed, tap-flipped weights. */
int ns_pg_op_dgrad(const float* dz, const float* W, int B, int S, int N, int Cin, int KW, float* dX, void* ws, size_t ws_bytes, void* stream);
/* The row-local backward of  y = dropout(LayerNorm(v)), v = relu(conv + b)  on M rows of F columns.  tail == 0: dy [M, F] is the
 * upstream gradient of y.  tail != 0: the upstream is g [M] through Linear(F, 1) and the mask (dy is ignored), wlin / ln_b are read,
 * d_wlin [F] and d_blin [1] are written.  Writes dz [M, F] = dv gated by v > 0, d_ln_g, d_ln_b, d_b [F] each (all required).  keep
 * [M, F] iff p_drop > 0. */
int ns_pg_op_row_backward(int tail, const float* dy, const float* g, const uint8_t* mask, const float* v, const float* ln_g,
                          const float* ln_b, const float* wlin, const uint8_t* keep, float p_drop, int M, int F, float* dz, float* d_ln_g,
                          float* d_ln_b, float* d_b, float* d_wlin, float* d_blin, void* ws, size_t ws_bytes, void* stream);

/* ==== MultiHeadAttention (self-attention): a training forward and its backward (transformer/SubLayers.py:8-59) =====================
 * Handle-less; nothing above changes (every other ABI version stays as it is).  With q = k = v = x [B, S, d], M = B * S rows, H heads,
 * dk = d / H, c = 1 / sqrt(dk):
 *   qkv = x [Wq; Wk; Wv]^T + [bq; bk; bv]      [M, 3d], head h at h * dk inside each third
 *   P   = softmax_j(c Q K^T), keys j >= lens[b] masked     per (b, h); never written to memory
 *   ctx = merge_heads(P V);  z = dropout(ctx Wfc^T + bfc) + x;  y = LayerNorm(z)
 * Padded QUERY rows are computed like any other and y is not masked (FFTBlock does that outside).  The weights are LIVE device tensors
 * in checkpoint layout; dropout is a uint8 keep-mask [M, d] (1 = kept) and p_drop.  Exact fp32 on the fp32 matrix cores; column sums,
 * row statistics and D = dctx . ctx in float64, rounded once.  No atomic, no host read; equal inputs give equal bits.
 * lens: int64 [B] on the device, NULL = every key valid.  An utterance with lens[b] == 0 has NaN in ctx (as the reference has). */
#define NS_AG_ABI_VERSION 1
int ns_ag_abi_version(void);
typedef struct ns_ag_shape { int32_t B, S, d, H; } ns_ag_shape;
/* Device pointers, 16-byte aligned, fp32, checkpoint layout. */
typedef struct ns_ag_weights {
  const float* wq;    /* [d, d] w_qs.weight */
  const float* bq;    /* [d] */
  const float* wk;    /* [d, d] w_ks.weight */
  const float* bk;    /* [d] */
  const float* wv;    /* [d, d] w_vs.weight */
  const float* bv;    /* [d] */
  const float* wfc;   /* [d, d] fc.weight */
  const float* bfc;   /* [d] */
  const float* ln_g;  /* [d] layer_norm.weight */
  const float* ln_b;  /* [d] */
} ns_ag_weights;
/* The outputs of ns_ag_backward: the same ten, shaped alike, and dx [B, S, d].  16-byte aligned.  NULL = not wanted: neither
 * computed nor written, and a launch none of whose outputs is wanted is not made. */
typedef struct ns_ag_grads {
  float *wq, *bq, *wk, *bk, *wv, *bv, *wfc, *bfc, *ln_g, *ln_b, *dx;
} ns_ag_grads;
/* Bytes of the workspace of ns_ag_forward / ns_ag_backward of this shape (0 and ns_last_error() for a refused shape), and of `saved`:
 * qkv [M, 3d] | ctx [M, d] | z [M, d] | lse [B, H, S] floats, in this order, dense. */
size_t ns_ag_ws_bytes(const ns_ag_shape* shape);
size_t ns_ag_saved_bytes(const ns_ag_shape* shape);
/* Kernel launches the calling thread's last ns_ag_* call enqueued. */
int ns_ag_last_launches(void);
/* Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a pointer that is not 16-byte
 * aligned (lens: 8), d not 256 or 512, d % H != 0, dk not in {32, 64, 128}, B * S * 3d >= 2^31, p_drop outside [0, 1), a keep-mask
 * without p_drop > 0 or p_drop > 0 without one, a workspace smaller than ns_ag_ws_bytes.
 * y [B, S, d].  saved: ns_ag_saved_bytes, or NULL (nothing kept, no lse launch: the no_grad forward).
 * Launches: 1 (pack) + G(M, 3d, d) + 1 (attention) + 1 (lse, only with `saved`) + G(M, d, d) + 1 (row), where G(M, N, K) is the
 * Conv1D-as-GEMM dispatch's own launch count for that shape (ns_plan_gemm_launches, 1 or 2). */
int ns_ag_forward(const ns_ag_shape* shape, const ns_ag_weights* weights, const float* x, const int64_t* lens, const uint8_t* keep,
                  float p_drop, float* y, void* saved, void* ws, size_t ws_bytes, void* stream);
/* The gradient of sum g[m, :] . y[m, :] (g [B, S, d], read on every row) with respect to every non-NULL member of grads, from `saved`
 * as ns_ag_forward wrote it for the same arguments.
 * Launches with every output wanted: 1 (pack) + 1 (row backward) + 2 (dWfc: GEMM, reduce) + G(M, d, d) (dctx) + 2 (attention
 * backward: the query-owning and the key-owning kernel) + 3 * 2 (dWq, dWk, dWv) + 1 (column sums of dqkv) + G(M, d, 3d) (dx, the
 * residual branch dz added in its epilogue) + 1 (final column sums) = 14 + G(M, d, d) + G(M, d, 3d).  An unwanted weight gradient
 * drops its 2 launches, dx its GEMM, the three projection biases their column sums; with nothing wanted upstream of ctx (only wfc,
 * bfc, ln_g, ln_b) the pack, dctx and the attention backward are dropped too. */
int ns_ag_backward(const ns_ag_shape* shape, const ns_ag_weights* weights, const float* x, const int64_t* lens, const uint8_t* keep,
                   float p_drop, const void* saved, const float* g, const ns_ag_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* Each new kernel alone.  lse [B, H, S] from qkv [B*S, 3d]: one launch. */
int ns_ag_op_lse(const float* qkv, const int64_t* lens, int B, int S, int d, int H, float* lse, void* stream);
/* dqkv [B*S, 3d] = (dQ | dK | dV) from qkv, ctx [B*S, d], lse and dctx [B*S, d]; dK and dV rows at keys >= lens[b] are +0.0 and
 * nothing those rows of qkv hold is read into a sum.  ws: B * H * S floats (D).  Two launches. */
int ns_ag_op_attention_backward(const float* qkv, const float* ctx, const float* lse, const float* dctx, const int64_t* lens, int B, int S,
                                int d, int H, float* dqkv, void* ws, size_t ws_bytes, void* stream);
/* The row-local backward of y = LayerNorm(z), z = dropout(u) + x on M rows of d columns from dy [M, d] and the saved z: dz (the
 * residual branch of dx), du = dz keep / (1 - p), d_ln_g, d_ln_b and d_bfc = column sums of du (all required).  keep [M, d] iff
 * p_drop > 0.  ws: ceil(M / 64) * 5 * d doubles.  Two launches. */
int ns_ag_op_row_backward(const float* dy, const float* z, const float* ln_g, const uint8_t* keep, float p_drop, int M, int d, float* dz,
                          float* du, float* d_ln_g, float* d_ln_b, float* d_bfc, void* ws, size_t ws_bytes, void* stream);

/* ==== MultiHeadAttention as cross-attention: a training forward and its backward (FFTBlock2.crs_attn, transformer/Layers.py:61-64) ====
 * Handle-less; nothing above changes (every other ABI version stays as it is).  With q = tgt [B, T, d], k = v = src [B, L, d], H heads,
 * dk = d / H, c = 1 / sqrt(dk):
 *   Q  = tgt Wq^T + bq                      [B*T, d]
 *   KV = src [Wk; Wv]^T + [bk; bv]          [B*L, 2d] = K | V, head h at h * dk inside each half (what ns_aln_op_cross_attention reads)
 *   A  = softmax_l(c Q K^T), keys l >= src_lens[b] masked     [B, H, T, L], WRITTEN: final probabilities, exact 0 at masked keys
 *   ctx = merge_heads(A V);  z = dropout(ctx Wfc^T + bfc) + tgt;  y = LayerNorm(z)
 * Padded QUERY rows are computed like any other and y is not masked (FFTBlock2 does that outside).  The map A is an output of the
 * forward and an input of the backward, with an upstream gradient dA of its own (the guided-attention loss, ns_lossg_backward's
 * d_attn).  Exact fp32 on the fp32 matrix cores; column sums, row statistics and D in float64, rounded once.  No atomic, no host read;
 * equal inputs give equal bits.  src_lens: int64 [B] on the device, required.  An utterance with src_lens[b] == 0 has NaN in A and ctx
 * (as the reference has). */
#define NS_XG_ABI_VERSION 1
int ns_xg_abi_version(void);
typedef struct ns_xg_shape { int32_t B, T, L, d, H; } ns_xg_shape;
/* Device pointers, 16-byte aligned, fp32, checkpoint layout: the ten of ns_ag_weights. */
typedef struct ns_xg_weights {
  const float* wq;    /* [d, d] w_qs.weight */
  const float* bq;    /* [d] */
  const float* wk;    /* [d, d] w_ks.weight */
  const float* bk;    /* [d] */
  const float* wv;    /* [d, d] w_vs.weight */
  const float* bv;    /* [d] */
  const float* wfc;   /* [d, d] fc.weight */
  const float* bfc;   /* [d] */
  const float* ln_g;  /* [d] layer_norm.weight */
  const float* ln_b;  /* [d] */
} ns_xg_weights;
/* The outputs of ns_xg_backward: the same ten, shaped alike, dtgt [B, T, d] and dsrc [B, L, d].  16-byte aligned.  NULL = not wanted:
 * neither computed nor written, and a launch none of whose outputs is wanted is not made. */
typedef struct ns_xg_grads {
  float *wq, *bq, *wk, *bk, *wv, *bv, *wfc, *bfc, *ln_g, *ln_b, *dtgt, *dsrc;
} ns_xg_grads;
/* Bytes of the workspace of ns_xg_forward / ns_xg_backward of this shape (0 and ns_last_error() for a refused shape), and of `saved`:
 * q [B*T, d] | kv [B*L, 2d] | ctx [B*T, d] | z [B*T, d] floats, in this order, dense. */
size_t ns_xg_ws_bytes(const ns_xg_shape* shape);
size_t ns_xg_saved_bytes(const ns_xg_shape* shape);
/* The number of query parts the key-owning backward kernel of this shape is split into, nsplit: a function of (B, H, T, L) alone, in
 * [1, 8] (0 and ns_last_error() for a refused shape).  With W = ceil(L / 128) * H * B workgroups and Q = ceil(T / 32) query tiles:
 * nsplit = 1, doubled while nsplit < 8, W * nsplit < 256 and Q / (2 nsplit) >= 4 (integer division).  So nsplit = 1 when T <= 224. */
int ns_xg_kv_splits(const ns_xg_shape* shape);
/* Kernel launches the calling thread's last ns_xg_* call enqueued. */
int ns_xg_last_launches(void);
/* Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a pointer that is not 16-byte
 * aligned (src_lens: 8), d not 256 or 512, d % H != 0, dk not in {64, 128}, B * H * T * L >= 2^31, B * max(T, L) * 2d >= 2^31, p_drop
 * outside [0, 1), a keep-mask without p_drop > 0 or p_drop > 0 without one, a workspace smaller than ns_xg_ws_bytes.
 * y [B, T, d], attn [B, H, T, L] (both written).  saved: ns_xg_saved_bytes, or NULL (nothing kept: the no_grad forward; attn is written
 * all the same).
 * Launches: 1 (pack) + G(B*T, d, d) (q) + G(B*L, 2d, d) (kv) + 1 (attention) + G(B*T, d, d) (fc) + 1 (row), where G(M, N, K) is the
 * Conv1D-as-GEMM dispatch's own launch count for that shape (ns_plan_gemm_launches, 1 or 2). */
int ns_xg_forward(const ns_xg_shape* shape, const ns_xg_weights* weights, const float* tgt, const float* src, const int64_t* src_lens,
                  const uint8_t* keep, float p_drop, float* y, float* attn, void* saved, void* ws, size_t ws_bytes, void* stream);
/* The gradient of sum g . y + sum dA . A (g [B, T, d], read on every row; dA [B, H, T, L] or NULL = zero, never read at keys l >=
 * src_lens[b]) with respect to every non-NULL member of grads, from `saved` and `attn` as ns_xg_forward wrote them for the same arguments.
 * Launches with every output wanted: 1 (pack) + 1 (row backward) + 2 (dWfc: GEMM, reduce) + G(B*T, d, d) (dctx) + 2 (attention
 * backward: the query-owning and the key-owning kernel) + 1 if nsplit > 1 (the sum of the parts) + 3 * 2 (dWq, dWk, dWv) + 2 (column
 * sums of dq and of dk | dv) + G(B*T, d, d) (dtgt, the residual branch dz added in its epilogue) + G(B*L, d, 2d) (dsrc) + 2 (final
 * column sums: over B*L row blocks, over B*T row blocks) = 16 + (nsplit > 1) + 2 G(B*T, d, d) + G(B*L, d, 2d).  An unwanted weight
 * gradient drops its 2 launches, dtgt / dsrc its GEMM, bq / (bk and bv) their column sums, (bk and bv) their final sum; with nothing
 * wanted that reads dK | dV (wk, bk, wv, bv, dsrc) the key-owning kernel and the sum of its parts are dropped; with nothing wanted
 * upstream of ctx (only wfc, bfc, ln_g, ln_b) the pack, dctx and the attention backward are dropped too. */
int ns_xg_backward(const ns_xg_shape* shape, const ns_xg_weights* weights, const float* tgt, const float* src, const int64_t* src_lens,
                   const uint8_t* keep, float p_drop, const void* saved, const float* attn, const float* g, const float* dA,
                   const ns_xg_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* The new kernels alone.  dq [B*T, d] and dkv [B*L, 2d] = (dK | dV) from q, kv, ctx [B*T, d], attn, dctx [B*T, d] and dA (nullable); dK
 * and dV rows at keys >= src_lens[b] are +0.0, and nothing those rows of kv or those columns of dA hold is read into a sum.  kv_splits
 * in [0, 8]: the number of query parts, 0 = ns_xg_kv_splits.  ws: B * H * T floats (D), rounded up to 256 bytes, plus, for more than
 * one part, parts * B * L * 2d floats.  Two launches, three with more than one part. */
int ns_xg_op_attention_backward(const float* q, const float* kv, const float* ctx, const float* attn, const float* dctx, const float* dA,
                                const int64_t* src_lens, int B, int T, int L, int d, int H, int kv_splits, float* dq, float* dkv, void* ws,
                                size_t ws_bytes, void* stream);

/* ==== PostNet: a training forward with train-mode BatchNorm1d and its backward (transformer/Layers.py:107-177) ====================
 * Handle-less; nothing above changes (every other ABI version stays as it is).  x [B, T, n_mel], M = B * T rows, layers i = 0 .. n - 1
 * with channels C_0 = n_mel, C_1 .. C_{n-1} = emb, C_n = n_mel, K taps ("same" padding (K - 1) / 2 per utterance), h_{-1} = x:
 *   u_i = conv_i(h_{i-1}) + b_i
 *   training: mu_i, var_i = mean and BIASED variance of u_i over ALL M rows (no mask); running_mean = 0.9 running_mean + 0.1 mu,
 *             running_var = 0.9 running_var + 0.1 var M / (M - 1), num_batches_tracked += 1, written by the kernels of the forward
 *   else:     mu_i, var_i = running_mean, running_var, which are only read
 *   n_i = gamma_i (u_i - mu_i) / sqrt(var_i + 1e-5) + beta_i
 *   h_i = keep_i / (1 - p_drop) * tanh(n_i) for i < n - 1, h_{n-1} = keep_{n-1} / (1 - p_drop) * n_{n-1};  y = h_{n-1} (no residual)
 * The weights are LIVE device tensors in checkpoint layout; dropout is n uint8 keep-masks [M, C_{i+1}] (1 = kept) and p_drop.  Exact
 * fp32 GEMMs on the fp32 matrix cores; every column sum, mu and rstd in float64, every stored value rounded once.  No atomic, no host
 * read; equal inputs give equal bits. */
#define NS_PN_ABI_VERSION 1
#define NS_PN_MAX_LAYERS 5
int ns_pn_abi_version(void);
typedef struct ns_pn_shape { int32_t B, T, n_mel, emb, K, n; } ns_pn_shape;
/* Device pointers of one layer, 16-byte aligned (num_batches_tracked: 8), fp32, checkpoint layout.  The three buffers are written by
 * ns_pn_forward with training != 0 and are never written otherwise. */
typedef struct ns_pn_layer {
  const float* w;      /* [C_{i+1}, C_i, K] convolutions.{i}.0.conv.weight */
  const float* b;      /* [C_{i+1}] convolutions.{i}.0.conv.bias */
  const float* gamma;  /* [C_{i+1}] convolutions.{i}.1.weight */
  const float* beta;   /* [C_{i+1}] convolutions.{i}.1.bias */
  float* running_mean; /* [C_{i+1}] */
  float* running_var;  /* [C_{i+1}] */
  int64_t* num_batches_tracked; /* [] int64 */
} ns_pn_layer;
typedef struct ns_pn_weights { ns_pn_layer layer[NS_PN_MAX_LAYERS]; } ns_pn_weights;  /* layers >= n are ignored */
/* The outputs of ns_pn_backward, shaped like the parameters, and dx [B, T, n_mel].  16-byte aligned.  NULL = not wanted: neither
 * computed nor written, and a launch none of whose outputs is wanted is not made. */
typedef struct ns_pn_layer_grads { float *w, *b, *gamma, *beta; } ns_pn_layer_grads;
typedef struct ns_pn_grads { ns_pn_layer_grads layer[NS_PN_MAX_LAYERS]; float* dx; } ns_pn_grads;
/* Bytes of the workspace of every ns_pn_forward / ns_pn_backward of this shape (0 and ns_last_error() for a refused shape), and of
 * `saved`: u_0 | h_0 | u_1 | h_1 | ... | u_{n-1} as floats ([M, C_{i+1}] each; h_{n-1} is y and is not kept), then per layer mu [emb] and
 * rstd [emb] as float64: 4 M (2 (n - 1) emb + n_mel) + 16 n emb bytes. */
size_t ns_pn_ws_bytes(const ns_pn_shape* shape);
size_t ns_pn_saved_bytes(const ns_pn_shape* shape);
/* Kernel launches the calling thread's last ns_pn_* call enqueued. */
int ns_pn_last_launches(void);
/* Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a pointer that is not 16-byte
 * aligned, emb not 256 or 512, n_mel not a multiple of 16 in [16, 128], K even or above 9, n outside [2, 5], B * T * emb >= 2^31,
 * training with B * T == 1, a shape the Conv1D-as-GEMM dispatch or the weight gradient's plan refuses, p_drop outside [0, 1),
 * keep-masks without p_drop > 0 or p_drop > 0 without all n of them, a workspace smaller than ns_pn_ws_bytes.
 * y [B, T, n_mel].  keep: n pointers (NULL itself allowed when p_drop == 0).  saved: ns_pn_saved_bytes, or NULL (nothing kept).
 * Launches: ceil(n / 2) (pack) + per layer G(M, C_{i+1}, K C_i) (the dispatch's own count, ns_plan_gemm_launches) + 1 (column sums,
 * training only) + 1 (finish) + 1 (apply). */
int ns_pn_forward(const ns_pn_shape* shape, const ns_pn_weights* weights, int training, const float* x, const uint8_t* const* keep,
                  float p_drop, float* y, void* saved, void* ws, size_t ws_bytes, void* stream);
/* The gradient of sum g . y (g [B, T, n_mel]) with respect to every non-NULL member of grads, from `saved` as ns_pn_forward wrote it
 * for the same arguments.  training != 0: the batch statistics are differentiated; else mu and var are constants.  No buffer is
 * written.  Layers are walked from the last to the first and the walk stops below the lowest layer anything is wanted from.
 * Per visited layer: 1 (column sums of dy and dy xhat) + 1 (finish) — both dropped when training == 0 and neither gamma nor beta is
 * wanted — + 1 (dz) + 2 (d_weight: GEMM, reduce; 3 on the last layer, whose dz is padded to 128 columns and whose first n_mel rows
 * are copied out) + G (dh_{i-1}, or dx on layer 0; not on the lowest visited layer unless that is layer 0 and dx is wanted); plus
 * ceil(k / 2) pack launches for the k data gradients and 1 for all wanted d_bias. */
int ns_pn_backward(const ns_pn_shape* shape, const ns_pn_weights* weights, int training, const float* x, const uint8_t* const* keep,
                   float p_drop, const void* saved, const float* g, const ns_pn_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* Each new kernel alone, on M rows of C columns (C a multiple of 16 up to 512).  stats [2][C] float64 = mu | rstd.
 * training != 0: from u [M, C], and running_mean / running_var / num_batches_tracked (all three or none) updated; ws: ceil(M / 32) * 2
 * * C doubles; two launches.  training == 0: from running_mean / running_var alone (u unused); one launch. */
int ns_pn_op_stats(const float* u, int M, int C, int training, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                   double* stats, void* ws, size_t ws_bytes, void* stream);
/* h [M, C] = keep / (1 - p) * tanh(gamma (u - mu) rstd + beta); last != 0: without the tanh.  keep [M, C] iff p_drop > 0.  One launch. */
int ns_pn_op_apply(const float* u, const double* stats, const float* gamma, const float* beta, const uint8_t* keep, float p_drop, int last,
                   int M, int C, float* h, void* stream);
/* With dy = dh keep / (1 - p) (1 - (h (1 - p))^2) (last != 0: without the tanh factor, h unused) and xhat = (u - mu) rstd:
 * d_beta = sum dy, d_gamma = sum dy xhat (both required), means [2][C] float64 = their means over M.  ws as ns_pn_op_stats.  Two launches. */
int ns_pn_op_bwd_reduce(const float* dh, const float* u, const float* h, const double* stats, const uint8_t* keep, float p_drop, int last,
                        int M, int C, float* d_gamma, float* d_beta, double* means, void* ws, size_t ws_bytes, void* stream);
/* dz [M, ldz] = gamma rstd (dy - means[0] - xhat means[1]), or gamma rstd dy when means is NULL (eval); ldz = C, or 128 >= C with
 * columns [C, 128) written as zeros.  d_bias [C] (nullable) = column sums of the unrounded float64 dz.  ws: ceil(M / 32) * C doubles.
 * One launch, two with d_bias. */
int ns_pn_op_bwd_apply(const float* dh, const float* u, const float* h, const double* stats, const double* means, const float* gamma,
                       const uint8_t* keep, float p_drop, int last, int M, int C, int ldz, float* dz, float* d_bias, void* ws,
                       size_t ws_bytes, void* stream);
/* dW [N, Cin, KW] for N < 128 (a multiple of 16) from dz [B*S, 128] whose columns [N, 128) are zero: the N = 128 plan of
 * ns_pg_plan_wgrad into a scratch, the first N rows copied out.  ws: the plan's floats + 128 * Cin * KW floats, each rounded up to
 * 256 bytes.  Three launches. */
int ns_pn_op_wgrad_narrow(const float* dz, const float* X, int B, int S, int N, int Cin, int KW, float* dW, void* ws, size_t ws_bytes,
                          void* stream);

/* ==== VarianceAdaptor: the two pieces its training path lacked, forward and backward (model/modules.py:17-159, 195-230) ============
 * Handle-less; nothing above changes (every other ABI version stays as it is).  The three predictors are ns_pg_*; these are the
 * variance embedding (bucketize + nn.Embedding + add) and the length regulator.  Every sum is float64 in an order that depends on the
 * shape alone and is rounded once: no atomic, no host read; equal inputs give equal bits.
 * Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a misaligned pointer (16 bytes
 * for the float tensors and the workspace, 8 for int64, 4 for int32, target and bins), a non-positive size, D not a multiple of 4,
 * n_bins < 2, rows * D >= 2^31, a shape ns_va_plan_embed refuses, a workspace smaller than ns_va_embed_ws_bytes. */
#define NS_VA_ABI_VERSION 1
int ns_va_abi_version(void);
/* Kernel launches the calling thread's last ns_va_* call enqueued. */
int ns_va_last_launches(void);
/* The embedding gradient's plan, without a GPU: out = { row blocks, rows per block, slab width (columns per workgroup), column slabs,
 * LDS bytes per workgroup (n_bins * slab * 8, at most 65536), launches, threads per workgroup, 0 }.  Row blocks are ceil(M / 512); the
 * slab is the widest power of two up to 64 whose table fits.  Returns 0, or nonzero with ns_last_error() for a shape it cannot hold
 * (D % 4 != 0, n_bins < 2, n_bins > 2048: a table past the limit even at 4 columns); there is no fall-back. */
int ns_va_plan_embed(int M, int D, int n_bins, int32_t out[8]);
/* Bytes of ns_va_op_embed_bwd's workspace: float64 partials [row blocks][n_bins][D]; 0 and ns_last_error() for a refused shape. */
size_t ns_va_embed_ws_bytes(int M, int D, int n_bins);
/* y [M, D] = x + table[idx], idx [M] (int32, written) = torch.bucketize(target [M], bins [n_bins - 1]) with right=False, NaN ->
 * n_bins - 1: the index ns_op_bucketize gives.  Unmasked: every row takes the embedding of its target.  One launch. */
int ns_va_op_embed_fwd(const float* x, const float* target, const float* bins, const float* table, int M, int D, int n_bins, float* y,
                       int32_t* idx, void* stream);
/* d_table [n_bins, D] = the sum of g [M, D]'s rows per index, over all M rows; a bin no row hits is +0.0; an index outside [0, n_bins)
 * contributes nothing.  (The gradient of x is g itself.)  Two launches. */
int ns_va_op_embed_bwd(const float* g, const int32_t* idx, int M, int D, int n_bins, float* d_table, void* ws, size_t ws_bytes, void* stream);
/* duration [B, L] int64 non-NULL: cum [B, L] (int32, inclusive prefix sums of max(d, 0), saturated at 2^31 - 1) and mel_len [B] (int64,
 * the uncropped total) are written (one launch).  out [B, T, D] non-NULL: frame t of utterance b = x [B, L, D]'s row of the phoneme
 * whose [cum[l-1], cum[l]) holds t, +0.0 at and past the total; frames at or past T are dropped (one launch; reads cum, which the same
 * call may have written).  At least one of the two; duration NULL takes cum as input and leaves mel_len alone. */
int ns_va_op_lr_fwd(const float* x, const int64_t* duration, int B, int L, int D, int T, float* out, int32_t* cum, int64_t* mel_len,
                    void* stream);
/* d_x [B, L, D] = the sum of g [B, T, D] over t in [cum[l-1], min(cum[l], T)) in t order; +0.0 for duration 0.  Frames at or past an
 * utterance's total are never read.  One launch. */
int ns_va_op_lr_bwd(const float* g, const int32_t* cum, int B, int L, int D, int T, float* d_x, void* stream);
/* ---- the Gaussian length regulator in the hard one's place (model/modules.py:162-192 wired as length_regulator = "gaussian") --------
 * Additions to the family; NS_VA_ABI_VERSION stays 1.  With c_l = cumsum(d)_l - d_l / 2, d = max(duration, 0), and
 * lim_b = min(max(mel_len_b, 0), T):
 *   w_lt = expf(-0.01f (t - c_l)^2) / (sum_l expf(-0.01f (t - c_l)^2) + 1e-20f)
 *   out[b, t] = sum_l w_lt x[b, l] for t < lim_b, +0.0 at and past it          d_x[b, l] = sum_{t < lim_b} w_lt g[b, t]
 * Only x takes a gradient (the durations are integers, the range is the constant 10).  The backward generates the forward's own
 * weights, bit for bit, and sums in t order on the fp32 matrix cores; no atomic, no host read; equal inputs give equal bits.
 * Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a misaligned pointer (16 bytes
 * for the float tensors and the workspace, 8 for int64), a non-positive size, B > 65535, D not a multiple of 4, B * L * D or
 * B * T * D >= 2^31, T >= 2^20 (below it the fp32 centres are exact), a workspace smaller than ns_va_gu_ws_bytes. */
/* Bytes of the workspace of ns_va_op_gu_fwd and ns_va_op_gu_bwd at this shape (the larger of the two; D does not enter); 0 and
 * ns_last_error() for a refused shape. */
size_t ns_va_gu_ws_bytes(int B, int L, int T);
/* duration [B, L] int64 -> mel_len [B] (int64, the uncropped total of max(d, 0)) and saved [B, L] (fp32, the centres: all the backward
 * keeps besides mel_len); out [B, T, D] from x [B, L, D] by the launch the inference side makes on the dense grid.  Three launches
 * (prepare, centres, upsample).  out NULL: the prepare launch alone (x and T are not read; ws as for T = 1) — for a caller that must
 * read mel_len before it can choose T. */
int ns_va_op_gu_fwd(const float* x, const int64_t* duration, int B, int L, int D, int T, float* out, float* saved, int64_t* mel_len, void* ws,
                    size_t ws_bytes, void* stream);
/* d_x [B, L, D] from g [B, T, D], the saved centres and own_len [B] (int64: the forward's mel_len; NULL: every row below T is live, the
 * reference module's plain form).  Rows of g at or past lim_b, and rows further than 102 frames from every centre of a 32-phoneme tile,
 * are never read by that tile.  w_out (nullable) [B, L, T]: the weights the backward used, +0.0 where it used none (B * L * T < 2^31).
 * Two launches (denominators, contraction). */
int ns_va_op_gu_bwd(const float* g, const float* saved, const int64_t* own_len, int B, int L, int D, int T, float* d_x, float* w_out, void* ws,
                    size_t ws_bytes, void* stream);
/* The same with the 102-frame band switched off: every tile walks every row below lim_b.  The same bits for finite g; for
 * tools/gaussian_grad_bench.py and the band's test only. */
int ns_va_op_gu_bwd_unbanded(const float* g, const float* saved, const int64_t* own_len, int B, int L, int D, int T, float* d_x, float* w_out,
                             void* ws, size_t ws_bytes, void* stream);

/* ==== PositionwiseFeedForward: a training forward and its backward (transformer/SubLayers.py:62-95) ================================
 * Handle-less; nothing above changes (every other ABI version stays as it is).  With x [B, S, d], M = B * S rows, "same"-padded
 * convolutions along S whose taps never leave an utterance's [0, S) rows (a tap outside reads zero):
 *   h = relu(conv_K1(x, w1) + b1)               [M, d_inner]
 *   u = conv_K2(h, w2) + b2                     [M, d]
 *   z = u keep / (1 - p_drop) + x;  y = LayerNorm(z) ln_g + ln_b          y is not masked (FFTBlock does that outside)
 * The weights are LIVE device tensors in checkpoint (torch Conv1d) layout; dropout is a uint8 keep-mask [M, d] (1 = kept) and p_drop.
 * Exact fp32 on the fp32 matrix cores; row statistics and column sums in float64, rounded once.  No atomic, no host read; equal
 * inputs give equal bits.  The ReLU backward gates on the SAVED h (dh = h > 0 ? da : +0.0, a select), so the gradients are those of
 * the forward that ran. */
#define NS_FG_ABI_VERSION 1
int ns_fg_abi_version(void);
typedef struct ns_fg_shape { int32_t B, S, d, d_inner, K1, K2; } ns_fg_shape;
/* Device pointers, 16-byte aligned, fp32, checkpoint layout. */
typedef struct ns_fg_weights {
  const float* w1;    /* [d_inner, d, K1] w_1.weight */
  const float* b1;    /* [d_inner] */
  const float* w2;    /* [d, d_inner, K2] w_2.weight */
  const float* b2;    /* [d] */
  const float* ln_g;  /* [d] layer_norm.weight */
  const float* ln_b;  /* [d] */
} ns_fg_weights;
/* The outputs of ns_fg_backward: the same six, shaped alike, and dx [B, S, d].  16-byte aligned.  NULL = not wanted: neither computed
 * nor written, and a launch none of whose outputs is wanted is not made. */
typedef struct ns_fg_grads {
  float *w1, *b1, *w2, *b2, *ln_g, *ln_b, *dx;
} ns_fg_grads;
/* Bytes of the workspace of ns_fg_forward / ns_fg_backward of this shape (0 and ns_last_error() for a refused shape), and of `saved`:
 * h [M, d_inner] | z [M, d] floats, in this order, dense. */
size_t ns_fg_ws_bytes(const ns_fg_shape* shape);
size_t ns_fg_saved_bytes(const ns_fg_shape* shape);
/* Kernel launches the calling thread's last ns_fg_* call enqueued. */
int ns_fg_last_launches(void);
/* Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a pointer that is not 16-byte
 * aligned, d not 256 or 512, d_inner not a positive multiple of 256, K1 or K2 not odd and positive, B * S * d_inner >= 2^31, a shape
 * the Conv1D-as-GEMM dispatch or the weight gradient's plan (ns_pg_plan_wgrad) refuses, p_drop outside [0, 1), a keep-mask without
 * p_drop > 0 or p_drop > 0 without one, a workspace smaller than ns_fg_ws_bytes.
 * y [B, S, d].  saved: ns_fg_saved_bytes, or NULL (nothing kept: the no_grad forward; the same launches, the same y).
 * Launches: 1 (pack of w1 and w2) + G(M, d_inner, K1 d) (h, bias and ReLU in its epilogue) + G(M, d, K2 d_inner) (u) + 1 (row), where
 * G(M, N, KW Cin) is the Conv1D-as-GEMM dispatch's own launch count for that shape (ns_plan_gemm_launches(M, N, Cin, KW, 0), 1 or 2). */
int ns_fg_forward(const ns_fg_shape* shape, const ns_fg_weights* weights, const float* x, const uint8_t* keep, float p_drop, float* y,
                  void* saved, void* ws, size_t ws_bytes, void* stream);
/* The gradient of sum g[m, :] . y[m, :] (g [B, S, d], read on every row) with respect to every non-NULL member of grads, from `saved`
 * as ns_fg_forward wrote it for the same arguments.
 * Launches with every output wanted: 1 (row backward: dz, du, the partials of d_ln_g, d_ln_b, d_b2) + 2 (dW2: GEMM, reduce) + 1 (pack
 * of the transposed, tap-flipped w2 and w1) + G(M, d_inner, K2 d) (da) + 1 (ReLU gate, with the partials of d_b1) + 1 (d_b1: column
 * finish at width d_inner) + 2 (dW1) + G(M, d, K1 d_inner) (dx, the residual branch dz added in its epilogue) + 1 (column finish at
 * width d: d_ln_g, d_ln_b, d_b2) = 9 + G(M, d_inner, K2 d) + G(M, d, K1 d_inner).  An unwanted weight gradient drops its 2 launches, dx
 * its GEMM, b1 its column finish, all of ln_g, ln_b and b2 theirs; with none of w1, b1 and dx wanted the pack, da and the gate are
 * dropped too: the row backward, dW2's two and the last finish remain.  With no output wanted nothing is launched. */
int ns_fg_backward(const ns_fg_shape* shape, const ns_fg_weights* weights, const float* x, const uint8_t* keep, float p_drop,
                   const void* saved, const float* g, const ns_fg_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* The new kernel alone.  dh [M, d_inner] = h > 0 ? da : +0.0 (a select: what da holds where h <= 0 reaches nothing; dh may be da) and,
 * unless d_b1 is NULL, d_b1 [d_inner] = the column sums of dh: float64 partials per 64 rows, added in ascending order, rounded once.
 * d_inner a positive multiple of 256, M * d_inner < 2^31.  ws (needed with d_b1 only): ceil(M / 64) * 5 * d_inner doubles.
 * One launch, two with d_b1. */
int ns_fg_op_relu_gate(const float* da, const float* h, int M, int d_inner, float* dh, float* d_b1, void* ws, size_t ws_bytes,
                       void* stream);
/* ---- The opt-in "bf16" matmul mode of the same layer (additions: NS_FG_ABI_VERSION is unchanged) ----------------------------------
 * Mixed precision with fp32 master weights.  Parameters, gradients, x, h, z, y, biases, the LayerNorm, dropout, the residuals, the ReLU
 * gate and every column sum stay fp32 / float64 exactly as above; `saved` has the same layout (ns_fg_saved_bytes).  Only the six
 * contractions change: each rounds BOTH operands to bf16 (round to nearest even, the plain cast: a NaN survives) and accumulates in
 * fp32 on the bf16 matrix cores:
 *   h   = relu(conv_K1(bf x, bf w1) + b1)        u = conv_K2(bf h, bf w2) + b2
 *   dW2 = wgrad(bf du, bf h)                     da = conv(bf du, bf w2 transposed, tap-flipped);   dh = gate(da, saved h)
 *   dW1 = wgrad(bf dh, bf x)                     dx = conv(bf dh, bf w1 transposed, tap-flipped) + dz   (dz added in fp32)
 * Taps never cross utterances; a weight-gradient element whose every tap lies outside its utterance is exactly +0.0.  No atomic, no
 * host read; every sum has one order that depends on the shape alone.  The live weights are rounded into bf16 planes by a pack launch
 * of each call.  The three module-level entry points take the arguments of their namesakes above and refuse alike; the shape must
 * also pass the bf16 GEMM and ns_fg_plan_wgrad_bf16 (both hold for every shape the checks above admit).
 * Launches: forward 4 (pack, h, u, row).  Backward with every output wanted 11: the list of ns_fg_backward with G = 1 (the bf16 GEMM
 * is always one launch); the same outputs drop the same launches.  ns_fg_last_launches reports them. */
size_t ns_fg_ws_bytes_bf16(const ns_fg_shape* shape);
int ns_fg_forward_bf16(const ns_fg_shape* shape, const ns_fg_weights* weights, const float* x, const uint8_t* keep, float p_drop, float* y,
                       void* saved, void* ws, size_t ws_bytes, void* stream);
int ns_fg_backward_bf16(const ns_fg_shape* shape, const ns_fg_weights* weights, const float* x, const uint8_t* keep, float p_drop,
                        const void* saved, const float* g, const ns_fg_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* Host only.  The split of the bf16 weight gradient: the fields of ns_pg_plan_wgrad, with rows of m per range a multiple of the
 * 32-row stage.  Refuses what ns_pg_plan_wgrad refuses, and Cin that is not a multiple of 32. */
int ns_fg_plan_wgrad_bf16(int M, int N, int Cin, int KW, int32_t out[8]);
/* The new launches alone, on caller-supplied inputs (test hooks).  Every pointer 16-byte aligned; N and Cin positive multiples of 32,
 * KW odd, B * S * max(N, Cin) < 2^31; each refuses before any HIP call.  ws: ns_fg_op_bf16_ws_bytes(B, S, N, Cin, KW) bytes (0 and
 * ns_last_error() for a refused shape), enough for either op below.
 * ns_fg_op_wgrad_bf16: dW [N, Cin, KW] (torch layout) = sum_m bf(dz[m, n]) bf(X[m + j - pad, c]) from dz [B*S, N] and X [B*S, Cin]; also
 * needs a shape ns_fg_plan_wgrad_bf16 accepts (N a multiple of 128).  Two launches (GEMM, reduce).
 * ns_fg_op_conv_bf16: W [N, Cin, KW] is the torch-layout fp32 weight; the pack launch, then the bf16 GEMM, through the code the
 * module calls.  transposed == 0, the forward form: y [B*S, N] = act(conv(bf x [B*S, Cin], bf W) + bias) + resid.  transposed != 0, the
 * data gradient: y [B*S, Cin] = sum_j sum_n bf(x[m - j + pad, n]) bf(W[n][c][j]) + bias + resid from x [B*S, N].  bias and resid are
 * nullable and added in fp32; act: 0 none, 1 ReLU; y must be neither x nor resid.  Two launches. */
size_t ns_fg_op_bf16_ws_bytes(int B, int S, int N, int Cin, int KW);
int ns_fg_op_wgrad_bf16(const float* dz, const float* X, int B, int S, int N, int Cin, int KW, float* dW, void* ws, size_t ws_bytes,
                        void* stream);
int ns_fg_op_conv_bf16(const float* x, const float* W, const float* bias, const float* resid, int B, int S, int N, int Cin, int KW,
                       int transposed, int act, float* y, void* ws, size_t ws_bytes, void* stream);

/* ==== TxtEncoder / MelDecoder: what the training stacks add to their FFT blocks (transformer/Models.py:33-100, 176-244) =============
 * Handle-less, no workspace; nothing above changes (every other ABI version stays as it is).  Four single-launch ops: the two forward
 * entries of the stacks (kernels the inference path already runs), the gradient of the word-embedding table, and the row mask of an
 * FFT block (transformer/Layers.py:43,46).  No atomic, no host read; equal inputs give equal bits.
 * Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a misaligned pointer (16 bytes
 * for the float tensors, 8 for int64; the uint8 mask needs none), D not 256 or 512, n_vocab < 2, B * S * D (M * D) >= 2^31, a
 * non-positive size, and, for the row mask, mask and lens both NULL or y == x.
 * The stacks of stacks.py (python) launch, over L FFT blocks, each A(forward) = ns_ag_forward's and F(forward) = ns_fg_forward's count:
 *   forward    1 (ns_st_op_embed_pos, or ns_st_op_add_pos) + sum over layers (A + 1 (row mask) + F + 1 (row mask)), + 1 when the
 *              position table is regenerated (eval() past max_seq_len: ns_op_sinusoid_table)
 *   backward   the mirror, sum over layers (1 + F(backward) + 1 + A(backward)), + 1 for the table gradient (ns_st_op_embed_grad),
 *              which a frozen embedding drops; the position add has no backward launch (its gradient is grad_output itself). */
#define NS_ST_ABI_VERSION 1 /* what ns_st_abi_version() returns */
int ns_st_abi_version(void);
/* Kernel launches the calling thread's last ns_st_* call enqueued. */
int ns_st_last_launches(void);
/* out [B, S, D] = emb[texts[b, s], :] + pos[s, :] (transformer/Models.py:83-91: src_word_emb(src_seq) + position_enc[:, :S]).  texts
 * int64 [B, S]; emb [n_vocab, D]; pos [>= S, D].  A token outside [0, n_vocab) reads row 0 (PAD); nn.Embedding would raise, this has no
 * host read to raise from.  One launch. */
int ns_st_op_embed_pos(const int64_t* texts, const float* emb, const float* pos, int B, int S, int D, int n_vocab, float* out,
                       void* stream);
/* out [B, S, D] = x + pos[s, :] (transformer/Models.py:221-233: enc_seq + position table); pos [>= S, D].  One launch. */
int ns_st_op_add_pos(const float* x, const float* pos, int B, int S, int D, float* out, void* stream);
/* d_table [n_vocab, D] = the sum of g [M, D]'s rows per token id (the backward of nn.Embedding(n_vocab, D, padding_idx=0),
 * transformer/Models.py:56-58), texts int64 [M]: float64 accumulation in ascending m, rounded once.  Row 0 (PAD) is +0.0 and g at a PAD
 * row is never read; an id no row carries is +0.0; a token outside [0, n_vocab) contributes to no row.  One launch. */
int ns_st_op_embed_grad(const float* g, const int64_t* texts, int M, int D, int n_vocab, float* d_table, void* stream);
/* y [B, S, D] = padded(b, s) ? +0.0 : x (masked_fill(mask.unsqueeze(-1), 0), transformer/Layers.py:43,46; its backward is the same op
 * on the gradient).  A select: x in a padded row is not read.  padded = mask[b, s] != 0 (uint8 [B, S]) when mask is given, else
 * s >= lens[b] (int64 [B]); at least one of the two.  Out of place.  One launch. */
int ns_st_op_row_mask(const float* x, const uint8_t* mask, const int64_t* lens, int B, int S, int D, float* y, void* stream);

/* ==== MelEncoder: the Prenet and the position add behind it, a training forward and its backward ===================================
 * (transformer/Models.py:145-146,151,162; transformer/Layers.py:11-26).  Handle-less; nothing above changes (every other ABI version
 * stays as it is).  With mels [B, T, n_mel], M = B * T rows:
 *   xin = mels with frame 0 of every utterance replaced by +0.0 (Models.py:145-146)     [M, n_mel]
 *   h1 = relu(xin w1^T + b1);  h2 = relu(h1 w2^T + b2)  (Layers.py:23)                   [M, d] each
 *   y  = h2 keep / (1 - p_drop) + pos[t, :]             (Layers.py:24, Models.py:151,162)
 * The weights are LIVE device tensors in checkpoint (torch nn.Linear) layout; dropout is a uint8 keep-mask [M, d] (nonzero = kept) and
 * p_drop.  Exact fp32 on the fp32 matrix cores; y and the column sums in float64, rounded once.  No atomic, no host read; equal inputs
 * give equal bits.  Both ReLU backwards gate on the SAVED activations (a select), so the gradients are those of the forward that ran.
 * The stack of FFTBlock2 behind it (Layers.py:51-70) is composed in python from ns_xg_*, ns_fg_* and ns_st_op_row_mask. */
#define NS_ME_ABI_VERSION 1 /* what ns_me_abi_version() returns */
int ns_me_abi_version(void);
typedef struct ns_me_shape { int32_t B, T, n_mel, d; } ns_me_shape;
/* Device pointers, 16-byte aligned, fp32, checkpoint layout. */
typedef struct ns_me_weights {
  const float* w1; /* [d, n_mel] prenet.w_1.weight (Layers.py:18) */
  const float* b1; /* [d] */
  const float* w2; /* [d, d] prenet.w_2.weight (Layers.py:19) */
  const float* b2; /* [d] */
} ns_me_weights;
/* The outputs of ns_me_backward: dmels [B, T, n_mel] and the four parameter gradients, shaped as the weights.  16-byte aligned.  NULL =
 * not wanted: neither computed nor written, and a launch none of whose outputs is wanted is not made. */
typedef struct ns_me_grads {
  float *dmels, *w1, *b1, *w2, *b2;
} ns_me_grads;
/* Bytes of the workspace of ns_me_forward / ns_me_backward of this shape (0 and ns_last_error() for a refused shape), and of `saved`:
 * xin [M, n_mel] | h1 [M, d] | h2 [M, d] floats, in this order, dense. */
size_t ns_me_ws_bytes(const ns_me_shape* shape);
size_t ns_me_saved_bytes(const ns_me_shape* shape);
/* Kernel launches the calling thread's last ns_me_* call enqueued. */
int ns_me_last_launches(void);
/* Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null argument, a pointer that is not 16-byte
 * aligned, d not 256 or 512, n_mel not a positive multiple of 4, B or T not positive, B * T * max(d, n_mel) >= 2^31, a shape the Conv1D-as-GEMM
 * dispatch or the weight gradient's plan (ns_pg_plan_wgrad) refuses (the dispatch takes Cin only as a multiple of 16, so in effect n_mel
 * must be one: 4, 20 or 84 are refused with its message), p_drop outside [0, 1), a keep-mask without p_drop > 0 or
 * p_drop > 0 without one, a workspace smaller than ns_me_ws_bytes.
 * mels is never written.  pos [>= T, d] (the position table of the call).  y [B, T, d].  saved: ns_me_saved_bytes, or NULL (nothing
 * kept: the no_grad forward; the same launches, the same y).
 * Launches: 1 (pack of w1 and w2) + 1 (frame-0 select) + G(M, d, n_mel) (h1, bias and ReLU in its epilogue) + G(M, d, d) (h2, the same)
 * + 1 (dropout + position add), where G(M, N, Cin) is the Conv1D-as-GEMM dispatch's own launch count for that shape
 * (ns_plan_gemm_launches(M, N, Cin, 1, 0), 1 or 2). */
int ns_me_forward(const ns_me_shape* shape, const ns_me_weights* weights, const float* mels, const float* pos, const uint8_t* keep,
                  float p_drop, float* y, void* saved, void* ws, size_t ws_bytes, void* stream);
/* The gradient of sum g[m, :] . y[m, :] (g [B, T, d], read only, on every row) with respect to every non-NULL member of grads, from
 * `saved` as ns_me_forward wrote it for the same arguments.  Frame 0 of dmels is +0.0 (the forward replaced that frame).
 * Launches with every output wanted: 1 (dropout + ReLU gate, with the partials of d_b2) + 1 (d_b2: column finish) + 2 (dW2: GEMM,
 * reduce) + 1 (pack of the transposed w2 and w1, one launch for both) + G(M, d, d) (da1) + 1 (ReLU gate, with the partials of d_b1) + 1
 * (d_b1: column finish) + 2 (dW1) + G(M, n_mel, d) (the data gradient) + 1 (frame-0 select into dmels) = 10 + G(M, d, d) +
 * G(M, n_mel, d).  An unwanted weight gradient drops its 2 launches, b1 and b2 their column finish, dmels its GEMM and its select;
 * with none of w1, b1 and dmels wanted the pack, da1 and the second gate are dropped too: the first gate, d_b2's finish and dW2's two
 * remain.  With no output wanted nothing is launched. */
int ns_me_backward(const ns_me_shape* shape, const ns_me_weights* weights, const uint8_t* keep, float p_drop, const void* saved,
                   const float* g, const ns_me_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* The two new kernels alone.  d 256 or 512, B * T * d (M * d) < 2^31, p_drop and keep as above.
 * y [B, T, d] = h2 k + pos[t, :] in float64, rounded once, k = 1 / (1 - p_drop) where keep [B, T, d] is nonzero and 0 where it is zero
 * (keep NULL at p_drop == 0: y = h2 + pos).  Out of place.  One launch. */
int ns_me_op_drop_pos(const float* h2, const float* pos, const uint8_t* keep, float p_drop, int B, int T, int d, float* y, void* stream);
/* dh [M, d] = (keep != 0 && h2 > 0) ? g / (1 - p_drop) : +0.0 (a select: what g holds behind a dropped or gated element reaches
 * nothing, a NaN in h2 gates like a zero; dh is not g, which is only read) and, unless d_b2 is NULL, d_b2 [d] = the column sums of dh:
 * float64 partials per 64 rows, added in ascending order, rounded once.  ws (needed with d_b2 only): ceil(M / 64) * 5 * d doubles.
 * One launch, two with d_b2. */
int ns_me_op_drop_relu_gate(const float* g, const float* h2, const uint8_t* keep, float p_drop, int M, int d, float* dh, float* d_b2,
                            void* ws, size_t ws_bytes, void* stream);

/* ==== Mel head: mel_linear and the PostNet residual, a training forward and its backward ===========================================
 * (model/fastspeech2_align.py:24,83,85).  Handle-less; nothing above changes (every other ABI version stays as it is).  With
 * x [B, T, d] (the decoder's output), M = B * T rows:
 *   y = x w^T + b                      (fastspeech2_align.py:83, nn.Linear(decoder_hidden, n_mel_channels) of line 24)   [M, n_mel]
 *   out = postnet(y) + y               (fastspeech2_align.py:85; the add is ns_mh_op_residual, the PostNet is ns_pn_*)
 * The weight is a LIVE device tensor in checkpoint (torch nn.Linear) layout.  Exact fp32 on the fp32 matrix cores; the bias gradient
 * in float64, rounded once.  No atomic, no host read; equal inputs give equal bits.  Nothing is saved between the two calls: the
 * backward needs x and g alone.  No row is masked: the reference masks none here (a padded row of y equals the bias). */
#define NS_MH_ABI_VERSION 1 /* what ns_mh_abi_version() returns */
int ns_mh_abi_version(void);
typedef struct ns_mh_shape { int32_t B, T, d, n_mel; } ns_mh_shape;
/* Device pointers, 16-byte aligned, fp32, checkpoint layout. */
typedef struct ns_mh_weights {
  const float* w; /* [n_mel, d] mel_linear.weight (fastspeech2_align.py:24) */
  const float* b; /* [n_mel] */
} ns_mh_weights;
/* The outputs of ns_mh_backward: dx [B, T, d] and the two parameter gradients, shaped as the weights.  16-byte aligned.  NULL = not
 * wanted: neither computed nor written, and a launch none of whose outputs is wanted is not made. */
typedef struct ns_mh_grads {
  float *dx, *w, *b;
} ns_mh_grads;
/* Bytes of the workspace of ns_mh_forward / ns_mh_backward of this shape (0 and ns_last_error() for a refused shape). */
size_t ns_mh_ws_bytes(const ns_mh_shape* shape);
/* Kernel launches the calling thread's last ns_mh_* call enqueued. */
int ns_mh_last_launches(void);
/* Every launching call returns nonzero with ns_last_error(), before any HIP call, on: a null shape or weights, a null argument, a
 * pointer that is not 16-byte aligned, d not 256 or 512, n_mel not a multiple of 16 in [16, 128], B or T not positive,
 * B * T * d >= 2^31, a shape the Conv1D-as-GEMM dispatch or the weight gradient's plan (ns_pg_plan_wgrad) refuses, a workspace smaller
 * than ns_mh_ws_bytes.
 * y [B, T, n_mel] = x w^T + b (fastspeech2_align.py:83).  x is never written.  At KW = 1 the nn.Linear layout is the dispatch's
 * packed form, so the live weight is read and there is no pack launch.
 * Launches: G(M, n_mel, d), the Conv1D-as-GEMM dispatch's own launch count for that shape (ns_plan_gemm_launches(M, n_mel, d, 1, 0),
 * 1 or 2). */
int ns_mh_forward(const ns_mh_shape* shape, const ns_mh_weights* weights, const float* x, float* y, void* ws, size_t ws_bytes,
                  void* stream);
/* The gradient of sum g[m, :] . y[m, :] (g [B, T, n_mel], read only, on every row) with respect to every non-NULL member of grads
 * (the backward of fastspeech2_align.py:83), from x as ns_mh_forward read it.
 * Launches: 1 (g padded to 128 columns, with the partials of d_b; wanted by w or b) + 1 (d_b: bias finish) + 3 (dW at the padded
 * width: GEMM, fixed-order reduce, copy of the first n_mel rows) + 1 (pack of w^T) + G(M, d, n_mel) (dx, reading g at row stride
 * n_mel) = 6 + G(M, d, n_mel) with every output wanted.  An unwanted output drops its launches; with no output wanted the call
 * validates and launches nothing. */
int ns_mh_backward(const ns_mh_shape* shape, const ns_mh_weights* weights, const float* x, const float* g, const ns_mh_grads* grads,
                   void* ws, size_t ws_bytes, void* stream);
/* The two new kernels alone.  n_mel a multiple of 16 in [16, 128], M positive.
 * dz [M, 128] = g [M, n_mel] with exact +0.0 in the columns [n_mel, 128), whatever dz held (the feed of the weight gradient at the
 * padded width); dz is not g, which is only read.  Unless d_bias is NULL, d_bias [n_mel] = the column sums of g: float64 partials per
 * 64 rows, added in ascending block order, rounded once.  ws (needed with d_bias only): ceil(M / 64) * n_mel doubles.  One launch, two
 * with d_bias. */
int ns_mh_op_pad_colsum(const float* g, int M, int n_mel, float* dz, float* d_bias, void* ws, size_t ws_bytes, void* stream);
/* out [M, n_mel] = p + x (fastspeech2_align.py:85: postnet(output) + output).  Out of place.  Its backward makes no launch: the
 * gradient of both operands is grad_output itself.  One launch. */
int ns_mh_op_residual(const float* p, const float* x, int M, int n_mel, float* out, void* stream);

/* ==== Dropout keep-masks: a counter-based generator, every mask of a training step in one launch ==================================
 * Handle-less; nothing above changes (every other ABI version stays as it is).  A mask is uint8 (1 = kept, 0 = dropped) over the flat
 * C order of its [B, S, C] elements, and its bytes are a pure function of (seed, call, stream, element index):
 *   generator  Philox4x32-10: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85,
 *              key = (seed & 0xffffffff, seed >> 32) of the 64-bit seed
 *   counter    (j, stream, call & 0xffffffff, call >> 32): stream is the 32-bit id of the mask within the call, call the 64-bit draw
 *              counter, j the block index within the mask
 *   element e  is word e & 3 of block j = e >> 2 (so a mask has fewer than 2^34 elements)
 *   keep       = word < thr, thr = floor((1.0 - p) * 4294967296.0) in float64 (ns_km_threshold)
 * So a mask does not depend on where it lies in an arena, on the masks drawn with it or on the launch geometry.
 * Arena: the masks of one draw lie back to back in the order given; a slot starts at a multiple of 16 bytes and is
 * ceil(n / 16) * 16 bytes long; the bytes of a slot behind element n - 1 are written as 0; nothing outside a slot is written.
 * No atomic, no host read, plain 16-byte vector stores; equal arguments give equal bits. */
#define NS_KM_ABI_VERSION 1      /* what ns_km_abi_version() returns */
#define NS_KM_MAX_MASKS 1024     /* masks of one table at most */
#define NS_KM_GRID_CAP 2048      /* workgroups of one ns_km_draw at most (256 threads, 4096 elements a turn); they loop over the chunks beyond */
#define NS_KM_TABLE_ROW_BYTES 32 /* a table is n_masks + 1 rows */
int ns_km_abi_version(void);
/* Kernel launches the calling thread's last ns_km_draw enqueued (1, or 0 after a refusal; ns_km_host_draw sets 0). */
int ns_km_last_launches(void);
/* One mask of a draw. */
typedef struct ns_km_mask {
  uint64_t n;      /* elements, in [1, 2^34) */
  uint32_t stream; /* the mask's id within the call */
  uint32_t thr;    /* ns_km_threshold of its drop probability; not 0 */
} ns_km_mask;
/* *thr = floor((1.0 - p) * 4294967296.0), evaluated in float64: 0.1 -> 3865470566, 0.2 -> 3435973836, 0.5 -> 2147483648.  Nonzero with
 * ns_last_error() on: a null thr, p outside (0, 1) (a NaN included), a threshold of 0 (p within 2^-32 of 1) or of 2^32 (1.0 - p == 1.0). */
int ns_km_threshold(double p, uint32_t* thr);
/* Bytes of the table of n_masks masks: (n_masks + 1) * NS_KM_TABLE_ROW_BYTES; 0 and ns_last_error() for n_masks outside
 * [1, NS_KM_MAX_MASKS]. */
size_t ns_km_table_bytes(int n_masks);
/* Pure host logic: validates the descriptors, lays the slots out in the order given and writes the table ns_km_draw's kernel reads
 * (per mask {arena byte offset, n, stream, thr, chunks of 4096 elements before it}, then a closing row) into table_host, and the
 * arena's size into *arena_bytes.  Nonzero with ns_last_error() on: a null pointer, n_masks outside [1, NS_KM_MAX_MASKS], an n of 0
 * or >= 2^34, a thr of 0, table_bytes below ns_km_table_bytes(n_masks). */
int ns_km_plan(const ns_km_mask* masks, int n_masks, void* table_host, size_t table_bytes, uint64_t* arena_bytes);
/* Draws every mask of the table into arena: EXACTLY ONE launch.  table_dev is a DEVICE copy of what ns_km_plan wrote (8-byte aligned;
 * the upload is the caller's host-to-device copy), arena a device buffer (16-byte aligned) of the planned arena_bytes.  Nonzero with
 * ns_last_error(), before any HIP call, on: a null or misaligned pointer, n_masks outside [1, NS_KM_MAX_MASKS], an arena shorter than
 * 16 * n_masks bytes (the least any plan of n_masks masks needs: the table lives on the device and is not read by the host).  The
 * kernel itself makes no store that would end behind arena + arena_bytes, so a short arena truncates the draw and is never overrun. */
int ns_km_draw(const void* table_dev, int n_masks, uint64_t seed, uint64_t call, void* arena, size_t arena_bytes, void* stream);
/* out[4] = Philox4x32-10 of ctr[4] under key[2], on the host (no GPU), through the inline function the kernel compiles.
 * ctr {0,0,0,0} key {0,0} -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8. */
int ns_km_op_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
/* ns_km_draw on the host (no GPU): fills arena_host from table_host (what ns_km_plan wrote) through the same inline functions.
 * Nonzero with ns_last_error() on: a null pointer, n_masks outside [1, NS_KM_MAX_MASKS], a table that is not a plan's (an n or thr it
 * would refuse, a slot out of place), an arena shorter than the plan's. */
int ns_km_host_draw(const void* table_host, int n_masks, uint64_t seed, uint64_t call, void* arena_host, size_t arena_bytes);

/* ==== Device-resident training set: a reference batch from one gather launch ================================
 * Handle-less; nothing above changes (every other ABI version stays as it is).  The store is packed, lives on the device and is only
 * read after its upload: mel [sum T_i, n_mel] fp32 (utterance i owns the rows [mel_off[i], mel_off[i + 1])), pitch and energy fp32 and
 * text int32 as ragged 1-D arrays whose slots each start at a multiple of four elements (16 bytes; ns_ds_plan pads them), speaker [N]
 * int32, one int64 offset table [N + 1] and one int32 length vector [N] per ragged array.  One launch turns the utterances
 * order[first .. first + B) into the reference's collated batch (dataset.py:88-118 and the 11-tuple branch of utils/tools.py:18-54):
 *   mels [B, Tmax, n_mel] fp32, pitches [B, Pmax] fp32, energies [B, Emax] fp32, texts [B, Lmax] int64, speakers / src_lens /
 *   mel_lens [B] int64.
 * EVERY element of every output is written: a valid element is the store's, bit for bit (-0.0 and denormals included), padding is
 * +0.0, or 0 in texts.  Mel rows move as 16-byte groups, the rest as dwords.  No atomic, no workspace, no host read; the grid is
 * capped and loops; an utterance may appear twice in a batch. */
#define NS_DS_ABI_VERSION 1 /* what ns_ds_abi_version() returns */
#define NS_DS_GRID_CAP 2048 /* workgroups of one ns_ds_gather at most (256 threads, one output group each a turn); they loop beyond */
int ns_ds_abi_version(void);
/* Kernel launches the calling thread's last ns_ds_gather / ns_ds_op_gather enqueued (1, or 0 after a refusal; ns_ds_plan and
 * ns_ds_host_gather set 0). */
int ns_ds_last_launches(void);
/* The four length vectors [N], always HOST memory: what every refusal about a batch's maxima is judged from. */
typedef struct ns_ds_lens {
  const int32_t* text;   /* L_i, phonemes */
  const int32_t* mel;    /* T_i, frames */
  const int32_t* pitch;  /* elements of utterance i's pitch (T_i or L_i: the caller's feature level) */
  const int32_t* energy; /* likewise */
} ns_ds_lens;
/* The four offset tables [N + 1], int64: mel in rows, the others in elements.  Row N is the array's size. */
typedef struct ns_ds_offsets {
  int64_t* mel;
  int64_t* pitch;
  int64_t* energy;
  int64_t* text;
} ns_ds_offsets;
/* The store.  Every pointer is device memory for ns_ds_gather / ns_ds_op_gather and host memory for ns_ds_host_gather. */
typedef struct ns_ds_store {
  const float* mel;       /* [mel_rows, n_mel], 16-byte aligned */
  const float* pitch;     /* [pitch_elems], 16-byte aligned */
  const float* energy;    /* [energy_elems], 16-byte aligned */
  const int32_t* text;    /* [text_elems], 16-byte aligned */
  const int32_t* speaker; /* [N] */
  const int64_t* mel_off; /* [N + 1] each, 8-byte aligned: what ns_ds_plan wrote */
  const int64_t* pitch_off;
  const int64_t* energy_off;
  const int64_t* text_off;
  const int32_t* text_len; /* [N] each: copies of the ns_ds_lens vectors in the store's memory */
  const int32_t* mel_len;
  const int32_t* pitch_len;
  const int32_t* energy_len;
  int64_t mel_rows; /* the sizes ns_ds_plan returned (bytes / 4 n_mel, bytes / 4): no element at or past them is read */
  int64_t pitch_elems;
  int64_t energy_elems;
  int64_t text_elems;
  int32_t N;
  int32_t n_mel; /* a multiple of 4 in [4, 128] */
} ns_ds_store;
/* The outputs of one batch (the store's memory space); B * Tmax * n_mel and every other output stay below 2^31 elements. */
typedef struct ns_ds_batch {
  float* mels;       /* [B, Tmax, n_mel], 16-byte aligned */
  float* pitches;    /* [B, Pmax] */
  float* energies;   /* [B, Emax] */
  int64_t* texts;    /* [B, Lmax], 8-byte aligned as the three below */
  int64_t* speakers; /* [B] */
  int64_t* src_lens; /* [B] */
  int64_t* mel_lens; /* [B] */
  int32_t B;
  int32_t Tmax;
  int32_t Pmax;
  int32_t Emax;
  int32_t Lmax;
} ns_ds_batch;
/* Pure host logic, no GPU: lays the N utterances out in the order given.  off->mel[i] = sum of the T before i; a slot of the three 1-D
 * arrays starts where the one before ends, rounded up to a multiple of four elements.  bytes[4] = the byte sizes of the packed mel,
 * pitch, energy and text arrays (each at least 16).  Nonzero with ns_last_error() on: a null pointer, N < 1, n_mel not a multiple
 * of 4 or outside [4, 128], a length below 1. */
int ns_ds_plan(const ns_ds_lens* lens, int N, int n_mel, const ns_ds_offsets* off, uint64_t bytes[4]);
/* The batch of order[first .. first + B): EXACTLY ONE launch.  order_dev is the device copy of the epoch's order (int32 [order_len]),
 * order_host the host's; lens are the host's length vectors.  Nonzero with ns_last_error(), before any HIP call, on: a null or
 * misaligned pointer, n_mel not a multiple of 4 or outside [4, 128], N < 1, B < 1, first < 0 or first + B > order_len, an order entry
 * outside [0, N), Tmax / Pmax / Emax / Lmax below the batch's own maximum (from lens), an output of 2^31 elements or more.  The
 * kernel reads the device copies of the tables; it reads no element at or past the store's stated sizes and writes the outputs only,
 * whatever those tables hold. */
int ns_ds_gather(const ns_ds_store* store, const ns_ds_lens* lens, const int32_t* order_dev, const int32_t* order_host, int64_t order_len,
                 int64_t first, const ns_ds_batch* out, void* stream);
/* The same launch with at most grid_cap workgroups (in [1, NS_DS_GRID_CAP]): a test hook that makes workgroups loop at a tiny shape. */
int ns_ds_op_gather(const ns_ds_store* store, const ns_ds_lens* lens, const int32_t* order_dev, const int32_t* order_host,
                    int64_t order_len, int64_t first, const ns_ds_batch* out, int grid_cap, void* stream);
/* ns_ds_gather on the host (no GPU): store, order_host and out are host memory; the same index arithmetic through the inline function
 * the kernel compiles.  Refuses what ns_ds_gather refuses (the alignments included: mel rows move as aligned 16-byte groups here too)
 * and offset tables that are not a plan's: any of the 4 (N + 1) entries that differs from what ns_ds_plan writes for lens, or a stated
 * size below the table's last row. */
int ns_ds_host_gather(const ns_ds_store* store, const ns_ds_lens* lens, const int32_t* order_host, int64_t order_len, int64_t first,
                      const ns_ds_batch* out);

#ifdef __cplusplus
}
#endif
#endif /* NAR_FS2_H */
