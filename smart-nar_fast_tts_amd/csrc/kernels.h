// Internal launch interface between the C-ABI (api.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ns {

enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };

// Packed rows (variable-length batches, api.hip forward_mel packed mode): the M activation rows are the utterances' WINDOWS
// laid end to end — utterance b owns rows [off[b], off[b] + win[b]), win[b] = min(len[b] + guard, T) — instead of the dense
// [B, S] grid in which the reference computes (and then discards) every padded frame.  Per row: its utterance, its position
// in the utterance, and its utterance's window length.  All nullptr = dense grid: b = m / S, t = m % S, window S.
struct RowMap {
  const int* row_b; const int* row_t; const int* row_w;  // [M] each
  const int* off; const int* win;                        // [B + 1], [B]
  // attention work list (attention.hip, packed launches): utterances in order of DESCENDING window, att_order[r] = the r-th
  // longest; att_off[r] = first workgroup of rank r, att_off[B] = att_wgs = sum_b ceil(win[b] / 128) * H.  Longest sweeps first:
  // the hardware hands workgroups to CUs in launch order, so the launch finishes when the work does, not when the XCD that drew
  // the longest utterance does.
  const int* att_off; const int* att_order; int att_wgs;
  int rows;                                              // M (host side)
};

// Row epilogue of a FULL-ROW tile (N == the tile width, 256 or 512): what the reference applies to every output row right
// after the contraction, done while the row is still on chip instead of by a second kernel over [M, N].
//   EPI_LN      Y[m,:] = LayerNorm_N(v[m,:]) * ln_g + ln_b, rows at t >= lens[b] written as zeros when lens != nullptr
//               (`layer_norm(output + residual)` + FFTBlock's masked_fill, transformer/SubLayers.py:57,93 + Layers.py:43,46;
//               the predictors' layer_norm_1, model/modules.py:260)
//   EPI_LN_PRED pred[m] = mask ? 0 : dot(LayerNorm_N(v[m,:]), wlin) + blin, optionally followed by the bucketize +
//               embedding (+ position) add into x_out [M, D] (VariancePredictor tail, model/modules.py:273-286,80-100,139-149);
//               Y is not written
// v = act(contraction + bias) + resid, exactly what the plain epilogue would have stored.
enum RowEpi : int { EPI_NONE = 0, EPI_LN = 1, EPI_LN_PRED = 2 };
struct RowEpilogue {
  const float* ln_g; const float* ln_b;
  const long long* lens;
  const float* wlin; const float* blin; float* pred; float control; const float* target;
  const float* bins; int n_edges; const float* emb; const float* x_in; const float* pos; float* x_out; int D;
  // ticketed form (small grids, gemm_conv.hip TICKET): the GEMM tiles N with BN < N, stores the raw rows into ConvGemm::Y
  // ([M, N], ldy == N) and the LAST workgroup to finish a row block applies the row epilogue, EPI_LN writing y_out [M, N].
  // ticket: conv_gemm_ticket_ints(M) zeroed ints, used by this launch only; nullptr selects the full-row tile.
  float* y_out; int* ticket;
  const int* row_b; const int* row_t;  // packed rows (RowMap): utterance / position of row m; nullptr = m / S, m % S
};
inline int conv_gemm_ticket_ints(int M) { return (M + 31) / 32; }
bool conv_gemm_ticket_ok(int M, int N, int Cin);  // shapes the ticketed form covers (row widths 256 / 512)

// Y[m, n] = act( sum_{j<KW} sum_{c<Cin} X[m + j - pad, c] * W[n][j*Cin + c] + bias[n] ) + resid[m, n]
// rows of X outside the utterance's [0, S) window read as zero ("same" zero padding of nn.Conv1d).
struct ConvGemm {
  const float* X; int ldx;
  const float* W;               // packed [N][KW*Cin], row stride ldw
  int ldw;                      // floats between weight rows; 0 = KW*Cin (dense)
  const unsigned short* Wb3;    // optional: the same weights as three bf16 planes [3][N][KW*Cin] (gemm_bf16x3.hip), else nullptr
  const unsigned short* Wbf;    // "bf16" mode: the weights rounded to one bf16 plane [N][KW][Cinp] (gemm_bf16.hip), else nullptr
  const float* bias;            // [N] or nullptr
  const float* resid; int ldr;  // [M, N] or nullptr
  float* Y; int ldy;
  int M, N, Cin, KW, pad, S;
  int m_base;                   // rows of the full matrix ahead of X / Y / resid row 0 (a launch over a row range of a larger
                                // problem, gemm_conv.hip split plan): the utterance position of row m is that of row m_base + m.
                                // Plain epilogues only (epi == EPI_NONE).
  int act;
  int epi;                      // RowEpi; != EPI_NONE requires conv_gemm_row_epilogue_ok(p)
  RowEpilogue e;
  RowMap rm;                    // packed rows: tap windows come from row_t / row_w instead of m % S / S
};
// Optional timing of one launch_conv_gemm / launch_attention call: the events ride ON the dispatch packets
// (hipExtLaunchKernel's start / stop events: the kernel's own begin / end timestamps), so timing a launch adds no marker
// packet and no idle gap to the stream — hipEventRecord pairs around the heavy launches cost ~6 us each, 3 % of a forward.
// A plan of several launches gets `start` on its first and `stop` on its last kernel.  nullptr / {nullptr, nullptr} = untimed.
struct LaunchTiming { hipEvent_t start, stop; };
hipError_t launch_conv_gemm(const ConvGemm& p, hipStream_t st, const LaunchTiming* tm = nullptr);
// {bm, bn, rows} of the main launch, {bm, bn, rows} of the remainder (0 = none), the MFMA tile edge of the launch(es) (32 / 16),
// the cost model's estimate in us
bool conv_gemm_plan(int M, int N, int Cin, int KW, int out[8]);
// every launch of launch_conv_gemm for this shape, recorded by the dispatch itself: {BM, BN, BK, KS, MF, ROWEPI, TICKET, rows} per launch;
// epi 0 = plain, 1 = LayerNorm on the full-row tile, 2 = LayerNorm on the ticketed ladder; returns the number of launches (0 = refused)
int conv_gemm_describe(int M, int N, int Cin, int KW, int epi, int out[2][8]);
bool conv_gemm_tile16_enabled();  // the 16-row tile family is in use (planner on, NS_TILE16 != 0)
int conv_gemm_row_tile(int M, int N, int K = 256);  // height of the full-row (LayerNorm epilogue) tile for M rows of N = 256 / 512 columns, contraction length K
int conv_gemm_acc_chunk();  // k values per accumulation chunk of the long contractions (gemm_conv.hip ACC2; NS_ACC_CHUNK, 0 = one sequential sum)
// NS_PLAN=0 in the environment: the round-3 one-tile-per-launch rules (A/B runs of the planner; read once)
bool launch_planner_enabled();
// opt-in "bf16x3" precision mode (gemm_bf16x3.hip): same contraction from an exact 3-way bf16 split of both operands
bool conv_gemm_b3_ok(int M, int N, int Cin, int KW, int epi);  // epi: EPI_NONE or EPI_LN
int conv_gemm_b3_tile(int M, int N);                           // rows of a plain launch's tile: 256 or 128 (both 256 columns wide)
hipError_t launch_conv_gemm_b3(const ConvGemm& p, hipStream_t st);
void split_weights_b3(const float* w, size_t n, unsigned short* hi, unsigned short* mid, unsigned short* lo);
// opt-in "bf16" precision mode (gemm_bf16.hip): both operands rounded to bf16, fp32 accumulation, at every launch size
bool conv_gemm_bf16_ok(int M, int N, int Cin, int KW, int epi);  // epi: EPI_NONE, or EPI_LN (the 64 x 256 full-row tile)
void conv_gemm_bf16_plan(int M, int N, int* bm, int* bn);     // tile of a plain launch
hipError_t launch_conv_gemm_bf16(const ConvGemm& p, hipStream_t st);
size_t bf16_plane_elems(int N, int KW, int Cin);               // N * KW * (Cin rounded up to 32)
void round_weights_bf16(const float* w, int N, int KW, int Cin, unsigned short* dst);
// true when launch_conv_gemm has a full-row tile for this shape (so p.epi may be set); otherwise the caller runs the
// plain GEMM followed by the row kernel
bool conv_gemm_row_epilogue_ok(int M, int N, int Cin);

// Fused multi-head self attention over the packed projection buffer qkv [B*S, 3*d]
// (cols [0,d) = Q, [d,2d) = K, [2d,3d) = V, head h at offset h*dk inside each).
// out [B*S, d] = merge_heads( softmax(Q K^T / sqrt(dk) + (-inf at keys >= lens[b])) V )
// scratch (optional, scratch_floats floats): enables the split-key path, taken by launches of fewer than
// ATT_SPLIT_MAX_BLOCKS workgroups: up to ATT_SPLIT_MAX key ranges, each needing B*S*(H*dk + 2*H) floats
// (16, not 8: a single 788-frame utterance has 14 (query tile, head) pairs x 25 key tiles; 13 two-tile ranges instead of 8
//  four-tile ranges take the decoder attention from 24.5 to ~19 us, single-utterance p50 1.08 -> 1.06 ms, same box)
constexpr int ATT_SPLIT_MAX = 16, ATT_SPLIT_MAX_BLOCKS = 128;
// tickets (nullable): attention_ticket_ints(B, S, H) ZEROED ints for the strip kernel's last-arriver merge (small grids)
inline int attention_ticket_ints(int B, int S, int H) { return B * H * ((S + 31) / 32); }
bool attention_uses_tickets(int B, int S, int H);  // false: launch_attention(B, S, H, ...) never touches `tickets` (pass nullptr)
// rm (packed rows): utterance b's rows start at rm->off[b] and number rm->win[b] <= S (S = the longest window); no split-key path
// bf16 (the "bf16" precision mode, decoder only): Q K^T and P V on the bf16 matrix cores from operands rounded to bf16,
// scores scaled, masked and soft-maxed in fp32
hipError_t launch_attention(const float* qkv, const long long* lens, int B, int S, int H, int dk, float* out, float* scratch,
                            size_t scratch_floats, int* tickets, hipStream_t st, const RowMap* rm = nullptr, const LaunchTiming* tm = nullptr,
                            bool bf16 = false);
// key ranges per 128-query tile the dense launch of (B, S, H, dk) will use when it has the scratch for them (1 = no split):
// the caller sizes `scratch` as attention_split(...) * B*S*(H*dk + 2*H) floats
int attention_split(int B, int S, int H, int dk);
// the same for a packed launch: att_wgs workgroups on the work list, S = the longest window, Mp packed rows
int attention_split_packed(int att_wgs, int S, int dk, size_t Mp, int d);
// What a packed launch_attention of this shape does, decided by the function the launch itself asks: form 0 = k_attention_strip on
// the packed rows, 1 = k_attention on the flat work list; nsplit key ranges per strip workgroup group / per work-list workgroup;
// merge = a k_attention_merge launch follows; tiles = 32-key tiles per range of an utterance whose window is S (a strip's range is
// one wave's share).  scratch_floats = 0: no scratch.
struct AttentionPackedPlan { int form, nsplit, merge, tiles; };
AttentionPackedPlan attention_plan_packed(int B, int S, int H, int dk, int att_wgs, size_t Mp, size_t scratch_floats, bool has_tickets);
// The same for the dense (grid) launch, rm == nullptr: kernel 0 = k_attention_strip, 1 = k_attention; nsplit = key-range workgroups
// per strip / per 128-query tile; merge 0 = none, 1 = the last arriver of a strip's workgroups (tickets), 2 = a k_attention_merge
// launch; tiles = 32-key tiles per wave of a strip / per range of k_attention, of an utterance of S keys.  scratch_floats = 0: no scratch.
struct AttentionDensePlan { int kernel, nsplit, merge, tiles; };
AttentionDensePlan attention_plan_dense(int B, int S, int H, int dk, size_t scratch_floats, bool has_tickets);

// ---- row kernels (rowops.hip) -----------------------------------------------------------------
// y = LayerNorm_C(x) * g + b ; rows with t >= lens[b] are written as zero when lens != nullptr
hipError_t launch_layernorm(const float* x, const float* g, const float* b, float* y, int M, int C, int S,
                            const long long* lens, hipStream_t st, const RowMap* rm = nullptr);
// pred[m] = mask ? 0 : dot(LayerNorm_C(x[m]), wlin) + blin            (variance predictor tail)
// if emb != nullptr additionally  x_out[m,:] = x_in[m,:] + emb[bucketize(pred[m]*control, bins)] (+ pos[t,:])
hipError_t launch_ln_linear_embed(const float* x, const float* g, const float* b, const float* wlin, const float* blin,
                                  float* pred, int M, int C, int S, const long long* lens, float control,
                                  const float* target, const float* bins, int n_bins, const float* emb, const float* x_in, const float* pos,
                                  float* x_out, int D, hipStream_t st, const RowMap* rm = nullptr);
// out[m,:] = emb[texts[m],:] + pos[t,:]
// token ids outside [0, n_vocab) read row 0 (and are reported by launch_duration_tail)
// zero / nzero (nullable): ticket counters of the forward phase this kernel opens, zeroed by it (rowops.hip zero_words);
// the same pair on launch_length_regulate / launch_gaussian_upsampling
hipError_t launch_embed_pos(const long long* texts, const float* emb, const float* pos, float* out, int M, int S, int D, int n_vocab,
                            int* zero, int nzero, hipStream_t st);
hipError_t launch_add_pos(const float* x, const float* pos, float* out, int M, int S, int D, hipStream_t st, const RowMap* rm = nullptr);
hipError_t launch_bucketize(const float* v, int n, const float* bins, int n_edges, long long* idx, hipStream_t st);
hipError_t launch_mask_from_lengths(const long long* lens, int B, int max_len, uint8_t* mask, hipStream_t st);
hipError_t launch_sinusoid(int n_pos, int d, float* out, hipStream_t st);
hipError_t launch_duration_round(const float* log_d, int n, float d_control, float* d_rounded, hipStream_t st);
hipError_t launch_duration_scan(const float* d_rounded, int B, int L, int32_t* cum, long long* mel_lens, hipStream_t st);
// mel_mask (nullable): also writes get_mask_from_lengths(mel_len) for the [B,T] frame grid
// status (nullable, [B] int32): per-utterance NS_STATUS_* bits of ns_forward_mel (needs mel_lens for the bad-token bit)
hipError_t launch_length_regulate(const float* x, const int32_t* cum, int B, int L, int D, int T, float* out, uint8_t* mel_mask,
                                  const long long* mel_lens, int32_t* status, int* zero, int nzero, hipStream_t st);
// phase-1 tail in one launch: src mask, duration_round (two copies), duration_scan; mel_lens[b] = -1 when utterance b
// holds a token id outside [0, n_vocab) (texts may be nullptr: no check)
hipError_t launch_duration_tail(const float* log_d, const long long* src_lens, const long long* texts, int n_vocab, int B, int L,
                                float d_control, float* d_rounded, float* d_keep, int32_t* cum, long long* mel_lens, uint8_t* src_mask,
                                long long* mel_lens_host /* nullable: device-visible host copy */, hipStream_t st);
// the teacher-forced forward's phase-1 tail in one launch: the same from GIVEN int64 durations [B, L] (model/modules.py:128-130) —
// src mask, d_keep = (float)d, cum = prefix sums of max(d, 0), mel_lens[b] = total (or -1 for a bad token id; texts nullable)
hipError_t launch_duration_target_tail(const long long* d_targets, const long long* src_lens, const long long* texts, int n_vocab, int B, int L,
                                       float* d_keep, int32_t* cum, long long* mel_lens, uint8_t* src_mask, hipStream_t st);
// Packed variant of launch_length_regulate (kernels.h RowMap).  Builds the plan first: win[b] = min(max(mel_lens[b], 0) + guard, T),
// off = exclusive scan, row maps for the Mp = sum(win) rows (the caller computed the same Mp from its host copy of mel_lens);
// then gathers the encoder rows into the packed layout (frames at t >= mel_len[b] are zero).  status as launch_length_regulate.
// plan: int storage for off [B+1], win [B], row_b / row_t / row_w [Mp] — pack_plan_ints(B, Mp) ints; *rm receives the pointers.
constexpr int PACK_GUARD = 20;  // frames kept past an utterance's end: the PostNet's reach (5 layers x 2) twice over, see api.hip
inline size_t pack_plan_ints(int B, size_t Mp) { return (size_t)4 * B + 4 + 3 * Mp; }
// the plan's layout: off [B+1] | win [B] + 1 unused | att_off [B+1] | att_order [B] + 1 unused | row_b [Mp] | row_t [Mp] | row_w [Mp]
void plan_pointers(int* plan, int B, int Mp, RowMap* rm);
// H: attention heads of the stack that will run on these rows (the plan's attention work list is per head)
hipError_t launch_length_regulate_packed(const float* x, const int32_t* cum, int B, int L, int D, int T, int Mp, int H, float* out,
                                         const long long* mel_lens, int32_t* status, int* zero, int nzero, int* plan, RowMap* rm,
                                         hipStream_t st);
// dst[r, :] = row[:] for r < rows (n % 4 == 0)
hipError_t launch_broadcast_row(const float* row, float* dst, int rows, int n, hipStream_t st);
hipError_t launch_pack_vector(const RowMap& rm, int T, const float* src, float* dst, int Mp, hipStream_t st);
// the packing plan and row maps alone (launch_length_regulate_packed builds them as a side effect of its gather)
hipError_t launch_pack_plan(const long long* mel_lens, int B, int T, int H, int Mp, int* plan, RowMap* rm, hipStream_t st, int guard = PACK_GUARD);
// Phase 1 on packed PHONEME rows (api.hip forward_durations): utterance b keeps min(src_len[b] + PHONEME_GUARD, L) rows.  In the
// FFT blocks a valid phoneme never reads a padded one except as zeros (masked_fill ahead of every convolution, -inf keys); the
// variance predictors have no mask between their two convolutions (model/modules.py:245-286), so the last valid
// phoneme reads ONE row past the utterance's end — a row that must be computed, from zeroed encoder output, like the reference does.
constexpr int PHONEME_GUARD = 2;
hipError_t launch_store_lens(const long long* host, int n, long long* dst, hipStream_t st);  // dst[i] = host[i], values passed as kernel arguments
hipError_t launch_pack_plan_only(const long long* lens, int B, int T, int H, int Mp, int* plan, RowMap* rm, hipStream_t st, int guard);
// (also writes the row maps of *rm: launch_pack_plan_only + this kernel = the whole plan)
hipError_t launch_embed_pos_packed(const long long* texts, const float* emb, const float* pos, float* out, const RowMap& rm, int B, int Mp, int L,
                                   int D, int n_vocab, int* zero, int nzero, hipStream_t st);
hipError_t launch_unpack_phase1(const RowMap& rm, const long long* lens, int B, int S, int D, const float* rows_p, float* rows, const float* vec_p,
                                float* vec, hipStream_t st);
// dst [B*S, D] (any D) = the packed rows of src where t < min(lens[b], win[b]), zeros elsewhere
hipError_t launch_unpack_rows(const RowMap& rm, const long long* lens, int B, int S, int D, const float* src, float* dst, hipStream_t st);
// padded outputs from packed rows (api.hip forward_mel): see k_unpack_outputs in rowops.hip
hipError_t launch_unpack_outputs(const RowMap& rm, int B, int T, int n_mel, const long long* mel_lens, const float* mel_p, const float* post_p,
                                 const float* p_p, const float* e_p, const float* mel_bias, const float* post_const, float* mel,
                                 float* post, float* p_pred, float* e_pred, uint8_t* mel_mask, hipStream_t st);
hipError_t launch_gaussian_upsampling(const float* x, const float* dur, int B, int L, int D, int T, int T_out,
                                      float* out, float* s, float* w, const long long* own_len, int32_t* status, int* zero, int nzero,
                                      hipStream_t st, const RowMap* rm = nullptr);  // rm: out is the packed layout (w must be nullptr)

// ---- HiFi-GAN vocoder (vocoder.hip) -----------------------------------------------------------
// One implicit GEMM over a grid of Sg rows per utterance (Sg = S_in for a "same" Conv1d, S_in + 1 for a polyphase transposed conv):
//   v[m, n] = sum_{j < KW} sum_{c < Cin} act_in(X[b, t + off0 + j dil, c]) W[n][j Cin + c]   (rows outside [0, S_in) read zero)
//   v = v + bias[n % Cb]; v = lrelu(v, out_slope) if out_act; v = v + R[o] if R
//   mrf 0: Y[o] = v   1: Y[o] = Y[o] + v   2: Y[o] = (Y[o] + v) / mrf_div
// with m = b Sg + t and o = b out_ustride + (t N + n - out_shift), stored only when 0 <= t N + n - out_shift < out_ustride.
// act_in(x) = lrelu(x, in_slope) when in_act, else x.  Cin % 32 == 0, N % 32 == 0, X / W 16-byte aligned.
struct VocGemm {
  const float* X; const float* W; const float* bias; const float* R; float* Y;
  int B, S_in, Sg, Cin, KW, dil, off0, N, Cb;
  long long out_ustride, out_shift;
  int in_act; float in_slope; int out_act; float out_slope;
  int mrf; float mrf_div;
  const unsigned short* Wbf;  // "bf16" matmul mode: W rounded to bf16 (RNE), same packed layout (k_voc_gemm ignores it)
};
bool voc_gemm_ok(const VocGemm& p);
hipError_t launch_voc_gemm(const VocGemm& p, hipStream_t st);
// opt-in "bf16" matmul mode (vocoder_bf16.hip): the same GEMM from the bf16 plane p.Wbf and bf16-rounded activations, fp32 accumulation
hipError_t launch_voc_gemm_bf16(const VocGemm& p, hipStream_t st);
// wav[b, t] = tanh(bias[0] + sum_j sum_c lrelu(x[b, t + j - (KW-1)/2, c], slope) w[j C + c]) over [B, S, C] time-major x
size_t voc_post_lds_bytes(int C, int KW);
hipError_t launch_voc_post(const float* x, const float* w, const float* bias, float* wav, int B, int S, int C, int KW, float slope, hipStream_t st);
// dst [B, T, C] = src [B, C, T] transposed
hipError_t launch_voc_transpose(const float* src, float* dst, int B, int C, int T, hipStream_t st);
// ---- reference-mel aligner (cross_attention.hip) -----------------------------------------------
// ScaledDotProductAttention of FFTBlock2.crs_attn with its probabilities as an output (transformer/Modules.py:14-25,
// SubLayers.py:47-54): q [B*T, H*dk], kv [B*L, 2*H*dk] (columns [0, d) = K, [d, 2d) = V, head h at h*dk inside each) ->
// ctx [B*T, H*dk] (merged heads) and attn [B, H, T, L] = softmax(q k^T / sqrt(dk) + (-inf at keys >= src_lens[b])).
// Key-only mask: every query row is computed.  dk in {64, 128}; q and kv 16-byte aligned.
bool cross_attention_ok(int H, int dk);
hipError_t launch_cross_attention(const float* q, const float* kv, const long long* src_lens, int B, int T, int L, int H, int dk,
                                  float* ctx, float* attn, hipStream_t st);
// x [B*T, C] = mels with frame 0 of every utterance replaced by zeros (transformer/Models.py:145-146); C % 4 == 0, 16-byte aligned
hipError_t launch_aln_input(const float* mels, float* x, int B, int T, int C, hipStream_t st);
// out [B, L] int64: frames of utterance b whose head-summed last-layer alignment peaks at phoneme i (zeroes `out` first)
hipError_t launch_aln_durations(const float* attn_last, const long long* src_lens, const long long* mel_lens, int B, int H, int T, int L,
                                long long* out, hipStream_t st);
// ---- FastSpeech2Loss (loss.hip; model/loss.py:149-250).  The device-side mirror of ns_loss_args (include/nar_fs2.h).
struct LossArgs {
  int B, L, T, H, n_mel, pitch_frame_level, energy_frame_level;
  long long mel_targets_stride, d_targets_stride;  // floats between utterances of mel_targets; elements between rows of d_targets
  const float *mel, *postnet, *mel_targets;        // [B, T, n_mel] x 2, [B, T' >= T, n_mel]
  const unsigned char* mel_masks;                  // [B, T], nonzero = padded
  const float *pitch, *pitch_targets, *energy, *energy_targets;  // [B, T] at frame_level, [B, L] at phoneme_level
  const float* log_d; const long long* d_targets; const unsigned char* src_masks;  // [B, L], [B, L' >= L], [B, L]
  const long long *src_lens, *mel_lens;            // [B]; mel_lens = the batch's INPUT lengths
  const float* attn[4];                            // [B, H, T, L] each; head 0 is read in place
};
constexpr int LOSS_FRAME_ROWS = 64;      // frame rows per workgroup
constexpr int LOSS_PHONEME_ROWS = 1024;  // phoneme rows per workgroup
constexpr int LOSS_ATTN_ROWS = 16;       // query rows (of one utterance, four maps) per workgroup
constexpr int LOSS_SLOT_SUMS = 6, LOSS_SLOT_WORDS = 8, LOSS_SLOT_BYTES = 64;  // six float64 sums + two int64 counts
// slots of the partial workspace = workgroups of k_loss_partial; a function of (B, L, T) alone
long long loss_slots(int B, int L, int T, int* n_frame_wgs, int* n_phoneme_wgs);
// requires what ns_loss_forward (loss_api.hip) validates; ws >= loss_slots(...) * LOSS_SLOT_BYTES, uninitialised
// record (nullable): LOSSG_RECORD_WORDS int64 written by k_loss_final next to out7 — the three counts the backward divides by
hipError_t launch_loss(const LossArgs& a, void* ws, float* out7, hipStream_t st, long long* record = nullptr);
// ---- FastSpeech2Loss backward (lossgrad.hip): the gradient of sum_i g[i] * out7[i] with respect to the nine predictions.
constexpr int LOSSG_RECORD_WORDS = 4, LOSSG_RECORD_BYTES = 32;  // n_frames, n_phonemes, n_attn, 0 (int64)
struct LossGrads {
  float *mel, *postnet, *pitch, *energy, *log_d;  // shaped like the predictions, contiguous, 16-byte aligned; nullptr = not written
  float* attn[4];                                  // [B, H, T, L] each
};
constexpr int LOSSG_FRAME_ROWS = 64;       // frame rows per workgroup (n_mel / 4 vectors each)
constexpr int LOSSG_PHONEME_ROWS = 1024;   // phoneme rows per workgroup: one 16-byte group per thread
constexpr int LOSSG_ATTN_ELEMS = 4096;     // map elements per workgroup: four 16-byte groups per thread, four maps
// workgroups of k_lossg_backward; a segment none of whose outputs is wanted has none
long long lossg_wgs(const LossArgs& a, const LossGrads& d, int* n_frame_wgs, int* n_phoneme_wgs);
// requires what ns_lossg_backward (lossgrad_api.hip) validates; record and g7 are read on the device only
hipError_t launch_lossg(const LossArgs& a, const long long* record, const float* g7, const LossGrads& d, hipStream_t st);
// ---- wave-to-mel front end (melfront.hip; audio/stft.py:52-81,159-178, audio/tools.py:8-15) ----------------------------------
// rows [B, S, hop]: the clipped, reflect-padded wave of utterance b (n_b = clamp(wav_lens[b], 0, n_max) samples) laid out as S * hop
// consecutive samples; zeros from sample n_b + fl on, all zeros when n_b <= fl / 2.  mel_lens_out (nullable) [B] = n_b / hop + 1 or 0.
hipError_t launch_mel_frame_rows(const float* wav, long long ld, const long long* wav_lens, int B, long long n_max, int fl, int hop, int S,
                                 float* rows, long long* mel_lens_out, hipStream_t st, bool clip = true);  // clip = false: no clip (Griffin-Lim)
// packed spectrum [B * S, fl] (column 0 = re_0, 1 = re_{fl/2}, 2k = re_k, 2k + 1 = im_k) -> mel [B, T, n_mel] = log(max(band sums, clip)) (taken in double, rounded once),
// energy [B, T]; zeros at frames t >= mel_lens[b].  band [n_mel][3] = {first bin, bins, offset into bw}; fl <= MEL_MAX_FILTER.
constexpr int MEL_MAX_FILTER = 4096;
hipError_t launch_mel_project(const float* spec, const long long* wav_lens, int B, int S, long long n_max, int T, int fl, int hop, int n_mel,
                              float clip, const int* band, const float* bw, float* mel, float* energy, hipStream_t st);
// ---- Griffin-Lim mel-to-wave (griffinlim.hip; audio/stft.py:83-122, audio/audio_processing.py:7-82, audio/tools.py:18-34) -------------
// Every kernel derives an utterance's frame count the same way: Tg_b = clamp(lens[b] - drop, 0, Tg), and 0 when the wave it stands
// for, hop (Tg_b - 1) samples, is filter_length / 2 or shorter (the reference's reflect pad refuses it).  Packed spectrum rows as in
// launch_mel_project: column 0 = re_0, 1 = re_{fl/2}, 2k = re_k, 2k + 1 = im_k.
// mag [B, Tg, fl/2 + 1] = scaling * sum_m expf(mel[b, t, m]) mel_basis[m, k] (m ascending) from mel [B, T_mel, n_mel]; zeros at t >= Tg_b
hipError_t launch_gl_mel_to_mag(const float* mel, const long long* lens, int drop, int B, int T_mel, int Tg, int fl, int hop, int n_mel,
                                float scaling, const float* mel_basis, float* mag, hipStream_t st);
// X [B * Tg, fl] packed = mag (cos, sin)(angles), both [B, Tg, fl/2 + 1]; zero rows at t >= Tg_b
hipError_t launch_gl_recombine(const float* mag, const float* angles, const long long* lens, int drop, int B, int Tg, int fl, int hop,
                               float* X, hipStream_t st);
// X [B * Tg, fl] packed = mag * Y / |Y| per bin from the packed spectrum Y [B * S, fl]; (mag, 0) where Y == 0; zero rows at t >= Tg_b
hipError_t launch_gl_rephase(const float* Y, const float* mag, const long long* lens, int drop, int B, int Tg, int S, int fl, int hop,
                             float* X, hipStream_t st);
// wave [B, ld] from frames [B * Tg, fl]: overlap-add in ascending t, / window_sum (> FLT_MIN; rebuilt per sample from wsq [fl] doubles
// in the reference's order and rounding), * fl / hop, trimmed by fl / 2; zeros at s >= n_b = hop (Tg_b - 1); wave_lens_out [B] = n_b
hipError_t launch_gl_overlap_add(const float* frames, const long long* lens, int drop, int B, int Tg, int fl, int hop, const double* wsq,
                                 float* wave, long long ld, long long* wave_lens_out, hipStream_t st);
// wave_lens_out [B] = n_b alone
hipError_t launch_gl_wave_lens(const long long* lens, int drop, int B, int Tg, int fl, int hop, long long* wave_lens_out, hipStream_t st);
// magnitude, phase [B, T, fl/2 + 1] = sqrtf(re^2 + im^2), atan2f(im, re) of Y [B * S, fl] packed; zeros at t >= n_b / hop + 1 (or n_b <= fl/2)
hipError_t launch_gl_polar(const float* Y, const long long* wav_lens, long long n_max, int B, int S, int T, int fl, int hop, float* magnitude,
                           float* phase, hipStream_t st);
// ---- variance targets and dataset statistics (vartargets.hip; preprocessor/preprocessor.py:188-227, 61-133, 289-310) -----------
// The device-side mirror of ns_vt_args / ns_vt_state (include/nar_fs2.h).
struct VtArgs {
  int B, L, T, pitch_frame_level, energy_frame_level, pitch_normalization, energy_normalization;
  long long durations_stride;
  const float *pitch, *energy;
  const long long *durations, *src_lens;
  float *pitch_targets, *energy_targets;
  long long* frame_lens;
  uint8_t* valid;
};
struct VtState { double count[2], mean[2], m2[2], min[2], max[2]; };
constexpr int VT_SORT_CAPACITY = 8192;  // floats of one (utterance, feature) sorted in LDS (32 KiB)
constexpr int VT_SLOT_BYTES = 32;       // fit: count, mean, M2 (+ pad); normalize: min, max (+ pad) — doubles
// workspace = [B * T] float64 contour + [B * T] int32 next-voiced index (targets), or 2 * B slots (fit, normalize)
size_t vt_ws_bytes(int B, int L, int T);
hipError_t launch_vt_state_init(VtState* state, hipStream_t st);
hipError_t launch_vt_targets(const VtArgs& a, void* ws, hipStream_t st);
hipError_t launch_vt_fit(const VtArgs& a, VtState* state, void* ws, hipStream_t st);
hipError_t launch_vt_normalize(const VtArgs& a, VtState* state, void* ws, hipStream_t st);
// ---- ScheduledOptim's training-step tail (optim.hip; model/optimizer.py:10-15,24,28 and train.py:91-95) -------------------------
// The device-side mirrors of ns_opt_tensor / ns_opt_record / ns_opt_hyper (include/nar_fs2.h).
struct OptTensor {
  float* p; float* g;      // g == nullptr: skipped, as torch skips p.grad is None
  long long numel;
  long long state_off;     // floats into exp_avg / exp_avg_sq, a multiple of 4
  int lag;                 // the tensor's own step count is global_step - lag
  int chunk_begin;         // chunks of the tensors before this one; every tensor owns max(1, ceil(numel / OPT_CHUNK)) chunks
};
struct OptRecord { double norm64; float total_norm; float clip_coef; };
struct OptHyper { double lr, beta1, beta2, eps, weight_decay; long long global_step; int fuse_clip, zero_grads; };
constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = 4096;      // elements per chunk: four 16-byte groups per thread
constexpr int OPT_MAX_GRID = 2048;   // 256 CUs x 8 workgroups; the chunks beyond are grid-strided
// slots [n_chunks] float64, uninitialised; record written by the second launch
hipError_t launch_opt_grad_norm(const OptTensor* table, int n_tensors, int n_chunks, float max_norm, double* slots, OptRecord* record, hipStream_t st);
hipError_t launch_opt_scale(const OptTensor* table, int n_tensors, int n_chunks, const OptRecord* record, hipStream_t st);
hipError_t launch_opt_adam(const OptTensor* table, int n_tensors, int n_chunks, const OptHyper& h, float* exp_avg, float* exp_avg_sq,
                           const OptRecord* record, hipStream_t st);
hipError_t launch_opt_zero(const OptTensor* table, int n_tensors, int n_chunks, hipStream_t st);
// ---- VariancePredictor training forward / backward (predgrad.hip; model/modules.py:233-286) -------------------------------------
// Weight gradient of a "same"-padded Conv1d over row-major activations: dW[n][c][j] = sum_m dz[m, n] X[m + j - pad, c], a
// N x (KW * Cin) GEMM contracted over the M rows, split over row ranges (PgWgradPlan) whose partial tiles a second pass sums.
constexpr int PG_TILE_N = 128, PG_TILE_C = 128, PG_STEP_ROWS = 16;  // output tile of a workgroup; rows of m per LDS stage
constexpr int PG_WG_TARGET = 256;                                   // workgroups the split aims at: one per CU
constexpr int PG_ROW_BLOCK = 64;                                    // rows per workgroup of the row backward = rows per column partial
constexpr int PG_SLOTS = 5;                                         // column sums per row block: d_ln_g, d_ln_b, d_b, d_wlin, d_blin
struct PgWgradPlan { int tile_n, tile_c, rows, ranges, tiles, chunk; long long ws_floats; };
// a function of the shape (and of the process-wide accumulation chunk) alone; false: refused (N % 128, Cin % 4, sizes)
bool pg_plan_wgrad(int M, int N, int Cin, int KW, PgWgradPlan* out);
inline int pg_row_blocks(int M) { return (M + PG_ROW_BLOCK - 1) / PG_ROW_BLOCK; }
// partial [ranges][N][KW * Cin] floats (uninitialised); two launches: the GEMM, then the fixed-order sum into dW [N][Cin][KW]
// ldz: floats between rows of dz (0 = N; a column block of a wider matrix, attngrad_api.hip)
hipError_t launch_pg_wgrad(const float* dz, const float* X, int M, int S, int N, int Cin, int KW, const PgWgradPlan& pl, float* partial,
                           float* dW, hipStream_t st, int ldz = 0);
// one launch, up to two convolutions (a null w skips one): w [N][Cin][KW] -> wp [N][KW*Cin] (the forward's form, nullable) and
// wt [Cin][KW*N] with wt[c][j*N + n] = w[n][c][KW-1-j] (the data gradient's form, nullable)
struct PgPack { const float* w; float* wp; float* wt; int N, Cin, KW; };
hipError_t launch_pg_pack(const PgPack& a, const PgPack& b, hipStream_t st);
// h [M, F] = (LayerNorm(v) * ln_g + ln_b) * keep * scale (h nullable); wlin != nullptr additionally pred[m] = mask[m] ? +0 : h[m] . wlin + blin
hipError_t launch_pg_row_forward(const float* v, const float* ln_g, const float* ln_b, const uint8_t* keep, float scale, float* h,
                                 const float* wlin, const float* blin, const uint8_t* mask, float* pred, int M, int F, hipStream_t st);
// see ns_pg_op_row_backward (nar_fs2.h); part: [pg_row_blocks(M)][PG_SLOTS][F] doubles, uninitialised
struct PgRowBackward {
  int tail, M, F; float scale;
  const float *dy, *g, *v, *ln_g, *ln_b, *wlin; const uint8_t *mask, *keep;
  float* dz; double* part;
};
hipError_t launch_pg_row_backward(const PgRowBackward& a, hipStream_t st);
// part[blk][slot][:] = column sums of rows [64 blk, 64 blk + 64) of src[:, slot * F .. slot * F + F), src rows of parts * F floats,
// parts in [1, PG_SLOTS]: a matrix alone (1), dQ | dK | dV of the self-attention (3), dQ (1) and dK | dV (2) of the cross-attention
hipError_t launch_pg_colsum(const float* src, int M, int F, int parts, double* part, hipStream_t st);
// out[i][:] = sum over blocks, ascending, of part[i / PG_SLOTS][blk][i % PG_SLOTS][:] for the up to 2 * PG_SLOTS non-null outputs
// (slot 4 is a scalar: column 0 only); part holds `stages` arrays of [nblk][PG_SLOTS][F] doubles
struct PgColFinal { float* out[2 * PG_SLOTS]; };
hipError_t launch_pg_col_final(const double* part, int nblk, int F, const PgColFinal& o, hipStream_t st);
// ---- MultiHeadAttention training forward / backward, self-attention (attngrad.hip; transformer/SubLayers.py:8-59) ------------------
// qkv [B*S, 3d] in launch_attention's layout; lse, D [B, H, S]; lens [B] nullable (= S); dk in {32, 64, 128}.
// lse[b, h, i] = log sum_{j < lens[b]} exp(q_i . k_j / sqrt(dk)); one launch
hipError_t launch_ag_lse(const float* qkv, const long long* lens, int B, int S, int H, int dk, float* lse, hipStream_t st);
// dqkv [B*S, 3d] = (dQ | dK | dV) from dctx [B*S, d]; two launches: the query-owning kernel (writes D[b, h, i] = dctx_i . ctx_i and
// dQ), then the key-owning kernel (reads D, writes dK and dV; +0.0 at keys >= lens[b])
hipError_t launch_ag_attention_backward(const float* qkv, const float* ctx, const float* lse, const float* dctx, const long long* lens, int B,
                                        int S, int H, int dk, float* D, float* dqkv, hipStream_t st);
// z (nullable) = u * keep * scale + x, y = LayerNorm(z) * ln_g + ln_b; rows of F = 256 / 512; keep uint8 [M, F] nullable
hipError_t launch_ag_row_forward(const float* u, const float* x, const uint8_t* keep, float scale, const float* ln_g, const float* ln_b, float* z,
                                 float* y, int M, int F, hipStream_t st);
// LayerNorm backward from the saved z: dz, du = dz * keep * scale; part [pg_row_blocks(M)][PG_SLOTS][F] doubles, slots 0 .. 2 written
// (d_ln_g, d_ln_b, column sums of du), summed by launch_pg_col_final
struct AgRowBackward {
  int M, F; float scale;
  const float *dy, *z, *ln_g; const uint8_t* keep;
  float *dz, *du; double* part;
};
hipError_t launch_ag_row_backward(const AgRowBackward& a, hipStream_t st);
// one launch: wp [3d][d] = Wq | Wk | Wv and bp [3d] (the forward's form), wt [d][3d] = wp^T and wfct [d][d] = Wfc^T (the data
// gradients' form); each output nullable
struct AgPack { const float *wq, *wk, *wv, *bq, *bk, *bv, *wfc; float *wp, *bp, *wt, *wfct; int d; };
hipError_t launch_ag_pack(const AgPack& p, hipStream_t st);
// ---- MultiHeadAttention training backward, cross-attention (xattngrad.hip; FFTBlock2.crs_attn, transformer/Layers.py:61-64) -------
// q, ctx, dctx [B*T, d]; kv [B*L, 2d] = K | V (launch_cross_attention's layout); attn, dattn [B, H, T, L] (dattn nullable); D [B, H, T];
// lens [B] = src_lens; dk in {64, 128}.
// the number of query parts of the key-owning kernel, a function of the shape alone, in [1, 8]
int xg_kv_splits(int B, int H, int T, int L);
// dq [B*T, d] and dkv [B*L, 2d] = (dK | dV), +0.0 at keys >= lens[b].  The query-owning kernel (writes D and dQ), then — unless dkv
// is null — the key-owning kernel over nsplit query parts and, for nsplit > 1, the fixed-order sum of partial [nsplit][B*L][2d].
hipError_t launch_xg_attention_backward(const float* q, const float* kv, const float* ctx, const float* attn, const float* dctx, const float* dattn,
                                        const long long* lens, int B, int T, int L, int H, int dk, int nsplit, float* D, float* partial, float* dq,
                                        float* dkv, hipStream_t st);
// one launch: wkv [2d][d] = Wk | Wv and bkv [2d] (the forward's form), wkvt [d][2d] = wkv^T, wqt = Wq^T and wfct = Wfc^T [d][d] (the
// data gradients' form); each output nullable
struct XgPack { const float *wq, *wk, *wv, *bk, *bv, *wfc; float *wkv, *bkv, *wkvt, *wqt, *wfct; int d; };
hipError_t launch_xg_pack(const XgPack& p, hipStream_t st);
// ---- PostNet training forward / backward with train-mode BatchNorm (postnetgrad.hip; transformer/Layers.py:107-177) ----------------
// Activations are row-major [M, C], C a multiple of 16 up to 512.  A column reduction gives every workgroup PN_ROW_BLOCK rows and all
// columns: thread (r, cg) owns the 16-byte column group cg and the rows r, r + 256 / (C / 4), ... of the block, sums in float64, and the
// row lanes are added in ascending order through LDS: part [pn_row_blocks(M)][slots][C] doubles, uninitialised.  The finish adds the
// blocks as 16 ascending segments, the segments in ascending order.  No atomics; every order depends on the shape alone.
constexpr int PN_ROW_BLOCK = 32;
constexpr int PN_MAX_LAYERS = 5;
constexpr int PN_PAD_N = 128;  // width the last layer's dz is padded to: the narrowest N pg_plan_wgrad takes
inline int pn_row_blocks(int M) { return (M + PN_ROW_BLOCK - 1) / PN_ROW_BLOCK; }
// part[blk][0][:] = sum u, part[blk][1][:] = sum u^2 over the block's rows
hipError_t launch_pn_stats(const float* u, int M, int C, double* part, hipStream_t st);
// What follows a column reduction.  mode PN_FIN_TRAIN: stats [2][C] doubles = mu, 1 / sqrt(biased var + 1e-5) from the two sums, and
// (running_mean non-null) running_mean = 0.9 running_mean + 0.1 mu, running_var = 0.9 running_var + 0.1 var M / (M - 1),
// *num_batches_tracked += 1.  PN_FIN_EVAL: stats from running_mean / running_var, no partials read, nothing else written.
// PN_FIN_BWD: from sum dy and sum dy xhat: out0 = d_beta, out1 = d_gamma (floats, nullable), stats = the two means (nullable).
enum PnFinMode : int { PN_FIN_TRAIN = 0, PN_FIN_EVAL = 1, PN_FIN_BWD = 2 };
struct PnFinish {
  int mode, nblk, C, M;
  const double* part; double* stats;
  float *running_mean, *running_var; long long* num_batches_tracked;
  float *out0, *out1;
};
hipError_t launch_pn_finish(const PnFinish& a, hipStream_t st);
// h [M, C] = keep * scale * tanh(gamma (u - mu) rstd + beta), without the tanh when last; keep uint8 [M, C] nullable
hipError_t launch_pn_apply(const float* u, const double* stats, const float* gamma, const float* beta, const uint8_t* keep, float scale, int last,
                           int M, int C, float* h, hipStream_t st);
// dy = dh keep scale (1 - (h / scale)^2) (last: dy = dh keep scale; h is not read), xhat = (u - mu) rstd.
// reduce: part[blk][0][:] = sum dy, part[blk][1][:] = sum dy xhat.
// apply:  dz [M, ldz] = gamma rstd (dy - means[0] - xhat means[1]), or gamma rstd dy when means is null (eval); columns [C, ldz) are
//         written as zeros; bias_part [blk][C] (nullable) = column sums of the unrounded float64 dz.  ldz = C, or PN_PAD_N >= C.
struct PnBackward {
  int M, C, ldz, last; float scale;
  const float *dh, *u, *h, *gamma; const double *stats, *means; const uint8_t* keep;
  double* part; float* dz; double* bias_part;
};
hipError_t launch_pn_bwd_reduce(const PnBackward& a, hipStream_t st);
hipError_t launch_pn_bwd_apply(const PnBackward& a, hipStream_t st);
// out[l][:] = the ascending sum over blocks of part[l] [nblk][C[l]] for every layer with a non-null out; one launch (none when all null)
struct PnBiasFinish { const double* part[PN_MAX_LAYERS]; float* out[PN_MAX_LAYERS]; int C[PN_MAX_LAYERS]; int nblk; };
hipError_t launch_pn_bias_finish(const PnBiasFinish& a, hipStream_t st);
// dst[i] = src[i], i < n, n a multiple of 4, both 16-byte aligned
hipError_t launch_pn_copy(const float* src, float* dst, long long n, hipStream_t st);
// ---- VarianceAdaptor training pieces (adaptorgrad.hip; model/modules.py:17-159, 195-230) --------------------
// The embedding gradient's plan, a function of the shape alone: row blocks of VA_ROW_BLOCK rows, column slabs of `slab` columns (the
// widest power of two up to 64 whose n_bins x slab float64 table fits VA_LDS_LIMIT), one 64-thread workgroup per (row block, slab).
constexpr int VA_ROW_BLOCK = 512;
constexpr int VA_LDS_LIMIT = 65536;
struct VaEmbedPlan { int row_blocks, rows_per_block, slab, n_slabs, lds_bytes, launches; long long ws_bytes; };
bool va_plan_embed(int M, int D, int n_bins, VaEmbedPlan* plan);  // false: D % 4 != 0, n_bins < 2, a table past the limit, M <= 0
// y[m, :] = x[m, :] + table[idx[m], :], idx[m] = wave_bucketize(bins, n_bins - 1, target[m]) written as int32; one wave per row
hipError_t launch_va_embed_fwd(const float* x, const float* target, const float* bins, const float* table, int M, int D, int n_bins, float* y,
                               int32_t* idx, hipStream_t st);
// d_table[k, :] = the sum of g[m, :] over the rows with idx[m] == k, in float64: part [row_blocks][n_bins][D] doubles (uninitialised)
// hold each block's sums in row order, the finish adds the blocks in ascending order and rounds once.  A bin no row hits is +0.0; an
// index outside [0, n_bins) contributes nothing.  Two launches, no atomics.
hipError_t launch_va_embed_bwd(const float* g, const int32_t* idx, int M, int D, int n_bins, const VaEmbedPlan& plan, double* part, float* d_table,
                               hipStream_t st);
// cum[b][l] = the inclusive prefix sum of max(duration[b][l], 0), saturated at INT32_MAX; mel_len[b] = the whole sum (int64)
hipError_t launch_va_duration_scan(const long long* duration, int B, int L, int32_t* cum, long long* mel_len, hipStream_t st);
// d_x[b, l, :] = the sum of g[b, t, :] over t in [cum[l-1], min(cum[l], T)) in t order, float64, rounded once; +0.0 for an empty range.
// One wave per phoneme, 16-byte lanes.
hipError_t launch_va_lr_bwd(const float* g, const int32_t* cum, int B, int L, int D, int T, float* d_x, hipStream_t st);
// the calling thread's ns_va_* launch counter (adaptorgrad_api.hip), for the family's entry points in other files
int& va_launch_counter();
// ---- Gaussian length regulator, training side (gaussgrad.hip; model/modules.py:162-192) ----------------------
// dur_f [B, L] = (float)max(duration, 0) for launch_gaussian_upsampling, mel_len [B] = the integer total, centres [B, L] = the serial
// fp32 scan k_gauss_centers makes from dur_f (the same bits)
hipError_t launch_gu_prepare(const long long* duration, int B, int L, float* dur_f, float* centres, long long* mel_len, hipStream_t st);
// S [B, T] = sum_l expf(-0.01f (t - c_l)^2) + 1e-20f in k_gauss_upsample's order, written for t < lim_b = min(max(own_len[b], 0), T)
// (own_len nullable: T)
hipError_t launch_gu_denominators(const float* centres, const long long* own_len, int B, int L, int T, float* S, hipStream_t st);
// d_x [B, L, D] = sum_{t < lim_b} (expf(-0.01f (t - c_l)^2) / S_t) g[b, t] in t order on the fp32 matrix cores; band: walk only the
// frames within 102 of the tile's centres (an identity); w_out (nullable) [B, L, T]: the weights used, +0.0 where none was
hipError_t launch_gu_bwd(const float* g, const float* centres, const float* S, const long long* own_len, int B, int L, int D, int T, bool band,
                         float* d_x, float* w_out, hipStream_t st);
// ---- PositionwiseFeedForward training backward (ffngrad.hip; transformer/SubLayers.py:62-95) ----------------
// dh [M, F] = h > 0 ? da : +0.0 (a select; dh may be da), F a multiple of 256; part (nullable) [pg_row_blocks(M)][PG_SLOTS][F] doubles,
// uninitialised: slot 0 of a block = the column sums of its rows of dh, summed by launch_pg_col_final at this F.  One launch.
hipError_t launch_fg_relu_gate(const float* da, const float* h, int M, int F, float* dh, double* part, hipStream_t st);
// ---- opt-in "bf16" matmul mode of the same layer (ffngrad_bf16.hip) ------------------------------------------
// The weight gradient with both operands rounded to bf16 (nearest even) and fp32 accumulation: k_pg_wgrad's tile, split and partial
// layout at FGB_STAGE rows of m per LDS stage; Cin a multiple of 32.  The plan has pg_plan_wgrad's fields and refusals.
constexpr int FGB_STAGE = 32;
bool fg_plan_wgrad_bf16(int M, int N, int Cin, int KW, PgWgradPlan* out);
// dW [N][Cin][KW] (torch layout); partial: plan.ws_floats floats.  Two launches: the GEMM, and k_pg_wgrad_reduce (predgrad.hip).
hipError_t launch_fg_wgrad_bf16(const float* dz, const float* X, int M, int S, int N, int Cin, int KW, const PgWgradPlan& pl, float* partial,
                                float* dW, hipStream_t st);
__global__ void k_pg_wgrad_reduce(const float* __restrict__ partial, int ranges, int N, int Cin, int KW, float* __restrict__ dW);
// w [N][Cin][KW] (torch layout, fp32) -> wp [N][KW][Cin] and / or wt [Cin][KW][N] with wt[c][j][n] = w[n][c][KW-1-j], both bf16 rounded
// to nearest even: the planes launch_conv_gemm_bf16 reads through ConvGemm::Wbf (N and Cin multiples of 32: no channel padding).
// Either output may be null; w == nullptr skips the entry.  Two weights per launch.
struct FgPackBf { const float* w; unsigned short* wp; unsigned short* wt; int N, Cin, KW; };
hipError_t launch_fg_pack_bf16(const FgPackBf& a, const FgPackBf& b, hipStream_t st);
// ---- TxtEncoder / MelDecoder training stacks (stackgrad.hip; transformer/Models.py:33-100, 176-244) ---------
// d_table [n_vocab, D] = the sum of g [M, D]'s rows per token id, float64 in ascending m, rounded once; row 0 (PAD) and an id no row
// carries are +0.0; a token outside [0, n_vocab) contributes nothing; g at a PAD row is not read.  D a multiple of 256.  One launch.
hipError_t launch_st_embed_grad(const float* g, const long long* texts, int M, int D, int n_vocab, float* d_table, hipStream_t st);
// y [M, D] = padded(m) ? +0.0 : x[m, :] (a select; out of place), padded(m) = mask[m] != 0, or m % S >= lens[m / S] without a mask.
// D a multiple of 256.  One launch.
hipError_t launch_st_row_mask(const float* x, const uint8_t* mask, const long long* lens, int M, int S, int D, float* y, hipStream_t st);
// ---- MelEncoder training: Prenet (melencgrad.hip; transformer/Models.py:103-173, Layers.py:11-26) ----------
// y [M, F] = h2 k + pos[m % T, :], k = scale where keep [M, F] is nonzero and 0 where it is zero (keep nullable: k = scale); float64,
// rounded once.  F a multiple of 256; pos [>= T, F].  Out of place.  One launch.
hipError_t launch_me_drop_pos(const float* h2, const float* pos, const uint8_t* keep, float scale, int M, int T, int F, float* y, hipStream_t st);
// dh [M, F] = (keep != 0 && h2 > 0) ? g scale : +0.0 (a select; dh is not g); part (nullable) as launch_fg_relu_gate's.  One launch.
hipError_t launch_me_drop_relu_gate(const float* g, const float* h2, const uint8_t* keep, float scale, int M, int F, float* dh, double* part,
                                    hipStream_t st);
// ---- mel head training: mel_linear and the PostNet residual (melheadgrad.hip; model/fastspeech2_align.py:24,83,85) --
// dz [M, PN_PAD_N] = g [M, n_mel] with +0.0 in the columns [n_mel, PN_PAD_N) (dz uninitialised, g only read); part (nullable)
// [pg_row_blocks(M)][n_mel] doubles, uninitialised: the column sums of g per 64 rows, summed by launch_pn_bias_finish at
// nblk = pg_row_blocks(M).  n_mel a multiple of 4 up to PN_PAD_N.  One launch.
hipError_t launch_mh_pad_colsum(const float* g, int M, int n_mel, float* dz, double* part, hipStream_t st);
// out [M, n_mel] = p + x; n_mel a multiple of 4.  Out of place.  One launch.
hipError_t launch_mh_residual(const float* p, const float* x, int M, int n_mel, float* out, hipStream_t st);
// sets ns_last_error() (api.hip) and returns 1
int api_fail(const char* msg);

}  // namespace ns
