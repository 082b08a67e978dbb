// C-ABI of the reference-mel aligner (include/nar_fs2.h ns_aln_*): the reference's MelEncoder (transformer/Models.py:103-173) —
// Prenet (transformer/Layers.py:11-26), position rows, a stack of FFTBlock2 cross-attention blocks (Layers.py:51-70) — with its
// attention maps as an output, plus the duration count over the last layer's map.  A separate handle with its own arena and
// workspace; always exact fp32.  Host-side only; every byte of device memory comes from the caller.
#include <cstdio>

#include "../../include/nar_fs2.h"
#include "host_core.h"

using namespace ns;

namespace {
constexpr int PRENET_IN = 80, PRENET_DIM = 256;  // Prenet is hard-coded 80 -> 256 -> 256 (transformer/Layers.py:18-19)

struct Layer { ConvW q, kv, fc, w1, w2; size_t ln1_g, ln1_b, ln2_g, ln2_b; };  // kv: K | V fused, [2d, d]

struct Work {
  float *xin, *xa, *xb, *x1, *q, *ctx, *t1, *hid, *kv, *pos_ext;
  int* ticket_block;  // zeroed at the forward's start
  Tickets tk;         // the cursor over it ("two_launch": disabled)
};
}  // namespace

struct ns_aligner {
  int d, H, n_layer, d_inner, k1, k2, n_mel, max_seq_len, row_epilogue;
  WeightRegistry weights;
  Arena ar;
  ConvW prenet1, prenet2;
  size_t pos;
  std::vector<Layer> layers;
  float* arena = nullptr;
  bool ready = false;
  const float* P(size_t off) const { return arena + off; }
};

static void expect(ns_aligner* a, const std::string& name, std::vector<int64_t> shape, bool optional = false) {
  a->weights.expect(name, std::move(shape), optional);
}

extern "C" int ns_aln_abi_version(void) { return NS_ALN_ABI_VERSION; }

extern "C" int ns_aln_create(const ns_config* cfg, ns_aligner** out) {
  if (!cfg || !out) return api_fail("ns_aln_create: null argument");
  const ns_config& c = *cfg;
  // Prenet() takes no arguments (80 -> 256 -> 256, transformer/Layers.py:15-19) and feeds d_model-wide blocks; crs_attn.w_ks /
  // w_vs are Linear(d_model, ...) applied to the TEXT encoder's output (transformer/SubLayers.py:19-20, Layers.py:62-64)
  if (c.d_dec != PRENET_DIM || c.d_enc != c.d_dec)
    return api_fail("ns_aln_create: the aligner exists only for encoder_hidden == decoder_hidden == 256: Prenet is hard-coded 80 -> 256 -> 256 "
                 "(transformer/Layers.py:18-19) and crs_attn.w_ks / w_vs take d_model inputs from the text encoder (transformer/SubLayers.py:19-20); got encoder_hidden " +
                 std::to_string(c.d_enc) + ", decoder_hidden " + std::to_string(c.d_dec));
  if (c.n_mel != PRENET_IN) return api_fail("ns_aln_create: Prenet.w_1 is Linear(80, 256) (transformer/Layers.py:18): n_mel must be 80");
  if (c.n_dec_head <= 0 || c.d_dec % c.n_dec_head || !cross_attention_ok(c.n_dec_head, c.d_dec / c.n_dec_head))
    return api_fail("ns_aln_create: decoder_hidden / decoder_head must be 128 or 64 (the head widths k_cross_attention covers; transformer/Models.py:113-116), got decoder_head " +
                 std::to_string(c.n_dec_head));
  if (c.n_dec_layer < 1 || c.d_inner <= 0 || c.d_inner % 32 || c.ffn_k1 < 1 || !(c.ffn_k1 & 1) || c.ffn_k2 < 1 || !(c.ffn_k2 & 1) || c.max_seq_len < 1)
    return api_fail("ns_aln_create: bad layer count, conv_filter_size or conv_kernel_size (transformer/Models.py:111-119)");
  ns_aligner* a = new ns_aligner();
  a->d = c.d_dec; a->H = c.n_dec_head; a->n_layer = c.n_dec_layer; a->d_inner = c.d_inner; a->k1 = c.ffn_k1; a->k2 = c.ffn_k2;
  a->n_mel = c.n_mel; a->max_seq_len = c.max_seq_len; a->row_epilogue = c.row_epilogue;
  const int d = a->d, di = a->d_inner;
  expect(a, "mel_encoder.prenet.w_1.weight", {d, PRENET_IN});
  expect(a, "mel_encoder.prenet.w_1.bias", {d});
  expect(a, "mel_encoder.prenet.w_2.weight", {d, d});
  expect(a, "mel_encoder.prenet.w_2.bias", {d});
  expect(a, "mel_encoder.position_enc", {1, c.max_seq_len + 1, d}, true);  // a deterministic table: regenerated when absent
  a->prenet1 = a->ar.conv(d, 1, PRENET_IN);
  a->prenet2 = a->ar.conv(d, 1, d);
  a->pos = a->ar.take((size_t)(c.max_seq_len + 1) * d);
  for (int i = 0; i < a->n_layer; ++i) {
    const std::string p = "mel_encoder.layer_stack." + std::to_string(i);
    for (const char* w : {"w_qs", "w_ks", "w_vs", "fc"}) {
      expect(a, p + ".crs_attn." + w + ".weight", {d, d});
      expect(a, p + ".crs_attn." + w + ".bias", {d});
    }
    expect(a, p + ".crs_attn.layer_norm.weight", {d});
    expect(a, p + ".crs_attn.layer_norm.bias", {d});
    expect(a, p + ".pos_ffn.w_1.weight", {di, d, a->k1});
    expect(a, p + ".pos_ffn.w_1.bias", {di});
    expect(a, p + ".pos_ffn.w_2.weight", {d, di, a->k2});
    expect(a, p + ".pos_ffn.w_2.bias", {d});
    expect(a, p + ".pos_ffn.layer_norm.weight", {d});
    expect(a, p + ".pos_ffn.layer_norm.bias", {d});
    Layer l;
    l.q = a->ar.conv(d, 1, d);
    l.kv = a->ar.conv(2 * d, 1, d);
    l.fc = a->ar.conv(d, 1, d);
    l.ln1_g = a->ar.take(d); l.ln1_b = a->ar.take(d);
    l.w1 = a->ar.conv(di, a->k1, d);
    l.w2 = a->ar.conv(d, a->k2, di);
    l.ln2_g = a->ar.take(d); l.ln2_b = a->ar.take(d);
    a->layers.push_back(l);
  }
  *out = a;
  return 0;
}

extern "C" void ns_aln_destroy(ns_aligner* a) { delete a; }
extern "C" size_t ns_aln_arena_bytes(const ns_aligner* a) { return a ? a->ar.n * sizeof(float) : 0; }

extern "C" int ns_aln_bind_arena(ns_aligner* a, void* dev, size_t bytes) {
  return bind_arena(a, dev, bytes, ns_aln_arena_bytes(a), "ns_aln_bind_arena", "arena too small (ns_aln_arena_bytes)");
}

extern "C" int ns_aln_check_weight(ns_aligner* a, const char* name, const int64_t* shape, int ndim) {
  return check_weight(a, name, shape, ndim, "ns_aln_check_weight");
}

extern "C" int ns_aln_set_weight(ns_aligner* a, const char* name, const float* host, const int64_t* shape, int ndim) {
  return set_weight(a, name, host, shape, ndim, "ns_aln_set_weight");
}

extern "C" int ns_aln_finalize_weights(ns_aligner* a, void* stream) {
  if (!a) return api_fail("ns_aln_finalize_weights: null argument");
  if (!a->arena) return api_fail("ns_aln_finalize_weights: no arena bound (ns_aln_bind_arena)");
  const std::vector<std::string> missing = a->weights.missing();
  if (!missing.empty()) return api_fail("ns_aln_finalize_weights: missing keys: " + join_names(missing));
  auto S = [&](const std::string& k) -> const std::vector<float>& { return a->weights.data(k); };
  std::vector<float> img(a->ar.n, 0.f);
  auto cp = [&](size_t off, const std::string& k) { const auto& v = S(k); std::copy(v.begin(), v.end(), img.begin() + off); };
  const int d = a->d;
  cp(a->prenet1.w, "mel_encoder.prenet.w_1.weight"); cp(a->prenet1.b, "mel_encoder.prenet.w_1.bias");
  cp(a->prenet2.w, "mel_encoder.prenet.w_2.weight"); cp(a->prenet2.b, "mel_encoder.prenet.w_2.bias");
  if (a->weights.is_set("mel_encoder.position_enc")) cp(a->pos, "mel_encoder.position_enc");
  else host_sinusoid(a->max_seq_len + 1, d, &img[a->pos]);
  for (int i = 0; i < a->n_layer; ++i) {
    const Layer& l = a->layers[i];
    const std::string p = "mel_encoder.layer_stack." + std::to_string(i);
    cp(l.q.w, p + ".crs_attn.w_qs.weight"); cp(l.q.b, p + ".crs_attn.w_qs.bias");
    cp(l.kv.w, p + ".crs_attn.w_ks.weight"); cp(l.kv.w + (size_t)d * d, p + ".crs_attn.w_vs.weight");  // K | V fused: [2d, d]
    cp(l.kv.b, p + ".crs_attn.w_ks.bias"); cp(l.kv.b + d, p + ".crs_attn.w_vs.bias");
    cp(l.fc.w, p + ".crs_attn.fc.weight"); cp(l.fc.b, p + ".crs_attn.fc.bias");
    cp(l.ln1_g, p + ".crs_attn.layer_norm.weight"); cp(l.ln1_b, p + ".crs_attn.layer_norm.bias");
    pack_conv(S(p + ".pos_ffn.w_1.weight"), a->d_inner, d, a->k1, &img[l.w1.w]); cp(l.w1.b, p + ".pos_ffn.w_1.bias");
    pack_conv(S(p + ".pos_ffn.w_2.weight"), d, a->d_inner, a->k2, &img[l.w2.w]); cp(l.w2.b, p + ".pos_ffn.w_2.bias");
    cp(l.ln2_g, p + ".pos_ffn.layer_norm.weight"); cp(l.ln2_b, p + ".pos_ffn.layer_norm.bias");
  }
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(hipMemcpyAsync(a->arena, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st));
  NS_HIP(hipStreamSynchronize(st));  // img is a local
  a->weights.release();
  a->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ workspace
static Work carve(const ns_aligner* a, Bump& bp, int B, int L, int T) {
  Work w;
  const size_t M = (size_t)B * T, d = a->d;
  w.xin = bp.f(M * a->n_mel);
  w.xa = bp.f(M * d); w.xb = bp.f(M * d); w.x1 = bp.f(M * d);
  w.q = bp.f(M * d); w.ctx = bp.f(M * d); w.t1 = bp.f(M * d);
  w.hid = bp.f(M * a->d_inner);
  w.kv = bp.f((size_t)B * L * 2 * d);
  w.pos_ext = T > a->max_seq_len ? bp.f((size_t)T * d) : nullptr;
  w.ticket_block = (int*)bp.raw(TICKET_INTS * sizeof(int));
  w.tk.base = a->row_epilogue == 0 ? w.ticket_block : nullptr;
  w.tk.used = 0;
  return w;
}

extern "C" size_t ns_aln_ws_bytes(const ns_aligner* a, int B, int L, int T) {
  if (!a || B <= 0 || L <= 0 || T <= 0) return 256;
  Bump bp(nullptr);
  carve(a, bp, B, L, T);
  return bp.off + 256;
}

// ------------------------------------------------------------------------------------------------ launches
// the contraction of weight w over the M rows of X ([M, w.cin], utterances of S rows), `+ resid` (nullable), into Y [M, w.cout]
static ConvGemm prepare(const ns_aligner* a, const ConvW& w, const float* X, const float* resid, float* Y, int M, int S, int act) {
  ConvGemm p;
  memset(&p, 0, sizeof(p));
  p.X = X; p.ldx = w.cin; p.W = a->P(w.w); p.bias = a->P(w.b); p.resid = resid; p.ldr = w.cout; p.Y = Y; p.ldy = w.cout;
  p.M = M; p.N = w.cout; p.Cin = w.cin; p.KW = w.kw; p.pad = (w.kw - 1) / 2; p.S = S; p.act = act;
  return p;
}
static int gemm(const ns_aligner* a, const ConvW& w, const float* X, const float* resid, float* Y, int M, int S, int act, hipStream_t st) {
  NS_HIP(launch_conv_gemm(prepare(a, w, X, resid, Y, M, S, act), st));
  return 0;
}

// Y = mask(LayerNorm(conv_w(X) + resid)), g / b the LayerNorm's weights: the ladder of the decoder's blocks (host_core.h gemm_ln_fp32)
static int gemm_ln(const ns_aligner* a, const ConvW& w, const float* X, const float* resid, float* tmp, float* Y, int M, int S, size_t g,
                   size_t b, const long long* lens, Work& wk, hipStream_t st) {
  RowEpilogue e;
  memset(&e, 0, sizeof(e));
  e.ln_g = a->P(g); e.ln_b = a->P(b); e.lens = lens;
  return gemm_ln_fp32(prepare(a, w, X, resid, nullptr, M, S, ACT_NONE), e, tmp, Y, wk.tk, st);
}

static int check_ready(const ns_aligner* a, const char* who) {
  if (!a) return api_fail(std::string(who) + ": null aligner");
  if (!a->ready || !a->arena) return api_fail(std::string(who) + ": weights not finalized (ns_aln_finalize_weights)");
  return 0;
}

extern "C" int ns_aln_forward(ns_aligner* a, const float* src_output, const int64_t* src_lens, const float* mels, const int64_t* mel_lens,
                              int B, int L, int T, float* tgt_output, float* attn_all_layers, int64_t* durations, void* ws, size_t ws_bytes,
                              void* stream) {
  NS_TRY(check_ready(a, "ns_aln_forward"));
  if (B < 0 || L < 0 || T < 0) return api_fail("ns_aln_forward: negative size");
  if (B == 0 || T == 0) return 0;
  if (L == 0) return api_fail("ns_aln_forward: L must be >= 1 (softmax over an empty key axis)");
  if (!src_output || !src_lens || !mels || !mel_lens || !tgt_output || !attn_all_layers || !durations || !ws) return api_fail("ns_aln_forward: null argument");
  if ((long long)B * T >= (1ll << 31) / a->d_inner || (long long)B * L >= (1ll << 31) / (2 * a->d)) return api_fail("ns_aln_forward: problem too large");
  if (ws_bytes < ns_aln_ws_bytes(a, B, L, T)) return api_fail("ns_aln_forward: workspace too small (ns_aln_ws_bytes)");
  if ((uintptr_t)ws & 255) return api_fail("ns_aln_forward: workspace must be 256-byte aligned");
  if (((uintptr_t)mels | (uintptr_t)src_output | (uintptr_t)tgt_output) & 15) return api_fail("ns_aln_forward: mels, src_output and tgt_output must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long* slens = reinterpret_cast<const long long*>(src_lens);
  const long long* mlens = reinterpret_cast<const long long*>(mel_lens);
  Bump bp(ws);
  Work w = carve(a, bp, B, L, T);
  const int M = B * T, d = a->d, H = a->H;
  NS_HIP(hipMemsetAsync(w.ticket_block, 0, TICKET_INTS * sizeof(int), st));
  // input: frame 0 := zeros (transformer/Models.py:145-146); `mels` itself is never written
  NS_HIP(launch_aln_input(mels, w.xin, B, T, a->n_mel, st));
  // Prenet: relu(w_2(relu(w_1(x)))), dropout = identity in eval() (transformer/Layers.py:22-26)
  NS_TRY(gemm(a, a->prenet1, w.xin, nullptr, w.t1, M, T, ACT_RELU, st));
  NS_TRY(gemm(a, a->prenet2, w.t1, nullptr, w.xb, M, T, ACT_RELU, st));
  // position rows: the cached parameter, or the regenerated table for T > max_seq_len (transformer/Models.py:149-164)
  const float* pos = a->P(a->pos);
  if (T > a->max_seq_len) {
    NS_HIP(launch_sinusoid(T, d, w.pos_ext, st));
    pos = w.pos_ext;
  }
  NS_HIP(launch_add_pos(w.xb, pos, w.xa, M, T, d, st));
  float* cur = w.xa;
  float* alt = w.xb;
  const size_t attn_layer = (size_t)B * H * T * (size_t)L;
  for (int i = 0; i < a->n_layer; ++i) {
    const Layer& l = a->layers[i];
    float* dst = (i + 1 == a->n_layer) ? tgt_output : alt;
    // FFTBlock2.forward (transformer/Layers.py:61-70): crs_attn(tgt, src, src), masked_fill, pos_ffn, masked_fill
    NS_TRY(gemm(a, l.q, cur, nullptr, w.q, M, T, ACT_NONE, st));
    NS_TRY(gemm(a, l.kv, src_output, nullptr, w.kv, B * L, L, ACT_NONE, st));
    NS_HIP(launch_cross_attention(w.q, w.kv, slens, B, T, L, H, d / H, w.ctx, attn_all_layers + (size_t)i * attn_layer, st));
    NS_TRY(gemm_ln(a, l.fc, w.ctx, cur, w.t1, w.x1, M, T, l.ln1_g, l.ln1_b, mlens, w, st));
    NS_TRY(gemm(a, l.w1, w.x1, nullptr, w.hid, M, T, ACT_RELU, st));
    NS_TRY(gemm_ln(a, l.w2, w.hid, w.x1, w.t1, dst, M, T, l.ln2_g, l.ln2_b, mlens, w, st));
    if (dst != tgt_output) { alt = cur; cur = dst; }
  }
  // EXTENSION beyond the reference: per-phoneme frame counts from the last layer's alignment
  NS_HIP(launch_aln_durations(attn_all_layers + (size_t)(a->n_layer - 1) * attn_layer, slens, mlens, B, H, T, L, reinterpret_cast<long long*>(durations), st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ per-operator entry points
extern "C" int ns_aln_op_cross_attention(const float* q, const float* kv, const int64_t* src_lens, int B, int T, int L, int H, int dk,
                                         float* ctx, float* attn, void* stream) {
  if (!q || !kv || !src_lens || !ctx || !attn || B <= 0 || T <= 0 || L <= 0) return api_fail("ns_aln_op_cross_attention: bad argument");
  if (!cross_attention_ok(H, dk)) return api_fail("ns_aln_op_cross_attention: dk must be 64 or 128");
  NS_HIP(launch_cross_attention(q, kv, reinterpret_cast<const long long*>(src_lens), B, T, L, H, dk, ctx, attn, (hipStream_t)stream));
  return 0;
}

// k_aln_input alone: x [B, T, C] = mels with frame 0 of every utterance replaced by zeros; C % 4 == 0, both pointers 16-byte aligned
extern "C" int ns_aln_op_input(const float* mels, float* x, int B, int T, int C, void* stream) {
  if (!mels || !x || B <= 0 || T <= 0 || C <= 0) return api_fail("ns_aln_op_input: bad argument");
  if ((C & 3) || (((uintptr_t)mels | (uintptr_t)x) & 15)) return api_fail("ns_aln_op_input: C must be a multiple of 4 and the pointers 16-byte aligned");
  NS_HIP(launch_aln_input(mels, x, B, T, C, (hipStream_t)stream));
  return 0;
}

extern "C" int ns_aln_op_durations(const float* attn_last, const int64_t* src_lens, const int64_t* mel_lens, int B, int H, int T, int L,
                                   int64_t* out, void* stream) {
  if (!attn_last || !src_lens || !mel_lens || !out || B <= 0 || H <= 0 || T < 0 || L <= 0) return api_fail("ns_aln_op_durations: bad argument");
  NS_HIP(launch_aln_durations(attn_last, reinterpret_cast<const long long*>(src_lens), reinterpret_cast<const long long*>(mel_lens), B, H, T, L,
                               reinterpret_cast<long long*>(out), (hipStream_t)stream));
  return 0;
}
