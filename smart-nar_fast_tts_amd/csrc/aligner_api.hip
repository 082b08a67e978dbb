// C-ABI of the reference-mel aligner (include/nar_fs2.h ns_aln_*): the reference's MelEncoder (transformer/Models.py:103-173) —
// Prenet (transformer/Layers.py:11-26), position rows, a stack of FFTBlock2 cross-attention blocks (Layers.py:51-70) — with its
// attention maps as an output, plus the duration count over the last layer's map.  A separate handle with its own arena and
// workspace; always exact fp32.  Host-side only; every byte of device memory comes from the caller.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/nar_fs2.h"
#include "kernels.h"

using namespace ns;

static int afail(const std::string& s) { return api_fail(s.c_str()); }
#define ALN_HIP(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return afail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define ALN_TRY(expr)    \
  do {                   \
    int rc_ = (expr);    \
    if (rc_) return rc_; \
  } while (0)

namespace {
constexpr int PRENET_IN = 80, PRENET_DIM = 256;  // Prenet is hard-coded 80 -> 256 -> 256 (transformer/Layers.py:18-19)
constexpr int ALN_TICKET_INTS = 16384;           // ticket counters of one forward (gemm_conv.hip TICKET), zeroed at its start

struct Staged { std::vector<int64_t> shape; std::vector<float> data; bool set = false, optional = false; };
struct Layer { size_t wq, bq, wkv, bkv, fc, fc_b, ln1_g, ln1_b, w1, w1_b, w2, w2_b, ln2_g, ln2_b; };
size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }  // floats: 256-byte aligned offsets

struct Bump {
  char* base; size_t off = 0;
  explicit Bump(void* p) : base((char*)p) {}
  float* f(size_t n) { return (float*)raw(n * sizeof(float)); }
  void* raw(size_t bytes) {
    size_t o = off; off += (bytes + 255) & ~(size_t)255;
    return base ? base + o : nullptr;
  }
};
struct Work {
  float *xin, *xa, *xb, *x1, *q, *ctx, *t1, *hid, *kv, *pos_ext;
  int* tickets; int used;
  int* take(int n) {
    if (!tickets || used + n > ALN_TICKET_INTS) return nullptr;
    int* t = tickets + used;
    used += n;
    return t;
  }
};
}  // namespace

struct ns_aligner {
  int d, H, n_layer, d_inner, k1, k2, n_mel, max_seq_len, row_epilogue;
  std::map<std::string, Staged> staged;
  size_t n_floats = 0;
  size_t p_w1, p_b1, p_w2, p_b2, pos;
  std::vector<Layer> layers;
  float* arena = nullptr;
  bool ready = false;
  size_t take(size_t n) { size_t o = n_floats; n_floats += align64(n); return o; }
  const float* P(size_t off) const { return arena + off; }
};

static void expect(ns_aligner* a, const std::string& name, std::vector<int64_t> shape, bool optional = false) {
  Staged& s = a->staged[name];
  s.shape = std::move(shape);
  s.optional = optional;
}

extern "C" int ns_aln_abi_version(void) { return NS_ALN_ABI_VERSION; }

extern "C" int ns_aln_create(const ns_config* cfg, ns_aligner** out) {
  if (!cfg || !out) return afail("ns_aln_create: null argument");
  const ns_config& c = *cfg;
  // Prenet() takes no arguments (80 -> 256 -> 256, transformer/Layers.py:15-19) and feeds d_model-wide blocks; crs_attn.w_ks /
  // w_vs are Linear(d_model, ...) applied to the TEXT encoder's output (transformer/SubLayers.py:19-20, Layers.py:62-64)
  if (c.d_dec != PRENET_DIM || c.d_enc != c.d_dec)
    return afail("ns_aln_create: the aligner exists only for encoder_hidden == decoder_hidden == 256: Prenet is hard-coded 80 -> 256 -> 256 "
                 "(transformer/Layers.py:18-19) and crs_attn.w_ks / w_vs take d_model inputs from the text encoder (transformer/SubLayers.py:19-20); got encoder_hidden " +
                 std::to_string(c.d_enc) + ", decoder_hidden " + std::to_string(c.d_dec));
  if (c.n_mel != PRENET_IN) return afail("ns_aln_create: Prenet.w_1 is Linear(80, 256) (transformer/Layers.py:18): n_mel must be 80");
  if (c.n_dec_head <= 0 || c.d_dec % c.n_dec_head || !cross_attention_ok(c.n_dec_head, c.d_dec / c.n_dec_head))
    return afail("ns_aln_create: decoder_hidden / decoder_head must be 128 or 64 (the head widths k_cross_attention covers; transformer/Models.py:113-116), got decoder_head " +
                 std::to_string(c.n_dec_head));
  if (c.n_dec_layer < 1 || c.d_inner <= 0 || c.d_inner % 32 || c.ffn_k1 < 1 || !(c.ffn_k1 & 1) || c.ffn_k2 < 1 || !(c.ffn_k2 & 1) || c.max_seq_len < 1)
    return afail("ns_aln_create: bad layer count, conv_filter_size or conv_kernel_size (transformer/Models.py:111-119)");
  ns_aligner* a = new ns_aligner();
  a->d = c.d_dec; a->H = c.n_dec_head; a->n_layer = c.n_dec_layer; a->d_inner = c.d_inner; a->k1 = c.ffn_k1; a->k2 = c.ffn_k2;
  a->n_mel = c.n_mel; a->max_seq_len = c.max_seq_len; a->row_epilogue = c.row_epilogue;
  const int d = a->d, di = a->d_inner;
  expect(a, "mel_encoder.prenet.w_1.weight", {d, PRENET_IN});
  expect(a, "mel_encoder.prenet.w_1.bias", {d});
  expect(a, "mel_encoder.prenet.w_2.weight", {d, d});
  expect(a, "mel_encoder.prenet.w_2.bias", {d});
  expect(a, "mel_encoder.position_enc", {1, c.max_seq_len + 1, d}, true);  // a deterministic table: regenerated when absent
  a->p_w1 = a->take((size_t)d * PRENET_IN); a->p_b1 = a->take(d);
  a->p_w2 = a->take((size_t)d * d); a->p_b2 = a->take(d);
  a->pos = a->take((size_t)(c.max_seq_len + 1) * d);
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
    l.wq = a->take((size_t)d * d); l.bq = a->take(d);
    l.wkv = a->take((size_t)2 * d * d); l.bkv = a->take(2 * d);
    l.fc = a->take((size_t)d * d); l.fc_b = a->take(d);
    l.ln1_g = a->take(d); l.ln1_b = a->take(d);
    l.w1 = a->take((size_t)di * a->k1 * d); l.w1_b = a->take(di);
    l.w2 = a->take((size_t)d * a->k2 * di); l.w2_b = a->take(d);
    l.ln2_g = a->take(d); l.ln2_b = a->take(d);
    a->layers.push_back(l);
  }
  *out = a;
  return 0;
}

extern "C" void ns_aln_destroy(ns_aligner* a) { delete a; }
extern "C" size_t ns_aln_arena_bytes(const ns_aligner* a) { return a ? a->n_floats * sizeof(float) : 0; }

extern "C" int ns_aln_bind_arena(ns_aligner* a, void* dev, size_t bytes) {
  if (!a || !dev) return afail("ns_aln_bind_arena: null argument");
  if (bytes < ns_aln_arena_bytes(a)) return afail("ns_aln_bind_arena: arena too small (ns_aln_arena_bytes)");
  if ((uintptr_t)dev & 255) return afail("ns_aln_bind_arena: arena must be 256-byte aligned");
  a->arena = (float*)dev;
  a->ready = false;
  return 0;
}

static int lookup(ns_aligner* a, const char* name_c, const int64_t* shape, int ndim, Staged** slot, size_t* count, const char* who) {
  if (!a || !name_c) return afail(std::string(who) + ": null argument");
  auto it = a->staged.find(name_c);
  if (it == a->staged.end()) return afail(std::string(who) + ": unexpected key '" + name_c + "'");
  Staged& s = it->second;
  if ((int)s.shape.size() != ndim) return afail(std::string(who) + ": rank mismatch for '" + name_c + "'");
  if (ndim > 0 && !shape) return afail(std::string(who) + ": null shape for '" + name_c + "'");
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] != s.shape[i])
      return afail(std::string(who) + ": size mismatch for '" + name_c + "': dim " + std::to_string(i) + " is " + std::to_string(shape[i]) +
                   ", expected " + std::to_string(s.shape[i]));
    n *= (size_t)shape[i];
  }
  *slot = &s;
  *count = n;
  return 0;
}

extern "C" int ns_aln_check_weight(ns_aligner* a, const char* name, const int64_t* shape, int ndim) {
  Staged* s; size_t n;
  return lookup(a, name, shape, ndim, &s, &n, "ns_aln_check_weight");
}

extern "C" int ns_aln_set_weight(ns_aligner* a, const char* name, const float* host, const int64_t* shape, int ndim) {
  Staged* s; size_t n;
  ALN_TRY(lookup(a, name, shape, ndim, &s, &n, "ns_aln_set_weight"));
  if (!host) return afail(std::string("ns_aln_set_weight: null data for '") + name + "'");
  s->data.assign(host, host + n);
  s->set = true;
  a->ready = false;
  return 0;
}

extern "C" int ns_aln_finalize_weights(ns_aligner* a, void* stream) {
  if (!a) return afail("ns_aln_finalize_weights: null argument");
  if (!a->arena) return afail("ns_aln_finalize_weights: no arena bound (ns_aln_bind_arena)");
  std::string missing;
  for (auto& kv : a->staged)
    if (!kv.second.set && !kv.second.optional) missing += (missing.empty() ? "" : ", ") + kv.first;
  if (!missing.empty()) return afail("ns_aln_finalize_weights: missing keys: " + missing);
  auto S = [&](const std::string& k) -> const std::vector<float>& { return a->staged[k].data; };
  std::vector<float> img(a->n_floats, 0.f);
  auto cp = [&](size_t off, const std::string& k) { const auto& v = S(k); std::copy(v.begin(), v.end(), img.begin() + off); };
  // Conv1d [out][in][k] -> [out][k][in] (tap-major K of the implicit GEMM)
  auto pack_conv = [&](size_t off, const std::string& k, int cout, int cin, int kw) {
    const auto& w = S(k);
    for (int o = 0; o < cout; ++o)
      for (int c = 0; c < cin; ++c)
        for (int j = 0; j < kw; ++j) img[off + ((size_t)o * kw + j) * cin + c] = w[((size_t)o * cin + c) * kw + j];
  };
  const int d = a->d;
  cp(a->p_w1, "mel_encoder.prenet.w_1.weight"); cp(a->p_b1, "mel_encoder.prenet.w_1.bias");
  cp(a->p_w2, "mel_encoder.prenet.w_2.weight"); cp(a->p_b2, "mel_encoder.prenet.w_2.bias");
  if (a->staged["mel_encoder.position_enc"].set) cp(a->pos, "mel_encoder.position_enc");
  else {  // transformer/Models.py:10-30
    for (int p = 0; p <= a->max_seq_len; ++p)
      for (int j = 0; j < d; ++j) {
        const double ang = (double)p / std::pow(10000.0, (double)(2 * (j / 2)) / (double)d);
        img[a->pos + (size_t)p * d + j] = (float)((j & 1) ? std::cos(ang) : std::sin(ang));
      }
  }
  for (int i = 0; i < a->n_layer; ++i) {
    const Layer& l = a->layers[i];
    const std::string p = "mel_encoder.layer_stack." + std::to_string(i);
    cp(l.wq, p + ".crs_attn.w_qs.weight"); cp(l.bq, p + ".crs_attn.w_qs.bias");
    cp(l.wkv, p + ".crs_attn.w_ks.weight"); cp(l.wkv + (size_t)d * d, p + ".crs_attn.w_vs.weight");  // K | V fused: [2d, d]
    cp(l.bkv, p + ".crs_attn.w_ks.bias"); cp(l.bkv + d, p + ".crs_attn.w_vs.bias");
    cp(l.fc, p + ".crs_attn.fc.weight"); cp(l.fc_b, p + ".crs_attn.fc.bias");
    cp(l.ln1_g, p + ".crs_attn.layer_norm.weight"); cp(l.ln1_b, p + ".crs_attn.layer_norm.bias");
    pack_conv(l.w1, p + ".pos_ffn.w_1.weight", a->d_inner, d, a->k1); cp(l.w1_b, p + ".pos_ffn.w_1.bias");
    pack_conv(l.w2, p + ".pos_ffn.w_2.weight", d, a->d_inner, a->k2); cp(l.w2_b, p + ".pos_ffn.w_2.bias");
    cp(l.ln2_g, p + ".pos_ffn.layer_norm.weight"); cp(l.ln2_b, p + ".pos_ffn.layer_norm.bias");
  }
  hipStream_t st = (hipStream_t)stream;
  ALN_HIP(hipMemcpyAsync(a->arena, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st));
  ALN_HIP(hipStreamSynchronize(st));  // img is a local
  for (auto& kv : a->staged) { kv.second.data.clear(); kv.second.data.shrink_to_fit(); kv.second.set = false; }
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
  w.tickets = (int*)bp.raw(ALN_TICKET_INTS * sizeof(int));
  w.used = 0;
  return w;
}

extern "C" size_t ns_aln_ws_bytes(const ns_aligner* a, int B, int L, int T) {
  if (!a || B <= 0 || L <= 0 || T <= 0) return 256;
  Bump bp(nullptr);
  carve(a, bp, B, L, T);
  return bp.off + 256;
}

// ------------------------------------------------------------------------------------------------ launches
static int gemm(const float* X, int ldx, const float* W, const float* bias, const float* resid, float* Y, int M, int N, int Cin, int KW,
                int S, int act, hipStream_t st, const RowEpilogue* epi = nullptr) {
  ConvGemm p;
  memset(&p, 0, sizeof(p));
  p.X = X; p.ldx = ldx; p.W = W; p.bias = bias; p.resid = resid; p.ldr = N; p.Y = Y; p.ldy = N;
  p.M = M; p.N = N; p.Cin = Cin; p.KW = KW; p.pad = (KW - 1) / 2; p.S = S; p.act = act;
  p.epi = epi ? EPI_LN : EPI_NONE;
  if (epi) p.e = *epi;
  ALN_HIP(launch_conv_gemm(p, st));
  return 0;
}

// Y = mask(LayerNorm(conv(X) + resid)): the full-row tile on large launches, the ticketed ladder on small ones (the rule of the
// decoder's blocks, api.hip gemm_ln), two launches when neither applies
static int gemm_ln(const float* X, int ldx, const float* W, const float* bias, const float* resid, float* tmp, float* Y, int M, int N, int Cin,
                   int KW, int S, const float* g, const float* b, const long long* lens, const ns_aligner* a, Work& w, hipStream_t st) {
  RowEpilogue e;
  memset(&e, 0, sizeof(e));
  e.ln_g = g; e.ln_b = b; e.lens = lens;
  if (conv_gemm_row_epilogue_ok(M, N, Cin) && (M + 31) / 32 >= 200) return gemm(X, ldx, W, bias, resid, Y, M, N, Cin, KW, S, ACT_NONE, st, &e);
  if (a->row_epilogue == 0 && conv_gemm_ticket_ok(M, N, Cin) && (e.ticket = w.take(conv_gemm_ticket_ints(M))) != nullptr) {
    e.y_out = Y;
    return gemm(X, ldx, W, bias, resid, tmp, M, N, Cin, KW, S, ACT_NONE, st, &e);
  }
  ALN_TRY(gemm(X, ldx, W, bias, resid, tmp, M, N, Cin, KW, S, ACT_NONE, st));
  ALN_HIP(launch_layernorm(tmp, g, b, Y, M, N, S, lens, st));
  return 0;
}

static int check_ready(const ns_aligner* a, const char* who) {
  if (!a) return afail(std::string(who) + ": null aligner");
  if (!a->ready || !a->arena) return afail(std::string(who) + ": weights not finalized (ns_aln_finalize_weights)");
  return 0;
}

extern "C" int ns_aln_forward(ns_aligner* a, const float* src_output, const int64_t* src_lens, const float* mels, const int64_t* mel_lens,
                              int B, int L, int T, float* tgt_output, float* attn_all_layers, int64_t* durations, void* ws, size_t ws_bytes,
                              void* stream) {
  ALN_TRY(check_ready(a, "ns_aln_forward"));
  if (B < 0 || L < 0 || T < 0) return afail("ns_aln_forward: negative size");
  if (B == 0 || T == 0) return 0;
  if (L == 0) return afail("ns_aln_forward: L must be >= 1 (softmax over an empty key axis)");
  if (!src_output || !src_lens || !mels || !mel_lens || !tgt_output || !attn_all_layers || !durations || !ws) return afail("ns_aln_forward: null argument");
  if ((long long)B * T >= (1ll << 31) / a->d_inner || (long long)B * L >= (1ll << 31) / (2 * a->d)) return afail("ns_aln_forward: problem too large");
  if (ws_bytes < ns_aln_ws_bytes(a, B, L, T)) return afail("ns_aln_forward: workspace too small (ns_aln_ws_bytes)");
  if ((uintptr_t)ws & 255) return afail("ns_aln_forward: workspace must be 256-byte aligned");
  if (((uintptr_t)mels | (uintptr_t)src_output | (uintptr_t)tgt_output) & 15) return afail("ns_aln_forward: mels, src_output and tgt_output must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long* slens = reinterpret_cast<const long long*>(src_lens);
  const long long* mlens = reinterpret_cast<const long long*>(mel_lens);
  Bump bp(ws);
  Work w = carve(a, bp, B, L, T);
  const int M = B * T, d = a->d, H = a->H;
  ALN_HIP(hipMemsetAsync(w.tickets, 0, ALN_TICKET_INTS * sizeof(int), st));
  // input: frame 0 := zeros (transformer/Models.py:145-146); `mels` itself is never written
  ALN_HIP(launch_aln_input(mels, w.xin, B, T, a->n_mel, st));
  // Prenet: relu(w_2(relu(w_1(x)))), dropout = identity in eval() (transformer/Layers.py:22-26)
  ALN_TRY(gemm(w.xin, a->n_mel, a->P(a->p_w1), a->P(a->p_b1), nullptr, w.t1, M, d, a->n_mel, 1, T, ACT_RELU, st));
  ALN_TRY(gemm(w.t1, d, a->P(a->p_w2), a->P(a->p_b2), nullptr, w.xb, M, d, d, 1, T, ACT_RELU, st));
  // position rows: the cached parameter, or the regenerated table for T > max_seq_len (transformer/Models.py:149-164)
  const float* pos = a->P(a->pos);
  if (T > a->max_seq_len) {
    ALN_HIP(launch_sinusoid(T, d, w.pos_ext, st));
    pos = w.pos_ext;
  }
  ALN_HIP(launch_add_pos(w.xb, pos, w.xa, M, T, d, st));
  float* cur = w.xa;
  float* alt = w.xb;
  const size_t attn_layer = (size_t)B * H * T * (size_t)L;
  for (int i = 0; i < a->n_layer; ++i) {
    const Layer& l = a->layers[i];
    float* dst = (i + 1 == a->n_layer) ? tgt_output : alt;
    // FFTBlock2.forward (transformer/Layers.py:61-70): crs_attn(tgt, src, src), masked_fill, pos_ffn, masked_fill
    ALN_TRY(gemm(cur, d, a->P(l.wq), a->P(l.bq), nullptr, w.q, M, d, d, 1, T, ACT_NONE, st));
    ALN_TRY(gemm(src_output, d, a->P(l.wkv), a->P(l.bkv), nullptr, w.kv, B * L, 2 * d, d, 1, L, ACT_NONE, st));
    ALN_HIP(launch_cross_attention(w.q, w.kv, slens, B, T, L, H, d / H, w.ctx, attn_all_layers + (size_t)i * attn_layer, st));
    ALN_TRY(gemm_ln(w.ctx, d, a->P(l.fc), a->P(l.fc_b), cur, w.t1, w.x1, M, d, d, 1, T, a->P(l.ln1_g), a->P(l.ln1_b), mlens, a, w, st));
    ALN_TRY(gemm(w.x1, d, a->P(l.w1), a->P(l.w1_b), nullptr, w.hid, M, a->d_inner, d, a->k1, T, ACT_RELU, st));
    ALN_TRY(gemm_ln(w.hid, a->d_inner, a->P(l.w2), a->P(l.w2_b), w.x1, w.t1, dst, M, d, a->d_inner, a->k2, T, a->P(l.ln2_g), a->P(l.ln2_b), mlens, a, w,
                    st));
    if (dst != tgt_output) { alt = cur; cur = dst; }
  }
  // EXTENSION beyond the reference: per-phoneme frame counts from the last layer's alignment
  ALN_HIP(launch_aln_durations(attn_all_layers + (size_t)(a->n_layer - 1) * attn_layer, slens, mlens, B, H, T, L, reinterpret_cast<long long*>(durations), st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ per-operator entry points
extern "C" int ns_aln_op_cross_attention(const float* q, const float* kv, const int64_t* src_lens, int B, int T, int L, int H, int dk,
                                         float* ctx, float* attn, void* stream) {
  if (!q || !kv || !src_lens || !ctx || !attn || B <= 0 || T <= 0 || L <= 0) return afail("ns_aln_op_cross_attention: bad argument");
  if (!cross_attention_ok(H, dk)) return afail("ns_aln_op_cross_attention: dk must be 64 or 128");
  ALN_HIP(launch_cross_attention(q, kv, reinterpret_cast<const long long*>(src_lens), B, T, L, H, dk, ctx, attn, (hipStream_t)stream));
  return 0;
}

extern "C" int ns_aln_op_durations(const float* attn_last, const int64_t* src_lens, const int64_t* mel_lens, int B, int H, int T, int L,
                                   int64_t* out, void* stream) {
  if (!attn_last || !src_lens || !mel_lens || !out || B <= 0 || H <= 0 || T < 0 || L <= 0) return afail("ns_aln_op_durations: bad argument");
  ALN_HIP(launch_aln_durations(attn_last, reinterpret_cast<const long long*>(src_lens), reinterpret_cast<const long long*>(mel_lens), B, H, T, L,
                               reinterpret_cast<long long*>(out), (hipStream_t)stream));
  return 0;
}
