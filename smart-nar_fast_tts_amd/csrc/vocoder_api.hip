// C-ABI of the HiFi-GAN vocoder (include/nar_fs2.h ns_voc_*): config validation, weight registry / packing, workspace plan
// and the launch sequence of hifigan.Generator.forward.  Host-side only; every byte of device memory comes from the caller.
#include <cstdio>

#include "../../include/nar_fs2.h"
#include "host_core.h"

using namespace ns;

namespace {
constexpr float LRELU_SLOPE = 0.1f;   // hifigan/models.py LRELU_SLOPE
constexpr float POST_SLOPE = 0.01f;   // F.leaky_relu's default, what the generator applies ahead of conv_post
constexpr int PRE_POST_K = 7;         // conv_pre / conv_post: kernel 7, padding 3
constexpr int N_DIL = 3;              // ResBlock1: three (c1, c2) pairs

struct Conv { size_t w = 0, b = 0, wbf = 0; int cin = 0, cout = 0, k = 0, dil = 1; };  // wbf: bf16 plane, bytes past the fp32 image
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }  // bytes
}  // namespace

struct ns_vocoder {
  ns_voc_config cfg;
  WeightRegistry weights;
  Arena ar;               // the fp32 image
  size_t bf16_bytes = 0;  // the bf16 planes of matmul mode 1: one per upsampler and resblock conv weight, after the fp32 image
  int matmul = 0;         // 0 fp32, 1 bf16 (ns_voc_set_matmul)
  Conv pre, post;
  std::vector<Conv> ups;     // polyphase weights [u Cout][2 Cin], bias [Cout]
  std::vector<Conv> c1, c2;  // [(n_rb i + j) * 3 + n]
  float* arena = nullptr;
  bool ready = false;

  size_t take_bf16(size_t n) { size_t o = bf16_bytes; bf16_bytes += align256(n * 2); return o; }
  int ch(int i) const { return cfg.initial_channel >> i; }  // channels after upsampler i - 1 (ch(0) = C0)
  long long hop() const { long long h = 1; for (int i = 0; i < cfg.n_up; ++i) h *= cfg.up_rates[i]; return h; }
};

static void expect(ns_vocoder* v, const std::string& name, std::vector<int64_t> shape) { v->weights.expect(name, std::move(shape)); }

extern "C" int ns_voc_abi_version(void) { return NS_VOC_ABI_VERSION; }

extern "C" int ns_voc_create(const ns_voc_config* cfg, ns_vocoder** out) {
  if (!cfg || !out) return api_fail("ns_voc_create: null argument");
  const ns_voc_config& c = *cfg;
  if (c.resblock != 1) return api_fail("ns_voc_create: only resblock \"1\" (ResBlock1, the LJSpeech / universal HiFi-GAN generators) is supported");
  if (c.n_mel <= 0 || c.n_mel % 16) return api_fail("ns_voc_create: n_mel must be a positive multiple of 16");
  if (c.n_up < 1 || c.n_up > 4) return api_fail("ns_voc_create: n_up (len(upsample_rates)) must be 1..4");
  if (c.n_rb < 1 || c.n_rb > 4) return api_fail("ns_voc_create: n_rb (len(resblock_kernel_sizes)) must be 1..4");
  for (int i = 0; i < c.n_up; ++i) {
    const int u = c.up_rates[i], k = c.up_kernels[i];
    if (u < 2 || u % 2) return api_fail("ns_voc_create: upsample rate " + std::to_string(i) + " must be even (padding (k - u) / 2 = u / 2)");
    if (k != 2 * u) return api_fail("ns_voc_create: upsample kernel " + std::to_string(i) + " must be 2 * rate (the polyphase form covers k = 2u)");
  }
  for (int i = 1; i <= c.n_up; ++i) {
    const int chi = c.initial_channel >> i;
    if (c.initial_channel <= 0 || (chi << i) != c.initial_channel || chi % 32)
      return api_fail("ns_voc_create: initial_channel >> i must be a multiple of 32 for i = 1..n_up");
  }
  for (int j = 0; j < c.n_rb; ++j) {
    if (c.rb_kernels[j] < 1 || !(c.rb_kernels[j] & 1)) return api_fail("ns_voc_create: resblock kernel sizes must be odd");
    for (int n = 0; n < N_DIL; ++n)
      if (c.rb_dilations[j][n] < 1) return api_fail("ns_voc_create: ResBlock1 takes three dilations >= 1 per resblock");
    if (c.rb_dilations[j][3] != 0) return api_fail("ns_voc_create: ResBlock1 takes exactly three dilations (rb_dilations[j][3] must be 0)");
  }
  if ((long long)c.initial_channel * 7 > (1 << 20)) return api_fail("ns_voc_create: initial_channel too large");
  if (voc_post_lds_bytes(c.initial_channel >> c.n_up, PRE_POST_K) > 65536) return api_fail("ns_voc_create: last channel count too large for conv_post");
  ns_vocoder* v = new ns_vocoder();
  v->cfg = c;
  const int C0 = c.initial_channel;
  expect(v, "conv_pre.weight", {C0, c.n_mel, PRE_POST_K});
  expect(v, "conv_pre.bias", {C0});
  v->pre.cin = c.n_mel; v->pre.cout = C0; v->pre.k = PRE_POST_K;
  v->pre.w = v->ar.take((size_t)C0 * c.n_mel * PRE_POST_K); v->pre.b = v->ar.take(C0);
  for (int i = 0; i < c.n_up; ++i) {
    const int cin = v->ch(i), cout = v->ch(i + 1), k = c.up_kernels[i], u = c.up_rates[i];
    const std::string p = "ups." + std::to_string(i);
    expect(v, p + ".weight", {cin, cout, k});
    expect(v, p + ".bias", {cout});
    Conv q; q.cin = cin; q.cout = cout; q.k = k;
    q.w = v->ar.take((size_t)u * cout * 2 * cin); q.b = v->ar.take(cout); q.wbf = v->take_bf16((size_t)u * cout * 2 * cin);
    v->ups.push_back(q);
    for (int j = 0; j < c.n_rb; ++j) {
      const int r = c.n_rb * i + j, kk = c.rb_kernels[j];
      for (int n = 0; n < N_DIL; ++n)
        for (int which = 1; which <= 2; ++which) {
          const std::string p2 = "resblocks." + std::to_string(r) + ".convs" + std::to_string(which) + "." + std::to_string(n);
          expect(v, p2 + ".weight", {cout, cout, kk});
          expect(v, p2 + ".bias", {cout});
          Conv w; w.cin = cout; w.cout = cout; w.k = kk; w.dil = which == 1 ? c.rb_dilations[j][n] : 1;
          w.w = v->ar.take((size_t)cout * cout * kk); w.b = v->ar.take(cout); w.wbf = v->take_bf16((size_t)cout * cout * kk);
          (which == 1 ? v->c1 : v->c2).push_back(w);
        }
    }
  }
  const int cl = v->ch(c.n_up);
  expect(v, "conv_post.weight", {1, cl, PRE_POST_K});
  expect(v, "conv_post.bias", {1});
  v->post.cin = cl; v->post.cout = 1; v->post.k = PRE_POST_K;
  v->post.w = v->ar.take((size_t)cl * PRE_POST_K); v->post.b = v->ar.take(1);
  *out = v;
  return 0;
}

extern "C" void ns_voc_destroy(ns_vocoder* v) { delete v; }
extern "C" size_t ns_voc_arena_bytes(const ns_vocoder* v) {
  return v ? v->ar.n * sizeof(float) + (v->matmul == 1 ? v->bf16_bytes : 0) : 0;
}

extern "C" int ns_voc_set_matmul(ns_vocoder* v, int mode) {
  if (!v) return api_fail("ns_voc_set_matmul: null vocoder");
  if (mode != 0 && mode != 1) return api_fail("ns_voc_set_matmul: mode must be 0 (fp32) or 1 (bf16), got " + std::to_string(mode));
  if (v->arena) return api_fail("ns_voc_set_matmul: the arena is already bound (call it between ns_voc_create and ns_voc_bind_arena)");
  v->matmul = mode;
  return 0;
}

extern "C" int ns_voc_bind_arena(ns_vocoder* v, void* dev, size_t bytes) { return bind_arena(v, dev, bytes, ns_voc_arena_bytes(v), "ns_voc_bind_arena"); }

extern "C" int ns_voc_check_weight(ns_vocoder* v, const char* name, const int64_t* shape, int ndim) {
  return check_weight(v, name, shape, ndim, "ns_voc_check_weight");
}

extern "C" int ns_voc_set_weight(ns_vocoder* v, const char* name, const float* host, const int64_t* shape, int ndim) {
  return set_weight(v, name, host, shape, ndim, "ns_voc_set_weight");
}

// ConvTranspose1d [cin][cout][2u] -> polyphase [u cout][2 cin]: row (r, co), tap 0 = x[q - 1] . W[:, co, r + u], tap 1 = x[q] . W[:, co, r]
static void pack_transposed(const std::vector<float>& w, int cin, int cout, int u, float* dst) {
  const int k = 2 * u;
  for (int r = 0; r < u; ++r)
    for (int co = 0; co < cout; ++co) {
      float* row = dst + ((size_t)r * cout + co) * 2 * cin;
      for (int c = 0; c < cin; ++c) {
        row[c] = w[((size_t)c * cout + co) * k + r + u];
        row[cin + c] = w[((size_t)c * cout + co) * k + r];
      }
    }
}

extern "C" int ns_voc_finalize_weights(ns_vocoder* v, void* stream) {
  if (!v) return api_fail("ns_voc_finalize_weights: null argument");
  if (!v->arena) return api_fail("ns_voc_finalize_weights: no arena bound (ns_voc_bind_arena)");
  const std::vector<std::string> missing = v->weights.missing();
  if (!missing.empty()) return api_fail("ns_voc_finalize_weights: missing key '" + missing[0] + "'");
  auto S = [&](const std::string& k) -> const std::vector<float>& { return v->weights.data(k); };
  std::vector<float> img(v->ar.n, 0.f);
  auto cp = [&](size_t off, const std::string& k) { const auto& d = S(k); std::copy(d.begin(), d.end(), img.begin() + off); };
  const ns_voc_config& c = v->cfg;
  pack_conv(S("conv_pre.weight"), v->pre.cout, v->pre.cin, PRE_POST_K, &img[v->pre.w]);
  cp(v->pre.b, "conv_pre.bias");
  for (int i = 0; i < c.n_up; ++i) {
    const Conv& q = v->ups[i];
    const std::string p = "ups." + std::to_string(i);
    pack_transposed(S(p + ".weight"), q.cin, q.cout, c.up_rates[i], &img[q.w]);
    cp(q.b, p + ".bias");
    for (int j = 0; j < c.n_rb; ++j)
      for (int n = 0; n < N_DIL; ++n) {
        const int r = c.n_rb * i + j, idx = r * N_DIL + n;
        for (int which = 1; which <= 2; ++which) {
          const Conv& w = (which == 1 ? v->c1 : v->c2)[idx];
          const std::string p2 = "resblocks." + std::to_string(r) + ".convs" + std::to_string(which) + "." + std::to_string(n);
          pack_conv(S(p2 + ".weight"), w.cout, w.cin, w.k, &img[w.w]);
          cp(w.b, p2 + ".bias");
        }
      }
  }
  pack_conv(S("conv_post.weight"), 1, v->post.cin, PRE_POST_K, &img[v->post.w]);  // [1][7][C]
  cp(v->post.b, "conv_post.bias");
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(hipMemcpyAsync(v->arena, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st));
  std::vector<unsigned short> bf;
  if (v->matmul == 1) {  // every GEMM weight rounded to bf16 (RNE) once, in its packed layout
    bf.assign(v->bf16_bytes / 2, 0);
    auto rnd = [&](const Conv& w, int rows, int taps, int cin) { round_weights_bf16(&img[w.w], rows, taps, cin, &bf[w.wbf / 2]); };
    for (int i = 0; i < c.n_up; ++i) {
      rnd(v->ups[i], c.up_rates[i] * v->ups[i].cout, 2, v->ups[i].cin);
      for (size_t idx = (size_t)c.n_rb * i * N_DIL; idx < (size_t)c.n_rb * (i + 1) * N_DIL; ++idx) {
        rnd(v->c1[idx], v->c1[idx].cout, v->c1[idx].k, v->c1[idx].cin);
        rnd(v->c2[idx], v->c2[idx].cout, v->c2[idx].k, v->c2[idx].cin);
      }
    }
    NS_HIP(hipMemcpyAsync((char*)v->arena + v->ar.n * sizeof(float), bf.data(), v->bf16_bytes, hipMemcpyHostToDevice, st));
  }
  NS_HIP(hipStreamSynchronize(st));  // img and bf are locals
  v->weights.release();
  v->ready = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------ launches
static const float* A(const ns_vocoder* v, size_t off) { return v->arena + off; }
// the bf16 plane of a GEMM weight in matmul mode 1, else nullptr (the fp32 kernel)
static const unsigned short* Abf(const ns_vocoder* v, const Conv& w) {
  return v->matmul == 1 ? (const unsigned short*)((const char*)v->arena + v->ar.n * sizeof(float) + w.wbf) : nullptr;
}
// every k_voc_gemm launch goes through here: the bf16 kernel when the weights have a bf16 plane
static hipError_t voc_gemm(const VocGemm& p, hipStream_t st) { return p.Wbf ? launch_voc_gemm_bf16(p, st) : launch_voc_gemm(p, st); }

// "same" Conv1d of the resblocks: [B, S, cin] -> [B, S, cout]
static VocGemm same_conv(const ns_vocoder* v, const Conv& w, const float* x, int B, int S, float* y) {
  VocGemm p{};
  p.X = x; p.W = A(v, w.w); p.Wbf = Abf(v, w); p.bias = A(v, w.b); p.R = nullptr; p.Y = y;
  p.B = B; p.S_in = S; p.Sg = S; p.Cin = w.cin; p.KW = w.k; p.dil = w.dil; p.off0 = -w.dil * (w.k - 1) / 2;
  p.N = w.cout; p.Cb = w.cout;
  p.out_ustride = (long long)S * w.cout; p.out_shift = 0;
  p.in_act = 1; p.in_slope = LRELU_SLOPE; p.out_act = 0; p.out_slope = LRELU_SLOPE;
  p.mrf = 0; p.mrf_div = 1.f;
  return p;
}

// one resblock launch in the form stage() gives it: same_conv() with the input / output leaky ReLU switches, the residual and the
// multi-receptive-field step (0 store, 1 y += v, 2 y = (y + v) / n_rb) set, nothing else
static VocGemm form_conv(const ns_vocoder* v, const Conv& w, const float* x, const float* resid, float* y, int B, int S, int in_act,
                         int out_act, int mrf) {
  VocGemm p = same_conv(v, w, x, B, S, y);
  p.in_act = in_act ? 1 : 0;
  p.out_act = out_act ? 1 : 0;
  p.R = resid;
  p.mrf = mrf;
  p.mrf_div = (float)v->cfg.n_rb;
  return p;
}

static int upsample(const ns_vocoder* v, int i, const float* x, int B, int S, float* y, hipStream_t st) {
  const Conv& w = v->ups[i];
  const int u = v->cfg.up_rates[i];
  VocGemm p{};
  p.X = x; p.W = A(v, w.w); p.Wbf = Abf(v, w); p.bias = A(v, w.b); p.R = nullptr; p.Y = y;
  p.B = B; p.S_in = S; p.Sg = S + 1; p.Cin = w.cin; p.KW = 2; p.dil = 1; p.off0 = -1;
  p.N = u * w.cout; p.Cb = w.cout;
  p.out_ustride = (long long)S * u * w.cout; p.out_shift = (long long)(u / 2) * w.cout;
  p.in_act = 1; p.in_slope = LRELU_SLOPE; p.out_act = 0; p.out_slope = LRELU_SLOPE;
  p.mrf = 0; p.mrf_div = 1.f;
  NS_HIP(voc_gemm(p, st));
  return 0;
}

// upsampler i + its resblocks: x [B, S, 2 ch] -> xs [B, S u, ch]; U, CUR, H: scratch of B S u ch floats each
static int stage(const ns_vocoder* v, int i, const float* x, int B, int S, float* xs, float* U, float* CUR, float* H, hipStream_t st) {
  const ns_voc_config& c = v->cfg;
  const int So = S * c.up_rates[i];
  NS_TRY(upsample(v, i, x, B, S, U, st));
  for (int j = 0; j < c.n_rb; ++j) {
    for (int n = 0; n < N_DIL; ++n) {
      const int idx = (c.n_rb * i + j) * N_DIL + n;
      const float* in = n == 0 ? U : CUR;
      NS_HIP(voc_gemm(form_conv(v, v->c1[idx], in, nullptr, H, B, So, 1, 1, 0), st));  // lrelu(c1(.), 0.1): c2's input
      int mrf = 0;
      if (n == N_DIL - 1 && c.n_rb > 1) mrf = j == 0 ? 0 : (j == c.n_rb - 1 ? 2 : 1);  // xs = rb0(x); xs += rb_j(x); x = xs / n_rb
      NS_HIP(voc_gemm(form_conv(v, v->c2[idx], H, in, n == N_DIL - 1 ? xs : CUR, B, So, 0, 0, mrf), st));
    }
  }
  return 0;
}

static size_t act_floats(const ns_vocoder* v, int T) {  // the largest activation of one utterance, in floats
  const ns_voc_config& c = v->cfg;
  size_t a = (size_t)T * (c.n_mel > c.initial_channel ? c.n_mel : c.initial_channel);
  size_t s = (size_t)T;
  for (int i = 0; i < c.n_up; ++i) {
    s *= (size_t)c.up_rates[i];
    const size_t ai = s * (size_t)v->ch(i + 1);
    if (ai > a) a = ai;
  }
  return a;
}

extern "C" size_t ns_voc_ws_bytes(const ns_vocoder* v, int B, int T) {
  if (!v || B <= 0 || T <= 0) return 0;
  return 4 * align64((size_t)B * act_floats(v, T)) * sizeof(float);
}

static int check_ready(const ns_vocoder* v, const char* who) {
  if (!v) return api_fail(std::string(who) + ": null vocoder");
  if (!v->ready || !v->arena) return api_fail(std::string(who) + ": weights not finalized (ns_voc_finalize_weights)");
  return 0;
}

static int conv_pre(const ns_vocoder* v, const float* mel_tm, int B, int T, float* y, hipStream_t st) {
  ConvGemm g{};
  g.X = mel_tm; g.ldx = v->cfg.n_mel;
  g.W = A(v, v->pre.w); g.ldw = 0; g.Wb3 = nullptr; g.Wbf = nullptr;
  g.bias = A(v, v->pre.b); g.resid = nullptr; g.ldr = 0;
  g.Y = y; g.ldy = v->pre.cout;
  g.M = B * T; g.N = v->pre.cout; g.Cin = v->pre.cin; g.KW = PRE_POST_K; g.pad = (PRE_POST_K - 1) / 2; g.S = T;
  g.m_base = 0; g.act = ACT_NONE; g.epi = EPI_NONE;
  NS_HIP(launch_conv_gemm(g, st));
  return 0;
}

extern "C" int ns_voc_forward(ns_vocoder* v, const float* mel, int mel_layout, int B, int T, float* wav, void* ws, size_t ws_bytes, void* stream) {
  NS_TRY(check_ready(v, "ns_voc_forward"));
  if (B < 0 || T < 0) return api_fail("ns_voc_forward: negative size");
  if (B == 0 || T == 0) return 0;
  if (!mel || !wav || !ws) return api_fail("ns_voc_forward: null argument");
  if (mel_layout != NS_VOC_MEL_CHANNEL_MAJOR && mel_layout != NS_VOC_MEL_TIME_MAJOR) return api_fail("ns_voc_forward: mel_layout must be 0 ([B, n_mel, T]) or 1 ([B, T, n_mel])");
  if ((long long)B * T * v->hop() * v->cfg.initial_channel > (1ll << 40)) return api_fail("ns_voc_forward: problem too large");
  if (ws_bytes < ns_voc_ws_bytes(v, B, T)) return api_fail("ns_voc_forward: workspace too small (ns_voc_ws_bytes)");
  if ((uintptr_t)ws & 255) return api_fail("ns_voc_forward: workspace must be 256-byte aligned");
  if (mel_layout == NS_VOC_MEL_TIME_MAJOR && ((uintptr_t)mel & 15)) return api_fail("ns_voc_forward: a time-major mel must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t buf = align64((size_t)B * act_floats(v, T));
  float* U = (float*)ws;
  float* XS = U + buf;
  float* CUR = XS + buf;
  float* H = CUR + buf;
  const float* mel_tm = mel;
  if (mel_layout == NS_VOC_MEL_CHANNEL_MAJOR) {
    NS_HIP(launch_voc_transpose(mel, U, B, v->cfg.n_mel, T, st));
    mel_tm = U;
  }
  NS_TRY(conv_pre(v, mel_tm, B, T, XS, st));
  int S = T;
  for (int i = 0; i < v->cfg.n_up; ++i) {
    // the upsampler reads XS into U, the resblocks then rebuild XS: the stage's input is dead once U is written
    NS_TRY(stage(v, i, XS, B, S, XS, U, CUR, H, st));
    S *= v->cfg.up_rates[i];
  }
  NS_HIP(launch_voc_post(XS, A(v, v->post.w), A(v, v->post.b), wav, B, S, v->post.cin, PRE_POST_K, POST_SLOPE, st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ per-operator entry points
// "resblocks.{r}.convs{1,2}.{n}" -> its conv, nullptr for any other name
static const Conv* resblock_conv(const ns_vocoder* v, const char* name) {
  int r = -1, which = 0, n = -1;
  char tail = 0;
  if (sscanf(name, "resblocks.%d.convs%d.%d%c", &r, &which, &n, &tail) != 3 || r < 0 || r >= v->cfg.n_up * v->cfg.n_rb ||
      (which != 1 && which != 2) || n < 0 || n >= N_DIL)
    return nullptr;
  return &(which == 1 ? v->c1 : v->c2)[r * N_DIL + n];
}

extern "C" int ns_voc_op_conv(ns_vocoder* v, const char* name_c, const float* x, int B, int S, float* out, void* stream) {
  NS_TRY(check_ready(v, "ns_voc_op_conv"));
  if (!name_c || !x || !out || B <= 0 || S <= 0) return api_fail("ns_voc_op_conv: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const std::string name(name_c);
  if (name == "conv_pre") return conv_pre(v, x, B, S, out, st);
  if (name == "conv_post") {
    NS_HIP(launch_voc_post(x, A(v, v->post.w), A(v, v->post.b), out, B, S, v->post.cin, PRE_POST_K, POST_SLOPE, st));
    return 0;
  }
  const Conv* w = resblock_conv(v, name_c);
  if (!w) return api_fail("ns_voc_op_conv: unknown module '" + name + "' (conv_pre, conv_post or resblocks.{r}.convs{1,2}.{n})");
  NS_HIP(voc_gemm(same_conv(v, *w, x, B, S, out), st));
  return 0;
}

extern "C" int ns_voc_op_conv_form(ns_vocoder* v, const char* name, const float* x, const float* resid, float* y, int B, int S, int in_act,
                                   int out_act, int mrf, void* stream) {
  // every argument is checked on the host before the handle's state: a refused call has made no HIP call
  if (!v) return api_fail("ns_voc_op_conv_form: null vocoder");
  if (!name || !x || !y || B <= 0 || S <= 0) return api_fail("ns_voc_op_conv_form: bad argument");
  const Conv* w = resblock_conv(v, name);
  if (!w) return api_fail("ns_voc_op_conv_form: unknown module '" + std::string(name) + "' (resblocks.{r}.convs{1,2}.{n})");
  if (mrf < 0 || mrf > 2) return api_fail("ns_voc_op_conv_form: mrf must be 0 (store), 1 (y += v) or 2 (y = (y + v) / n_rb), got " + std::to_string(mrf));
  if ((uintptr_t)x & 15) return api_fail("ns_voc_op_conv_form: x must be 16-byte aligned");
  NS_TRY(check_ready(v, "ns_voc_op_conv_form"));
  NS_HIP(voc_gemm(form_conv(v, *w, x, resid, y, B, S, in_act, out_act, mrf), (hipStream_t)stream));
  return 0;
}

extern "C" int ns_voc_op_upsample(ns_vocoder* v, int i, const float* x, int B, int S, float* out, void* stream) {
  NS_TRY(check_ready(v, "ns_voc_op_upsample"));
  if (i < 0 || i >= v->cfg.n_up || !x || !out || B <= 0 || S <= 0) return api_fail("ns_voc_op_upsample: bad argument");
  return upsample(v, i, x, B, S, out, (hipStream_t)stream);
}

extern "C" size_t ns_voc_op_stage_ws_bytes(const ns_vocoder* v, int i, int B, int S) {
  if (!v || i < 0 || i >= v->cfg.n_up || B <= 0 || S <= 0) return 0;
  return 3 * align64((size_t)B * S * v->cfg.up_rates[i] * v->ch(i + 1)) * sizeof(float);
}

extern "C" int ns_voc_op_stage(ns_vocoder* v, int i, const float* x, int B, int S, float* out, void* ws, size_t ws_bytes, void* stream) {
  NS_TRY(check_ready(v, "ns_voc_op_stage"));
  if (i < 0 || i >= v->cfg.n_up || !x || !out || !ws || B <= 0 || S <= 0) return api_fail("ns_voc_op_stage: bad argument");
  if (ws_bytes < ns_voc_op_stage_ws_bytes(v, i, B, S)) return api_fail("ns_voc_op_stage: workspace too small (ns_voc_op_stage_ws_bytes)");
  if ((uintptr_t)ws & 255) return api_fail("ns_voc_op_stage: workspace must be 256-byte aligned");
  const size_t buf = align64((size_t)B * S * v->cfg.up_rates[i] * v->ch(i + 1));
  float* U = (float*)ws;
  return stage(v, i, x, B, S, out, U, U + buf, U + 2 * buf, (hipStream_t)stream);
}
