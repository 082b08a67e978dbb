// C-ABI of the PostNet training forward and backward (include/nar_fs2.h ns_pn_*; transformer/Layers.py:107-177).  No handle: the
// weights and the BatchNorm buffers are the caller's live tensors in checkpoint layout, the workspace and the saved activations belong
// to the caller.  Host-side only; every argument is validated before the first HIP call.  The GEMMs are the existing ones: the
// Conv1D-as-GEMM dispatch (forward, data gradient), the predictor's weight gradient and its pack kernel, reached through train_api.h.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

static_assert(sizeof(ns_pn_shape) == 24, "ns_pn_shape layout");
static_assert(sizeof(ns_pn_layer) == 7 * sizeof(void*) && sizeof(ns_pn_weights) == 35 * sizeof(void*), "ns_pn_weights layout");
static_assert(sizeof(ns_pn_grads) == 21 * sizeof(void*), "ns_pn_grads layout");
static_assert(NS_PN_MAX_LAYERS == PN_MAX_LAYERS, "layer count");

namespace {
thread_local int t_launches = 0;
thread_local const Counted counted{"ns_pn", &t_launches};

struct Ws {  // the workspace of one shape, carved in this order
  float* wp[PN_MAX_LAYERS];       // packed weights, the forward's form
  float* wt[PN_MAX_LAYERS];       // packed weights, the data gradient's form
  float* partial;                 // the weight gradient's per-range tiles (the largest of the layers')
  float* dwpad;                   // [128][emb][K]: the last layer's weight gradient at the padded width
  double* colpart;                // [row blocks][2][emb]
  double* biaspart[PN_MAX_LAYERS];  // [row blocks][C_{i+1}]
  double* means;                  // [2][emb]
  double* stats;                  // [n][2][emb]: mu | rstd of a forward that saves nothing
  float *a, *b;                   // [M, emb] each: u / h of a forward that saves nothing, dz / dh of the backward
};

inline int cin_of(const ns_pn_shape& s, int i) { return i == 0 ? s.n_mel : s.emb; }
inline int cout_of(const ns_pn_shape& s, int i) { return i == s.n - 1 ? s.n_mel : s.emb; }
// the width of the weight gradient's GEMM of layer i: the last layer's n_mel is padded to the narrowest width the plan takes
inline int wgrad_n(const ns_pn_shape& s, int i) { return i == s.n - 1 ? PN_PAD_N : s.emb; }

int check_dims(const ns_pn_shape& s, const std::string& w) {
  if (s.B <= 0 || s.T <= 0) return api_fail(w + "B and T must be positive, got " + std::to_string(s.B) + " x " + std::to_string(s.T));
  if (s.emb != 256 && s.emb != 512) return api_fail(w + "emb must be 256 or 512, got " + std::to_string(s.emb));
  if (s.n_mel < 16 || s.n_mel > 128 || s.n_mel % 16 != 0) return api_fail(w + "n_mel must be a multiple of 16 in [16, 128], got " + std::to_string(s.n_mel));
  if (s.K <= 0 || s.K % 2 == 0 || s.K > 9) return api_fail(w + "K must be odd and at most 9, got " + std::to_string(s.K));
  if (s.n < 2 || s.n > PN_MAX_LAYERS) return api_fail(w + "n must lie in [2, 5], got " + std::to_string(s.n));
  if ((long long)s.B * s.T * s.emb >= (1ll << 31)) return api_fail(w + "problem too large: B * T * emb must stay below 2^31");
  return 0;
}

int carve(const ns_pn_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int M = s.B * s.T, nblk = pn_row_blocks(M);
  Bump bump(base);
  long long pmax = 0;
  int rec[2][8];
  for (int i = 0; i < s.n; ++i) {
    const int ci = cin_of(s, i), co = cout_of(s, i);
    if (conv_gemm_describe(M, co, ci, s.K, 0, rec) <= 0 || conv_gemm_describe(M, ci, co, s.K, 0, rec) <= 0)
      return api_fail(w + "the Conv1D-as-GEMM dispatch refuses layer " + std::to_string(i) + " of this shape");
    PgWgradPlan pl;
    if (!pg_plan_wgrad(M, wgrad_n(s, i), ci, s.K, &pl)) return api_fail(w + "the weight gradient's plan refuses layer " + std::to_string(i) + " of this shape");
    pmax = pl.ws_floats > pmax ? pl.ws_floats : pmax;
  }
  for (int i = 0; i < s.n; ++i) ws->wp[i] = bump.f((size_t)cout_of(s, i) * s.K * cin_of(s, i));
  for (int i = 0; i < s.n; ++i) ws->wt[i] = bump.f((size_t)cout_of(s, i) * s.K * cin_of(s, i));
  ws->partial = bump.f((size_t)pmax);
  ws->dwpad = bump.f((size_t)PN_PAD_N * s.emb * s.K);
  ws->colpart = (double*)bump.raw((size_t)nblk * 2 * s.emb * sizeof(double));
  for (int i = 0; i < s.n; ++i) ws->biaspart[i] = (double*)bump.raw((size_t)nblk * cout_of(s, i) * sizeof(double));
  ws->means = (double*)bump.raw((size_t)2 * s.emb * sizeof(double));
  ws->stats = (double*)bump.raw((size_t)s.n * 2 * s.emb * sizeof(double));
  ws->a = bump.f((size_t)M * s.emb);
  ws->b = bump.f((size_t)M * s.emb);
  *bytes = bump.off;
  return 0;
}

size_t saved_floats(const ns_pn_shape& s) { return (size_t)s.B * s.T * ((size_t)2 * (s.n - 1) * s.emb + s.n_mel); }

// u_i, h_i (null for the last layer) and the statistics of layer i inside `saved`
struct Saved { float* u[PN_MAX_LAYERS]; float* h[PN_MAX_LAYERS]; double* stats[PN_MAX_LAYERS]; };
Saved saved_pointers(const ns_pn_shape& s, void* saved) {
  Saved v;
  const size_t M = (size_t)s.B * s.T;
  float* p = (float*)saved;
  for (int i = 0; i < s.n; ++i) {
    v.u[i] = p; p += M * cout_of(s, i);
    v.h[i] = nullptr;
    if (i < s.n - 1) { v.h[i] = p; p += M * s.emb; }
  }
  double* d = (double*)p;  // (a multiple of 16 bytes in: every block above is M * C floats, C a multiple of 16)
  for (int i = 0; i < s.n; ++i) v.stats[i] = d + (size_t)i * 2 * s.emb;
  return v;
}

// what ns_pn_forward and ns_pn_backward check alike, in this order; `io` names y or g
int common(const std::string& w, const ns_pn_shape* s, const ns_pn_weights* k, int training, const float* x, const uint8_t* const* keep, float p_drop,
           const void* saved, const void* ws_mem, NamedPtr io) {
  NS_TRY(check_dims(*s, w));
  if (training && (long long)s->B * s->T == 1) return api_fail(w + "training needs more than one row: the batch variance of B * T == 1 value per channel is undefined");
  for (int i = 0; i < s->n; ++i) {
    const ns_pn_layer& l = k->layer[i];
    NS_TRY(check_weights({{"w", l.w}, {"b", l.b}, {"gamma", l.gamma}, {"beta", l.beta}, {"running_mean", l.running_mean},
                          {"running_var", l.running_var}, {"num_batches_tracked", l.num_batches_tracked, 8}},
                         w, "layer[" + std::to_string(i) + "]."));
  }
  NS_TRY(check_drop(keep, s->n, p_drop, w));
  return check_aligned(w, {{"x", x}, {"saved", saved}, {"the workspace", ws_mem}, io});
}

int check_op(const std::string& w, int M, int C, float p_drop, const uint8_t* keep, std::initializer_list<NamedPtr> al) {
  if (M <= 0) return api_fail(w + "M must be positive, got " + std::to_string(M));
  if (C <= 0 || C % 16 != 0 || C > 512) return api_fail(w + "C must be a multiple of 16 up to 512, got " + std::to_string(C));
  if ((long long)M * C >= (1ll << 31)) return api_fail(w + "problem too large: M * C must stay below 2^31");
  NS_TRY(check_drop({keep}, p_drop, w));
  return check_aligned(w, al);
}
}  // namespace

extern "C" int ns_pn_abi_version(void) { return NS_PN_ABI_VERSION; }
extern "C" int ns_pn_last_launches(void) { return t_launches; }

extern "C" size_t ns_pn_ws_bytes(const ns_pn_shape* s) {
  return size_query("ns_pn_ws_bytes", s, check_dims, [](const ns_pn_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" size_t ns_pn_saved_bytes(const ns_pn_shape* s) {
  return size_query("ns_pn_saved_bytes", s, check_dims, [](const ns_pn_shape& s, const std::string&) {
    return saved_floats(s) * sizeof(float) + (size_t)s.n * 2 * s.emb * sizeof(double);
  });
}

extern "C" int ns_pn_forward(const ns_pn_shape* s, const ns_pn_weights* k, int training, const float* x, const uint8_t* const* keep, float p_drop,
                             float* y, void* saved, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_pn_forward: ";
  t_launches = 0;
  if (!s || !k || !x || !y || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(common(w, s, k, training, x, keep, p_drop, saved, ws_mem, {"y", y}));
  Ws ws;
  NS_TRY(carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, &ws, w));
  const int M = s->B * s->T, K = s->K, n = s->n, pad = (K - 1) / 2, nblk = pn_row_blocks(M);
  const float scale = 1.f / (1.f - p_drop);
  hipStream_t st = (hipStream_t)stream;
  Saved sv;
  if (saved) sv = saved_pointers(*s, saved);
  PgPack packs[PN_MAX_LAYERS];
  for (int i = 0; i < n; ++i) packs[i] = PgPack{k->layer[i].w, ws.wp[i], nullptr, cout_of(*s, i), cin_of(*s, i), K};
  NS_TRY(counted.pack(packs, n, st));
  const float* h_in = x;
  for (int i = 0; i < n; ++i) {
    const ns_pn_layer& l = k->layer[i];
    const int ci = cin_of(*s, i), co = cout_of(*s, i), last = i == n - 1;
    float* u = saved ? sv.u[i] : ws.a;
    float* h = last ? y : (saved ? sv.h[i] : ws.b);
    double* stats = saved ? sv.stats[i] : ws.stats + (size_t)i * 2 * s->emb;
    NS_TRY(counted.conv(h_in, ci, ws.wp[i], l.b, nullptr, u, M, s->T, co, ci, K, pad, ACT_NONE, st));
    PnFinish fin;
    memset(&fin, 0, sizeof(fin));
    fin.mode = training ? PN_FIN_TRAIN : PN_FIN_EVAL; fin.nblk = nblk; fin.C = co; fin.M = M; fin.part = ws.colpart; fin.stats = stats;
    fin.running_mean = l.running_mean; fin.running_var = l.running_var; fin.num_batches_tracked = (long long*)l.num_batches_tracked;
    if (training) {
      NS_HIP(launch_pn_stats(u, M, co, ws.colpart, st));
      ++t_launches;
    }
    NS_HIP(launch_pn_finish(fin, st));
    ++t_launches;
    NS_HIP(launch_pn_apply(u, stats, l.gamma, l.beta, keep ? keep[i] : nullptr, scale, last, M, co, h, st));
    ++t_launches;
    h_in = h;
  }
  return 0;
}

extern "C" int ns_pn_backward(const ns_pn_shape* s, const ns_pn_weights* k, int training, const float* x, const uint8_t* const* keep, float p_drop,
                              const void* saved, const float* g, const ns_pn_grads* d, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_pn_backward: ";
  t_launches = 0;
  if (!s || !k || !x || !saved || !g || !d || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(common(w, s, k, training, x, keep, p_drop, saved, ws_mem, {"g", g}));
  const int n = s->n;
  std::vector<NamedPtr> outs = {{"dx", d->dx}};
  for (int i = 0; i < n; ++i) {
    const ns_pn_layer_grads& gl = d->layer[i];
    outs.push_back({"w", gl.w}); outs.push_back({"b", gl.b}); outs.push_back({"gamma", gl.gamma}); outs.push_back({"beta", gl.beta});
  }
  NS_TRY(check_grads(outs, w));
  Ws ws;
  NS_TRY(carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, &ws, w));
  const int M = s->B * s->T, K = s->K, padT = K - 1 - (K - 1) / 2, nblk = pn_row_blocks(M);
  const float scale = 1.f / (1.f - p_drop);
  hipStream_t st = (hipStream_t)stream;
  const Saved sv = saved_pointers(*s, const_cast<void*>(saved));

  int lo = n;  // the lowest layer anything is wanted from
  if (d->dx) lo = 0;
  for (int i = 0; i < lo; ++i)
    if (d->layer[i].w || d->layer[i].b || d->layer[i].gamma || d->layer[i].beta) lo = i;
  if (lo == n) return 0;
  auto dgrad_wanted = [&](int i) { return i > lo || (i == 0 && d->dx != nullptr); };

  PgPack packs[PN_MAX_LAYERS];
  int npack = 0;
  for (int i = 0; i < n; ++i)
    if (dgrad_wanted(i)) packs[npack++] = PgPack{k->layer[i].w, nullptr, ws.wt[i], cout_of(*s, i), cin_of(*s, i), K};
  NS_TRY(counted.pack(packs, npack, st));

  PnBiasFinish bias;
  memset(&bias, 0, sizeof(bias));
  bias.nblk = nblk;
  const float* dh = g;
  for (int i = n - 1; i >= lo; --i) {
    const ns_pn_layer& l = k->layer[i];
    const ns_pn_layer_grads& gl = d->layer[i];
    const int ci = cin_of(*s, i), co = cout_of(*s, i), last = i == n - 1;
    const float* h_in = i == 0 ? x : sv.h[i - 1];
    PnBackward a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.C = co; a.ldz = last ? PN_PAD_N : co; a.last = last; a.scale = scale;
    a.dh = dh; a.u = sv.u[i]; a.h = sv.h[i]; a.gamma = l.gamma; a.stats = sv.stats[i]; a.keep = keep ? keep[i] : nullptr;
    a.part = ws.colpart; a.dz = ws.a;
    if (training || gl.gamma || gl.beta) {
      NS_HIP(launch_pn_bwd_reduce(a, st));
      PnFinish fin;
      memset(&fin, 0, sizeof(fin));
      fin.mode = PN_FIN_BWD; fin.nblk = nblk; fin.C = co; fin.M = M; fin.part = ws.colpart; fin.stats = training ? ws.means : nullptr;
      fin.out0 = gl.beta; fin.out1 = gl.gamma;
      NS_HIP(launch_pn_finish(fin, st));
      t_launches += 2;
    }
    if (!(gl.w || gl.b || dgrad_wanted(i))) continue;  // (only gamma / beta of the lowest layer: no dz)
    a.means = training ? ws.means : nullptr;
    if (gl.b) { a.bias_part = ws.biaspart[i]; bias.part[i] = ws.biaspart[i]; bias.out[i] = gl.b; bias.C[i] = co; }
    NS_HIP(launch_pn_bwd_apply(a, st));
    ++t_launches;
    if (gl.w) {
      if (last) {
        NS_TRY(counted.wgrad_narrow(ws.a, h_in, M, s->T, co, ci, K, ws.partial, ws.dwpad, gl.w, st));
      } else {
        PgWgradPlan pl;
        pg_plan_wgrad(M, co, ci, K, &pl);  // (accepted by carve above)
        NS_HIP(launch_pg_wgrad(ws.a, h_in, M, s->T, co, ci, K, pl, ws.partial, gl.w, st));
        t_launches += 2;
      }
    }
    if (dgrad_wanted(i)) {
      NS_TRY(counted.conv(ws.a, a.ldz, ws.wt[i], nullptr, nullptr, i == 0 ? d->dx : ws.b, M, s->T, ci, co, K, padT, ACT_NONE, st));
      dh = ws.b;
    }
  }
  bool any_bias = false;
  for (int i = 0; i < n; ++i) any_bias = any_bias || bias.out[i];
  if (any_bias) {
    NS_HIP(launch_pn_bias_finish(bias, st));
    ++t_launches;
  }
  return 0;
}

extern "C" int ns_pn_op_stats(const float* u, int M, int C, int training, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                              double* stats, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_pn_op_stats: ";
  t_launches = 0;
  if (!stats || (training ? (!u || !ws_mem) : (!running_mean || !running_var))) return api_fail(w + "null argument");
  const bool buffers = running_mean || running_var || num_batches_tracked;
  if (training && buffers && !(running_mean && running_var && num_batches_tracked)) return api_fail(w + "the three buffers come together or not at all");
  NS_TRY(check_op(w, M, C, 0.f, nullptr, {{"u", u}, {"running_mean", running_mean}, {"running_var", running_var}, {"stats", stats}, {"the workspace", ws_mem},
                                           {"num_batches_tracked", num_batches_tracked, 8}}));
  if (training && M == 1) return api_fail(w + "training needs more than one row");
  const size_t need = (size_t)pn_row_blocks(M) * 2 * C * sizeof(double);
  if (training && ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  PnFinish fin;
  memset(&fin, 0, sizeof(fin));
  fin.mode = training ? PN_FIN_TRAIN : PN_FIN_EVAL; fin.nblk = pn_row_blocks(M); fin.C = C; fin.M = M; fin.part = (const double*)ws_mem; fin.stats = stats;
  fin.running_mean = running_mean; fin.running_var = running_var; fin.num_batches_tracked = (long long*)num_batches_tracked;
  if (training) {
    NS_HIP(launch_pn_stats(u, M, C, (double*)ws_mem, st));
    ++t_launches;
  }
  NS_HIP(launch_pn_finish(fin, st));
  ++t_launches;
  return 0;
}

extern "C" int ns_pn_op_apply(const float* u, const double* stats, const float* gamma, const float* beta, const uint8_t* keep, float p_drop, int last,
                              int M, int C, float* h, void* stream) {
  const std::string w = "ns_pn_op_apply: ";
  t_launches = 0;
  if (!u || !stats || !gamma || !beta || !h) return api_fail(w + "null argument");
  NS_TRY(check_op(w, M, C, p_drop, keep, {{"u", u}, {"stats", stats}, {"gamma", gamma}, {"beta", beta}, {"h", h}}));
  NS_HIP(launch_pn_apply(u, stats, gamma, beta, keep, 1.f / (1.f - p_drop), last != 0, M, C, h, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_pn_op_bwd_reduce(const float* dh, const float* u, const float* h, const double* stats, const uint8_t* keep, float p_drop, int last,
                                   int M, int C, float* d_gamma, float* d_beta, double* means, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_pn_op_bwd_reduce: ";
  t_launches = 0;
  if (!dh || !u || (!last && !h) || !stats || !d_gamma || !d_beta || !means || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_op(w, M, C, p_drop, keep, {{"dh", dh}, {"u", u}, {"h", h}, {"stats", stats}, {"d_gamma", d_gamma}, {"d_beta", d_beta}, {"means", means},
                                              {"the workspace", ws_mem}}));
  const size_t need = (size_t)pn_row_blocks(M) * 2 * C * sizeof(double);
  if (ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  PnBackward a;
  memset(&a, 0, sizeof(a));
  a.M = M; a.C = C; a.ldz = C; a.last = last != 0; a.scale = 1.f / (1.f - p_drop);
  a.dh = dh; a.u = u; a.h = h; a.stats = stats; a.keep = keep; a.part = (double*)ws_mem;
  NS_HIP(launch_pn_bwd_reduce(a, st));
  PnFinish fin;
  memset(&fin, 0, sizeof(fin));
  fin.mode = PN_FIN_BWD; fin.nblk = pn_row_blocks(M); fin.C = C; fin.M = M; fin.part = a.part; fin.stats = means; fin.out0 = d_beta; fin.out1 = d_gamma;
  NS_HIP(launch_pn_finish(fin, st));
  t_launches += 2;
  return 0;
}

extern "C" int ns_pn_op_bwd_apply(const float* dh, const float* u, const float* h, const double* stats, const double* means, const float* gamma,
                                  const uint8_t* keep, float p_drop, int last, int M, int C, int ldz, float* dz, float* d_bias, void* ws_mem,
                                  size_t ws_bytes, void* stream) {
  const std::string w = "ns_pn_op_bwd_apply: ";
  t_launches = 0;
  if (!dh || !u || (!last && !h) || !stats || !gamma || !dz || (d_bias && !ws_mem)) return api_fail(w + "null argument");
  NS_TRY(check_op(w, M, C, p_drop, keep, {{"dh", dh}, {"u", u}, {"h", h}, {"stats", stats}, {"means", means}, {"gamma", gamma}, {"dz", dz},
                                              {"d_bias", d_bias}, {"the workspace", ws_mem}}));
  if (ldz != C && !(ldz == PN_PAD_N && C < PN_PAD_N)) return api_fail(w + "ldz must be C, or 128 for C below 128, got " + std::to_string(ldz));
  const size_t need = (size_t)pn_row_blocks(M) * C * sizeof(double);
  if (d_bias && ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  PnBackward a;
  memset(&a, 0, sizeof(a));
  a.M = M; a.C = C; a.ldz = ldz; a.last = last != 0; a.scale = 1.f / (1.f - p_drop);
  a.dh = dh; a.u = u; a.h = h; a.gamma = gamma; a.stats = stats; a.means = means; a.keep = keep; a.dz = dz;
  a.bias_part = d_bias ? (double*)ws_mem : nullptr;
  NS_HIP(launch_pn_bwd_apply(a, st));
  ++t_launches;
  if (d_bias) {
    PnBiasFinish bias;
    memset(&bias, 0, sizeof(bias));
    bias.nblk = pn_row_blocks(M); bias.part[0] = a.bias_part; bias.out[0] = d_bias; bias.C[0] = C;
    NS_HIP(launch_pn_bias_finish(bias, st));
    ++t_launches;
  }
  return 0;
}

extern "C" int ns_pn_op_wgrad_narrow(const float* dz, const float* X, int B, int S, int N, int Cin, int KW, float* dW, void* ws_mem, size_t ws_bytes,
                                     void* stream) {
  const std::string w = "ns_pn_op_wgrad_narrow: ";
  t_launches = 0;
  if (!dz || !X || !dW || !ws_mem) return api_fail(w + "null argument");
  if (B <= 0 || S <= 0) return api_fail(w + "B and S must be positive, got " + std::to_string(B) + " x " + std::to_string(S));
  if (N < 16 || N >= PN_PAD_N || N % 16 != 0) return api_fail(w + "N must be a multiple of 16 below 128, got " + std::to_string(N));
  if (Cin <= 0 || Cin % 4 != 0) return api_fail(w + "Cin must be a multiple of 4, got " + std::to_string(Cin));
  if (KW <= 0 || KW % 2 == 0) return api_fail(w + "K must be odd, got " + std::to_string(KW));
  NS_TRY(check_aligned(w, {{"dz", dz}, {"X", X}, {"dW", dW}, {"the workspace", ws_mem}}));
  if ((long long)B * S >= (1ll << 31)) return api_fail(w + "problem too large for the weight gradient's split");
  const int M = B * S;
  PgWgradPlan pl;
  if (!pg_plan_wgrad(M, PN_PAD_N, Cin, KW, &pl)) return api_fail(w + "problem too large for the weight gradient's split");
  Bump bump(ws_mem);
  float* partial = bump.f((size_t)pl.ws_floats);
  float* dwpad = bump.f((size_t)PN_PAD_N * Cin * KW);
  if (ws_bytes < bump.off) return api_fail(w + "workspace too small: " + std::to_string(bump.off) + " bytes needed");
  return counted.wgrad_narrow(dz, X, M, S, N, Cin, KW, partial, dwpad, dW, (hipStream_t)stream);
}
