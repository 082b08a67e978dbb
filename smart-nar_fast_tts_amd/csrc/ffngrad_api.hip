// C-ABI of the PositionwiseFeedForward training forward and backward (include/nar_fs2.h ns_fg_*; transformer/SubLayers.py:62-95).
// No handle: the weights are the caller's live tensors in checkpoint layout, the workspace and the saved activations belong to the
// caller.  Host-side only; every argument is validated before the first HIP call.  Every launch but the ReLU gate (ffngrad.hip) is a
// kernel the other training ABIs already run: the Conv1D-as-GEMM dispatch (forward, data gradients), the predictor's weight gradient
// and its pack kernel, the attention's LayerNorm + residual + dropout row forward and backward, the column-partial finish.  The launch
// counts are stated in the header.
#include "../../include/nar_fs2.h"
#include "ffngrad_api.h"

using namespace ns;
using namespace ns::fg;

static_assert(sizeof(ns_fg_shape) == 24, "ns_fg_shape layout");
static_assert(sizeof(ns_fg_weights) == 6 * sizeof(void*) && sizeof(ns_fg_grads) == 7 * sizeof(void*), "ns_fg_weights / ns_fg_grads layout");

namespace {
thread_local int t_launches = 0;
thread_local const Counted counted{"ns_fg", &t_launches};

struct Ws {  // the workspace of one shape, carved in this order
  float *wp1, *wp2;   // [d_inner][K1 d] and [d][K2 d_inner]: the forward's form
  float *wt1, *wt2;   // [d][K1 d_inner] and [d_inner][K2 d]: the data gradients' form (transposed, taps flipped)
  float* partial;     // the weight gradients' per-range tiles (the larger of the two)
  double* colpart;    // [row blocks][PG_SLOTS][d]: d_ln_g, d_ln_b, d_b2
  double* gatepart;   // [row blocks][PG_SLOTS][d_inner]: d_b1 in slot 0
  float *a, *b;       // [M, d] each: u (forward); dz, du (backward)
  float* wide;        // [M, d_inner]: da, then dh in place (backward); h of a forward that saves nothing
};
}  // namespace

// what the "bf16" matmul mode's entry points (ffngrad_bf16_api.hip) share with these: ffngrad_api.h
int* ns::fg::launches() { return &t_launches; }

int ns::fg::check_dims(const ns_fg_shape& s, const std::string& w) {
  if (s.B <= 0 || s.S <= 0) return api_fail(w + "B and S must be positive, got " + std::to_string(s.B) + " x " + std::to_string(s.S));
  if (s.d != 256 && s.d != 512) return api_fail(w + "d must be 256 or 512, got " + std::to_string(s.d));
  if (s.d_inner <= 0 || s.d_inner % 256 != 0) return api_fail(w + "d_inner must be a positive multiple of 256, got " + std::to_string(s.d_inner));
  if (s.K1 <= 0 || s.K1 % 2 == 0) return api_fail(w + "K1 must be odd and positive, got " + std::to_string(s.K1));
  if (s.K2 <= 0 || s.K2 % 2 == 0) return api_fail(w + "K2 must be odd and positive, got " + std::to_string(s.K2));
  if ((long long)s.B * s.S * s.d_inner >= (1ll << 31)) return api_fail(w + "problem too large: B * S * d_inner must stay below 2^31");
  return 0;
}

std::vector<NamedPtr> ns::fg::params(const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_g, const float* ln_b) {
  return {{"w1", w1}, {"b1", b1}, {"w2", w2}, {"b2", b2}, {"ln_g", ln_g}, {"ln_b", ln_b}};
}

// the gate and, where d_b1 is wanted, the fixed-order sum of its partials: one or two launches
int ns::fg::relu_gate(const float* da, const float* h, int M, int di, float* dh, float* d_b1, double* part, hipStream_t st) {
  NS_HIP(launch_fg_relu_gate(da, h, M, di, dh, d_b1 ? part : nullptr, st));
  ++t_launches;
  return counted.col_finish(part, pg_row_blocks(M), di, {d_b1}, {}, st);
}

namespace {
int carve(const ns_fg_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int M = s.B * s.S, d = s.d, di = s.d_inner, nblk = pg_row_blocks(M);
  int rec[2][8];
  if (conv_gemm_describe(M, di, d, s.K1, 0, rec) <= 0 || conv_gemm_describe(M, d, di, s.K2, 0, rec) <= 0 ||
      conv_gemm_describe(M, di, d, s.K2, 0, rec) <= 0 || conv_gemm_describe(M, d, di, s.K1, 0, rec) <= 0)
    return api_fail(w + "the Conv1D-as-GEMM dispatch refuses this shape");
  PgWgradPlan pl1, pl2;
  if (!pg_plan_wgrad(M, di, d, s.K1, &pl1) || !pg_plan_wgrad(M, d, di, s.K2, &pl2)) return api_fail(w + "the weight gradient's plan refuses this shape");
  Bump bump(base);
  const size_t n1 = (size_t)di * s.K1 * d, n2 = (size_t)d * s.K2 * di;
  ws->wp1 = bump.f(n1); ws->wp2 = bump.f(n2); ws->wt1 = bump.f(n1); ws->wt2 = bump.f(n2);
  ws->partial = bump.f((size_t)(pl1.ws_floats > pl2.ws_floats ? pl1.ws_floats : pl2.ws_floats));
  ws->colpart = (double*)bump.raw((size_t)nblk * PG_SLOTS * d * sizeof(double));
  ws->gatepart = (double*)bump.raw((size_t)nblk * PG_SLOTS * di * sizeof(double));
  ws->a = bump.f((size_t)M * d); ws->b = bump.f((size_t)M * d);
  ws->wide = bump.f((size_t)M * di);
  *bytes = bump.off;
  return 0;
}

// what ns_fg_forward and ns_fg_backward check alike, in this order, and the carved workspace
int common(const std::string& w, const ns_fg_shape* s, const ns_fg_weights* k, const float* x, const uint8_t* keep, float p_drop, const void* saved,
           void* ws_mem, size_t ws_bytes, NamedPtr io, Ws* ws) {
  NS_TRY(check_dims(*s, w));
  NS_TRY(check_weights(params(k->w1, k->b1, k->w2, k->b2, k->ln_g, k->ln_b), w));
  NS_TRY(check_drop({keep}, p_drop, w));
  NS_TRY(check_aligned(w, {{"x", x}, {"saved", saved}, {"the workspace", ws_mem}, io}));
  return carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, ws, w);
}
}  // namespace

extern "C" int ns_fg_abi_version(void) { return NS_FG_ABI_VERSION; }
extern "C" int ns_fg_last_launches(void) { return t_launches; }

extern "C" size_t ns_fg_ws_bytes(const ns_fg_shape* s) {
  return size_query("ns_fg_ws_bytes", s, check_dims, [](const ns_fg_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" size_t ns_fg_saved_bytes(const ns_fg_shape* s) {
  return size_query("ns_fg_saved_bytes", s, check_dims, [](const ns_fg_shape& s, const std::string& w) {
    return carved_bytes(carve, s, w) ? (size_t)s.B * s.S * ((size_t)s.d_inner + s.d) * sizeof(float) : (size_t)0;
  });
}

extern "C" int ns_fg_forward(const ns_fg_shape* s, const ns_fg_weights* k, const float* x, const uint8_t* keep, float p_drop, float* y, void* saved,
                             void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_fg_forward: ";
  t_launches = 0;
  if (!s || !k || !x || !y || !ws_mem) return api_fail(w + "null argument");
  Ws ws;
  NS_TRY(common(w, s, k, x, keep, p_drop, saved, ws_mem, ws_bytes, {"y", y}, &ws));
  const int M = s->B * s->S, d = s->d, di = s->d_inner;
  float* h = saved ? (float*)saved : ws.wide;
  float* z = saved ? h + (size_t)M * di : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const PgPack packs[2] = {{k->w1, ws.wp1, nullptr, di, d, s->K1}, {k->w2, ws.wp2, nullptr, d, di, s->K2}};
  NS_TRY(counted.pack(packs, 2, st));
  NS_TRY(counted.conv(x, d, ws.wp1, k->b1, nullptr, h, M, s->S, di, d, s->K1, (s->K1 - 1) / 2, ACT_RELU, st));
  NS_TRY(counted.conv(h, di, ws.wp2, k->b2, nullptr, ws.a, M, s->S, d, di, s->K2, (s->K2 - 1) / 2, ACT_NONE, st));
  NS_HIP(launch_ag_row_forward(ws.a, x, keep, 1.f / (1.f - p_drop), k->ln_g, k->ln_b, z, y, M, d, st));
  ++t_launches;
  return 0;
}

extern "C" int ns_fg_backward(const ns_fg_shape* s, const ns_fg_weights* k, const float* x, const uint8_t* keep, float p_drop, const void* saved,
                              const float* g, const ns_fg_grads* dg, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_fg_backward: ";
  t_launches = 0;
  if (!s || !k || !x || !saved || !g || !dg || !ws_mem) return api_fail(w + "null argument");
  std::vector<NamedPtr> outs = params(dg->w1, dg->b1, dg->w2, dg->b2, dg->ln_g, dg->ln_b);
  outs.push_back({"dx", dg->dx});
  bool any = false;
  NS_TRY(check_grads(outs, w, &any));
  Ws ws;
  NS_TRY(common(w, s, k, x, keep, p_drop, saved, ws_mem, ws_bytes, {"g", g}, &ws));
  if (!any) return 0;
  const int M = s->B * s->S, d = s->d, di = s->d_inner, K1 = s->K1, K2 = s->K2, nblk = pg_row_blocks(M);
  const float* h = (const float*)saved;
  const float* z = h + (size_t)M * di;
  hipStream_t st = (hipStream_t)stream;
  const bool upstream = dg->w1 || dg->b1 || dg->dx;  // anything behind the ReLU
  float *dz = ws.a, *du = ws.b, *dh = ws.wide;
  PgWgradPlan pl;

  NS_HIP(launch_ag_row_backward(ag_row_backward_args(M, d, p_drop, g, z, k->ln_g, keep, dz, du, ws.colpart), st));
  ++t_launches;
  if (dg->w2) {
    pg_plan_wgrad(M, d, di, K2, &pl);  // (accepted by carve above)
    NS_HIP(launch_pg_wgrad(du, h, M, s->S, d, di, K2, pl, ws.partial, dg->w2, st));
    t_launches += 2;
  }
  if (upstream) {
    const PgPack packs[2] = {{k->w2, nullptr, ws.wt2, d, di, K2}, {k->w1, nullptr, ws.wt1, di, d, K1}};
    NS_TRY(counted.pack(packs, dg->dx ? 2 : 1, st));
    NS_TRY(counted.conv(du, d, ws.wt2, nullptr, nullptr, dh, M, s->S, di, d, K2, K2 - 1 - (K2 - 1) / 2, ACT_NONE, st));
    NS_TRY(relu_gate(dh, h, M, di, dh, dg->b1, ws.gatepart, st));
    if (dg->w1) {
      pg_plan_wgrad(M, di, d, K1, &pl);  // (accepted by carve above)
      NS_HIP(launch_pg_wgrad(dh, x, M, s->S, di, d, K1, pl, ws.partial, dg->w1, st));
      t_launches += 2;
    }
    if (dg->dx) NS_TRY(counted.conv(dh, di, ws.wt1, nullptr, dz, dg->dx, M, s->S, d, di, K1, K1 - 1 - (K1 - 1) / 2, ACT_NONE, st));
  }
  return counted.col_finish(ws.colpart, nblk, d, {dg->ln_g, dg->ln_b, dg->b2}, {}, st);
}

extern "C" int ns_fg_op_relu_gate(const float* da, const float* h, int M, int d_inner, float* dh, float* d_b1, void* ws_mem, size_t ws_bytes,
                                  void* stream) {
  const std::string w = "ns_fg_op_relu_gate: ";
  t_launches = 0;
  if (!da || !h || !dh || (d_b1 && !ws_mem)) return api_fail(w + "null argument");
  if (M <= 0) return api_fail(w + "M must be positive, got " + std::to_string(M));
  if (d_inner <= 0 || d_inner % 256 != 0) return api_fail(w + "d_inner must be a positive multiple of 256, got " + std::to_string(d_inner));
  if ((long long)M * d_inner >= (1ll << 31)) return api_fail(w + "problem too large: M * d_inner must stay below 2^31");
  NS_TRY(check_aligned(w, {{"da", da}, {"h", h}, {"dh", dh}, {"d_b1", d_b1}, {"the workspace", ws_mem}}));
  const size_t need = (size_t)pg_row_blocks(M) * PG_SLOTS * d_inner * sizeof(double);
  if (d_b1 && ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  return relu_gate(da, h, M, d_inner, dh, d_b1, (double*)ws_mem, (hipStream_t)stream);
}
