// C-ABI of the MelEncoder's Prenet with the position add behind it, training forward and backward (include/nar_fs2.h ns_me_*;
// transformer/Models.py:145-146,151,162, transformer/Layers.py:11-26).  No handle: the weights are the caller's
// live tensors in checkpoint (nn.Linear) layout, the workspace and the saved activations belong to the caller.  Host-side only; every
// argument is validated before the first HIP call.  Every launch but the two of melencgrad.hip is a kernel the other ABIs already
// run: the aligner's frame-0 select, the Conv1D-as-GEMM dispatch at KW = 1 (forward, data gradients), the predictor's weight gradient
// and its pack kernel, the feed-forward's ReLU gate, the column-partial finish.  The launch counts are stated in the header.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

static_assert(sizeof(ns_me_shape) == 16, "ns_me_shape layout");
static_assert(sizeof(ns_me_weights) == 4 * sizeof(void*) && sizeof(ns_me_grads) == 5 * sizeof(void*), "ns_me_weights / ns_me_grads layout");

namespace {
thread_local int t_launches = 0;
thread_local const Counted counted{"ns_me", &t_launches};

struct Ws {  // the workspace of one shape, carved in this order
  float *wp1, *wp2;  // [d][n_mel] and [d][d]: the forward's form
  float *wt1, *wt2;  // [n_mel][d] and [d][d]: the data gradients' form (transposed)
  float* partial;    // the weight gradients' per-range tiles (the larger of the two)
  double* colpart;   // [row blocks][PG_SLOTS][d]: d_b2, then d_b1, in slot 0
  float* xin;        // [M, n_mel]: the input of a forward that saves nothing; the data gradient ahead of the frame-0 select (backward)
  float *a, *b;      // [M, d] each: h1, h2 of a forward that saves nothing; dh2, then da1 and dh1 in place (backward)
};

// what every entry point checks of [B, T, d] rows (the gate's hook passes its M rows as B = M, T = 1)
int check_rows(const std::string& w, int B, int T, int d) {
  if (B <= 0 || T <= 0) return api_fail(w + "B and T must be positive, got " + std::to_string(B) + " x " + std::to_string(T));
  if (d != 256 && d != 512) return api_fail(w + "d must be 256 or 512, got " + std::to_string(d));
  if ((long long)B * T * d >= (1ll << 31)) return api_fail(w + "problem too large: B * T * d must stay below 2^31");
  return 0;
}

int check_dims(const ns_me_shape& s, const std::string& w) {
  NS_TRY(check_rows(w, s.B, s.T, s.d));
  if (s.n_mel <= 0 || s.n_mel % 4 != 0) return api_fail(w + "n_mel must be a positive multiple of 4, got " + std::to_string(s.n_mel));
  if ((long long)s.B * s.T * s.n_mel >= (1ll << 31)) return api_fail(w + "problem too large: B * T * n_mel must stay below 2^31");
  return 0;
}

int carve(const ns_me_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int M = s.B * s.T, d = s.d, c = s.n_mel, nblk = pg_row_blocks(M);
  int rec[2][8];
  if (conv_gemm_describe(M, d, c, 1, 0, rec) <= 0 || conv_gemm_describe(M, d, d, 1, 0, rec) <= 0 || conv_gemm_describe(M, c, d, 1, 0, rec) <= 0)
    return api_fail(w + "the Conv1D-as-GEMM dispatch refuses this shape");
  PgWgradPlan pl1, pl2;
  if (!pg_plan_wgrad(M, d, c, 1, &pl1) || !pg_plan_wgrad(M, d, d, 1, &pl2)) return api_fail(w + "the weight gradient's plan refuses this shape");
  Bump bump(base);
  const size_t n1 = (size_t)d * c, n2 = (size_t)d * d;
  ws->wp1 = bump.f(n1); ws->wp2 = bump.f(n2); ws->wt1 = bump.f(n1); ws->wt2 = bump.f(n2);
  ws->partial = bump.f((size_t)(pl1.ws_floats > pl2.ws_floats ? pl1.ws_floats : pl2.ws_floats));
  ws->colpart = (double*)bump.raw((size_t)nblk * PG_SLOTS * d * sizeof(double));
  ws->xin = bump.f((size_t)M * c);
  ws->a = bump.f((size_t)M * d); ws->b = bump.f((size_t)M * d);
  *bytes = bump.off;
  return 0;
}

std::vector<NamedPtr> params(const float* w1, const float* b1, const float* w2, const float* b2) {
  return {{"w1", w1}, {"b1", b1}, {"w2", w2}, {"b2", b2}};
}

// what ns_me_forward and ns_me_backward check alike, in this order, and the carved workspace
int common(const std::string& w, const ns_me_shape* s, const ns_me_weights* k, const uint8_t* keep, float p_drop, const void* saved, void* ws_mem,
           size_t ws_bytes, std::initializer_list<NamedPtr> io, Ws* ws) {
  NS_TRY(check_dims(*s, w));
  NS_TRY(check_weights(params(k->w1, k->b1, k->w2, k->b2), w));
  NS_TRY(check_drop({keep}, p_drop, w));
  NS_TRY(check_aligned(w, {{"saved", saved}, {"the workspace", ws_mem}}));
  NS_TRY(check_aligned(w, io));
  return carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, ws, w);
}

// the dropout + ReLU gate and, where d_b2 is wanted, the fixed-order sum of its partials: one or two launches
int drop_relu_gate(const float* g, const float* h2, const uint8_t* keep, float p_drop, int M, int d, float* dh, float* d_b2, double* part,
                   hipStream_t st) {
  NS_HIP(launch_me_drop_relu_gate(g, h2, keep, 1.f / (1.f - p_drop), M, d, dh, d_b2 ? part : nullptr, st));
  ++t_launches;
  return counted.col_finish(part, pg_row_blocks(M), d, {d_b2}, {}, st);
}

}  // namespace

extern "C" int ns_me_abi_version(void) { return NS_ME_ABI_VERSION; }
extern "C" int ns_me_last_launches(void) { return t_launches; }

extern "C" size_t ns_me_ws_bytes(const ns_me_shape* s) {
  return size_query("ns_me_ws_bytes", s, check_dims, [](const ns_me_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" size_t ns_me_saved_bytes(const ns_me_shape* s) {
  return size_query("ns_me_saved_bytes", s, check_dims, [](const ns_me_shape& s, const std::string& w) {
    return carved_bytes(carve, s, w) ? (size_t)s.B * s.T * ((size_t)s.n_mel + 2 * (size_t)s.d) * sizeof(float) : (size_t)0;
  });
}

extern "C" int ns_me_forward(const ns_me_shape* s, const ns_me_weights* k, const float* mels, const float* pos, const uint8_t* keep, float p_drop,
                             float* y, void* saved, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_me_forward: ";
  t_launches = 0;
  if (!s || !k || !mels || !pos || !y || !ws_mem) return api_fail(w + "null argument");
  Ws ws;
  NS_TRY(common(w, s, k, keep, p_drop, saved, ws_mem, ws_bytes, {{"mels", mels}, {"pos", pos}, {"y", y}}, &ws));
  const int M = s->B * s->T, d = s->d, c = s->n_mel;
  float* xin = saved ? (float*)saved : ws.xin;
  float* h1 = saved ? xin + (size_t)M * c : ws.a;
  float* h2 = saved ? h1 + (size_t)M * d : ws.b;
  hipStream_t st = (hipStream_t)stream;
  const PgPack packs[2] = {{k->w1, ws.wp1, nullptr, d, c, 1}, {k->w2, ws.wp2, nullptr, d, d, 1}};
  NS_TRY(counted.pack(packs, 2, st));
  NS_HIP(launch_aln_input(mels, xin, s->B, s->T, c, st));
  ++t_launches;
  NS_TRY(counted.conv(xin, c, ws.wp1, k->b1, nullptr, h1, M, s->T, d, c, 1, 0, ACT_RELU, st));
  NS_TRY(counted.conv(h1, d, ws.wp2, k->b2, nullptr, h2, M, s->T, d, d, 1, 0, ACT_RELU, st));
  NS_HIP(launch_me_drop_pos(h2, pos, keep, 1.f / (1.f - p_drop), M, s->T, d, y, st));
  ++t_launches;
  return 0;
}

extern "C" int ns_me_backward(const ns_me_shape* s, const ns_me_weights* k, const uint8_t* keep, float p_drop, const void* saved, const float* g,
                              const ns_me_grads* dg, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_me_backward: ";
  t_launches = 0;
  if (!s || !k || !saved || !g || !dg || !ws_mem) return api_fail(w + "null argument");
  std::vector<NamedPtr> outs = params(dg->w1, dg->b1, dg->w2, dg->b2);
  outs.push_back({"dmels", dg->dmels});
  bool any = false;
  NS_TRY(check_grads(outs, w, &any));
  Ws ws;
  NS_TRY(common(w, s, k, keep, p_drop, saved, ws_mem, ws_bytes, {{"g", g}}, &ws));
  if (!any) return 0;
  const int M = s->B * s->T, d = s->d, c = s->n_mel;
  const float* xin = (const float*)saved;
  const float* h1 = xin + (size_t)M * c;
  const float* h2 = h1 + (size_t)M * d;
  hipStream_t st = (hipStream_t)stream;
  const bool upstream = dg->w1 || dg->b1 || dg->dmels;  // anything behind the first ReLU
  float *dh2 = ws.a, *dh1 = ws.b;
  PgWgradPlan pl;

  NS_TRY(drop_relu_gate(g, h2, keep, p_drop, M, d, dh2, dg->b2, ws.colpart, st));
  if (dg->w2) {
    pg_plan_wgrad(M, d, d, 1, &pl);  // (accepted by carve above)
    NS_HIP(launch_pg_wgrad(dh2, h1, M, s->T, d, d, 1, pl, ws.partial, dg->w2, st));
    t_launches += 2;
  }
  if (!upstream) return 0;
  const PgPack packs[2] = {{k->w2, nullptr, ws.wt2, d, d, 1}, {k->w1, nullptr, ws.wt1, d, c, 1}};
  NS_TRY(counted.pack(packs, dg->dmels ? 2 : 1, st));
  NS_TRY(counted.conv(dh2, d, ws.wt2, nullptr, nullptr, dh1, M, s->T, d, d, 1, 0, ACT_NONE, st));
  NS_HIP(launch_fg_relu_gate(dh1, h1, M, d, dh1, dg->b1 ? ws.colpart : nullptr, st));  // (the finish of d_b2 is ahead on the stream)
  ++t_launches;
  NS_TRY(counted.col_finish(ws.colpart, pg_row_blocks(M), d, {dg->b1}, {}, st));
  if (dg->w1) {
    pg_plan_wgrad(M, d, c, 1, &pl);  // (accepted by carve above)
    NS_HIP(launch_pg_wgrad(dh1, xin, M, s->T, d, c, 1, pl, ws.partial, dg->w1, st));
    t_launches += 2;
  }
  if (dg->dmels) {
    NS_TRY(counted.conv(dh1, d, ws.wt1, nullptr, nullptr, ws.xin, M, s->T, c, d, 1, 0, ACT_NONE, st));
    NS_HIP(launch_aln_input(ws.xin, dg->dmels, s->B, s->T, c, st));
    ++t_launches;
  }
  return 0;
}

extern "C" int ns_me_op_drop_pos(const float* h2, const float* pos, const uint8_t* keep, float p_drop, int B, int T, int d, float* y, void* stream) {
  const std::string w = "ns_me_op_drop_pos: ";
  t_launches = 0;
  if (!h2 || !pos || !y) return api_fail(w + "null argument");
  NS_TRY(check_rows(w, B, T, d));
  NS_TRY(check_drop({keep}, p_drop, w));
  if (h2 == y) return api_fail(w + "y must not be h2 (the op is out of place)");
  NS_TRY(check_aligned(w, {{"h2", h2}, {"pos", pos}, {"y", y}}));
  NS_HIP(launch_me_drop_pos(h2, pos, keep, 1.f / (1.f - p_drop), B * T, T, d, y, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_me_op_drop_relu_gate(const float* g, const float* h2, const uint8_t* keep, float p_drop, int M, int d, float* dh, float* d_b2,
                                       void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_me_op_drop_relu_gate: ";
  t_launches = 0;
  if (!g || !h2 || !dh || (d_b2 && !ws_mem)) return api_fail(w + "null argument");
  if (M <= 0) return api_fail(w + "M must be positive, got " + std::to_string(M));
  NS_TRY(check_rows(w, M, 1, d));
  NS_TRY(check_drop({keep}, p_drop, w));
  if (g == dh) return api_fail(w + "dh must not be g (the op is out of place)");
  NS_TRY(check_aligned(w, {{"g", g}, {"h2", h2}, {"dh", dh}, {"d_b2", d_b2}, {"the workspace", ws_mem}}));
  const size_t need = (size_t)pg_row_blocks(M) * PG_SLOTS * d * sizeof(double);
  if (d_b2 && ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  return drop_relu_gate(g, h2, keep, p_drop, M, d, dh, d_b2, (double*)ws_mem, (hipStream_t)stream);
}
