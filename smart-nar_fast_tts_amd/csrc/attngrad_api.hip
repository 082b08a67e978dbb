// C-ABI of the MultiHeadAttention training forward and backward (include/nar_fs2.h ns_ag_*; transformer/SubLayers.py:8-59, self-attention).
// No handle: the weights are the caller's live tensors in checkpoint layout, the workspace and the saved activations belong to the
// caller.  Host-side only; every argument is validated before the first HIP call.  The four Linears run on what predgrad.hip and
// gemm_conv.hip already have (launch_conv_gemm at KW = 1, launch_pg_wgrad, launch_pg_col_final); the launch counts are stated in the
// header.  The checks, the parameter table, the size queries, the counted GEMM launch and the column-partial finish it shares with the
// other training ABIs are train_api.h's.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

static_assert(sizeof(ns_ag_shape) == 16, "ns_ag_shape layout");
static_assert(sizeof(ns_ag_weights) == 10 * sizeof(void*) && sizeof(ns_ag_grads) == 11 * sizeof(void*), "ns_ag_weights / ns_ag_grads layout");

namespace {
thread_local int t_launches = 0;
thread_local const Counted counted{"ns_ag", &t_launches};

struct Ws {  // the workspace of one shape, carved in this order
  float *wp, *bp, *wt, *wfct;  // [3d][d] and [3d] (forward), [d][3d] and [d][d] (data gradients)
  float* partial;              // the weight gradient's per-range tiles
  double* colpart;             // [2][row blocks][PG_SLOTS][d]
  float *a, *b, *c;            // [M, d] each: u (forward); dz, du, dctx (backward)
  float* wide;                 // [M, 3d]: dqkv (backward), qkv of a forward that saves nothing
  float* stat;                 // [B, H, S]: D (backward)
};

int check_dims(int B, int S, int d, int H, const std::string& w) {
  if (B <= 0 || S <= 0) return api_fail(w + "B and S must be positive, got " + std::to_string(B) + " x " + std::to_string(S));
  if (d != 256 && d != 512) return api_fail(w + "d must be 256 or 512, got " + std::to_string(d));
  if (H <= 0 || d % H != 0) return api_fail(w + "d must be a multiple of H, got d = " + std::to_string(d) + ", H = " + std::to_string(H));
  const int dk = d / H;
  if (dk != 32 && dk != 64 && dk != 128) return api_fail(w + "d / H must be 32, 64 or 128, got " + std::to_string(dk));
  if ((long long)B * S * 3 * d >= (1ll << 31)) return api_fail(w + "problem too large: B * S * 3d must stay below 2^31");
  return 0;
}

int carve(const ns_ag_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int M = s.B * s.S, d = s.d;
  PgWgradPlan pl;
  if (!pg_plan_wgrad(M, d, d, 1, &pl)) return api_fail(w + "problem too large for the weight gradient's split");
  Bump bump(base);
  const size_t dd = (size_t)d * d, md = (size_t)M * d;
  ws->wp = bump.f(3 * dd); ws->bp = bump.f(3 * (size_t)d); ws->wt = bump.f(3 * dd); ws->wfct = bump.f(dd);
  ws->partial = bump.f((size_t)pl.ws_floats);
  ws->colpart = (double*)bump.raw((size_t)2 * pg_row_blocks(M) * PG_SLOTS * d * sizeof(double));
  ws->a = bump.f(md); ws->b = bump.f(md); ws->c = bump.f(md);
  ws->wide = bump.f(3 * md);
  ws->stat = bump.f((size_t)s.B * s.H * s.S);
  *bytes = bump.off;
  return 0;
}

int check_shape(const ns_ag_shape& s, const std::string& w) { return check_dims(s.B, s.S, s.d, s.H, w); }

// what ns_ag_forward and ns_ag_backward check alike, in this order, and the carved workspace
int common(const std::string& w, const ns_ag_shape* s, const ns_ag_weights* k, const float* x, const int64_t* lens, const uint8_t* keep, float p_drop,
           const void* saved, void* ws_mem, size_t ws_bytes, Ws* ws) {
  NS_TRY(check_shape(*s, w));
  NS_TRY(check_weights(attn_params(*k), w));
  NS_TRY(check_drop({keep}, p_drop, w));
  NS_TRY(check_aligned(w, {{"x", x}, {"saved", saved}, {"the workspace", ws_mem}, {"lens", lens, 8}}));
  return carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, ws, w);
}
}  // namespace

extern "C" int ns_ag_abi_version(void) { return NS_AG_ABI_VERSION; }
extern "C" int ns_ag_last_launches(void) { return t_launches; }

extern "C" size_t ns_ag_ws_bytes(const ns_ag_shape* s) {
  return size_query("ns_ag_ws_bytes", s, check_shape, [](const ns_ag_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" size_t ns_ag_saved_bytes(const ns_ag_shape* s) {
  return size_query("ns_ag_saved_bytes", s, check_shape, [](const ns_ag_shape& s, const std::string&) {
    return ((size_t)5 * s.B * s.S * s.d + (size_t)s.B * s.H * s.S) * sizeof(float);
  });
}

extern "C" int ns_ag_forward(const ns_ag_shape* s, const ns_ag_weights* k, const float* x, const int64_t* lens, const uint8_t* keep, float p_drop,
                             float* y, void* saved, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_ag_forward: ";
  t_launches = 0;
  if (!s || !k || !x || !y || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_aligned(w, {{"y", y}}));
  Ws ws;
  NS_TRY(common(w, s, k, x, lens, keep, p_drop, saved, ws_mem, ws_bytes, &ws));
  const int M = s->B * s->S, d = s->d, H = s->H, dk = d / H;
  const size_t md = (size_t)M * d;
  float* qkv = saved ? (float*)saved : ws.wide;
  float* ctx = saved ? qkv + 3 * md : ws.c;
  float* z = saved ? qkv + 4 * md : nullptr;
  float* lse = saved ? qkv + 5 * md : nullptr;
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(launch_ag_pack(AgPack{k->wq, k->wk, k->wv, k->bq, k->bk, k->bv, k->wfc, ws.wp, ws.bp, nullptr, nullptr, d}, st));
  ++t_launches;
  NS_TRY(counted.gemm(x, ws.wp, ws.bp, nullptr, qkv, M, s->S, 3 * d, d, st));
  NS_HIP(launch_attention(qkv, (const long long*)lens, s->B, s->S, H, dk, ctx, nullptr, 0, nullptr, st));
  ++t_launches;
  if (lse) {
    NS_HIP(launch_ag_lse(qkv, (const long long*)lens, s->B, s->S, H, dk, lse, st));
    ++t_launches;
  }
  NS_TRY(counted.gemm(ctx, k->wfc, k->bfc, nullptr, ws.a, M, s->S, d, d, st));
  NS_HIP(launch_ag_row_forward(ws.a, x, keep, 1.f / (1.f - p_drop), k->ln_g, k->ln_b, z, y, M, d, st));
  ++t_launches;
  return 0;
}

extern "C" int ns_ag_backward(const ns_ag_shape* s, const ns_ag_weights* k, const float* x, const int64_t* lens, const uint8_t* keep, float p_drop,
                              const void* saved, const float* g, const ns_ag_grads* dg, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_ag_backward: ";
  t_launches = 0;
  if (!s || !k || !x || !saved || !g || !dg || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_aligned(w, {{"g", g}}));
  std::vector<NamedPtr> outs = attn_params(*dg);
  outs.push_back({"dx", dg->dx});
  bool any = false;
  NS_TRY(check_grads(outs, w, &any));
  Ws ws;
  NS_TRY(common(w, s, k, x, lens, keep, p_drop, saved, ws_mem, ws_bytes, &ws));
  if (!any) return 0;
  const int M = s->B * s->S, d = s->d, H = s->H, dk = d / H, nblk = pg_row_blocks(M);
  const size_t md = (size_t)M * d;
  const float* qkv = (const float*)saved;
  const float* ctx = qkv + 3 * md;
  const float* z = qkv + 4 * md;
  const float* lse = qkv + 5 * md;
  hipStream_t st = (hipStream_t)stream;
  const bool bias3 = dg->bq || dg->bk || dg->bv;
  const bool upstream = dg->dx || dg->wq || dg->wk || dg->wv || bias3;  // anything behind ctx
  PgWgradPlan pl;
  pg_plan_wgrad(M, d, d, 1, &pl);  // (accepted by carve above)
  float *dz = ws.a, *du = ws.b, *dctx = ws.c, *dqkv = ws.wide;
  double* part_row = ws.colpart + (size_t)nblk * PG_SLOTS * d;  // stage 1; stage 0 holds the three thirds of dqkv

  if (upstream) {
    NS_HIP(launch_ag_pack(AgPack{k->wq, k->wk, k->wv, k->bq, k->bk, k->bv, k->wfc, nullptr, nullptr, dg->dx ? ws.wt : nullptr, ws.wfct, d}, st));
    ++t_launches;
  }
  NS_HIP(launch_ag_row_backward(ag_row_backward_args(M, d, p_drop, g, z, k->ln_g, keep, dz, du, part_row), st));
  ++t_launches;
  if (dg->wfc) {
    NS_HIP(launch_pg_wgrad(du, ctx, M, s->S, d, d, 1, pl, ws.partial, dg->wfc, st));
    t_launches += 2;
  }
  if (upstream) {
    NS_TRY(counted.gemm(du, ws.wfct, nullptr, nullptr, dctx, M, s->S, d, d, st));
    NS_HIP(launch_ag_attention_backward(qkv, ctx, lse, dctx, (const long long*)lens, s->B, s->S, H, dk, ws.stat, dqkv, st));
    t_launches += 2;
    float* dw[3] = {dg->wq, dg->wk, dg->wv};
    for (int i = 0; i < 3; ++i)
      if (dw[i]) {
        NS_HIP(launch_pg_wgrad(dqkv + (size_t)i * d, x, M, s->S, d, d, 1, pl, ws.partial, dw[i], st, 3 * d));
        t_launches += 2;
      }
    if (bias3) {
      NS_HIP(launch_pg_colsum(dqkv, M, d, 3, ws.colpart, st));
      ++t_launches;
    }
    if (dg->dx) NS_TRY(counted.gemm(dqkv, ws.wt, nullptr, dz, dg->dx, M, s->S, d, 3 * d, st));
  }
  return counted.col_finish(ws.colpart, nblk, d, {dg->bq, dg->bk, dg->bv}, {dg->ln_g, dg->ln_b, dg->bfc}, st);
}

extern "C" int ns_ag_op_lse(const float* qkv, const int64_t* lens, int B, int S, int d, int H, float* lse, void* stream) {
  const std::string w = "ns_ag_op_lse: ";
  t_launches = 0;
  if (!qkv || !lse) return api_fail(w + "null argument");
  NS_TRY(check_dims(B, S, d, H, w));
  NS_TRY(check_aligned(w, {{"qkv", qkv}, {"lse", lse, 4}, {"lens", lens, 8}}));
  NS_HIP(launch_ag_lse(qkv, (const long long*)lens, B, S, H, d / H, lse, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_ag_op_attention_backward(const float* qkv, const float* ctx, const float* lse, const float* dctx, const int64_t* lens, int B, int S,
                                           int d, int H, float* dqkv, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_ag_op_attention_backward: ";
  t_launches = 0;
  if (!qkv || !ctx || !lse || !dctx || !dqkv || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_dims(B, S, d, H, w));
  NS_TRY(check_aligned(w, {{"qkv", qkv}, {"ctx", ctx}, {"dctx", dctx}, {"dqkv", dqkv}, {"the workspace", ws_mem}, {"lse", lse, 4}, {"lens", lens, 8}}));
  const size_t need = (size_t)B * H * S * sizeof(float);
  if (ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  NS_HIP(launch_ag_attention_backward(qkv, ctx, lse, dctx, (const long long*)lens, B, S, H, d / H, (float*)ws_mem, dqkv, (hipStream_t)stream));
  t_launches += 2;
  return 0;
}

extern "C" int ns_ag_op_row_backward(const float* dy, const float* z, const float* ln_g, const uint8_t* keep, float p_drop, int M, int d, float* dz,
                                     float* du, float* d_ln_g, float* d_ln_b, float* d_bfc, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_ag_op_row_backward: ";
  t_launches = 0;
  if (!dy || !z || !ln_g || !dz || !du || !d_ln_g || !d_ln_b || !d_bfc || !ws_mem) return api_fail(w + "null argument");
  if (M <= 0) return api_fail(w + "M must be positive");
  if (d != 256 && d != 512) return api_fail(w + "d must be 256 or 512, got " + std::to_string(d));
  if ((long long)M * d >= (1ll << 31)) return api_fail(w + "problem too large");
  NS_TRY(check_drop({keep}, p_drop, w));
  NS_TRY(check_aligned(w, {{"dy", dy}, {"z", z}, {"ln_g", ln_g}, {"dz", dz}, {"du", du}, {"d_ln_g", d_ln_g}, {"d_ln_b", d_ln_b}, {"d_bfc", d_bfc},
                           {"the workspace", ws_mem}}));
  const size_t need = (size_t)pg_row_blocks(M) * PG_SLOTS * d * sizeof(double);
  if (ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws_mem;
  NS_HIP(launch_ag_row_backward(ag_row_backward_args(M, d, p_drop, dy, z, ln_g, keep, dz, du, part), st));
  ++t_launches;
  return counted.col_finish(part, pg_row_blocks(M), d, {d_ln_g, d_ln_b, d_bfc}, {}, st);
}
