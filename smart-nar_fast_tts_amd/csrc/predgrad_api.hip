// C-ABI of the VariancePredictor training forward and backward (include/nar_fs2.h ns_pg_*; model/modules.py:233-286).  No handle:
// the weights are the caller's live tensors in checkpoint layout, the workspace and the saved activations belong to the caller.
// Host-side only; every argument is validated before the first HIP call.  The checks, the size queries, the counted GEMM and pack
// launches and the column-partial finish it shares with the other training ABIs are train_api.h's.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

static_assert(sizeof(ns_pg_shape) == 20, "ns_pg_shape layout");
static_assert(sizeof(ns_pg_weights) == 10 * sizeof(void*) && sizeof(ns_pg_grads) == 11 * sizeof(void*), "ns_pg_weights / ns_pg_grads layout");

namespace {
thread_local int t_launches = 0;
thread_local const Counted counted{"ns_pg", &t_launches};

struct Ws {  // the workspace of one shape, carved in this order
  float *w1p, *w1t, *w2p, *w2t;  // packed weights: forward form and data-gradient form of both convolutions
  float* partial;                // the weight gradient's per-range tiles (the larger of the two convolutions')
  double* colpart;               // [2][row blocks][PG_SLOTS][F]
  float *a, *b, *c;              // [M, F] each: dz2 / dh1 / dz1 of the backward, v1 / h1 / v2 of a forward that saves nothing
};

int check_dims(int B, int S, int F, int Cin, int K, int cin_mult, const std::string& w) {
  if (B <= 0 || S <= 0) return api_fail(w + "B and S must be positive, got " + std::to_string(B) + " x " + std::to_string(S));
  if (K <= 0 || K % 2 == 0) return api_fail(w + "K must be odd, got " + std::to_string(K));
  if (F != 256 && F != 512) return api_fail(w + "F must be 256 or 512, got " + std::to_string(F));
  if (Cin <= 0 || Cin % cin_mult != 0) return api_fail(w + "Cin must be a multiple of " + std::to_string(cin_mult) + ", got " + std::to_string(Cin));
  const long long M = (long long)B * S;
  if (M * (F > Cin ? F : Cin) >= (1ll << 31)) return api_fail(w + "problem too large: B * S * max(F, Cin) must stay below 2^31");
  return 0;
}

int carve(const ns_pg_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int M = s.B * s.S;
  PgWgradPlan p1, p2;
  if (!pg_plan_wgrad(M, s.F, s.Cin, s.K, &p1) || !pg_plan_wgrad(M, s.F, s.F, s.K, &p2)) return api_fail(w + "problem too large for the weight gradient's split");
  Bump bump(base);
  const size_t n1 = (size_t)s.F * s.K * s.Cin, n2 = (size_t)s.F * s.K * s.F, mf = (size_t)M * s.F;
  ws->w1p = bump.f(n1); ws->w1t = bump.f(n1); ws->w2p = bump.f(n2); ws->w2t = bump.f(n2);
  ws->partial = bump.f((size_t)(p1.ws_floats > p2.ws_floats ? p1.ws_floats : p2.ws_floats));
  ws->colpart = (double*)bump.raw((size_t)2 * pg_row_blocks(M) * PG_SLOTS * s.F * sizeof(double));
  ws->a = bump.f(mf); ws->b = bump.f(mf); ws->c = bump.f(mf);
  *bytes = bump.off;
  return 0;
}

// the ten parameters of ns_pg_weights or ns_pg_grads, in ABI order (blin is one float)
template <class T>
std::vector<NamedPtr> ten(const T& k) {
  return {{"w1", k.w1}, {"b1", k.b1}, {"ln1_g", k.ln1_g}, {"ln1_b", k.ln1_b}, {"w2", k.w2}, {"b2", k.b2}, {"ln2_g", k.ln2_g}, {"ln2_b", k.ln2_b},
          {"wlin", k.wlin}, {"blin", k.blin, 4}};
}

// the size queries take any Cin the weight gradient does; the layer itself needs a multiple of 16 (common)
int check_shape(const ns_pg_shape& s, const std::string& w) { return check_dims(s.B, s.S, s.F, s.Cin, s.K, 4, w); }

// what ns_pg_forward and ns_pg_backward check alike, in this order; `scalar` names pred or g, a [B, S] tensor of floats
int common(const std::string& w, const ns_pg_shape* s, const ns_pg_weights* k, const float* x, const uint8_t* keep1, const uint8_t* keep2,
           float p_drop, const void* saved, const void* ws_mem, NamedPtr scalar) {
  NS_TRY(check_dims(s->B, s->S, s->F, s->Cin, s->K, 16, w));
  NS_TRY(check_weights(ten(*k), w));
  NS_TRY(check_drop({keep1, keep2}, p_drop, w));
  NS_TRY(check_aligned(w, {{"x", x}, {"saved", saved}, {"the workspace", ws_mem}, scalar}));
  return 0;
}
}  // namespace

extern "C" int ns_pg_abi_version(void) { return NS_PG_ABI_VERSION; }
extern "C" int ns_pg_last_launches(void) { return t_launches; }

extern "C" int ns_pg_plan_wgrad(int M, int N, int Cin, int KW, int32_t out[8]) {
  if (!out) return api_fail("ns_pg_plan_wgrad: null argument");
  PgWgradPlan p;
  if (!pg_plan_wgrad(M, N, Cin, KW, &p))
    return api_fail("ns_pg_plan_wgrad: refused (M > 0, N a multiple of 128, Cin a multiple of 4, KW odd, sizes below 2^31)");
  out[0] = p.tile_n; out[1] = p.tile_c; out[2] = p.rows; out[3] = p.ranges; out[4] = p.tiles; out[5] = (int32_t)p.ws_floats; out[6] = p.chunk; out[7] = 0;
  return 0;
}

extern "C" size_t ns_pg_ws_bytes(const ns_pg_shape* s) {
  return size_query("ns_pg_ws_bytes", s, check_shape, [](const ns_pg_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" size_t ns_pg_saved_bytes(const ns_pg_shape* s) {
  return size_query("ns_pg_saved_bytes", s, check_shape,
                    [](const ns_pg_shape& s, const std::string&) { return (size_t)3 * s.B * s.S * s.F * sizeof(float); });
}

extern "C" int ns_pg_forward(const ns_pg_shape* s, const ns_pg_weights* k, const float* x, const uint8_t* mask, const uint8_t* keep1,
                             const uint8_t* keep2, float p_drop, float* pred, void* saved, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_pg_forward: ";
  t_launches = 0;
  if (!s || !k || !x || !pred || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(common(w, s, k, x, keep1, keep2, p_drop, saved, ws_mem, {"pred", pred, 4}));
  Ws ws;
  NS_TRY(carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, &ws, w));
  const int M = s->B * s->S, F = s->F, K = s->K, pad = (K - 1) / 2;
  const size_t mf = (size_t)M * F;
  float* v1 = saved ? (float*)saved : ws.a;
  float* h1 = saved ? v1 + mf : ws.b;
  float* v2 = saved ? v1 + 2 * mf : ws.c;
  const float scale = 1.f / (1.f - p_drop);
  hipStream_t st = (hipStream_t)stream;
  const PgPack packs[2] = {{k->w1, ws.w1p, nullptr, F, s->Cin, K}, {k->w2, ws.w2p, nullptr, F, F, K}};
  NS_TRY(counted.pack(packs, 2, st));
  NS_TRY(counted.conv(x, s->Cin, ws.w1p, k->b1, nullptr, v1, M, s->S, F, s->Cin, K, pad, ACT_RELU, st));
  NS_HIP(launch_pg_row_forward(v1, k->ln1_g, k->ln1_b, keep1, scale, h1, nullptr, nullptr, nullptr, nullptr, M, F, st));
  ++t_launches;
  NS_TRY(counted.conv(h1, F, ws.w2p, k->b2, nullptr, v2, M, s->S, F, F, K, pad, ACT_RELU, st));
  NS_HIP(launch_pg_row_forward(v2, k->ln2_g, k->ln2_b, keep2, scale, nullptr, k->wlin, k->blin, mask, pred, M, F, st));
  ++t_launches;
  return 0;
}

extern "C" int ns_pg_backward(const ns_pg_shape* s, const ns_pg_weights* k, const float* x, const uint8_t* mask, const uint8_t* keep1,
                              const uint8_t* keep2, float p_drop, const void* saved, const float* g, const ns_pg_grads* d, void* ws_mem,
                              size_t ws_bytes, void* stream) {
  const std::string w = "ns_pg_backward: ";
  t_launches = 0;
  if (!s || !k || !x || !saved || !g || !d || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(common(w, s, k, x, keep1, keep2, p_drop, saved, ws_mem, {"g", g, 4}));
  std::vector<NamedPtr> outs = ten(*d);
  outs.push_back({"dx", d->dx});
  NS_TRY(check_grads(outs, w));
  Ws ws;
  NS_TRY(carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, &ws, w));
  const int M = s->B * s->S, F = s->F, Cin = s->Cin, K = s->K, padT = K - 1 - (K - 1) / 2;
  const size_t mf = (size_t)M * F;
  const float* v1 = (const float*)saved;
  const float* h1 = v1 + mf;
  const float* v2 = v1 + 2 * mf;
  hipStream_t st = (hipStream_t)stream;
  const bool stage1 = d->w1 || d->b1 || d->ln1_g || d->ln1_b || d->dx;  // anything upstream of conv1d_2's input
  const bool stage2 = stage1 || d->w2 || d->b2 || d->ln2_g || d->ln2_b || d->wlin || d->blin;
  if (!stage2) return 0;
  PgWgradPlan p1, p2;
  pg_plan_wgrad(M, F, Cin, K, &p1);  // (both accepted by carve above)
  pg_plan_wgrad(M, F, F, K, &p2);
  const int nblk = pg_row_blocks(M);

  if (stage1 || d->dx) {
    const PgPack packs[2] = {{d->dx ? k->w1 : nullptr, nullptr, ws.w1t, F, Cin, K}, {stage1 ? k->w2 : nullptr, nullptr, ws.w2t, F, F, K}};
    NS_TRY(counted.pack(packs, 2, st));
  }
  NS_HIP(launch_pg_row_backward(pg_row_backward_args(1, M, F, p_drop, nullptr, g, mask, v2, k->ln2_g, k->ln2_b, k->wlin, keep2, ws.a, ws.colpart), st));
  ++t_launches;
  if (d->w2) {
    NS_HIP(launch_pg_wgrad(ws.a, h1, M, s->S, F, F, K, p2, ws.partial, d->w2, st));
    t_launches += 2;
  }
  if (stage1) {
    NS_TRY(counted.conv(ws.a, F, ws.w2t, nullptr, nullptr, ws.b, M, s->S, F, F, K, padT, ACT_NONE, st));
    NS_HIP(launch_pg_row_backward(pg_row_backward_args(0, M, F, p_drop, ws.b, nullptr, nullptr, v1, k->ln1_g, nullptr, nullptr, keep1, ws.c,
                                                       ws.colpart + (size_t)nblk * PG_SLOTS * F), st));
    ++t_launches;
    if (d->w1) {
      NS_HIP(launch_pg_wgrad(ws.c, x, M, s->S, F, Cin, K, p1, ws.partial, d->w1, st));
      t_launches += 2;
    }
    if (d->dx) NS_TRY(counted.conv(ws.c, F, ws.w1t, nullptr, nullptr, d->dx, M, s->S, Cin, F, K, padT, ACT_NONE, st));
  }
  // (a wanted d->ln1_g, ln1_b or b1 implies stage1, so stage 1 of the partials was written)
  return counted.col_finish(ws.colpart, nblk, F, {d->ln2_g, d->ln2_b, d->b2, d->wlin, d->blin}, {d->ln1_g, d->ln1_b, d->b1}, st);
}

extern "C" int ns_pg_op_wgrad(const float* dz, const float* X, int B, int S, int N, int Cin, int KW, float* dW, float* db, void* ws_mem,
                              size_t ws_bytes, void* stream) {
  const std::string w = "ns_pg_op_wgrad: ";
  t_launches = 0;
  if (!dz || !X || !dW || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_dims(B, S, N, Cin, KW, 4, w));
  NS_TRY(check_aligned(w, {{"dz", dz}, {"X", X}, {"dW", dW}, {"db", db}, {"the workspace", ws_mem}}));
  const int M = B * S;
  PgWgradPlan pl;
  if (!pg_plan_wgrad(M, N, Cin, KW, &pl)) return api_fail(w + "problem too large for the weight gradient's split");
  Bump bump(ws_mem);
  float* partial = bump.f((size_t)pl.ws_floats);
  double* colpart = (double*)bump.raw((size_t)pg_row_blocks(M) * PG_SLOTS * N * sizeof(double));
  if (ws_bytes < bump.off) return api_fail(w + "workspace too small: " + std::to_string(bump.off) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(launch_pg_wgrad(dz, X, M, S, N, Cin, KW, pl, partial, dW, st));
  t_launches += 2;
  if (db) {
    NS_HIP(launch_pg_colsum(dz, M, N, 1, colpart, st));
    ++t_launches;
    NS_TRY(counted.col_finish(colpart, pg_row_blocks(M), N, {db}, {}, st));
  }
  return 0;
}

extern "C" int ns_pg_op_dgrad(const float* dz, const float* W, int B, int S, int N, int Cin, int KW, float* dX, void* ws_mem, size_t ws_bytes,
                              void* stream) {
  const std::string w = "ns_pg_op_dgrad: ";
  t_launches = 0;
  if (!dz || !W || !dX || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_dims(B, S, N, Cin, KW, 16, w));
  NS_TRY(check_aligned(w, {{"dz", dz}, {"W", W}, {"dX", dX}, {"the workspace", ws_mem}}));
  Bump bump(ws_mem);
  float* wt = bump.f((size_t)N * Cin * KW);
  if (ws_bytes < bump.off) return api_fail(w + "workspace too small: " + std::to_string(bump.off) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  const PgPack one{W, nullptr, wt, N, Cin, KW};
  NS_TRY(counted.pack(&one, 1, st));
  return counted.conv(dz, N, wt, nullptr, nullptr, dX, B * S, S, Cin, N, KW, KW - 1 - (KW - 1) / 2, ACT_NONE, st);
}

extern "C" int ns_pg_op_row_backward(int tail, const float* dy, const float* g, const uint8_t* mask, const float* v, const float* ln_g,
                                     const float* ln_b, const float* wlin, const uint8_t* keep, float p_drop, int M, int F, float* dz,
                                     float* d_ln_g, float* d_ln_b, float* d_b, float* d_wlin, float* d_blin, void* ws_mem, size_t ws_bytes,
                                     void* stream) {
  const std::string w = "ns_pg_op_row_backward: ";
  t_launches = 0;
  if (!v || !ln_g || !dz || !d_ln_g || !d_ln_b || !d_b || !ws_mem) return api_fail(w + "null argument");
  if (tail ? (!g || !ln_b || !wlin || !d_wlin || !d_blin) : !dy) return api_fail(w + "null argument");
  NS_TRY(check_dims(M, 1, F, 4, 1, 4, w));
  NS_TRY(check_drop({keep, keep}, p_drop, w));  // (the texts of the two-mask entry points)
  NS_TRY(check_aligned(w, {{"dy", dy}, {"v", v}, {"ln_g", ln_g}, {"ln_b", ln_b}, {"wlin", wlin}, {"dz", dz}, {"d_ln_g", d_ln_g}, {"d_ln_b", d_ln_b},
                           {"d_b", d_b}, {"d_wlin", d_wlin}, {"the workspace", ws_mem}}));
  const size_t need = (size_t)pg_row_blocks(M) * PG_SLOTS * F * sizeof(double);
  if (ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws_mem;
  NS_HIP(launch_pg_row_backward(pg_row_backward_args(tail, M, F, p_drop, dy, g, tail ? mask : nullptr, v, ln_g, ln_b, wlin, keep, dz, part), st));
  ++t_launches;
  return counted.col_finish(part, pg_row_blocks(M), F, {d_ln_g, d_ln_b, d_b, tail ? d_wlin : nullptr, tail ? d_blin : nullptr}, {}, st);
}
