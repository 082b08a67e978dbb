// C-ABI of the opt-in "bf16" matmul mode of the PositionwiseFeedForward training layer (include/nar_fs2.h ns_fg_*_bf16; DESIGN.md
// section 36).  The six contractions of the layer run with both operands rounded to bf16 and fp32 accumulation: the forward and the
// data gradients on k_conv_gemm_bf16 (gemm_bf16.hip) from planes k_fg_pack_bf16 rounds from the live weights each call, the weight
// gradients on k_fg_wgrad_bf16 (ffngrad_bf16.hip).  Everything else is the fp32 mode's launch (ffngrad_api.hip): the row forward and
// backward, the ReLU gate on the saved h, the float64 column finishes, the weight gradient's reduce.  The arguments, their checks and
// their words are ffngrad_api.hip's (ffngrad_api.h); the launch counter is the family's one.  Host-side only; every argument is
// validated before the first HIP call.
#include "ffngrad_api.h"

using namespace ns;
using namespace ns::fg;

namespace {
Counted counted() { return Counted{"ns_fg", launches()}; }

struct Ws {  // the workspace of one shape, carved in this order
  unsigned short *wp1, *wp2;  // bf16 [d_inner][K1][d] and [d][K2][d_inner]: the forward's planes
  unsigned short *wt1, *wt2;  // bf16 [d][K1][d_inner] and [d_inner][K2][d]: the data gradients' planes (transposed, taps flipped)
  float* partial;             // the weight gradients' per-range tiles (the larger of the two)
  double* colpart;            // [row blocks][PG_SLOTS][d]: d_ln_g, d_ln_b, d_b2
  double* gatepart;           // [row blocks][PG_SLOTS][d_inner]: d_b1 in slot 0
  float *a, *b;               // [M, d] each: u (forward); dz, du (backward)
  float* wide;                // [M, d_inner]: da, then dh in place (backward); h of a forward that saves nothing
};

int carve(const ns_fg_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int M = s.B * s.S, d = s.d, di = s.d_inner, nblk = pg_row_blocks(M);
  if (!conv_gemm_bf16_ok(M, di, d, s.K1, EPI_NONE) || !conv_gemm_bf16_ok(M, d, di, s.K2, EPI_NONE) || !conv_gemm_bf16_ok(M, di, d, s.K2, EPI_NONE) ||
      !conv_gemm_bf16_ok(M, d, di, s.K1, EPI_NONE))
    return api_fail(w + "the Conv1D-as-GEMM dispatch refuses this shape");
  PgWgradPlan pl1, pl2;
  if (!fg_plan_wgrad_bf16(M, di, d, s.K1, &pl1) || !fg_plan_wgrad_bf16(M, d, di, s.K2, &pl2))
    return api_fail(w + "the weight gradient's plan refuses this shape");
  Bump bump(base);
  const size_t n1 = (size_t)di * s.K1 * d * sizeof(unsigned short), n2 = (size_t)d * s.K2 * di * sizeof(unsigned short);
  ws->wp1 = (unsigned short*)bump.raw(n1); ws->wp2 = (unsigned short*)bump.raw(n2);
  ws->wt1 = (unsigned short*)bump.raw(n1); ws->wt2 = (unsigned short*)bump.raw(n2);
  ws->partial = bump.f((size_t)(pl1.ws_floats > pl2.ws_floats ? pl1.ws_floats : pl2.ws_floats));
  ws->colpart = (double*)bump.raw((size_t)nblk * PG_SLOTS * d * sizeof(double));
  ws->gatepart = (double*)bump.raw((size_t)nblk * PG_SLOTS * di * sizeof(double));
  ws->a = bump.f((size_t)M * d); ws->b = bump.f((size_t)M * d);
  ws->wide = bump.f((size_t)M * di);
  *bytes = bump.off;
  return 0;
}

// what ns_fg_forward_bf16 and ns_fg_backward_bf16 check alike, in ffngrad_api.hip's order, and the carved workspace
int common(const std::string& w, const ns_fg_shape* s, const ns_fg_weights* k, const float* x, const uint8_t* keep, float p_drop, const void* saved,
           void* ws_mem, size_t ws_bytes, NamedPtr io, Ws* ws) {
  NS_TRY(check_dims(*s, w));
  NS_TRY(check_weights(params(k->w1, k->b1, k->w2, k->b2, k->ln_g, k->ln_b), w));
  NS_TRY(check_drop({keep}, p_drop, w));
  NS_TRY(check_aligned(w, {{"x", x}, {"saved", saved}, {"the workspace", ws_mem}, io}));
  size_t need = 0;
  NS_TRY(carve(*s, ws_mem, ws, &need, w));
  if (ws_bytes < need) return api_fail(w + "workspace too small (ns_fg_ws_bytes_bf16)");
  return 0;
}

// The two forms of one contraction from a plane of a weight W [N][Cin][KW] (torch layout), as the module and the hook run them.
// forward form: x [M, Cin] -> y [M, N] from wp [N][KW][Cin]
int conv_plane(const float* x, const unsigned short* wp, const float* bias, const float* resid, float* y, int M, int S, int N, int Cin, int KW,
               int act, hipStream_t st) {
  return counted().conv_bf16(x, Cin, wp, bias, resid, y, M, S, N, Cin, KW, (KW - 1) / 2, act, st);
}
// data gradient: x [M, N] -> y [M, Cin] from wt [Cin][KW][N] (transposed, taps flipped), resid added in fp32 in the epilogue
int conv_plane_t(const float* x, const unsigned short* wt, const float* bias, const float* resid, float* y, int M, int S, int N, int Cin, int KW,
                 int act, hipStream_t st) {
  return counted().conv_bf16(x, N, wt, bias, resid, y, M, S, Cin, N, KW, KW - 1 - (KW - 1) / 2, act, st);
}

// dW [N][Cin][KW] from dz [M, N] and X [M, Cin]: the GEMM and its fixed-order reduce, two launches
int wgrad(const float* dz, const float* X, int M, int S, int N, int Cin, int KW, float* partial, float* dW, hipStream_t st) {
  PgWgradPlan pl;
  if (!fg_plan_wgrad_bf16(M, N, Cin, KW, &pl)) return api_fail("ns_fg: the weight gradient's plan refuses this shape");
  NS_HIP(launch_fg_wgrad_bf16(dz, X, M, S, N, Cin, KW, pl, partial, dW, st));
  *launches() += 2;
  return 0;
}

// the shape of a test hook: B * S rows, a weight [N][Cin][KW]
int check_op(int B, int S, int N, int Cin, int KW, const std::string& w) {
  if (B <= 0 || S <= 0) return api_fail(w + "B and S must be positive, got " + std::to_string(B) + " x " + std::to_string(S));
  if (N <= 0 || N % 32 != 0) return api_fail(w + "N must be a positive multiple of 32, got " + std::to_string(N));
  if (Cin <= 0 || Cin % 32 != 0) return api_fail(w + "Cin must be a positive multiple of 32, got " + std::to_string(Cin));
  if (KW <= 0 || KW % 2 == 0) return api_fail(w + "KW must be odd and positive, got " + std::to_string(KW));
  if ((long long)B * S * (N > Cin ? N : Cin) >= (1ll << 31)) return api_fail(w + "problem too large: B * S * max(N, Cin) must stay below 2^31");
  if (2ll * N * KW * Cin >= (1ll << 31)) return api_fail(w + "problem too large: the weight's bf16 plane must stay below 2^31 bytes");
  return 0;
}

// the hooks' workspace: one bf16 plane of the weight, then the weight gradient's partial tiles (none where its plan refuses)
size_t op_carve(int B, int S, int N, int Cin, int KW, void* base, unsigned short** plane, float** partial) {
  Bump bump(base);
  *plane = (unsigned short*)bump.raw((size_t)N * Cin * KW * sizeof(unsigned short));
  PgWgradPlan pl;
  *partial = fg_plan_wgrad_bf16(B * S, N, Cin, KW, &pl) ? bump.f((size_t)pl.ws_floats) : nullptr;
  return bump.off;
}
}  // namespace

extern "C" int ns_fg_plan_wgrad_bf16(int M, int N, int Cin, int KW, int32_t out[8]) {
  if (!out) return api_fail("ns_fg_plan_wgrad_bf16: null argument");
  PgWgradPlan p;
  if (!fg_plan_wgrad_bf16(M, N, Cin, KW, &p))
    return api_fail("ns_fg_plan_wgrad_bf16: refused (M > 0, N a multiple of 128, Cin a multiple of 32, KW odd, sizes below 2^31)");
  out[0] = p.tile_n; out[1] = p.tile_c; out[2] = p.rows; out[3] = p.ranges; out[4] = p.tiles; out[5] = (int32_t)p.ws_floats; out[6] = p.chunk; out[7] = 0;
  return 0;
}

extern "C" size_t ns_fg_ws_bytes_bf16(const ns_fg_shape* s) {
  return size_query("ns_fg_ws_bytes_bf16", s, check_dims, [](const ns_fg_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" int ns_fg_forward_bf16(const ns_fg_shape* s, const ns_fg_weights* k, const float* x, const uint8_t* keep, float p_drop, float* y,
                                  void* saved, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_fg_forward_bf16: ";
  *launches() = 0;
  if (!s || !k || !x || !y || !ws_mem) return api_fail(w + "null argument");
  Ws ws;
  NS_TRY(common(w, s, k, x, keep, p_drop, saved, ws_mem, ws_bytes, {"y", y}, &ws));
  const int M = s->B * s->S, d = s->d, di = s->d_inner;
  float* h = saved ? (float*)saved : ws.wide;
  float* z = saved ? h + (size_t)M * di : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const FgPackBf packs[2] = {{k->w1, ws.wp1, nullptr, di, d, s->K1}, {k->w2, ws.wp2, nullptr, d, di, s->K2}};
  NS_TRY(counted().pack_bf16(packs, 2, st));
  NS_TRY(conv_plane(x, ws.wp1, k->b1, nullptr, h, M, s->S, di, d, s->K1, ACT_RELU, st));
  NS_TRY(conv_plane(h, ws.wp2, k->b2, nullptr, ws.a, M, s->S, d, di, s->K2, ACT_NONE, st));
  NS_HIP(launch_ag_row_forward(ws.a, x, keep, 1.f / (1.f - p_drop), k->ln_g, k->ln_b, z, y, M, d, st));
  ++*launches();
  return 0;
}

extern "C" int ns_fg_backward_bf16(const ns_fg_shape* s, const ns_fg_weights* k, const float* x, const uint8_t* keep, float p_drop,
                                   const void* saved, const float* g, const ns_fg_grads* dg, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_fg_backward_bf16: ";
  *launches() = 0;
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

  NS_HIP(launch_ag_row_backward(ag_row_backward_args(M, d, p_drop, g, z, k->ln_g, keep, dz, du, ws.colpart), st));
  ++*launches();
  if (dg->w2) NS_TRY(wgrad(du, h, M, s->S, d, di, K2, ws.partial, dg->w2, st));
  if (upstream) {
    const FgPackBf packs[2] = {{k->w2, nullptr, ws.wt2, d, di, K2}, {k->w1, nullptr, ws.wt1, di, d, K1}};
    NS_TRY(counted().pack_bf16(packs, dg->dx ? 2 : 1, st));
    NS_TRY(conv_plane_t(du, ws.wt2, nullptr, nullptr, dh, M, s->S, d, di, K2, ACT_NONE, st));
    NS_TRY(relu_gate(dh, h, M, di, dh, dg->b1, ws.gatepart, st));
    if (dg->w1) NS_TRY(wgrad(dh, x, M, s->S, di, d, K1, ws.partial, dg->w1, st));
    if (dg->dx) NS_TRY(conv_plane_t(dh, ws.wt1, nullptr, dz, dg->dx, M, s->S, di, d, K1, ACT_NONE, st));
  }
  return counted().col_finish(ws.colpart, nblk, d, {dg->ln_g, dg->ln_b, dg->b2}, {}, st);
}

extern "C" size_t ns_fg_op_bf16_ws_bytes(int B, int S, int N, int Cin, int KW) {
  if (check_op(B, S, N, Cin, KW, "ns_fg_op_bf16_ws_bytes: ")) return 0;
  unsigned short* plane;
  float* partial;
  return op_carve(B, S, N, Cin, KW, nullptr, &plane, &partial);
}

extern "C" int ns_fg_op_wgrad_bf16(const float* dz, const float* X, int B, int S, int N, int Cin, int KW, float* dW, void* ws_mem, size_t ws_bytes,
                                   void* stream) {
  const std::string w = "ns_fg_op_wgrad_bf16: ";
  *launches() = 0;
  if (!dz || !X || !dW || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_op(B, S, N, Cin, KW, w));
  NS_TRY(check_aligned(w, {{"dz", dz}, {"X", X}, {"dW", dW}, {"the workspace", ws_mem}}));
  PgWgradPlan pl;
  if (!fg_plan_wgrad_bf16(B * S, N, Cin, KW, &pl)) return api_fail(w + "the weight gradient's plan refuses this shape (ns_fg_plan_wgrad_bf16)");
  unsigned short* plane;
  float* partial;
  const size_t need = op_carve(B, S, N, Cin, KW, ws_mem, &plane, &partial);
  if (ws_bytes < need) return api_fail(w + "workspace too small (ns_fg_op_bf16_ws_bytes)");
  return wgrad(dz, X, B * S, S, N, Cin, KW, partial, dW, (hipStream_t)stream);
}

extern "C" int ns_fg_op_conv_bf16(const float* x, const float* W, const float* bias, const float* resid, int B, int S, int N, int Cin, int KW,
                                  int transposed, int act, float* y, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_fg_op_conv_bf16: ";
  *launches() = 0;
  if (!x || !W || !y || !ws_mem) return api_fail(w + "null argument");
  NS_TRY(check_op(B, S, N, Cin, KW, w));
  if (act != ACT_NONE && act != ACT_RELU) return api_fail(w + "act must be 0 (none) or 1 (ReLU), got " + std::to_string(act));
  if (y == x || y == resid) return api_fail(w + "y must not be x or resid");
  NS_TRY(check_aligned(w, {{"x", x}, {"W", W}, {"bias", bias}, {"resid", resid}, {"y", y}, {"the workspace", ws_mem}}));
  const int M = B * S;
  if (!conv_gemm_bf16_ok(M, transposed ? Cin : N, transposed ? N : Cin, KW, EPI_NONE)) return api_fail(w + "the Conv1D-as-GEMM dispatch refuses this shape");
  unsigned short* plane;
  float* partial;
  const size_t need = op_carve(B, S, N, Cin, KW, ws_mem, &plane, &partial);
  if (ws_bytes < need) return api_fail(w + "workspace too small (ns_fg_op_bf16_ws_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const FgPackBf pack = {W, transposed ? nullptr : plane, transposed ? plane : nullptr, N, Cin, KW};
  NS_TRY(counted().pack_bf16(&pack, 1, st));
  if (transposed) return conv_plane_t(x, plane, bias, resid, y, M, S, N, Cin, KW, act, st);
  return conv_plane(x, plane, bias, resid, y, M, S, N, Cin, KW, act, st);
}
