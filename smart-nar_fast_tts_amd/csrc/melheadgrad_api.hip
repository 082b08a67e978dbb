// C-ABI of the mel head, training forward and backward: mel_linear and the PostNet residual (include/nar_fs2.h ns_mh_*;
// model/fastspeech2_align.py:24,83,85).  No handle: the weight is the caller's live tensor in checkpoint
// (nn.Linear) layout, the workspace belongs to the caller, and nothing is saved: the backward needs x and g alone.  Host-side only;
// every argument is validated before the first HIP call.  Every launch but the two of melheadgrad.hip is a kernel the other ABIs
// already run: the Conv1D-as-GEMM dispatch at KW = 1 (forward, data gradient), the predictor's pack kernel, the padded weight
// gradient and the bias finish of the PostNet.  The launch counts are stated in the header.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

static_assert(sizeof(ns_mh_shape) == 16, "ns_mh_shape layout");
static_assert(sizeof(ns_mh_weights) == 2 * sizeof(void*) && sizeof(ns_mh_grads) == 3 * sizeof(void*), "ns_mh_weights / ns_mh_grads layout");

namespace {
thread_local int t_launches = 0;
thread_local const Counted counted{"ns_mh", &t_launches};

struct Ws {  // the workspace of one shape, carved in this order
  float* wt;         // [d][n_mel]: w^T, the data gradient's form
  float* partial;    // the weight gradient's per-range tiles
  float* dwpad;      // [128][d]: the weight gradient at the padded width
  double* biaspart;  // [row blocks][n_mel]
  float* dz;         // [M, 128]: g padded
};

int check_mel(const std::string& w, int n_mel) {
  if (n_mel < 16 || n_mel > PN_PAD_N || n_mel % 16 != 0) return api_fail(w + "n_mel must be a multiple of 16 in [16, 128], got " + std::to_string(n_mel));
  return 0;
}

int check_dims(const ns_mh_shape& s, const std::string& w) {
  if (s.B <= 0 || s.T <= 0) return api_fail(w + "B and T must be positive, got " + std::to_string(s.B) + " x " + std::to_string(s.T));
  if (s.d != 256 && s.d != 512) return api_fail(w + "d must be 256 or 512, got " + std::to_string(s.d));
  NS_TRY(check_mel(w, s.n_mel));
  if ((long long)s.B * s.T * s.d >= (1ll << 31)) return api_fail(w + "problem too large: B * T * d must stay below 2^31");
  return 0;
}

int carve(const ns_mh_shape& s, void* base, Ws* ws, size_t* bytes, const std::string& w) {
  const int M = s.B * s.T, d = s.d, c = s.n_mel;
  int rec[2][8];
  if (conv_gemm_describe(M, c, d, 1, 0, rec) <= 0 || conv_gemm_describe(M, d, c, 1, 0, rec) <= 0)
    return api_fail(w + "the Conv1D-as-GEMM dispatch refuses this shape");
  PgWgradPlan pl;
  if (!pg_plan_wgrad(M, PN_PAD_N, d, 1, &pl)) return api_fail(w + "the weight gradient's plan refuses this shape");
  Bump bump(base);
  ws->wt = bump.f((size_t)d * c);
  ws->partial = bump.f((size_t)pl.ws_floats);
  ws->dwpad = bump.f((size_t)PN_PAD_N * d);
  ws->biaspart = (double*)bump.raw((size_t)pg_row_blocks(M) * c * sizeof(double));
  ws->dz = bump.f((size_t)M * PN_PAD_N);
  *bytes = bump.off;
  return 0;
}

// what ns_mh_forward and ns_mh_backward check alike, in this order, and the carved workspace; `io` names y or g
int common(const std::string& w, const ns_mh_shape* s, const ns_mh_weights* k, const float* x, void* ws_mem, size_t ws_bytes, NamedPtr io, Ws* ws) {
  NS_TRY(check_dims(*s, w));
  NS_TRY(check_weights({{"w", k->w}, {"b", k->b}}, w));
  NS_TRY(check_aligned(w, {{"x", x}, io, {"the workspace", ws_mem}}));
  return carve_checked(carve, counted.abi, *s, ws_mem, ws_bytes, ws, w);
}

// the pad with the column partials and, where d_bias is wanted, their fixed-order sum: one or two launches
int pad_colsum(const float* g, int M, int n_mel, float* dz, float* d_bias, double* part, hipStream_t st) {
  NS_HIP(launch_mh_pad_colsum(g, M, n_mel, dz, d_bias ? part : nullptr, st));
  ++t_launches;
  if (!d_bias) return 0;
  PnBiasFinish bias;
  memset(&bias, 0, sizeof(bias));
  bias.nblk = pg_row_blocks(M); bias.part[0] = part; bias.out[0] = d_bias; bias.C[0] = n_mel;
  NS_HIP(launch_pn_bias_finish(bias, st));
  ++t_launches;
  return 0;
}
}  // namespace

extern "C" int ns_mh_abi_version(void) { return NS_MH_ABI_VERSION; }
extern "C" int ns_mh_last_launches(void) { return t_launches; }

extern "C" size_t ns_mh_ws_bytes(const ns_mh_shape* s) {
  return size_query("ns_mh_ws_bytes", s, check_dims, [](const ns_mh_shape& s, const std::string& w) { return carved_bytes(carve, s, w); });
}

extern "C" int ns_mh_forward(const ns_mh_shape* s, const ns_mh_weights* k, const float* x, float* y, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_mh_forward: ";
  t_launches = 0;
  if (!s || !k || !x || !y || !ws_mem) return api_fail(w + "null argument");
  Ws ws;
  NS_TRY(common(w, s, k, x, ws_mem, ws_bytes, {"y", y}, &ws));
  // at KW = 1 the nn.Linear layout [n_mel][d] is the dispatch's packed form: the live weight is read, no pack launch
  return counted.gemm(x, k->w, k->b, nullptr, y, s->B * s->T, s->T, s->n_mel, s->d, (hipStream_t)stream);
}

extern "C" int ns_mh_backward(const ns_mh_shape* s, const ns_mh_weights* k, const float* x, const float* g, const ns_mh_grads* dg, void* ws_mem,
                              size_t ws_bytes, void* stream) {
  const std::string w = "ns_mh_backward: ";
  t_launches = 0;
  if (!s || !k || !x || !g || !dg || !ws_mem) return api_fail(w + "null argument");
  bool any = false;
  NS_TRY(check_grads({{"dx", dg->dx}, {"w", dg->w}, {"b", dg->b}}, w, &any));
  Ws ws;
  NS_TRY(common(w, s, k, x, ws_mem, ws_bytes, {"g", g}, &ws));
  if (!any) return 0;
  const int M = s->B * s->T, d = s->d, c = s->n_mel;
  hipStream_t st = (hipStream_t)stream;
  if (dg->w || dg->b) NS_TRY(pad_colsum(g, M, c, ws.dz, dg->b, ws.biaspart, st));
  if (dg->w) NS_TRY(counted.wgrad_narrow(ws.dz, x, M, s->T, c, d, 1, ws.partial, ws.dwpad, dg->w, st));
  if (dg->dx) {
    const PgPack pack{k->w, nullptr, ws.wt, c, d, 1};
    NS_TRY(counted.pack(&pack, 1, st));
    NS_TRY(counted.conv(g, c, ws.wt, nullptr, nullptr, dg->dx, M, s->T, d, c, 1, 0, ACT_NONE, st));
  }
  return 0;
}

extern "C" int ns_mh_op_pad_colsum(const float* g, int M, int n_mel, float* dz, float* d_bias, void* ws_mem, size_t ws_bytes, void* stream) {
  const std::string w = "ns_mh_op_pad_colsum: ";
  t_launches = 0;
  if (!g || !dz || (d_bias && !ws_mem)) return api_fail(w + "null argument");
  if (M <= 0) return api_fail(w + "M must be positive, got " + std::to_string(M));
  NS_TRY(check_mel(w, n_mel));
  if ((long long)M * PN_PAD_N >= (1ll << 31)) return api_fail(w + "problem too large: M * 128 must stay below 2^31");
  if (g == dz) return api_fail(w + "dz must not be g (the op is out of place)");
  NS_TRY(check_aligned(w, {{"g", g}, {"dz", dz}, {"d_bias", d_bias}, {"the workspace", ws_mem}}));
  const size_t need = (size_t)pg_row_blocks(M) * n_mel * sizeof(double);
  if (d_bias && ws_bytes < need) return api_fail(w + "workspace too small: " + std::to_string(need) + " bytes needed");
  return pad_colsum(g, M, n_mel, dz, d_bias, (double*)ws_mem, (hipStream_t)stream);
}

extern "C" int ns_mh_op_residual(const float* p, const float* x, int M, int n_mel, float* out, void* stream) {
  const std::string w = "ns_mh_op_residual: ";
  t_launches = 0;
  if (!p || !x || !out) return api_fail(w + "null argument");
  if (M <= 0) return api_fail(w + "M must be positive, got " + std::to_string(M));
  NS_TRY(check_mel(w, n_mel));
  if ((long long)M * n_mel >= (1ll << 31)) return api_fail(w + "problem too large: M * n_mel must stay below 2^31");
  if (out == p || out == x) return api_fail(w + "out must be neither p nor x (the op is out of place)");
  NS_TRY(check_aligned(w, {{"p", p}, {"x", x}, {"out", out}}));
  NS_HIP(launch_mh_residual(p, x, M, n_mel, out, (hipStream_t)stream));
  ++t_launches;
  return 0;
}
