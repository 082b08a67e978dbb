// C-ABI of the VarianceAdaptor's training pieces (include/nar_fs2.h ns_va_*; model/modules.py:17-159, 195-230).  No handle: every
// tensor is the caller's.  Host-side only; every argument is validated before the first HIP call.  The length regulator's gather is the
// forward's own kernel (launch_length_regulate), unchanged.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

namespace {
thread_local int t_launches = 0;

int check_rows(const std::string& w, const char* rows, long long n, int D) {
  if (D <= 0 || D % 4 != 0) return api_fail(w + "D must be a positive multiple of 4, got " + std::to_string(D));
  if (n * D >= (1ll << 31)) return api_fail(w + "problem too large: " + rows + " * D must stay below 2^31");
  return 0;
}

int check_embed(const std::string& w, int M, int D, int n_bins, VaEmbedPlan* plan) {
  if (M <= 0) return api_fail(w + "M must be positive, got " + std::to_string(M));
  if (n_bins < 2) return api_fail(w + "n_bins must be at least 2, got " + std::to_string(n_bins));
  NS_TRY(check_rows(w, "M", M, D));
  if (!va_plan_embed(M, D, n_bins, plan))
    return api_fail(w + "the embedding gradient's plan cannot hold this shape: an n_bins x 4 float64 table past " + std::to_string(VA_LDS_LIMIT) +
                    " bytes of LDS, or more than 65535 column slabs (n_bins " + std::to_string(n_bins) + ", D " + std::to_string(D) + ")");
  return 0;
}

int check_lr(const std::string& w, int B, int L, int D, int T, bool need_T) {
  if (B <= 0 || L <= 0) return api_fail(w + "B and L must be positive, got " + std::to_string(B) + " x " + std::to_string(L));
  if (need_T && T <= 0) return api_fail(w + "T must be positive, got " + std::to_string(T));
  if ((long long)B * L >= (1ll << 31)) return api_fail(w + "problem too large: B * L must stay below 2^31");
  NS_TRY(check_rows(w, "B * L", (long long)B * L, D));
  if (need_T) NS_TRY(check_rows(w, "B * T", (long long)B * T, D));
  return 0;
}
}  // namespace

int& ns::va_launch_counter() { return t_launches; }  // gaussgrad_api.hip books its launches here

extern "C" int ns_va_abi_version(void) { return NS_VA_ABI_VERSION; }
extern "C" int ns_va_last_launches(void) { return t_launches; }

extern "C" int ns_va_plan_embed(int M, int D, int n_bins, int32_t out[8]) {
  const std::string w = "ns_va_plan_embed: ";
  if (out) for (int i = 0; i < 8; ++i) out[i] = 0;
  VaEmbedPlan p;
  NS_TRY(check_embed(w, M, D, n_bins, &p));
  if (out) {
    out[0] = p.row_blocks; out[1] = p.rows_per_block; out[2] = p.slab; out[3] = p.n_slabs; out[4] = p.lds_bytes; out[5] = p.launches; out[6] = 64;
  }
  return 0;
}

extern "C" size_t ns_va_embed_ws_bytes(int M, int D, int n_bins) {
  VaEmbedPlan p;
  if (check_embed("ns_va_embed_ws_bytes: ", M, D, n_bins, &p)) return 0;
  return (size_t)p.ws_bytes;
}

extern "C" int ns_va_op_embed_fwd(const float* x, const float* target, const float* bins, const float* table, int M, int D, int n_bins, float* y,
                                  int32_t* idx, void* stream) {
  const std::string w = "ns_va_op_embed_fwd: ";
  t_launches = 0;
  if (!x || !target || !bins || !table || !y || !idx) return api_fail(w + "null argument");
  VaEmbedPlan p;
  NS_TRY(check_embed(w, M, D, n_bins, &p));
  NS_TRY(check_aligned(w, {{"x", x}, {"table", table}, {"y", y}, {"target", target, 4}, {"bins", bins, 4}, {"idx", idx, 4}}));
  NS_HIP(launch_va_embed_fwd(x, target, bins, table, M, D, n_bins, y, idx, (hipStream_t)stream));
  ++t_launches;
  return 0;
}

extern "C" int ns_va_op_embed_bwd(const float* g, const int32_t* idx, int M, int D, int n_bins, float* d_table, void* ws_mem, size_t ws_bytes,
                                  void* stream) {
  const std::string w = "ns_va_op_embed_bwd: ";
  t_launches = 0;
  if (!g || !idx || !d_table || !ws_mem) return api_fail(w + "null argument");
  VaEmbedPlan p;
  NS_TRY(check_embed(w, M, D, n_bins, &p));
  NS_TRY(check_aligned(w, {{"g", g}, {"d_table", d_table}, {"the workspace", ws_mem}, {"idx", idx, 4}}));
  if (ws_bytes < (size_t)p.ws_bytes) return api_fail(w + "workspace too small (ns_va_embed_ws_bytes): " + std::to_string(p.ws_bytes) + " bytes needed");
  NS_HIP(launch_va_embed_bwd(g, idx, M, D, n_bins, p, (double*)ws_mem, d_table, (hipStream_t)stream));
  t_launches += p.launches;
  return 0;
}

extern "C" int ns_va_op_lr_fwd(const float* x, const int64_t* duration, int B, int L, int D, int T, float* out, int32_t* cum, int64_t* mel_len,
                               void* stream) {
  const std::string w = "ns_va_op_lr_fwd: ";
  t_launches = 0;
  if (!cum || (!duration && !out) || (duration && !mel_len) || (out && !x)) return api_fail(w + "null argument");
  NS_TRY(check_lr(w, B, L, D, T, out != nullptr));
  NS_TRY(check_aligned(w, {{"x", x}, {"out", out}, {"duration", duration, 8}, {"mel_len", mel_len, 8}, {"cum", cum, 4}}));
  hipStream_t st = (hipStream_t)stream;
  if (duration) {
    NS_HIP(launch_va_duration_scan((const long long*)duration, B, L, cum, (long long*)mel_len, st));
    ++t_launches;
  }
  if (out) {
    NS_HIP(launch_length_regulate(x, cum, B, L, D, T, out, nullptr, nullptr, nullptr, nullptr, 0, st));
    ++t_launches;
  }
  return 0;
}

extern "C" int ns_va_op_lr_bwd(const float* g, const int32_t* cum, int B, int L, int D, int T, float* d_x, void* stream) {
  const std::string w = "ns_va_op_lr_bwd: ";
  t_launches = 0;
  if (!g || !cum || !d_x) return api_fail(w + "null argument");
  NS_TRY(check_lr(w, B, L, D, T, true));
  NS_TRY(check_aligned(w, {{"g", g}, {"d_x", d_x}, {"cum", cum, 4}}));
  NS_HIP(launch_va_lr_bwd(g, cum, B, L, D, T, d_x, (hipStream_t)stream));
  ++t_launches;
  return 0;
}
