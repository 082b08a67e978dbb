// C-ABI of the Gaussian length regulator's training side (include/nar_fs2.h ns_va_gu_* / ns_va_op_gu_*; model/modules.py:162-192;
// DESIGN.md section 37): additions to the ns_va_* family, booked in its launch counter.  No handle: every tensor is the caller's.
// Host-side only; every argument is validated before the first HIP call.  The forward is the inference side's own launch
// (launch_gaussian_upsampling with own_len), unchanged.
#include "../../include/nar_fs2.h"
#include "train_api.h"

using namespace ns;

namespace {
constexpr long long GU_MAX_T = 1ll << 20;  // below it the fp32 centres of integer durations are exact

size_t up(size_t n, size_t a) { return (n + a - 1) / a * a; }

int check_gu(const std::string& w, int B, int L, int D, int T, bool need_T) {
  if (B <= 0 || L <= 0) return api_fail(w + "B and L must be positive, got " + std::to_string(B) + " x " + std::to_string(L));
  if (B > 65535) return api_fail(w + "B must stay below 65536, got " + std::to_string(B));
  if (need_T && T <= 0) return api_fail(w + "T must be positive, got " + std::to_string(T));
  if (need_T && T >= GU_MAX_T) return api_fail(w + "T must stay below 2^20, got " + std::to_string(T));
  if (D <= 0 || D % 4 != 0) return api_fail(w + "D must be a positive multiple of 4, got " + std::to_string(D));
  if ((long long)B * L * D >= (1ll << 31)) return api_fail(w + "problem too large: B * L * D must stay below 2^31");
  if (need_T && (long long)B * T * D >= (1ll << 31)) return api_fail(w + "problem too large: B * T * D must stay below 2^31");
  return 0;
}

// forward: the fp32 durations [B, L], then the forward launch's scratch (B sums, B L centres); backward: S [B, T]
size_t fwd_s_offset(int B, int L) { return up((size_t)B * L * sizeof(float), 16); }
size_t ws_need(int B, int L, int T) {
  const size_t fwd = fwd_s_offset(B, L) + ((size_t)B + (size_t)B * L) * sizeof(float), bwd = (size_t)B * T * sizeof(float);
  return up(fwd > bwd ? fwd : bwd, 256);
}

int gu_bwd(const char* who, const float* g, const float* saved, const int64_t* own_len, int B, int L, int D, int T, float* d_x, float* w_out,
           void* ws, size_t ws_bytes, void* stream, bool band) {
  const std::string w = std::string(who) + ": ";
  int& launches = va_launch_counter();
  launches = 0;
  if (!g || !saved || !d_x || !ws) return api_fail(w + "null argument");
  NS_TRY(check_gu(w, B, L, D, T, true));
  if (w_out && (long long)B * L * T >= (1ll << 31)) return api_fail(w + "problem too large: B * L * T must stay below 2^31 with w_out");
  NS_TRY(check_aligned(w, {{"g", g}, {"saved", saved}, {"d_x", d_x}, {"w_out", w_out}, {"the workspace", ws}, {"own_len", own_len, 8}}));
  if (ws_bytes < ws_need(B, L, T)) return api_fail(w + "workspace too small (ns_va_gu_ws_bytes): " + std::to_string(ws_need(B, L, T)) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  NS_HIP(launch_gu_denominators(saved, (const long long*)own_len, B, L, T, (float*)ws, st));
  ++launches;
  NS_HIP(launch_gu_bwd(g, saved, (const float*)ws, (const long long*)own_len, B, L, D, T, band, d_x, w_out, st));
  ++launches;
  return 0;
}
}  // namespace

extern "C" size_t ns_va_gu_ws_bytes(int B, int L, int T) {
  if (check_gu("ns_va_gu_ws_bytes: ", B, L, 4, T, true)) return 0;
  return ws_need(B, L, T);
}

extern "C" int ns_va_op_gu_fwd(const float* x, const int64_t* duration, int B, int L, int D, int T, float* out, float* saved, int64_t* mel_len,
                               void* ws, size_t ws_bytes, void* stream) {
  const std::string w = "ns_va_op_gu_fwd: ";
  int& launches = va_launch_counter();
  launches = 0;
  if (!duration || !saved || !mel_len || !ws || (out && !x)) return api_fail(w + "null argument");
  NS_TRY(check_gu(w, B, L, D, T, out != nullptr));
  NS_TRY(check_aligned(w, {{"x", x}, {"out", out}, {"saved", saved}, {"the workspace", ws}, {"duration", duration, 8}, {"mel_len", mel_len, 8}}));
  if (ws_bytes < ws_need(B, L, out ? T : 1))
    return api_fail(w + "workspace too small (ns_va_gu_ws_bytes): " + std::to_string(ws_need(B, L, out ? T : 1)) + " bytes needed");
  hipStream_t st = (hipStream_t)stream;
  float* dur_f = (float*)ws;
  float* s = (float*)((char*)ws + fwd_s_offset(B, L));
  NS_HIP(launch_gu_prepare((const long long*)duration, B, L, dur_f, saved, (long long*)mel_len, st));
  ++launches;
  if (!out) return 0;
  // the launch ns_forward_mel makes on the dense grid (ns_op_gaussian_regulate's dense form): T_out = T, own_len = the totals
  NS_HIP(launch_gaussian_upsampling(x, dur_f, B, L, D, T, T, out, s, nullptr, (const long long*)mel_len, nullptr, nullptr, 0, st));
  launches += 2;
  return 0;
}

extern "C" int ns_va_op_gu_bwd(const float* g, const float* saved, const int64_t* own_len, int B, int L, int D, int T, float* d_x, float* w_out,
                               void* ws, size_t ws_bytes, void* stream) {
  return gu_bwd("ns_va_op_gu_bwd", g, saved, own_len, B, L, D, T, d_x, w_out, ws, ws_bytes, stream, true);
}

extern "C" int ns_va_op_gu_bwd_unbanded(const float* g, const float* saved, const int64_t* own_len, int B, int L, int D, int T, float* d_x,
                                        float* w_out, void* ws, size_t ws_bytes, void* stream) {
  return gu_bwd("ns_va_op_gu_bwd_unbanded", g, saved, own_len, B, L, D, T, d_x, w_out, ws, ws_bytes, stream, false);
}
