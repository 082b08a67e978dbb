// Host-side helpers shared by the handle-less training ABIs (predgrad_api.hip ns_pg_*, attngrad_api.hip ns_ag_*):
// the argument checks whose texts the two state alike, the counted Conv1D-as-GEMM launch, the column-partial finish and the
// row-backward argument blocks.  Host-only, no kernels.  Each ABI keeps its own thread-local launch counter and passes it in; what
// differs between the layers (check_dims, Ws, carve) stays with the layer.
#pragma once
#include <initializer_list>

#include "host_core.h"

namespace ns {

inline bool misaligned(const void* p, int align = 16) { return ((uintptr_t)p & (uintptr_t)(align - 1)) != 0; }

// p_drop and the keep-masks of an entry point that takes one or two of them
inline int check_drop(std::initializer_list<const uint8_t*> keep, float p, const std::string& w) {
  const bool two = keep.size() > 1;
  bool all = true, any = false, skew = false;
  for (const uint8_t* k : keep) { all = all && k; any = any || k; skew = skew || misaligned(k); }
  if (!(p >= 0.f && p < 1.f)) return api_fail(w + "p_drop must lie in [0, 1)");
  if (p > 0.f && !all) return api_fail(w + (two ? "p_drop > 0 needs both keep-masks" : "p_drop > 0 needs a keep-mask"));
  if (p == 0.f && any) return api_fail(w + (two ? "keep-masks given although p_drop == 0" : "keep-mask given although p_drop == 0"));
  if (skew) return api_fail(w + (two ? "keep-masks must be 16-byte aligned" : "the keep-mask must be 16-byte aligned"));
  return 0;
}

// one field of a weights or grads block: its name in the header, its pointer, the alignment its readers need (a scalar: 4)
struct NamedPtr { const char* name; const void* p; int align = 16; };

inline int check_weights(const std::vector<NamedPtr>& t, const std::string& w) {
  for (const NamedPtr& e : t) {
    if (!e.p) return api_fail(w + "null weights->" + e.name);
    if (misaligned(e.p, e.align)) return api_fail(w + "weights->" + e.name + " must be 16-byte aligned");
  }
  return 0;
}

// gradient outputs: null = not wanted; *wanted: whether any is
inline int check_grads(const std::vector<NamedPtr>& t, const std::string& w, bool* wanted = nullptr) {
  bool any = false;
  for (const NamedPtr& e : t) {
    if (misaligned(e.p, e.align)) return api_fail(w + "every gradient must be 16-byte aligned");
    any = any || e.p;
  }
  if (wanted) *wanted = any;
  return 0;
}

// Y [M, N] = act(conv(X [M, Cin], W packed [N][KW * Cin]) + bias), dense operands, plain epilogue; a caller adds what else it needs
inline ConvGemm conv_gemm_args(const float* X, const float* W, const float* bias, float* Y, int M, int S, int N, int Cin, int KW, int pad, int act) {
  ConvGemm p;
  memset(&p, 0, sizeof(p));
  p.X = X; p.ldx = Cin; p.W = W; p.bias = bias; p.Y = Y; p.ldy = N;
  p.M = M; p.N = N; p.Cin = Cin; p.KW = KW; p.pad = pad; p.S = S; p.act = act; p.epi = EPI_NONE;
  return p;
}

// launch_conv_gemm through the forward's dispatch; adds the launches the dispatch makes for this shape to *launches
inline int counted_conv_gemm(const ConvGemm& p, const char* abi, int* launches, hipStream_t st) {
  int rec[2][8];
  const int n = conv_gemm_describe(p.M, p.N, p.Cin, p.KW, 0, rec);
  if (n <= 0) return api_fail(std::string(abi) + ": the Conv1D-as-GEMM dispatch refuses this shape");
  NS_HIP(launch_conv_gemm(p, st));
  *launches += n;
  return 0;
}

// the fixed-order sum of the column partials into the slots of stage 0 and stage 1 (k_pg_col_final): one launch, made and counted
// only when an output is wanted
inline int col_finish(const double* part, int nblk, int F, std::initializer_list<float*> stage0, std::initializer_list<float*> stage1,
                      int* launches, hipStream_t st) {
  PgColFinal fin;
  memset(&fin, 0, sizeof(fin));
  bool any = false;
  int i = 0;
  for (float* o : stage0) { fin.out[i++] = o; any = any || o; }
  i = PG_SLOTS;
  for (float* o : stage1) { fin.out[i++] = o; any = any || o; }
  if (!any) return 0;
  NS_HIP(launch_pg_col_final(part, nblk, F, fin, st));
  ++*launches;
  return 0;
}

inline PgRowBackward pg_row_backward_args(int tail, int M, int F, float p_drop, const float* dy, const float* g, const uint8_t* mask, const float* v,
                                          const float* ln_g, const float* ln_b, const float* wlin, const uint8_t* keep, float* dz, double* part) {
  PgRowBackward r;
  memset(&r, 0, sizeof(r));
  r.tail = tail != 0; r.M = M; r.F = F; r.scale = 1.f / (1.f - p_drop); r.dy = dy; r.g = g; r.mask = mask; r.v = v;
  r.ln_g = ln_g; r.ln_b = ln_b; r.wlin = wlin; r.keep = keep; r.dz = dz; r.part = part;
  return r;
}

inline AgRowBackward ag_row_backward_args(int M, int F, float p_drop, const float* dy, const float* z, const float* ln_g, const uint8_t* keep,
                                          float* dz, float* du, double* part) {
  AgRowBackward r;
  memset(&r, 0, sizeof(r));
  r.M = M; r.F = F; r.scale = 1.f / (1.f - p_drop); r.dy = dy; r.z = z; r.ln_g = ln_g; r.keep = keep; r.dz = dz; r.du = du; r.part = part;
  return r;
}

}  // namespace ns
