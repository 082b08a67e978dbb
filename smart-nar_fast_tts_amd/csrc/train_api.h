// Host-side helpers shared by the handle-less training ABIs (ns_pg_*, ns_ag_*, ns_xg_*, ns_pn_*, ns_va_*, ns_fg_* in the six *grad_api.hip;
// DESIGN.md section 20): the argument checks whose texts they state alike, the workspace and size-query wrappers, the counted launches
// of the kernels they share (Conv1D-as-GEMM, weight pack, column-partial finish, padded weight gradient) and the row-backward argument blocks.  Host-only, no
// kernels.  Each ABI keeps its own thread-local launch counter and hands it in as a Counted; what differs between the layers
// (check_dims, Ws, carve, the forward and backward bodies) stays with the layer.
#pragma once
#include <initializer_list>

#include "host_core.h"

namespace ns {

inline bool misaligned(const void* p, int align = 16) { return ((uintptr_t)p & (uintptr_t)(align - 1)) != 0; }

// one pointer an entry point takes or one field of a weights or grads block: its name in the header, the pointer, the alignment its
// readers need (a float scalar: 4, an int64: 8)
struct NamedPtr { const char* name; const void* p; int align = 16; };

// null passes: whether a pointer may be null is the entry point's own check
inline int check_aligned(const std::string& w, std::initializer_list<NamedPtr> t) {
  for (const NamedPtr& e : t)
    if (misaligned(e.p, e.align)) return api_fail(w + e.name + " must be " + std::to_string(e.align) + "-byte aligned");
  return 0;
}

// p_drop and the n keep-masks of an entry point; keep == nullptr = none of them given; `all` is how a refusal calls the n masks
inline int check_drop(const uint8_t* const* keep, int n, float p, const std::string& w, const char* all = "all n keep-masks") {
  bool every = keep != nullptr, any = false, skew = false;
  for (int i = 0; keep && i < n; ++i) { every = every && keep[i]; any = any || keep[i]; skew = skew || misaligned(keep[i]); }
  if (!(p >= 0.f && p < 1.f)) return api_fail(w + "p_drop must lie in [0, 1)");
  if (p > 0.f && !every) return api_fail(w + "p_drop > 0 needs " + all);
  if (p == 0.f && any) return api_fail(w + (n == 1 ? "keep-mask" : "keep-masks") + " given although p_drop == 0");
  if (skew) return api_fail(w + (n == 1 ? "the keep-mask" : "keep-masks") + " must be 16-byte aligned");
  return 0;
}
// an entry point that takes one or two masks as arguments of their own
inline int check_drop(std::initializer_list<const uint8_t*> keep, float p, const std::string& w) {
  return check_drop(keep.begin(), (int)keep.size(), p, w, keep.size() > 1 ? "both keep-masks" : "a keep-mask");
}

// `prefix` names the sub-block the fields sit in ("layer[2].")
inline int check_weights(const std::vector<NamedPtr>& t, const std::string& w, const std::string& prefix = "") {
  for (const NamedPtr& e : t) {
    if (!e.p) return api_fail(w + "null weights->" + prefix + e.name);
    if (misaligned(e.p, e.align)) return api_fail(w + "weights->" + prefix + e.name + " must be " + std::to_string(e.align) + "-byte aligned");
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

// the ten parameters of an attention-shaped weights or grads block (ns_ag_*, ns_xg_*), in ABI order
template <class T>
std::vector<NamedPtr> attn_params(const T& k) {
  return {{"wq", k.wq}, {"bq", k.bq}, {"wk", k.wk}, {"bk", k.bk}, {"wv", k.wv}, {"bv", k.bv}, {"wfc", k.wfc}, {"bfc", k.bfc}, {"ln_g", k.ln_g},
          {"ln_b", k.ln_b}};
}

// the layer's carve over the caller's workspace, refused where that is smaller than the layout
template <class Shape, class Ws>
int carve_checked(int (*carve)(const Shape&, void*, Ws*, size_t*, const std::string&), const char* abi, const Shape& s, void* ws_mem, size_t ws_bytes,
                  Ws* ws, const std::string& w) {
  size_t need = 0;
  NS_TRY(carve(s, ws_mem, ws, &need, w));
  if (ws_bytes < need) return api_fail(w + "workspace too small (" + abi + "_ws_bytes)");
  return 0;
}

// the bytes of the layout the layer's carve makes for s; 0 where it refuses
template <class Shape, class Ws>
size_t carved_bytes(int (*carve)(const Shape&, void*, Ws*, size_t*, const std::string&), const Shape& s, const std::string& w) {
  Ws ws;
  size_t bytes = 0;
  return carve(s, nullptr, &ws, &bytes, w) ? 0 : bytes;
}

// the body of an ns_*_ws_bytes / ns_*_saved_bytes: a null or refused shape (check(*s, w), the layer's check_dims) gives 0, else size(*s, w)
template <class Shape, class Check, class Size>
size_t size_query(const char* who, const Shape* s, Check check, Size size) {
  const std::string w = std::string(who) + ": ";
  if (!s) { api_fail(w + "null argument"); return 0; }
  if (check(*s, w)) return 0;
  return size(*s, w);
}

// The launches the layers share, counted into the calling ABI's own thread-local counter.
struct Counted {
  const char* abi;  // "ns_pg": named in a refusal
  int* launches;

  // Y [M, N] = act(conv(X [M, Cin] at row stride ldx, W packed [N][KW * Cin]) + bias) + resid, plain epilogue, through the forward's
  // dispatch; adds the launches the dispatch makes for this shape
  int conv(const float* X, int ldx, const float* W, const float* bias, const float* resid, float* Y, int M, int S, int N, int Cin, int KW, int pad,
           int act, hipStream_t st) const {
    ConvGemm p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.ldx = ldx; p.W = W; p.bias = bias; p.resid = resid; p.ldr = N; p.Y = Y; p.ldy = N;
    p.M = M; p.N = N; p.Cin = Cin; p.KW = KW; p.pad = pad; p.S = S; p.act = act; p.epi = EPI_NONE;
    int rec[2][8];
    const int n = conv_gemm_describe(M, N, Cin, KW, 0, rec);
    if (n <= 0) return api_fail(std::string(abi) + ": the Conv1D-as-GEMM dispatch refuses this shape");
    NS_HIP(launch_conv_gemm(p, st));
    *launches += n;
    return 0;
  }

  // the same contraction from the bf16 plane Wbf [N][KW][Cin] (k_fg_pack_bf16) with X rounded to bf16 in the kernel and fp32
  // accumulation (gemm_bf16.hip): the "bf16" matmul mode's sibling of conv.  Bias, activation and residual stay fp32, in the
  // kernel's own plain epilogue.  Always one launch.
  int conv_bf16(const float* X, int ldx, const unsigned short* Wbf, const float* bias, const float* resid, float* Y, int M, int S, int N, int Cin,
                int KW, int pad, int act, hipStream_t st) const {
    ConvGemm p;
    memset(&p, 0, sizeof(p));
    p.X = X; p.ldx = ldx; p.Wbf = Wbf; p.bias = bias; p.resid = resid; p.ldr = N; p.Y = Y; p.ldy = N;
    p.M = M; p.N = N; p.Cin = Cin; p.KW = KW; p.pad = pad; p.S = S; p.act = act; p.epi = EPI_NONE;
    if (!conv_gemm_bf16_ok(M, N, Cin, KW, EPI_NONE)) return api_fail(std::string(abi) + ": the bf16 Conv1D-as-GEMM refuses this shape");
    NS_HIP(launch_conv_gemm_bf16(p, st));
    ++*launches;
    return 0;
  }

  // k_fg_pack_bf16 over `count` weights, two per launch
  int pack_bf16(const FgPackBf* v, int count, hipStream_t st) const {
    const FgPackBf none{nullptr, nullptr, nullptr, 0, 0, 0};
    for (int i = 0; i < count; i += 2) {
      NS_HIP(launch_fg_pack_bf16(v[i], i + 1 < count ? v[i + 1] : none, st));
      ++*launches;
    }
    return 0;
  }

  // Y [M, N] = X [M, K] W[N][K]^T + bias + resid: the same at KW = 1
  int gemm(const float* X, const float* W, const float* bias, const float* resid, float* Y, int M, int S, int N, int K, hipStream_t st) const {
    return conv(X, K, W, bias, resid, Y, M, S, N, K, 1, 0, ACT_NONE, st);
  }

  // k_pg_pack over `count` weights, two per launch
  int pack(const PgPack* v, int count, hipStream_t st) const {
    const PgPack none{nullptr, nullptr, nullptr, 0, 0, 0};
    for (int i = 0; i < count; i += 2) {
      NS_HIP(launch_pg_pack(v[i], i + 1 < count ? v[i + 1] : none, st));
      ++*launches;
    }
    return 0;
  }

  // the fixed-order sum of the column partials into the slots of stage 0 and stage 1 (k_pg_col_final): one launch, made and counted
  // only when an output is wanted
  int col_finish(const double* part, int nblk, int F, std::initializer_list<float*> stage0, std::initializer_list<float*> stage1,
                 hipStream_t st) const {
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

  // the weight gradient at the padded width: dz [M, 128] with zero columns [N, 128) -> dwpad [128][Cin][KW] -> dW = its first N rows
  // (PostNet's last layer, mel_linear): the GEMM, its fixed-order reduce and the copy, three launches
  int wgrad_narrow(const float* dz, const float* X, int M, int S, int N, int Cin, int KW, float* partial, float* dwpad, float* dW,
                   hipStream_t st) const {
    PgWgradPlan pl;
    if (!pg_plan_wgrad(M, PN_PAD_N, Cin, KW, &pl)) return api_fail(std::string(abi) + ": the weight gradient's plan refuses this shape");
    NS_HIP(launch_pg_wgrad(dz, X, M, S, PN_PAD_N, Cin, KW, pl, partial, dwpad, st, PN_PAD_N));
    NS_HIP(launch_pn_copy(dwpad, dW, (long long)N * Cin * KW, st));
    *launches += 3;
    return 0;
  }
};

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
