// Host-side core shared by the three C-ABI handles (api.hip ns_model, vocoder_api.hip ns_vocoder, aligner_api.hip ns_aligner):
// error macros, the weight registry, arena / workspace carving, weight packing, the ticket cursor and the fp32 GEMM + LayerNorm
// ladder.  Host-only, no kernels; policy that differs between the handles (ignored keys, message texts) stays with the handle.
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"

namespace ns {

// every handle reports through one thread-local slot (api.hip: ns::api_fail, ns_last_error)
inline int api_fail(const std::string& s) { return api_fail(s.c_str()); }
#define NS_HIP(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return ns::api_fail(std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)
#define NS_TRY(expr)              \
  do {                            \
    int rc_ = (expr);             \
    if (rc_) return rc_;          \
  } while (0)

// ------------------------------------------------------------------------------------------- weight registry
// The state-dict entries a handle expects (reference key names, torch-native shapes) and their staged host copies between
// *_set_weight and *_finalize_weights.  `who` is the C-ABI entry point the error texts name.
struct Staged { std::vector<int64_t> shape; std::vector<float> data; bool set = false; bool optional = false; };

class WeightRegistry {
  std::map<std::string, Staged> entries;

 public:
  void expect(const std::string& name, std::vector<int64_t> shape, bool optional = false) {
    Staged& s = entries[name];
    s.shape = std::move(shape);
    s.optional = optional;
  }
  // name / rank / shape validation shared by *_check_weight (no side effect) and set()
  int lookup(const char* name, const int64_t* shape, int ndim, const char* who, Staged** slot, size_t* count) {
    auto it = entries.find(name);
    if (it == entries.end()) return api_fail(std::string(who) + ": unexpected key '" + name + "'");
    Staged& s = it->second;
    if ((int)s.shape.size() != ndim) return api_fail(std::string(who) + ": rank mismatch for '" + name + "'");
    if (ndim > 0 && !shape) return api_fail(std::string(who) + ": null shape for '" + name + "'");
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      if (shape[i] != s.shape[i]) {
        return api_fail(std::string(who) + ": size mismatch for '" + name + "': dim " + std::to_string(i) + " is " +
                        std::to_string(shape[i]) + ", expected " + std::to_string(s.shape[i]));
      }
      n *= (size_t)shape[i];
    }
    *slot = &s;
    *count = n;
    return 0;
  }
  int set(const char* name, const float* host, const int64_t* shape, int ndim, const char* who) {
    Staged* s; size_t n;
    NS_TRY(lookup(name, shape, ndim, who, &s, &n));
    if (!host) return api_fail(std::string(who) + ": null data for '" + name + "'");
    s->data.assign(host, host + n);
    s->set = true;
    return 0;
  }
  std::vector<std::string> missing() const {  // required entries nobody set, in key order
    std::vector<std::string> names;
    for (auto& kv : entries)
      if (!kv.second.set && !kv.second.optional) names.push_back(kv.first);
    return names;
  }
  bool is_set(const std::string& name) const { return entries.at(name).set; }
  const std::vector<float>& data(const std::string& name) const { return entries.at(name).data; }
  // frees the staged host copies and forgets that they were set: the next *_finalize_weights needs every key staged again
  void release() {
    for (auto& kv : entries) { kv.second.data.clear(); kv.second.data.shrink_to_fit(); kv.second.set = false; }
  }
};

inline std::string join_names(const std::vector<std::string>& names) {
  std::string s;
  for (auto& n : names) s += (s.empty() ? "" : ", ") + n;
  return s;
}

// *_check_weight / *_set_weight of a handle H {WeightRegistry weights; bool ready;}
template <class H>
int check_weight(H* h, const char* name, const int64_t* shape, int ndim, const char* who) {
  if (!h || !name) return api_fail(std::string(who) + ": null argument");
  Staged* s; size_t n;
  return h->weights.lookup(name, shape, ndim, who, &s, &n);
}
template <class H>
int set_weight(H* h, const char* name, const float* host, const int64_t* shape, int ndim, const char* who) {
  if (!h || !name) return api_fail(std::string(who) + ": null argument");
  NS_TRY(h->weights.set(name, host, shape, ndim, who));
  h->ready = false;
  return 0;
}

// ------------------------------------------------------------------------------------------- memory carving
inline size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }  // floats: 256-byte aligned offsets

// One Conv1d / Linear weight in an arena (float offsets): packed fp32 [cout][kw * cin] at w, bias [cout] at b.  b3: the same
// weights as three bf16 planes (the "bf16x3" mode), bf: as one rounded bf16 plane (the "bf16" mode); NO_PLANE = absent.
constexpr size_t NO_PLANE = (size_t)-1;
struct ConvW {
  size_t w = 0, b = 0, b3 = NO_PLANE, bf = NO_PLANE;
  int cout = 0, kw = 0, cin = 0;
  size_t elems() const { return (size_t)cout * kw * cin; }
  ConvW fp32() const { ConvW c = *this; c.b3 = c.bf = NO_PLANE; return c; }  // the same weight on the exact-fp32 kernels
};

struct Arena {  // weight offsets of a handle, in floats
  size_t n = 0;
  size_t take(size_t floats) { size_t o = n; n += align64(floats); return o; }
  // fp32 weight and bias only: a handle with planes takes them afterwards, where its arena layout has them
  ConvW conv(int cout, int kw, int cin) {
    ConvW c;
    c.cout = cout; c.kw = kw; c.cin = cin;
    c.w = take(c.elems()); c.b = take(cout);
    return c;
  }
};

// *_bind_arena of a handle H {float* arena; bool ready;}: `need` = the handle's *_arena_bytes
template <class H>
int bind_arena(H* h, void* dev, size_t bytes, size_t need, const char* who, const char* too_small = "arena too small") {
  if (!h || !dev) return api_fail(std::string(who) + ": null argument");
  if (bytes < need) return api_fail(std::string(who) + ": " + too_small);
  if ((uintptr_t)dev & 255) return api_fail(std::string(who) + ": arena must be 256-byte aligned");
  h->arena = (float*)dev;
  h->ready = false;
  return 0;
}

struct Bump {  // workspace carving, 256-byte steps; a null base only measures (the *_ws_bytes queries)
  char* base; size_t off = 0;
  explicit Bump(void* p) : base((char*)p) {}
  float* f(size_t n) { return (float*)raw(n * sizeof(float)); }
  void* raw(size_t bytes) {
    size_t o = off; off += (bytes + 255) & ~(size_t)255;
    return base ? base + o : nullptr;
  }
};

// conv weight [out][in][k] (torch) -> [out][k][in] (tap-major K for the implicit GEMM), optional per-out scale
inline void pack_conv(const std::vector<float>& w, int cout, int cin, int k, float* dst, const double* scale = nullptr) {
  for (int o = 0; o < cout; ++o)
    for (int c = 0; c < cin; ++c)
      for (int j = 0; j < k; ++j) {
        double v = w[((size_t)o * cin + c) * k + j];
        if (scale) v *= scale[o];
        dst[((size_t)o * k + j) * cin + c] = (float)v;
      }
}

inline void host_sinusoid(int n_pos, int d, float* dst) {  // transformer/Models.py:10-30
  for (int p = 0; p < n_pos; ++p)
    for (int j = 0; j < d; ++j) {
      const double ang = (double)p / std::pow(10000.0, (double)(2 * (j / 2)) / (double)d);
      dst[(size_t)p * d + j] = (float)((j & 1) ? std::cos(ang) : std::sin(ang));
    }
}

// ------------------------------------------------------------------------------------------- tickets
// ticket counters of one forward phase (gemm_conv.hip TICKET, attention.hip): zeroed as a block by the phase's first kernel,
// every ticketed launch then takes its own slice — no reset, no reuse inside a phase
constexpr int TICKET_INTS = 16384;

struct Tickets {
  int* base; int used;  // base == nullptr: disabled ("two_launch")
  int* take(int n) {    // nullptr when the block is spent or disabled (the caller then takes the two-launch form)
    if (!base || used + n > TICKET_INTS) return nullptr;
    int* t = base + used;
    used += n;
    return t;
  }
};

// ------------------------------------------------------------------------------------------- GEMM + LayerNorm, fp32
// A GEMM whose N columns are one whole activation row can run the row's LayerNorm in its epilogue (kernels.h
// RowEpilogue).  The full-row tile is at least 32 rows tall (48 / 80 / 112 between the steps: gemm_conv.hip conv_gemm_row_tile), so it
// is taken once the launch has about a workgroup per CU;
// below that the many-small-tiles + split-K ladder followed by the row kernel is faster (tools/lab/gemm_lab_ln.hip:
// M=16160 K=1024 93 -> 85 us, K=256 39.5 -> 31 us; M=2048 K=1024 21.6 -> 43 us).
inline bool fuse_row_epilogue(int M, int N, int Cin) {
  return conv_gemm_row_epilogue_ok(M, N, Cin) && (M + 31) / 32 >= 200;
}

// Y = mask(LayerNorm(act(conv(X)) + resid)) on the exact-fp32 kernels.  p: the contraction, prepared (operands, shape, act, packed
// rows) but for its output; e: ln_g / ln_b / lens (and row_b / row_t on packed rows).  ONE launch — the full-row tile when the
// launch is large enough, else the small-grid ladder with the ticketed row epilogue (raw rows through tmp, the last workgroup
// of a row block normalises it) — or two (GEMM -> tmp -> k_layernorm) when the ticket block is spent or disabled.
// (64x64 tiles with the ticketed epilogue in place of the full-row tile when its steps of 256 tiles fit the row count badly
//  were measured in round 4 and lose: at 572 workgroups the last arrivers' row work costs +12 us for a LayerNorm and +25 us
//  for a predictor tail, more than the finer steps save — B = 9: conv+LN 57 vs 56 us, conv+tail 80-86 vs 62, w_2 70.7 vs 70)
inline int gemm_ln_fp32(ConvGemm p, RowEpilogue e, float* tmp, float* Y, Tickets& tk, hipStream_t st, const RowMap* rm = nullptr) {
  p.ldy = p.N;
  if (fuse_row_epilogue(p.M, p.N, p.Cin)) {
    p.Y = Y; p.epi = EPI_LN; p.e = e;
    NS_HIP(launch_conv_gemm(p, st));
    return 0;
  }
  p.Y = tmp;
  if (conv_gemm_ticket_ok(p.M, p.N, p.Cin) && (e.ticket = tk.take(conv_gemm_ticket_ints(p.M))) != nullptr) {
    e.y_out = Y;
    p.epi = EPI_LN; p.e = e;
    NS_HIP(launch_conv_gemm(p, st));
    return 0;
  }
  p.epi = EPI_NONE;
  NS_HIP(launch_conv_gemm(p, st));
  NS_HIP(launch_layernorm(tmp, e.ln_g, e.ln_b, Y, p.M, p.N, p.S, e.lens, st, rm));
  return 0;
}

}  // namespace ns
