/* A plain-C caller of the ns_xg_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the
 * structs must have the layout the Python binding assumes, the size queries must work, and every refusal must be reached through
 * dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by tests/test_cross_attention_grad_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*bytes_fn)(const ns_xg_shape*);
typedef int (*splits_fn)(const ns_xg_shape*);
typedef int (*forward_fn)(const ns_xg_shape*, const ns_xg_weights*, const float*, const float*, const int64_t*, const uint8_t*, float, float*, float*,
                          void*, void*, size_t, void*);
typedef int (*backward_fn)(const ns_xg_shape*, const ns_xg_weights*, const float*, const float*, const int64_t*, const uint8_t*, float, const void*,
                           const float*, const float*, const float*, const ns_xg_grads*, void*, size_t, void*);
typedef int (*attn_bwd_fn)(const float*, const float*, const float*, const float*, const float*, const float*, const int64_t*, int, int, int, int, int,
                           int, float*, float*, void*, size_t, void*);

#define FWD(s_, w_, tgt_, src_, lens_, keep_, p_, y_, attn_, n_) forward(s_, w_, tgt_, src_, lens_, keep_, p_, y_, attn_, saved, ws, n_, 0)
#define BWD(s_, lens_, keep_, p_, saved_, attn_, g_, da_, n_) backward(s_, &w, x, src, lens_, keep_, p_, saved_, attn_, g_, da_, &d, ws, n_, 0)
#define OP(q_, da_, lens_, T_, L_, d_, H_, ks_, n_) attn_bwd(q_, src, x, attn, x, da_, lens_, 4, T_, L_, d_, H_, ks_, y, g, ws, n_, 0)
#define SAYS(text) (strstr(last_error(), text) != 0)

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* src = (float*)0x1800000; float* y = (float*)0x2000000; float* g = (float*)0x2100000;
  float* attn = (float*)0x2800000; float* da = (float*)0x2C00000;
  void* saved = (void*)0x3000000; void* ws = (void*)0x4000000;
  uint8_t* keep = (uint8_t*)0x5000000;
  int64_t* lens = (int64_t*)0x5100000;
  ns_xg_shape s, bad;
  ns_xg_weights w;
  ns_xg_grads d;
  size_t need;
  last_error_fn last_error; version_fn version, launches; bytes_fn ws_bytes, saved_bytes; splits_fn splits; forward_fn forward;
  backward_fn backward; attn_bwd_fn attn_bwd;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_xg_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_xg_last_launches");
  *(void**)(&ws_bytes) = dlsym(so, "ns_xg_ws_bytes");
  *(void**)(&saved_bytes) = dlsym(so, "ns_xg_saved_bytes");
  *(void**)(&splits) = dlsym(so, "ns_xg_kv_splits");
  *(void**)(&forward) = dlsym(so, "ns_xg_forward");
  *(void**)(&backward) = dlsym(so, "ns_xg_backward");
  *(void**)(&attn_bwd) = dlsym(so, "ns_xg_op_attention_backward");
  if (!last_error || !version || !launches || !ws_bytes || !saved_bytes || !splits || !forward || !backward || !attn_bwd) { printf("missing symbol\n"); return 4; }
  if (version() != NS_XG_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  if (sizeof(ns_xg_shape) != 20 || sizeof(ns_xg_weights) != 10 * sizeof(void*) || sizeof(ns_xg_grads) != 12 * sizeof(void*)) return 6;
  /* sizes */
  s.B = 16; s.T = 1000; s.L = 128; s.d = 256; s.H = 2;
  need = ws_bytes(&s);
  if (need < (size_t)4 * 16000 * 256 * 4 || saved_bytes(&s) != ((size_t)3 * 16000 * 256 + (size_t)2 * 2048 * 256) * 4) return 7;
  if (splits(&s) < 1 || splits(&s) > 8) return 70;
  bad = s; bad.T = 128;
  if (splits(&bad) != 1) return 71;
  bad = s; bad.d = 384;
  if (ws_bytes(&bad) != 0 || !SAYS("d must be 256 or 512")) return 8;
  bad = s; bad.H = 3;
  if (saved_bytes(&bad) != 0 || !SAYS("d must be a multiple of H")) return 9;
  bad = s; bad.H = 8;
  if (ws_bytes(&bad) != 0 || !SAYS("d / H must be 64 or 128")) return 10;
  bad = s; bad.H = 1;
  if (splits(&bad) != 0 || !SAYS("d / H must be 64 or 128")) return 72;
  if (ws_bytes(0) != 0 || !SAYS("null argument")) return 11;
  if (splits(0) != 0 || !SAYS("null argument")) return 73;
  /* the launching calls refuse before any HIP call */
  w.wq = (const float*)0x6000000; w.bq = (const float*)0x6010000; w.wk = (const float*)0x6100000; w.bk = (const float*)0x6110000;
  w.wv = (const float*)0x6200000; w.bv = (const float*)0x6210000; w.wfc = (const float*)0x6300000; w.bfc = (const float*)0x6310000;
  w.ln_g = (const float*)0x6400000; w.ln_b = (const float*)0x6410000;
  memset(&d, 0, sizeof(d));
  if (FWD(0, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("null argument")) return 12;
  if (FWD(&s, &w, 0, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("null argument")) return 13;
  if (FWD(&s, &w, x, 0, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("null argument")) return 74;
  if (FWD(&s, &w, x, src, 0, 0, 0.0f, y, attn, need) == 0 || !SAYS("null argument")) return 75;
  if (FWD(&s, &w, x, src, lens, 0, 0.0f, y, 0, need) == 0 || !SAYS("null argument")) return 76;
  if (FWD(&s, &w, x, src, lens, 0, 0.0f, y, attn, need - 1) == 0 || !SAYS("workspace too small")) return 14;
  bad = s; bad.d = 128;
  if (FWD(&bad, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("d must be 256 or 512")) return 15;
  bad = s; bad.H = 5;
  if (FWD(&bad, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("d must be a multiple of H")) return 16;
  bad = s; bad.H = 8;
  if (FWD(&bad, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("d / H must be 64 or 128")) return 17;
  bad = s; bad.L = 0;
  if (FWD(&bad, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("must be positive")) return 77;
  bad = s; bad.B = 1 << 10; bad.T = 1 << 10; bad.L = 1 << 10;
  if (FWD(&bad, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("B * H * T * L must stay below 2^31")) return 18;
  bad = s; bad.B = 1 << 11; bad.T = 1 << 11; bad.L = 1;
  if (FWD(&bad, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("B * max(T, L) * 2d must stay below 2^31")) return 78;
  if (FWD(&s, &w, x, src, lens, 0, 1.0f, y, attn, need) == 0 || !SAYS("p_drop must lie in [0, 1)")) return 19;
  if (FWD(&s, &w, x, src, lens, 0, -0.5f, y, attn, need) == 0 || !SAYS("p_drop must lie in [0, 1)")) return 20;
  if (FWD(&s, &w, x, src, lens, 0, 0.5f, y, attn, need) == 0 || !SAYS("needs a keep-mask")) return 21;
  if (FWD(&s, &w, x, src, lens, keep, 0.0f, y, attn, need) == 0 || !SAYS("although p_drop == 0")) return 22;
  if (FWD(&s, &w, x + 1, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("16-byte aligned")) return 23;
  if (FWD(&s, &w, x, src + 1, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("16-byte aligned")) return 79;
  if (FWD(&s, &w, x, src, lens, 0, 0.0f, y, attn + 1, need) == 0 || !SAYS("16-byte aligned")) return 80;
  if (FWD(&s, &w, x, src, (int64_t*)0x5100004, 0, 0.0f, y, attn, need) == 0 || !SAYS("src_lens must be 8-byte aligned")) return 24;
  w.ln_b = 0;
  if (FWD(&s, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("null weights->ln_b")) return 25;
  w.ln_b = (const float*)0x6410004;
  if (FWD(&s, &w, x, src, lens, 0, 0.0f, y, attn, need) == 0 || !SAYS("weights->ln_b must be 16-byte aligned")) return 26;
  w.ln_b = (const float*)0x6410000;
  if (BWD(&s, lens, 0, 0.0f, 0, attn, g, da, need) == 0 || !SAYS("null argument")) return 27;
  if (BWD(&s, lens, 0, 0.0f, saved, attn, 0, da, need) == 0 || !SAYS("null argument")) return 28;
  if (BWD(&s, lens, 0, 0.0f, saved, 0, g, da, need) == 0 || !SAYS("null argument")) return 81;
  if (BWD(&s, 0, 0, 0.0f, saved, attn, g, da, need) == 0 || !SAYS("null argument")) return 82;
  if (BWD(&s, lens, 0, 0.0f, saved, attn, g, da + 1, need) == 0 || !SAYS("g and dA must be 16-byte aligned")) return 83;
  d.dsrc = (float*)0x8000004;
  if (BWD(&s, lens, 0, 0.0f, saved, attn, g, da, need) == 0 || !SAYS("every gradient must be 16-byte aligned")) return 29;
  d.dsrc = 0;
  if (BWD(&s, lens, 0, 0.5f, saved, attn, g, da, need) == 0 || !SAYS("needs a keep-mask")) return 30;
  if (BWD(&s, lens, 0, 0.0f, saved, attn, g, da, 64) == 0 || !SAYS("workspace too small")) return 31;
  if (BWD(&s, lens, 0, 0.0f, saved, attn, g, da, need) != 0 || launches() != 0) return 32; /* nothing wanted: nothing launched */
  if (BWD(&s, lens, 0, 0.0f, saved, attn, g, 0, need) != 0 || launches() != 0) return 84;  /* dA is nullable */
  /* the new kernels alone */
  if (OP(0, da, lens, 100, 40, 256, 2, 0, need) == 0 || !SAYS("null argument")) return 33;
  if (OP(x, da, 0, 100, 40, 256, 2, 0, need) == 0 || !SAYS("null argument")) return 85;
  if (OP(x, da, lens, 100, 40, 256, 3, 0, need) == 0 || !SAYS("d must be a multiple of H")) return 34;
  if (OP(x, da, lens, 100, 40, 256, 8, 0, need) == 0 || !SAYS("d / H must be 64 or 128")) return 86;
  if (OP(x, da, lens, 100, 40, 200, 2, 0, need) == 0 || !SAYS("d must be 256 or 512")) return 37;
  if (OP(x, da, lens, 100, 40, 256, 2, 9, need) == 0 || !SAYS("kv_splits must lie in [0, 8]")) return 87;
  if (OP(x, da, lens, 100, 40, 256, 2, -1, need) == 0 || !SAYS("kv_splits must lie in [0, 8]")) return 88;
  if (OP(x, da + 1, lens, 100, 40, 256, 2, 0, need) == 0 || !SAYS("16-byte aligned")) return 36;
  if (OP(x, da, (int64_t*)0x5100004, 100, 40, 256, 2, 0, need) == 0 || !SAYS("src_lens must be 8-byte aligned")) return 89;
  if (OP(x, da, lens, 100, 40, 256, 2, 1, 16) == 0 || !SAYS("workspace too small")) return 35;
  /* one part needs D only, three parts their partial sums too */
  if (OP(x, 0, lens, 100, 40, 256, 2, 3, (size_t)4 * 2 * 100 * 4 + 256) == 0 || !SAYS("workspace too small")) return 90;
  printf("C caller ok\n");
  return 0;
}
