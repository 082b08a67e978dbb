/* A plain-C caller of the ns_ag_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the
 * structs must have the layout the Python binding assumes, the size queries must work, and every refusal must be reached through
 * dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by tests/test_attention_grad_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*bytes_fn)(const ns_ag_shape*);
typedef int (*forward_fn)(const ns_ag_shape*, const ns_ag_weights*, const float*, const int64_t*, const uint8_t*, float, float*, void*, void*, size_t,
                          void*);
typedef int (*backward_fn)(const ns_ag_shape*, const ns_ag_weights*, const float*, const int64_t*, const uint8_t*, float, const void*, const float*,
                           const ns_ag_grads*, void*, size_t, void*);
typedef int (*lse_fn)(const float*, const int64_t*, int, int, int, int, float*, void*);
typedef int (*attn_bwd_fn)(const float*, const float*, const float*, const float*, const int64_t*, int, int, int, int, float*, void*, size_t, void*);
typedef int (*row_bwd_fn)(const float*, const float*, const float*, const uint8_t*, float, int, int, float*, float*, float*, float*, float*, void*, size_t,
                          void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* y = (float*)0x2000000; float* g = (float*)0x2100000;
  void* saved = (void*)0x3000000; void* ws = (void*)0x4000000;
  uint8_t* keep = (uint8_t*)0x5000000;
  int64_t* lens = (int64_t*)0x5100000;
  ns_ag_shape s, bad;
  ns_ag_weights w;
  ns_ag_grads d;
  size_t need;
  last_error_fn last_error; version_fn version, launches; bytes_fn ws_bytes, saved_bytes; forward_fn forward; backward_fn backward;
  lse_fn lse; attn_bwd_fn attn_bwd; row_bwd_fn row_bwd;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_ag_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_ag_last_launches");
  *(void**)(&ws_bytes) = dlsym(so, "ns_ag_ws_bytes");
  *(void**)(&saved_bytes) = dlsym(so, "ns_ag_saved_bytes");
  *(void**)(&forward) = dlsym(so, "ns_ag_forward");
  *(void**)(&backward) = dlsym(so, "ns_ag_backward");
  *(void**)(&lse) = dlsym(so, "ns_ag_op_lse");
  *(void**)(&attn_bwd) = dlsym(so, "ns_ag_op_attention_backward");
  *(void**)(&row_bwd) = dlsym(so, "ns_ag_op_row_backward");
  if (!last_error || !version || !launches || !ws_bytes || !saved_bytes || !forward || !backward || !lse || !attn_bwd || !row_bwd) { printf("missing symbol\n"); return 4; }
  if (version() != NS_AG_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  if (sizeof(ns_ag_shape) != 16 || sizeof(ns_ag_weights) != 10 * sizeof(void*) || sizeof(ns_ag_grads) != 11 * sizeof(void*)) return 6;
  /* sizes */
  s.B = 16; s.S = 128; s.d = 256; s.H = 2;
  need = ws_bytes(&s);
  if (need < (size_t)6 * 2048 * 256 * 4 || saved_bytes(&s) != ((size_t)5 * 2048 * 256 + 16 * 2 * 128) * 4) return 7;
  bad = s; bad.d = 384;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "d must be 256 or 512")) return 8;
  bad = s; bad.H = 3;
  if (saved_bytes(&bad) != 0 || !strstr(last_error(), "d must be a multiple of H")) return 9;
  bad = s; bad.H = 1;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "d / H must be 32, 64 or 128")) return 10;
  if (ws_bytes(0) != 0 || !strstr(last_error(), "null argument")) return 11;
  /* the launching calls refuse before any HIP call */
  w.wq = (const float*)0x6000000; w.bq = (const float*)0x6010000; w.wk = (const float*)0x6100000; w.bk = (const float*)0x6110000;
  w.wv = (const float*)0x6200000; w.bv = (const float*)0x6210000; w.wfc = (const float*)0x6300000; w.bfc = (const float*)0x6310000;
  w.ln_g = (const float*)0x6400000; w.ln_b = (const float*)0x6410000;
  memset(&d, 0, sizeof(d));
  if (forward(0, &w, x, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 12;
  if (forward(&s, &w, 0, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 13;
  if (forward(&s, &w, x, lens, 0, 0.0f, y, saved, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 14;
  bad = s; bad.d = 128;
  if (forward(&bad, &w, x, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 15;
  bad = s; bad.H = 5;
  if (forward(&bad, &w, x, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "d must be a multiple of H")) return 16;
  bad = s; bad.H = 16;
  if (forward(&bad, &w, x, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "d / H must be 32, 64 or 128")) return 17;
  bad = s; bad.B = 1 << 11; bad.S = 1 << 11;
  if (forward(&bad, &w, x, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "problem too large")) return 18;
  if (forward(&s, &w, x, lens, 0, 1.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "p_drop must lie in [0, 1)")) return 19;
  if (forward(&s, &w, x, lens, 0, -0.5f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "p_drop must lie in [0, 1)")) return 20;
  if (forward(&s, &w, x, lens, 0, 0.5f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 21;
  if (forward(&s, &w, x, lens, keep, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "although p_drop == 0")) return 22;
  if (forward(&s, &w, x + 1, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "16-byte aligned")) return 23;
  if (forward(&s, &w, x, (int64_t*)0x5100004, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "lens must be 8-byte aligned")) return 24;
  w.ln_b = 0;
  if (forward(&s, &w, x, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null weights->ln_b")) return 25;
  w.ln_b = (const float*)0x6410004;
  if (forward(&s, &w, x, lens, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "weights->ln_b must be 16-byte aligned")) return 26;
  w.ln_b = (const float*)0x6410000;
  if (backward(&s, &w, x, lens, 0, 0.0f, 0, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 27;
  if (backward(&s, &w, x, lens, 0, 0.0f, saved, 0, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 28;
  d.dx = (float*)0x8000004;
  if (backward(&s, &w, x, lens, 0, 0.0f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "every gradient must be 16-byte aligned")) return 29;
  d.dx = 0;
  if (backward(&s, &w, x, lens, 0, 0.5f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 30;
  if (backward(&s, &w, x, lens, 0, 0.0f, saved, g, &d, ws, 64, 0) == 0 || !strstr(last_error(), "workspace too small")) return 31;
  if (backward(&s, &w, x, lens, 0, 0.0f, saved, g, &d, ws, need, 0) != 0 || launches() != 0) return 32; /* nothing wanted: nothing launched */
  /* each kernel alone */
  if (lse(0, lens, 16, 128, 256, 2, y, 0) == 0 || !strstr(last_error(), "null argument")) return 33;
  if (lse(x, lens, 16, 128, 256, 3, y, 0) == 0 || !strstr(last_error(), "d must be a multiple of H")) return 34;
  if (attn_bwd(x, x, x, x, lens, 16, 128, 256, 2, y, ws, 16, 0) == 0 || !strstr(last_error(), "workspace too small")) return 35;
  if (attn_bwd(x, x, x, x + 1, lens, 16, 128, 256, 2, y, ws, need, 0) == 0 || !strstr(last_error(), "16-byte aligned")) return 36;
  if (attn_bwd(x, x, x, x, lens, 16, 128, 200, 2, y, ws, need, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 37;
  if (row_bwd(x, x, x, 0, 0.0f, 64, 256, y, y, y, y, 0, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 38;
  if (row_bwd(x, x, x, 0, 0.3f, 64, 256, y, y, y, y, y, ws, need, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 39;
  if (row_bwd(x, x, x, 0, 0.0f, 64, 100, y, y, y, y, y, ws, need, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 40;
  if (row_bwd(x, x, x, 0, 0.0f, 64, 256, y, y, y, y, y, ws, 8, 0) == 0 || !strstr(last_error(), "workspace too small")) return 41;
  printf("C caller ok\n");
  return 0;
}
