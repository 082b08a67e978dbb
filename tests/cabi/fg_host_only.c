/* A plain-C caller of the ns_fg_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the
 * structs must have the layout the Python binding assumes, the size queries must work, and every refusal must be reached through
 * dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by tests/test_ffn_grad_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*bytes_fn)(const ns_fg_shape*);
typedef int (*forward_fn)(const ns_fg_shape*, const ns_fg_weights*, const float*, const uint8_t*, float, float*, void*, void*, size_t, void*);
typedef int (*backward_fn)(const ns_fg_shape*, const ns_fg_weights*, const float*, const uint8_t*, float, const void*, const float*,
                           const ns_fg_grads*, void*, size_t, void*);
typedef int (*gate_fn)(const float*, const float*, int, int, float*, float*, void*, size_t, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* y = (float*)0x2000000; float* g = (float*)0x2100000;
  void* saved = (void*)0x3000000; void* ws = (void*)0x4000000;
  uint8_t* keep = (uint8_t*)0x5000000;
  ns_fg_shape s, bad;
  ns_fg_weights w;
  ns_fg_grads d;
  size_t need;
  last_error_fn last_error; version_fn version, launches; bytes_fn ws_bytes, saved_bytes; forward_fn forward; backward_fn backward; gate_fn gate;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_fg_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_fg_last_launches");
  *(void**)(&ws_bytes) = dlsym(so, "ns_fg_ws_bytes");
  *(void**)(&saved_bytes) = dlsym(so, "ns_fg_saved_bytes");
  *(void**)(&forward) = dlsym(so, "ns_fg_forward");
  *(void**)(&backward) = dlsym(so, "ns_fg_backward");
  *(void**)(&gate) = dlsym(so, "ns_fg_op_relu_gate");
  if (!last_error || !version || !launches || !ws_bytes || !saved_bytes || !forward || !backward || !gate) { printf("missing symbol\n"); return 4; }
  if (version() != NS_FG_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  if (sizeof(ns_fg_shape) != 24 || sizeof(ns_fg_weights) != 6 * sizeof(void*) || sizeof(ns_fg_grads) != 7 * sizeof(void*)) return 6;
  /* sizes */
  s.B = 16; s.S = 128; s.d = 256; s.d_inner = 1024; s.K1 = 9; s.K2 = 1;
  need = ws_bytes(&s);
  if (need < (size_t)2048 * (1024 + 2 * 256) * 4 || saved_bytes(&s) != (size_t)2048 * (1024 + 256) * 4) return 7;
  bad = s; bad.d = 384;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "d must be 256 or 512")) return 8;
  bad = s; bad.d_inner = 1000;
  if (saved_bytes(&bad) != 0 || !strstr(last_error(), "d_inner must be a positive multiple of 256")) return 9;
  bad = s; bad.K1 = 8;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "K1 must be odd and positive")) return 10;
  if (ws_bytes(0) != 0 || !strstr(last_error(), "null argument")) return 11;
  /* the launching calls refuse before any HIP call */
  w.w1 = (const float*)0x6000000; w.b1 = (const float*)0x6f10000; w.w2 = (const float*)0x7000000; w.b2 = (const float*)0x7f10000;
  w.ln_g = (const float*)0x8400000; w.ln_b = (const float*)0x8410000;
  memset(&d, 0, sizeof(d));
  if (forward(0, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 12;
  if (forward(&s, &w, 0, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 13;
  if (forward(&s, &w, x, 0, 0.0f, y, saved, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 14;
  bad = s; bad.d = 128;
  if (forward(&bad, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 15;
  bad = s; bad.d_inner = 0;
  if (forward(&bad, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "d_inner must be a positive multiple of 256")) return 16;
  bad = s; bad.K2 = 2;
  if (forward(&bad, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "K2 must be odd and positive")) return 17;
  bad = s; bad.B = 1 << 11; bad.S = 1 << 10;
  if (forward(&bad, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "problem too large")) return 18;
  if (forward(&s, &w, x, 0, 1.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "p_drop must lie in [0, 1)")) return 19;
  if (forward(&s, &w, x, 0, -0.5f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "p_drop must lie in [0, 1)")) return 20;
  if (forward(&s, &w, x, 0, 0.5f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 21;
  if (forward(&s, &w, x, keep, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "although p_drop == 0")) return 22;
  if (forward(&s, &w, x + 1, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "16-byte aligned")) return 23;
  w.ln_b = 0;
  if (forward(&s, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null weights->ln_b")) return 25;
  w.ln_b = (const float*)0x8410004;
  if (forward(&s, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "weights->ln_b must be 16-byte aligned")) return 26;
  w.ln_b = (const float*)0x8410000;
  if (backward(&s, &w, x, 0, 0.0f, 0, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 27;
  if (backward(&s, &w, x, 0, 0.0f, saved, 0, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 28;
  d.dx = (float*)0x9000004;
  if (backward(&s, &w, x, 0, 0.0f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "every gradient must be 16-byte aligned")) return 29;
  d.dx = 0;
  if (backward(&s, &w, x, 0, 0.5f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 30;
  if (backward(&s, &w, x, 0, 0.0f, saved, g, &d, ws, 64, 0) == 0 || !strstr(last_error(), "workspace too small")) return 31;
  if (backward(&s, &w, x, 0, 0.0f, saved, g, &d, ws, need, 0) != 0 || launches() != 0) return 32; /* nothing wanted: nothing launched */
  /* the new kernel alone */
  if (gate(0, x, 64, 1024, y, g, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 33;
  if (gate(x, x, 64, 1024, y, g, 0, need, 0) == 0 || !strstr(last_error(), "null argument")) return 34;
  if (gate(x, x, 64, 1000, y, g, ws, need, 0) == 0 || !strstr(last_error(), "d_inner must be a positive multiple of 256")) return 35;
  if (gate(x, x, 0, 1024, y, g, ws, need, 0) == 0 || !strstr(last_error(), "M must be positive")) return 36;
  if (gate(x, x + 1, 64, 1024, y, g, ws, need, 0) == 0 || !strstr(last_error(), "16-byte aligned")) return 37;
  if (gate(x, x, 64, 1024, y, g, ws, 8, 0) == 0 || !strstr(last_error(), "workspace too small")) return 38;
  if (gate(x, x, 1 << 21, 1024, y, g, ws, need, 0) == 0 || !strstr(last_error(), "problem too large")) return 39;
  printf("C caller ok\n");
  return 0;
}
