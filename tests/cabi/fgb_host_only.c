/* A plain-C caller of the "bf16" additions to the ns_fg_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be
 * usable from C, the size queries and the plan must work, and every refusal must be reached through dlopen/dlsym without a GPU
 * (validation precedes the first HIP call).  Run by tests/test_ffn_bf16_host.py. */
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
typedef int (*plan_fn)(int, int, int, int, int32_t*);
typedef size_t (*op_bytes_fn)(int, int, int, int, int);
typedef int (*wgrad_fn)(const float*, const float*, int, int, int, int, int, float*, void*, size_t, void*);
typedef int (*conv_fn)(const float*, const float*, const float*, const float*, int, int, int, int, int, int, int, float*, void*, size_t, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* y = (float*)0x2000000; float* g = (float*)0x2100000;
  void* saved = (void*)0x3000000; void* ws = (void*)0x4000000;
  uint8_t* keep = (uint8_t*)0x5000000;
  ns_fg_shape s, bad;
  ns_fg_weights w;
  ns_fg_grads d;
  size_t need, need32, op_need;
  int32_t pl[8];
  last_error_fn last_error; version_fn launches; bytes_fn ws_bytes, ws_bytes32, saved_bytes; forward_fn forward; backward_fn backward;
  plan_fn plan; op_bytes_fn op_bytes; wgrad_fn wgrad; conv_fn conv;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&launches) = dlsym(so, "ns_fg_last_launches");
  *(void**)(&ws_bytes) = dlsym(so, "ns_fg_ws_bytes_bf16");
  *(void**)(&ws_bytes32) = dlsym(so, "ns_fg_ws_bytes");
  *(void**)(&saved_bytes) = dlsym(so, "ns_fg_saved_bytes");
  *(void**)(&forward) = dlsym(so, "ns_fg_forward_bf16");
  *(void**)(&backward) = dlsym(so, "ns_fg_backward_bf16");
  *(void**)(&plan) = dlsym(so, "ns_fg_plan_wgrad_bf16");
  *(void**)(&op_bytes) = dlsym(so, "ns_fg_op_bf16_ws_bytes");
  *(void**)(&wgrad) = dlsym(so, "ns_fg_op_wgrad_bf16");
  *(void**)(&conv) = dlsym(so, "ns_fg_op_conv_bf16");
  if (!last_error || !launches || !ws_bytes || !ws_bytes32 || !saved_bytes || !forward || !backward || !plan || !op_bytes || !wgrad || !conv) {
    printf("missing symbol\n");
    return 4;
  }
  /* sizes: bf16 planes where the fp32 workspace holds fp32 ones */
  s.B = 16; s.S = 128; s.d = 256; s.d_inner = 1024; s.K1 = 9; s.K2 = 1;
  need = ws_bytes(&s);
  need32 = ws_bytes32(&s);
  if (need < (size_t)2048 * (1024 + 2 * 256) * 4 || need >= need32 || saved_bytes(&s) != (size_t)2048 * (1024 + 256) * 4) return 7;
  bad = s; bad.d = 384;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "d must be 256 or 512")) return 8;
  bad = s; bad.K1 = 8;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "K1 must be odd and positive")) return 10;
  if (ws_bytes(0) != 0 || !strstr(last_error(), "null argument")) return 11;
  /* the plan */
  if (plan(2048, 1024, 256, 9, pl) != 0 || pl[0] != 128 || pl[1] != 128 || pl[2] % 32 != 0 || pl[3] * pl[2] < 2048 || pl[7] != 0) return 40;
  if (plan(2048, 1024, 48, 9, pl) == 0 || !strstr(last_error(), "refused")) return 41;
  if (plan(2048, 1000, 256, 9, pl) == 0 || !strstr(last_error(), "refused")) return 42;
  if (plan(2048, 1024, 256, 9, 0) == 0 || !strstr(last_error(), "null argument")) return 43;
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
  if (forward(&s, &w, x, 0, 0.5f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 21;
  if (forward(&s, &w, x, keep, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "although p_drop == 0")) return 22;
  if (forward(&s, &w, x + 1, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "16-byte aligned")) return 23;
  w.ln_b = 0;
  if (forward(&s, &w, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null weights->ln_b")) return 25;
  w.ln_b = (const float*)0x8410000;
  if (backward(&s, &w, x, 0, 0.0f, 0, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 27;
  if (backward(&s, &w, x, 0, 0.0f, saved, 0, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 28;
  d.dx = (float*)0x9000004;
  if (backward(&s, &w, x, 0, 0.0f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "every gradient must be 16-byte aligned")) return 29;
  d.dx = 0;
  if (backward(&s, &w, x, 0, 0.5f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 30;
  if (backward(&s, &w, x, 0, 0.0f, saved, g, &d, ws, 64, 0) == 0 || !strstr(last_error(), "workspace too small")) return 31;
  if (backward(&s, &w, x, 0, 0.0f, saved, g, &d, ws, need, 0) != 0 || launches() != 0) return 32; /* nothing wanted: nothing launched */
  /* the hooks */
  op_need = op_bytes(16, 128, 1024, 256, 9);
  if (op_need < (size_t)1024 * 256 * 9 * 2) return 50;
  if (op_bytes(16, 128, 1000, 256, 9) != 0 || !strstr(last_error(), "N must be a positive multiple of 32")) return 51;
  if (wgrad(0, x, 16, 128, 1024, 256, 9, y, ws, op_need, 0) == 0 || !strstr(last_error(), "null argument")) return 52;
  if (wgrad(g, x, 16, 128, 1024, 48, 9, y, ws, op_need, 0) == 0 || !strstr(last_error(), "Cin must be a positive multiple of 32")) return 53;
  if (wgrad(g, x, 16, 128, 1024, 256, 2, y, ws, op_need, 0) == 0 || !strstr(last_error(), "KW must be odd and positive")) return 54;
  if (wgrad(g, x + 1, 16, 128, 1024, 256, 9, y, ws, op_need, 0) == 0 || !strstr(last_error(), "X must be 16-byte aligned")) return 55;
  if (wgrad(g, x, 16, 128, 1024, 256, 9, y, ws, op_need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 56;
  if (wgrad(g, x, 16, 128, 160, 256, 9, y, ws, op_need, 0) == 0 || !strstr(last_error(), "plan refuses")) return 57;
  if (conv(x, 0, 0, 0, 16, 128, 1024, 256, 9, 0, 1, y, ws, op_need, 0) == 0 || !strstr(last_error(), "null argument")) return 58;
  if (conv(x, g, 0, 0, 16, 128, 1024, 256, 9, 0, 3, y, ws, op_need, 0) == 0 || !strstr(last_error(), "act must be 0 (none) or 1 (ReLU)")) return 59;
  if (conv(x, g, 0, 0, 16, 128, 1024, 256, 9, 1, 0, x, ws, op_need, 0) == 0 || !strstr(last_error(), "y must not be x or resid")) return 60;
  if (conv(x, g, g + 1, 0, 16, 128, 1024, 256, 9, 1, 0, y, ws, op_need, 0) == 0 || !strstr(last_error(), "bias must be 16-byte aligned")) return 61;
  if (conv(x, g, 0, 0, 16, 128, 1024, 256, 9, 0, 0, y, ws, 64, 0) == 0 || !strstr(last_error(), "workspace too small")) return 62;
  printf("C caller ok\n");
  return 0;
}
