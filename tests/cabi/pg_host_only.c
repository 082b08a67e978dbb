/* A plain-C caller of the ns_pg_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the
 * structs must have the layout the Python binding assumes, the host-only planner and size queries must work, and every refusal must
 * be reached through dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by tests/test_predictor_grad_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef int (*plan_fn)(int, int, int, int, int32_t*);
typedef size_t (*bytes_fn)(const ns_pg_shape*);
typedef int (*forward_fn)(const ns_pg_shape*, const ns_pg_weights*, const float*, const uint8_t*, const uint8_t*, const uint8_t*, float, float*, void*,
                          void*, size_t, void*);
typedef int (*backward_fn)(const ns_pg_shape*, const ns_pg_weights*, const float*, const uint8_t*, const uint8_t*, const uint8_t*, float, const void*,
                           const float*, const ns_pg_grads*, void*, size_t, void*);
typedef int (*wgrad_fn)(const float*, const float*, int, int, int, int, int, float*, float*, void*, size_t, void*);
typedef int (*dgrad_fn)(const float*, const float*, int, int, int, int, int, float*, void*, size_t, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* pred = (float*)0x2000000; float* g = (float*)0x2100000;
  void* saved = (void*)0x3000000; void* ws = (void*)0x4000000;
  uint8_t* keep = (uint8_t*)0x5000000;
  ns_pg_shape s, bad;
  ns_pg_weights w;
  ns_pg_grads d;
  int32_t plan[8], again[8];
  size_t need;
  last_error_fn last_error; version_fn version; plan_fn plan_wgrad; bytes_fn ws_bytes, saved_bytes; forward_fn forward; backward_fn backward;
  wgrad_fn wgrad; dgrad_fn dgrad;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_pg_abi_version");
  *(void**)(&plan_wgrad) = dlsym(so, "ns_pg_plan_wgrad");
  *(void**)(&ws_bytes) = dlsym(so, "ns_pg_ws_bytes");
  *(void**)(&saved_bytes) = dlsym(so, "ns_pg_saved_bytes");
  *(void**)(&forward) = dlsym(so, "ns_pg_forward");
  *(void**)(&backward) = dlsym(so, "ns_pg_backward");
  *(void**)(&wgrad) = dlsym(so, "ns_pg_op_wgrad");
  *(void**)(&dgrad) = dlsym(so, "ns_pg_op_dgrad");
  if (!last_error || !version || !plan_wgrad || !ws_bytes || !saved_bytes || !forward || !backward || !wgrad || !dgrad) { printf("missing symbol\n"); return 4; }
  if (version() != NS_PG_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  if (sizeof(ns_pg_shape) != 20 || sizeof(ns_pg_weights) != 10 * sizeof(void*) || sizeof(ns_pg_grads) != 11 * sizeof(void*)) return 6;
  /* the planner: M = 2048 rows of the 256 -> 256, k = 3 convolution: 12 tiles, at least 200 workgroups, the ranges cover [0, M) */
  if (plan_wgrad(2048, 256, 256, 3, plan) != 0) { printf("plan: %s\n", last_error()); return 7; }
  if (plan[0] != 128 || plan[1] != 128 || plan[4] != 12 || plan[3] * plan[4] < 200 || plan[2] % 16 != 0) return 8;
  if ((plan[3] - 1) * plan[2] >= 2048 || plan[3] * plan[2] < 2048 || plan[5] != plan[3] * 256 * 768) return 9;
  if (plan_wgrad(2048, 256, 256, 3, again) != 0 || memcmp(plan, again, sizeof(plan)) != 0) return 10;
  if (plan_wgrad(2048, 256, 256, 4, again) == 0 || !strstr(last_error(), "refused")) return 11;
  if (plan_wgrad(2048, 256, 256, 3, 0) == 0 || !strstr(last_error(), "null argument")) return 12;
  /* sizes */
  s.B = 16; s.S = 128; s.Cin = 256; s.F = 256; s.K = 3;
  need = ws_bytes(&s);
  if (need < (size_t)plan[5] * 4 || saved_bytes(&s) != (size_t)3 * 2048 * 256 * 4) return 13;
  bad = s; bad.F = 384;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "F must be 256 or 512")) return 14;
  /* the launching calls refuse before any HIP call */
  w.w1 = (const float*)0x6000000; w.b1 = (const float*)0x6010000; w.ln1_g = (const float*)0x6020000; w.ln1_b = (const float*)0x6030000;
  w.w2 = (const float*)0x6040000; w.b2 = (const float*)0x6050000; w.ln2_g = (const float*)0x6060000; w.ln2_b = (const float*)0x6070000;
  w.wlin = (const float*)0x6080000; w.blin = (const float*)0x6090000;
  memset(&d, 0, sizeof(d));
  if (forward(0, &w, x, 0, 0, 0, 0.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 15;
  if (forward(&s, &w, x, 0, 0, 0, 0.0f, pred, saved, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 16;
  bad = s; bad.K = 2;
  if (forward(&bad, &w, x, 0, 0, 0, 0.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "K must be odd")) return 17;
  bad = s; bad.Cin = 250;
  if (forward(&bad, &w, x, 0, 0, 0, 0.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "Cin must be a multiple of 16")) return 18;
  bad = s; bad.B = 1 << 12; bad.S = 1 << 11;
  if (forward(&bad, &w, x, 0, 0, 0, 0.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "problem too large")) return 19;
  if (forward(&s, &w, x, 0, 0, 0, 1.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "p_drop must lie in [0, 1)")) return 20;
  if (forward(&s, &w, x, 0, keep, 0, 0.5f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "needs both keep-masks")) return 21;
  if (forward(&s, &w, x, 0, keep, keep, 0.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "although p_drop == 0")) return 22;
  if (forward(&s, &w, x + 1, 0, 0, 0, 0.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "16-byte aligned")) return 23;
  w.ln2_b = 0;
  if (forward(&s, &w, x, 0, 0, 0, 0.0f, pred, saved, ws, need, 0) == 0 || !strstr(last_error(), "null weights->ln2_b")) return 24;
  w.ln2_b = (const float*)0x7000000;
  if (backward(&s, &w, x, 0, 0, 0, 0.0f, 0, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 25;
  d.dx = (float*)0x8000004;
  if (backward(&s, &w, x, 0, 0, 0, 0.0f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "every gradient must be 16-byte aligned")) return 26;
  d.dx = 0;
  if (backward(&s, &w, x, 0, 0, 0, 0.0f, saved, g, &d, ws, need, 0) != 0) return 27; /* nothing wanted: nothing launched */
  if (wgrad(x, x, 16, 128, 256, 256, 3, pred, 0, ws, 16, 0) == 0 || !strstr(last_error(), "workspace too small")) return 28;
  if (wgrad(x, x, 16, 128, 200, 256, 3, pred, 0, ws, need, 0) == 0 || !strstr(last_error(), "F must be 256 or 512")) return 29;
  if (dgrad(x, 0, 16, 128, 256, 256, 3, pred, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 30;
  if (dgrad(x, x, 16, 128, 256, 256, 6, pred, ws, need, 0) == 0 || !strstr(last_error(), "K must be odd")) return 31;
  printf("C caller ok\n");
  return 0;
}
