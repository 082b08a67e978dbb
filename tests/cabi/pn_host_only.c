/* A plain-C caller of the ns_pn_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the
 * structs must have the layout the Python binding assumes, the size queries must work, and every refusal must be reached through
 * dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by tests/test_postnet_grad_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*bytes_fn)(const ns_pn_shape*);
typedef int (*forward_fn)(const ns_pn_shape*, const ns_pn_weights*, int, const float*, const uint8_t* const*, float, float*, void*, void*, size_t, void*);
typedef int (*backward_fn)(const ns_pn_shape*, const ns_pn_weights*, int, const float*, const uint8_t* const*, float, const void*, const float*,
                           const ns_pn_grads*, void*, size_t, void*);
typedef int (*stats_fn)(const float*, int, int, int, float*, float*, int64_t*, double*, void*, size_t, void*);
typedef int (*apply_fn)(const float*, const double*, const float*, const float*, const uint8_t*, float, int, int, int, float*, void*);
typedef int (*reduce_fn)(const float*, const float*, const float*, const double*, const uint8_t*, float, int, int, int, float*, float*, double*, void*,
                         size_t, void*);
typedef int (*bwd_apply_fn)(const float*, const float*, const float*, const double*, const double*, const float*, const uint8_t*, float, int, int, int,
                            int, float*, float*, void*, size_t, void*);
typedef int (*narrow_fn)(const float*, const float*, int, int, int, int, int, float*, void*, size_t, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* y = (float*)0x2000000; float* g = (float*)0x2100000;
  double* st = (double*)0x2200000;
  void* saved = (void*)0x3000000; void* ws = (void*)0x4000000;
  const uint8_t* keep[NS_PN_MAX_LAYERS];
  ns_pn_shape s, bad;
  ns_pn_weights w;
  ns_pn_grads d;
  size_t need;
  int i;
  last_error_fn last_error; version_fn version; bytes_fn ws_bytes, saved_bytes; forward_fn forward; backward_fn backward;
  stats_fn stats; apply_fn apply; reduce_fn reduce; bwd_apply_fn bwd_apply; narrow_fn narrow;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_pn_abi_version");
  *(void**)(&ws_bytes) = dlsym(so, "ns_pn_ws_bytes");
  *(void**)(&saved_bytes) = dlsym(so, "ns_pn_saved_bytes");
  *(void**)(&forward) = dlsym(so, "ns_pn_forward");
  *(void**)(&backward) = dlsym(so, "ns_pn_backward");
  *(void**)(&stats) = dlsym(so, "ns_pn_op_stats");
  *(void**)(&apply) = dlsym(so, "ns_pn_op_apply");
  *(void**)(&reduce) = dlsym(so, "ns_pn_op_bwd_reduce");
  *(void**)(&bwd_apply) = dlsym(so, "ns_pn_op_bwd_apply");
  *(void**)(&narrow) = dlsym(so, "ns_pn_op_wgrad_narrow");
  if (!last_error || !version || !ws_bytes || !saved_bytes || !forward || !backward || !stats || !apply || !reduce || !bwd_apply || !narrow) {
    printf("missing symbol\n");
    return 4;
  }
  if (version() != NS_PN_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  if (sizeof(ns_pn_shape) != 24 || sizeof(ns_pn_layer) != 7 * sizeof(void*) || sizeof(ns_pn_weights) != 35 * sizeof(void*) ||
      sizeof(ns_pn_grads) != 21 * sizeof(void*))
    return 6;
  /* sizes: the flagship's 16 x 1010 rows, five layers */
  s.B = 16; s.T = 1010; s.n_mel = 80; s.emb = 512; s.K = 5; s.n = 5;
  need = ws_bytes(&s);
  if (need == 0) { printf("ws_bytes: %s\n", last_error()); return 7; }
  if (saved_bytes(&s) != (size_t)4 * 16160 * (8 * 512 + 80) + 16 * 5 * 512) return 8;
  bad = s; bad.emb = 384;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "emb must be 256 or 512")) return 9;
  if (saved_bytes(0) != 0 || !strstr(last_error(), "null argument")) return 10;
  /* the launching calls refuse before any HIP call */
  for (i = 0; i < NS_PN_MAX_LAYERS; ++i) {
    w.layer[i].w = (const float*)(size_t)(0x6000000 + 0x100000 * i); w.layer[i].b = (const float*)(size_t)(0x6010000 + 0x100000 * i);
    w.layer[i].gamma = (const float*)(size_t)(0x6020000 + 0x100000 * i); w.layer[i].beta = (const float*)(size_t)(0x6030000 + 0x100000 * i);
    w.layer[i].running_mean = (float*)(size_t)(0x6040000 + 0x100000 * i); w.layer[i].running_var = (float*)(size_t)(0x6050000 + 0x100000 * i);
    w.layer[i].num_batches_tracked = (int64_t*)(size_t)(0x6060000 + 0x100000 * i);
    keep[i] = (const uint8_t*)(size_t)(0x5000000 + 0x100000 * i);
  }
  memset(&d, 0, sizeof(d));
  if (forward(0, &w, 1, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 15;
  if (forward(&s, &w, 1, x, 0, 0.0f, y, saved, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 16;
  bad = s; bad.K = 4;
  if (forward(&bad, &w, 1, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "K must be odd and at most 9")) return 17;
  bad = s; bad.n_mel = 72;
  if (forward(&bad, &w, 1, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "n_mel must be a multiple of 16")) return 18;
  bad = s; bad.B = 1 << 11; bad.T = 1 << 11;
  if (forward(&bad, &w, 1, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "problem too large")) return 19;
  bad = s; bad.n = 6;
  if (forward(&bad, &w, 1, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "n must lie in [2, 5]")) return 20;
  bad = s; bad.B = 1; bad.T = 1;
  if (forward(&bad, &w, 1, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "training needs more than one row")) return 21;
  if (forward(&s, &w, 1, x, 0, 1.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "p_drop must lie in [0, 1)")) return 22;
  if (forward(&s, &w, 1, x, 0, 0.5f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "needs all n keep-masks")) return 23;
  if (forward(&s, &w, 1, x, keep, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "although p_drop == 0")) return 24;
  keep[4] = 0;
  if (forward(&s, &w, 1, x, keep, 0.5f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "needs all n keep-masks")) return 25;
  if (forward(&s, &w, 1, x + 1, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "16-byte aligned")) return 26;
  w.layer[3].running_mean = 0;
  if (forward(&s, &w, 0, x, 0, 0.0f, y, saved, ws, need, 0) == 0 || !strstr(last_error(), "null weights->layer[3].running_mean")) return 27;
  w.layer[3].running_mean = (float*)0x7000000;
  if (backward(&s, &w, 1, x, 0, 0.0f, 0, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 28;
  d.layer[2].w = (float*)0x8000004;
  if (backward(&s, &w, 1, x, 0, 0.0f, saved, g, &d, ws, need, 0) == 0 || !strstr(last_error(), "every gradient must be 16-byte aligned")) return 29;
  d.layer[2].w = 0;
  if (backward(&s, &w, 1, x, 0, 0.0f, saved, g, &d, ws, need, 0) != 0) return 30; /* nothing wanted: nothing launched */
  if (stats(x, 64, 80, 1, 0, 0, 0, st, ws, 16, 0) == 0 || !strstr(last_error(), "workspace too small")) return 31;
  if (stats(x, 64, 72, 1, 0, 0, 0, st, ws, need, 0) == 0 || !strstr(last_error(), "C must be a multiple of 16")) return 32;
  if (apply(x, st, x, x, 0, 0.5f, 0, 64, 80, y, 0) == 0 || !strstr(last_error(), "needs a keep-mask")) return 33;
  if (reduce(x, x, 0, st, 0, 0.0f, 0, 64, 80, y, y, st, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 34;
  if (bwd_apply(x, x, x, st, st, x, 0, 0.0f, 0, 64, 80, 96, y, 0, 0, 0, 0) == 0 || !strstr(last_error(), "ldz must be C, or 128")) return 35;
  if (narrow(x, x, 2, 32, 128, 512, 5, y, ws, need, 0) == 0 || !strstr(last_error(), "N must be a multiple of 16 below 128")) return 36;
  if (narrow(x, x, 2, 32, 80, 512, 5, y, ws, 1024, 0) == 0 || !strstr(last_error(), "workspace too small")) return 37;
  printf("C caller ok\n");
  return 0;
}
