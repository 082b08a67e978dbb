/* A plain-C caller of the ns_opt_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the
 * structs must have the layout the Python binding assumes, the host-only planner and table builder must work, and every refusal
 * must be reached through dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by tests/test_optim_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef int (*plan_fn)(const int64_t*, int, ns_opt_plan*);
typedef int (*build_fn)(const int64_t*, float* const*, float* const*, const int32_t*, int, void*, size_t);
typedef int (*norm_fn)(const ns_opt_plan*, const void*, size_t, float, void*, size_t, ns_opt_record*, void*);
typedef int (*scale_fn)(const ns_opt_plan*, const void*, size_t, const ns_opt_record*, void*);
typedef int (*adam_fn)(const ns_opt_plan*, const void*, size_t, const ns_opt_hyper*, float*, float*, int64_t, const ns_opt_record*, void*);
typedef int (*zero_fn)(const ns_opt_plan*, const void*, size_t, void*);

static ns_opt_hyper good(void) {
  ns_opt_hyper h;
  memset(&h, 0, sizeof(h));
  h.lr = 1e-3; h.beta1 = 0.9; h.beta2 = 0.98; h.eps = 1e-9; h.weight_decay = 0.0; h.global_step = 1;
  return h;
}

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  void* table = (void*)0x1000000; void* ws = (void*)0x2000000;
  ns_opt_record* rec = (ns_opt_record*)0x3000000;
  float* m = (float*)0x4000000; float* v = (float*)0x5000000;
  int64_t numels[4] = {0, 1, 5, NS_OPT_CHUNK + 1};
  int32_t lags[4] = {0, 2, 0, 1};
  float* params[4] = {0, (float*)0x10004, (float*)0x20000, (float*)0x30000};
  float* grads[4] = {0, (float*)0x40000, 0, (float*)0x50004};
  ns_opt_tensor rows[4];
  ns_opt_plan plan, bigger, bad;
  ns_opt_hyper h;
  last_error_fn last_error; version_fn version; plan_fn plan_sizes; build_fn build; norm_fn grad_norm; scale_fn scale; adam_fn adam; zero_fn zero;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_opt_abi_version");
  *(void**)(&plan_sizes) = dlsym(so, "ns_opt_plan_sizes");
  *(void**)(&build) = dlsym(so, "ns_opt_build_table");
  *(void**)(&grad_norm) = dlsym(so, "ns_opt_grad_norm");
  *(void**)(&scale) = dlsym(so, "ns_opt_scale_grads");
  *(void**)(&adam) = dlsym(so, "ns_opt_adam_step");
  *(void**)(&zero) = dlsym(so, "ns_opt_zero_grads");
  if (!last_error || !version || !plan_sizes || !build || !grad_norm || !scale || !adam || !zero) { printf("missing symbol\n"); return 4; }
  if (version() != NS_OPT_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  if (sizeof(ns_opt_tensor) != 40 || sizeof(ns_opt_plan) != 40 || sizeof(ns_opt_record) != 16 || sizeof(ns_opt_hyper) != 56) {
    printf("struct layout: %u %u %u %u\n", (unsigned)sizeof(ns_opt_tensor), (unsigned)sizeof(ns_opt_plan), (unsigned)sizeof(ns_opt_record), (unsigned)sizeof(ns_opt_hyper));
    return 6;
  }
  /* the planner: 1 + 1 + 1 + 2 chunks, 0 + 4 + 8 + 4100 state floats */
  if (plan_sizes(numels, 4, &plan) != 0) { printf("plan: %s\n", last_error()); return 7; }
  if (plan.n_tensors != 4 || plan.n_chunks != 5 || plan.table_bytes != 160 || plan.ws_bytes != 40 || plan.state_floats != 4112) return 8;
  numels[2] = 9;
  if (plan_sizes(numels, 4, &bigger) != 0 || bigger.state_floats < plan.state_floats || bigger.n_chunks < plan.n_chunks) return 9;
  numels[2] = 5;
  if (plan_sizes(numels, 0, &bad) == 0 || !strstr(last_error(), "n_tensors must be positive")) return 10;
  if (plan_sizes(0, 4, &bad) == 0 || !strstr(last_error(), "null argument")) return 11;
  numels[1] = -1;
  if (plan_sizes(numels, 4, &bad) == 0 || !strstr(last_error(), "negative size")) return 12;
  numels[1] = 1;
  /* the table builder */
  if (build(numels, params, grads, lags, 4, rows, sizeof(rows)) != 0) { printf("build: %s\n", last_error()); return 13; }
  if (rows[0].chunk_begin != 0 || rows[1].chunk_begin != 1 || rows[2].chunk_begin != 2 || rows[3].chunk_begin != 3) return 14;
  if (rows[0].state_offset != 0 || rows[1].state_offset != 0 || rows[2].state_offset != 4 || rows[3].state_offset != 12) return 15;
  if (rows[1].lag != 2 || rows[1].param != params[1] || rows[1].grad != grads[1] || rows[2].grad != 0 || rows[3].numel != NS_OPT_CHUNK + 1) return 16;
  if (build(numels, params, grads, lags, 4, rows, sizeof(rows) - 1) == 0 || !strstr(last_error(), "table too small")) return 17;
  lags[3] = -1;
  if (build(numels, params, grads, lags, 4, rows, sizeof(rows)) == 0 || !strstr(last_error(), "negative lag")) return 18;
  lags[3] = 1;
  /* the launching calls refuse before any HIP call */
  if (grad_norm(0, table, 160, 1.0f, ws, 40, rec, 0) == 0 || !strstr(last_error(), "null argument")) return 19;
  if (grad_norm(&plan, table, 159, 1.0f, ws, 40, rec, 0) == 0 || !strstr(last_error(), "table too small")) return 20;
  if (grad_norm(&plan, table, 160, 1.0f, ws, 39, rec, 0) == 0 || !strstr(last_error(), "workspace too small")) return 21;
  if (grad_norm(&plan, table, 160, 1.0f, ws, 40, 0, 0) == 0 || !strstr(last_error(), "null record")) return 22;
  if (scale(&plan, 0, 160, rec, 0) == 0 || !strstr(last_error(), "null argument")) return 23;
  if (zero(&plan, table, 8, 0) == 0 || !strstr(last_error(), "table too small")) return 24;
  bad = plan; bad.n_tensors = 0;
  if (zero(&bad, table, 160, 0) == 0 || !strstr(last_error(), "n_tensors must be positive")) return 25;
  h = good(); h.beta2 = 1.0;
  if (adam(&plan, table, 160, &h, m, v, 4112, 0, 0) == 0 || !strstr(last_error(), "betas must lie in [0, 1)")) return 26;
  h = good(); h.eps = -1e-9;
  if (adam(&plan, table, 160, &h, m, v, 4112, 0, 0) == 0 || !strstr(last_error(), "eps must be >= 0")) return 27;
  h = good(); h.lr = -1.0;
  if (adam(&plan, table, 160, &h, m, v, 4112, 0, 0) == 0 || !strstr(last_error(), "lr must be >= 0")) return 28;
  h = good(); h.global_step = 0;
  if (adam(&plan, table, 160, &h, m, v, 4112, 0, 0) == 0 || !strstr(last_error(), "global_step must be >= 1")) return 29;
  h = good();
  if (adam(&plan, table, 160, &h, m, v, 4111, 0, 0) == 0 || !strstr(last_error(), "state arena too small")) return 30;
  h.fuse_clip = 1;
  if (adam(&plan, table, 160, &h, m, v, 4112, 0, 0) == 0 || !strstr(last_error(), "null record")) return 31;
  printf("C caller ok\n");
  return 0;
}
