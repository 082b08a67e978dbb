/* A plain-C caller of the ns_vt_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the
 * structs must have the layout the Python binding assumes, and every refusal must be reached through dlopen/dlsym without a GPU
 * (validation precedes the first HIP call).  Run by tests/test_variance_targets_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*ws_fn)(int, int, int);
typedef int (*init_fn)(ns_vt_state*, void*);
typedef int (*targets_fn)(const ns_vt_args*, void*, size_t, void*);
typedef int (*state_fn)(const ns_vt_args*, ns_vt_state*, void*, size_t, void*);

static ns_vt_args good(void) {
  ns_vt_args a;
  memset(&a, 0, sizeof(a));
  a.B = 2; a.L = 12; a.T = 40; a.energy_frame_level = 1; a.pitch_normalization = 1; a.energy_normalization = 1;
  a.durations_stride = 12;
  /* made-up addresses: never dereferenced */
  a.pitch = (const float*)0x10000; a.energy = (const float*)0x20000; a.durations = (const int64_t*)0x30000;
  a.src_lens = (const int64_t*)0x40000; a.pitch_targets = (float*)0x50000; a.energy_targets = (float*)0x60000;
  a.frame_lens = (int64_t*)0x70000; a.valid = (uint8_t*)0x80000;
  return a;
}

int main(int argc, char** argv) {
  void* so;
  void* ws = (void*)0x2000000;
  ns_vt_state* st = (ns_vt_state*)0x3000000;
  ns_vt_args a;
  size_t need;
  last_error_fn last_error; version_fn version; ws_fn ws_bytes; init_fn init; targets_fn targets; state_fn fit; state_fn normalize;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_vt_abi_version");
  *(void**)(&ws_bytes) = dlsym(so, "ns_vt_ws_bytes");
  *(void**)(&init) = dlsym(so, "ns_vt_state_init");
  *(void**)(&targets) = dlsym(so, "ns_vt_targets");
  *(void**)(&fit) = dlsym(so, "ns_vt_fit");
  *(void**)(&normalize) = dlsym(so, "ns_vt_normalize");
  if (!last_error || !version || !ws_bytes || !init || !targets || !fit || !normalize) { printf("missing symbol\n"); return 4; }
  if (version() != NS_VT_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  if (sizeof(ns_vt_state) != 80 || sizeof(ns_vt_args) != 104) { printf("struct layout: %u %u\n", (unsigned)sizeof(ns_vt_state), (unsigned)sizeof(ns_vt_args)); return 6; }
  need = ws_bytes(2, 12, 40);
  if (need == 0 || ws_bytes(3, 12, 40) < need || ws_bytes(2, 12, 41) < need || ws_bytes(0, 0, 0) == 0) return 7;
  if (init(0, 0) == 0 || !strstr(last_error(), "null state")) return 8;
  if (targets(0, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 9;
  a = good(); a.T = -1;
  if (targets(&a, ws, need, 0) == 0 || !strstr(last_error(), "negative size")) return 10;
  a = good(); a.durations_stride = 11;
  if (targets(&a, ws, need, 0) == 0 || !strstr(last_error(), "durations_stride")) return 11;
  a = good();
  if (targets(&a, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 12;
  a = good(); a.durations = 0;
  if (targets(&a, ws, need, 0) == 0 || !strstr(last_error(), "null durations")) return 13;
  a = good(); a.T = NS_VT_SORT_CAPACITY + 1;
  if (fit(&a, st, ws, ws_bytes(2, 12, NS_VT_SORT_CAPACITY + 1), 0) == 0 || !strstr(last_error(), "sort capacity")) return 14;
  a = good();
  if (fit(&a, 0, ws, need, 0) == 0 || !strstr(last_error(), "null state")) return 15;
  if (normalize(&a, 0, ws, need, 0) == 0 || !strstr(last_error(), "null state")) return 16;
  a.pitch_targets = 0;
  if (normalize(&a, st, ws, need, 0) == 0 || !strstr(last_error(), "null pitch_targets")) return 17;
  printf("C caller ok\n");
  return 0;
}
