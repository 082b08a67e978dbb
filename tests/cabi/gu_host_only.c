/* A plain-C caller of the Gaussian length regulator's entry points in the ns_va_* family of include/nar_fs2.h (gcc -std=c99
 * -pedantic): the header must be usable from C, the workspace query must work, and every refusal must be reached through dlopen/dlsym
 * without a GPU (validation precedes the first HIP call).  Run by tests/test_gaussian_grad_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*bytes_fn)(int, int, int);
typedef int (*gu_fwd_fn)(const float*, const int64_t*, int, int, int, int, float*, float*, int64_t*, void*, size_t, void*);
typedef int (*gu_bwd_fn)(const float*, const float*, const int64_t*, int, int, int, int, float*, float*, void*, size_t, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* out = (float*)0x2000000; float* saved = (float*)0x2100000; float* w = (float*)0x2200000;
  int64_t* dur = (int64_t*)0x2300000; int64_t* len = (int64_t*)0x2400000;
  void* ws = (void*)0x4000000;
  size_t need;
  last_error_fn last_error; version_fn version, launches; bytes_fn ws_bytes; gu_fwd_fn fwd; gu_bwd_fn bwd, bwd_full;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_va_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_va_last_launches");
  *(void**)(&ws_bytes) = dlsym(so, "ns_va_gu_ws_bytes");
  *(void**)(&fwd) = dlsym(so, "ns_va_op_gu_fwd");
  *(void**)(&bwd) = dlsym(so, "ns_va_op_gu_bwd");
  *(void**)(&bwd_full) = dlsym(so, "ns_va_op_gu_bwd_unbanded");
  if (!last_error || !version || !launches || !ws_bytes || !fwd || !bwd || !bwd_full) { printf("missing symbol\n"); return 4; }
  if (version() != NS_VA_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  /* the flagship's 16 x 128 phonemes at 1010 frames: the backward's denominators are the larger half */
  need = ws_bytes(16, 128, 1010);
  if (need != 64768 /* 16 * 1010 floats, rounded up to 256 bytes */) { printf("ws_bytes: %lu\n", (unsigned long)need); return 6; }
  if (ws_bytes(16, 128, 1) != 16640 /* the forward's 16 * 128 + 16 + 16 * 128 floats, rounded up */) return 7;
  if (ws_bytes(0, 128, 1010) != 0 || !strstr(last_error(), "B and L must be positive")) return 8;
  if (ws_bytes(16, 128, 0) != 0 || !strstr(last_error(), "T must be positive")) return 9;
  if (ws_bytes(16, 128, 1 << 20) != 0 || !strstr(last_error(), "T must stay below 2^20")) return 10;
  if (ws_bytes(65536, 1, 4) != 0 || !strstr(last_error(), "B must stay below 65536")) return 11;
  /* the launching calls refuse before any HIP call */
  if (fwd(x, 0, 16, 128, 256, 1010, out, saved, len, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 15;
  if (fwd(0, dur, 16, 128, 256, 1010, out, saved, len, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 16;
  if (fwd(x, dur, 16, 128, 256, 1010, out, 0, len, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 17;
  if (fwd(x, dur, 16, 128, 250, 1010, out, saved, len, ws, need, 0) == 0 || !strstr(last_error(), "D must be a positive multiple of 4")) return 18;
  if (fwd(x, dur, 16, 128, 256, 0, out, saved, len, ws, need, 0) == 0 || !strstr(last_error(), "T must be positive")) return 19;
  if (fwd(x, dur, 16, 128, 256, 1 << 20, out, saved, len, ws, need, 0) == 0 || !strstr(last_error(), "T must stay below 2^20")) return 20;
  if (fwd(x, dur, 1 << 10, 128, 1 << 11, 1 << 10, out, saved, len, ws, need, 0) == 0 || !strstr(last_error(), "problem too large")) return 21;
  if (fwd(x + 1, dur, 16, 128, 256, 1010, out, saved, len, ws, need, 0) == 0 || !strstr(last_error(), "x must be 16-byte aligned")) return 22;
  if (fwd(x, (const int64_t*)((const char*)dur + 4), 16, 128, 256, 1010, out, saved, len, ws, need, 0) == 0 ||
      !strstr(last_error(), "duration must be 8-byte aligned"))
    return 23;
  if (fwd(x, dur, 16, 128, 256, 1010, out, saved, len, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 24;
  if (bwd(0, saved, len, 16, 128, 256, 1010, out, 0, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 25;
  if (bwd(x, saved, len, 16, 128, 256, 1010, 0, 0, ws, need, 0) == 0 || !strstr(last_error(), "null argument")) return 26;
  if (bwd(x, saved, 0, 16, 0, 256, 1010, out, 0, ws, need, 0) == 0 || !strstr(last_error(), "B and L must be positive")) return 27;
  if (bwd(x, saved, 0, 16, 128, 256, 1010, out + 1, 0, ws, need, 0) == 0 || !strstr(last_error(), "d_x must be 16-byte aligned")) return 28;
  if (bwd(x, saved, 0, 16, 128, 256, 1010, out, w + 2, ws, need, 0) == 0 || !strstr(last_error(), "w_out must be 16-byte aligned")) return 29;
  if (bwd(x, saved, len, 16, 128, 256, 1010, out, w, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 30;
  if (bwd(x, saved, len, 16, 128, 256, 1 << 20, out, w, ws, need, 0) == 0 || !strstr(last_error(), "T must stay below 2^20")) return 31;
  if (bwd_full(x, saved, len, 16, 128, 254, 1010, out, w, ws, need, 0) == 0 || !strstr(last_error(), "D must be a positive multiple of 4")) return 32;
  if (launches() != 0) return 33;
  printf("C caller ok\n");
  return 0;
}
