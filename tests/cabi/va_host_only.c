/* A plain-C caller of the ns_va_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, the plan and
 * size queries must work, and every refusal must be reached through dlopen/dlsym without a GPU (validation precedes the first HIP
 * call).  Run by tests/test_variance_adaptor_grad_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef int (*plan_fn)(int, int, int, int32_t*);
typedef size_t (*bytes_fn)(int, int, int);
typedef int (*embed_fwd_fn)(const float*, const float*, const float*, const float*, int, int, int, float*, int32_t*, void*);
typedef int (*embed_bwd_fn)(const float*, const int32_t*, int, int, int, float*, void*, size_t, void*);
typedef int (*lr_fwd_fn)(const float*, const int64_t*, int, int, int, int, float*, int32_t*, int64_t*, void*);
typedef int (*lr_bwd_fn)(const float*, const int32_t*, int, int, int, int, float*, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* y = (float*)0x2000000; float* t = (float*)0x2100000;
  int32_t* idx = (int32_t*)0x2200000; int64_t* dur = (int64_t*)0x2300000; int64_t* len = (int64_t*)0x2400000;
  void* ws = (void*)0x4000000;
  int32_t plan[8];
  size_t need;
  last_error_fn last_error; version_fn version, launches; plan_fn plan_embed; bytes_fn ws_bytes;
  embed_fwd_fn embed_fwd; embed_bwd_fn embed_bwd; lr_fwd_fn lr_fwd; lr_bwd_fn lr_bwd;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_va_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_va_last_launches");
  *(void**)(&plan_embed) = dlsym(so, "ns_va_plan_embed");
  *(void**)(&ws_bytes) = dlsym(so, "ns_va_embed_ws_bytes");
  *(void**)(&embed_fwd) = dlsym(so, "ns_va_op_embed_fwd");
  *(void**)(&embed_bwd) = dlsym(so, "ns_va_op_embed_bwd");
  *(void**)(&lr_fwd) = dlsym(so, "ns_va_op_lr_fwd");
  *(void**)(&lr_bwd) = dlsym(so, "ns_va_op_lr_bwd");
  if (!last_error || !version || !launches || !plan_embed || !ws_bytes || !embed_fwd || !embed_bwd || !lr_fwd || !lr_bwd) {
    printf("missing symbol\n");
    return 4;
  }
  if (version() != NS_VA_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  /* the plan and the sizes: the flagship's 16 x 1010 frame rows, 256 bins of 256 columns */
  if (plan_embed(16160, 256, 256, plan) != 0) { printf("plan: %s\n", last_error()); return 6; }
  if (plan[0] != 32 || plan[1] != 512 || plan[2] != 32 || plan[3] != 8 || plan[4] != 65536 || plan[5] != 2 || plan[6] != 64 || plan[7] != 0) return 7;
  need = ws_bytes(16160, 256, 256);
  if (need != (size_t)8 * 32 * 256 * 256) return 8;
  if (plan_embed(8, 254, 256, plan) == 0 || !strstr(last_error(), "D must be a positive multiple of 4") || plan[0] != 0) return 9;
  if (plan_embed(8, 256, 1, plan) == 0 || !strstr(last_error(), "n_bins must be at least 2")) return 10;
  if (plan_embed(8, 256, 4096, 0) == 0 || !strstr(last_error(), "cannot hold this shape")) return 11;
  if (ws_bytes(0, 256, 256) != 0 || !strstr(last_error(), "M must be positive")) return 12;
  /* the launching calls refuse before any HIP call */
  if (embed_fwd(x, t, t, x, 16160, 256, 256, y, 0, 0) == 0 || !strstr(last_error(), "null argument")) return 15;
  if (embed_fwd(x + 1, t, t, x, 16160, 256, 256, y, idx, 0) == 0 || !strstr(last_error(), "x must be 16-byte aligned")) return 16;
  if (embed_fwd(x, t, t, x, 16160, 256, 4096, y, idx, 0) == 0 || !strstr(last_error(), "cannot hold this shape")) return 17;
  if (embed_bwd(x, idx, 16160, 256, 256, y, ws, need - 1, 0) == 0 || !strstr(last_error(), "workspace too small")) return 18;
  if (embed_bwd(x, idx, 16160, 256, 256, y, 0, need, 0) == 0 || !strstr(last_error(), "null argument")) return 19;
  if (embed_bwd(x, idx, 1 << 20, 1 << 11, 8, y, ws, need, 0) == 0 || !strstr(last_error(), "problem too large")) return 20;
  if (lr_fwd(x, 0, 16, 128, 256, 1010, 0, idx, len, 0) == 0 || !strstr(last_error(), "null argument")) return 21;
  if (lr_fwd(x, dur, 16, 128, 256, 0, y, idx, len, 0) == 0 || !strstr(last_error(), "T must be positive")) return 22;
  if (lr_fwd(x, dur, 16, 128, 250, 1010, y, idx, len, 0) == 0 || !strstr(last_error(), "D must be a positive multiple of 4")) return 23;
  if (lr_fwd(x, (const int64_t*)((const char*)dur + 4), 16, 128, 256, 1010, y, idx, len, 0) == 0 || !strstr(last_error(), "duration must be 8-byte aligned"))
    return 24;
  if (lr_bwd(x, idx, 16, 0, 256, 1010, y, 0) == 0 || !strstr(last_error(), "B and L must be positive")) return 25;
  if (lr_bwd(x, idx, 16, 128, 256, 1010, y + 1, 0) == 0 || !strstr(last_error(), "d_x must be 16-byte aligned")) return 26;
  if (lr_bwd(x, 0, 16, 128, 256, 1010, y, 0) == 0 || !strstr(last_error(), "null argument")) return 27;
  if (launches() != 0) return 28;
  printf("C caller ok\n");
  return 0;
}
