/* A plain-C caller of the ns_mh_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C and every
 * refusal must be reached through dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by
 * tests/test_train_align_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*bytes_fn)(const ns_mh_shape*);
typedef int (*forward_fn)(const ns_mh_shape*, const ns_mh_weights*, const float*, float*, void*, size_t, void*);
typedef int (*backward_fn)(const ns_mh_shape*, const ns_mh_weights*, const float*, const float*, const ns_mh_grads*, void*, size_t, void*);
typedef int (*pad_fn)(const float*, int, int, float*, float*, void*, size_t, void*);
typedef int (*residual_fn)(const float*, const float*, int, int, float*, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* y = (float*)0x2000000; float* g = (float*)0x3000000; float* dz = (float*)0x4000000;
  void* ws = (void*)0x6000000;
  ns_mh_shape s = {2, 8, 256, 80}, bad;
  ns_mh_weights k = {(const float*)0x8000000, (const float*)0x8100000}, kbad;
  ns_mh_grads d = {(float*)0x9000000, (float*)0x9100000, (float*)0x9200000}, none = {0, 0, 0}, dbad;
  size_t n;
  last_error_fn last_error; version_fn version, launches; bytes_fn ws_bytes; forward_fn forward; backward_fn backward; pad_fn pad;
  residual_fn residual;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_mh_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_mh_last_launches");
  *(void**)(&ws_bytes) = dlsym(so, "ns_mh_ws_bytes");
  *(void**)(&forward) = dlsym(so, "ns_mh_forward");
  *(void**)(&backward) = dlsym(so, "ns_mh_backward");
  *(void**)(&pad) = dlsym(so, "ns_mh_op_pad_colsum");
  *(void**)(&residual) = dlsym(so, "ns_mh_op_residual");
  if (!last_error || !version || !launches || !ws_bytes || !forward || !backward || !pad || !residual) { printf("missing symbol\n"); return 4; }
  if (version() != NS_MH_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  /* sizes */
  n = ws_bytes(&s);
  if (n == 0 || n % 256 != 0) return 6;
  bad = s; bad.d = 128;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "d must be 256 or 512")) return 7;
  bad = s; bad.n_mel = 84;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "n_mel must be a multiple of 16 in [16, 128]")) return 8;
  bad = s; bad.n_mel = 144;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "n_mel must be a multiple of 16 in [16, 128]")) return 9;
  if (ws_bytes(0) != 0 || !strstr(last_error(), "null argument")) return 10;
  bad = s; bad.B = 1 << 12; bad.T = 1 << 11;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "B * T * d must stay below 2^31")) return 11;
  /* ns_mh_forward */
  if (forward(0, &k, x, y, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 20;
  if (forward(&s, 0, x, y, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 21;
  if (forward(&s, &k, 0, y, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 22;
  if (forward(&s, &k, x, 0, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 23;
  bad = s; bad.B = 0;
  if (forward(&bad, &k, x, y, ws, n, 0) == 0 || !strstr(last_error(), "must be positive")) return 24;
  bad = s; bad.d = 384;
  if (forward(&bad, &k, x, y, ws, n, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 25;
  bad = s; bad.n_mel = 0;
  if (forward(&bad, &k, x, y, ws, n, 0) == 0 || !strstr(last_error(), "n_mel must be a multiple of 16")) return 26;
  kbad = k; kbad.b = 0;
  if (forward(&s, &kbad, x, y, ws, n, 0) == 0 || !strstr(last_error(), "null weights->b")) return 27;
  kbad = k; kbad.w = (const float*)0x8000004;
  if (forward(&s, &kbad, x, y, ws, n, 0) == 0 || !strstr(last_error(), "weights->w must be 16-byte aligned")) return 28;
  if (forward(&s, &k, x + 1, y, ws, n, 0) == 0 || !strstr(last_error(), "x must be 16-byte aligned")) return 29;
  if (forward(&s, &k, x, y + 2, ws, n, 0) == 0 || !strstr(last_error(), "y must be 16-byte aligned")) return 30;
  if (forward(&s, &k, x, y, ws, n - 1, 0) == 0 || !strstr(last_error(), "workspace too small (ns_mh_ws_bytes)")) return 31;
  /* ns_mh_backward */
  if (backward(&s, &k, 0, g, &d, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 40;
  if (backward(&s, &k, x, 0, &d, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 41;
  if (backward(&s, &k, x, g, 0, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 42;
  if (backward(&s, &k, x, g, &d, 0, n, 0) == 0 || !strstr(last_error(), "null argument")) return 43;
  dbad = d; dbad.w = (float*)0x9100004;
  if (backward(&s, &k, x, g, &dbad, ws, n, 0) == 0 || !strstr(last_error(), "every gradient must be 16-byte aligned")) return 44;
  bad = s; bad.T = -1;
  if (backward(&bad, &k, x, g, &d, ws, n, 0) == 0 || !strstr(last_error(), "must be positive")) return 45;
  if (backward(&s, &k, x, g + 1, &d, ws, n, 0) == 0 || !strstr(last_error(), "g must be 16-byte aligned")) return 46;
  if (backward(&s, &k, x, g, &d, ws, 0, 0) == 0 || !strstr(last_error(), "workspace too small")) return 47;
  if (backward(&s, &k, x, g, &none, ws, n, 0) != 0 || launches() != 0) return 48; /* nothing wanted: accepted, nothing launched */
  /* the two kernels alone */
  if (pad(0, 16, 80, dz, y, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "null argument")) return 50;
  if (pad(g, 16, 80, 0, y, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "null argument")) return 51;
  if (pad(g, 16, 80, dz, y, 0, 0, 0) == 0 || !strstr(last_error(), "null argument")) return 52;
  if (pad(g, 0, 80, dz, y, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "M must be positive")) return 53;
  if (pad(g, 16, 20, dz, y, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "n_mel must be a multiple of 16")) return 54;
  if (pad(g, 1 << 24, 80, dz, y, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "problem too large")) return 55;
  if (pad(g, 16, 80, g, y, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "out of place")) return 56;
  if (pad(g, 16, 80, dz, y + 1, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "d_bias must be 16-byte aligned")) return 57;
  if (pad(g, 16, 80, dz, y, ws, 16, 0) == 0 || !strstr(last_error(), "workspace too small")) return 58;
  if (residual(0, x, 16, 80, y, 0) == 0 || !strstr(last_error(), "null argument")) return 60;
  if (residual(g, x, 0, 80, y, 0) == 0 || !strstr(last_error(), "M must be positive")) return 61;
  if (residual(g, x, 16, 136, y, 0) == 0 || !strstr(last_error(), "n_mel must be a multiple of 16")) return 62;
  if (residual(g, x, 16, 80, x, 0) == 0 || !strstr(last_error(), "out of place")) return 63;
  if (residual(g, x + 1, 16, 80, y, 0) == 0 || !strstr(last_error(), "x must be 16-byte aligned")) return 64;
  if (launches() != 0) return 70; /* a refused call launched nothing */
  printf("C caller ok\n");
  return 0;
}
