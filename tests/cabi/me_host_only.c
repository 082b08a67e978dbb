/* A plain-C caller of the ns_me_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C and every
 * refusal must be reached through dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by
 * tests/test_mel_encoder_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef size_t (*bytes_fn)(const ns_me_shape*);
typedef int (*forward_fn)(const ns_me_shape*, const ns_me_weights*, const float*, const float*, const uint8_t*, float, float*, void*, void*, size_t,
                          void*);
typedef int (*backward_fn)(const ns_me_shape*, const ns_me_weights*, const uint8_t*, float, const void*, const float*, const ns_me_grads*, void*,
                           size_t, void*);
typedef int (*drop_pos_fn)(const float*, const float*, const uint8_t*, float, int, int, int, float*, void*);
typedef int (*gate_fn)(const float*, const float*, const uint8_t*, float, int, int, float*, float*, void*, size_t, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* mels = (float*)0x1000000; float* pos = (float*)0x2000000; float* y = (float*)0x3000000; float* g = (float*)0x4000000;
  void* saved = (void*)0x5000000; void* ws = (void*)0x6000000; uint8_t* keep = (uint8_t*)0x7000000;
  ns_me_shape s = {2, 8, 80, 256}, bad;
  ns_me_weights k = {(const float*)0x8000000, (const float*)0x8100000, (const float*)0x8200000, (const float*)0x8300000}, kbad;
  ns_me_grads d = {(float*)0x9000000, (float*)0x9100000, (float*)0x9200000, (float*)0x9300000, (float*)0x9400000}, none = {0, 0, 0, 0, 0}, dbad;
  size_t n;
  last_error_fn last_error; version_fn version, launches; bytes_fn ws_bytes, saved_bytes; forward_fn forward; backward_fn backward;
  drop_pos_fn drop_pos; gate_fn gate;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_me_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_me_last_launches");
  *(void**)(&ws_bytes) = dlsym(so, "ns_me_ws_bytes");
  *(void**)(&saved_bytes) = dlsym(so, "ns_me_saved_bytes");
  *(void**)(&forward) = dlsym(so, "ns_me_forward");
  *(void**)(&backward) = dlsym(so, "ns_me_backward");
  *(void**)(&drop_pos) = dlsym(so, "ns_me_op_drop_pos");
  *(void**)(&gate) = dlsym(so, "ns_me_op_drop_relu_gate");
  if (!last_error || !version || !launches || !ws_bytes || !saved_bytes || !forward || !backward || !drop_pos || !gate) { printf("missing symbol\n"); return 4; }
  if (version() != NS_ME_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  /* sizes */
  n = ws_bytes(&s);
  if (n == 0 || saved_bytes(&s) != (size_t)2 * 8 * (80 + 2 * 256) * sizeof(float)) return 6;
  bad = s; bad.d = 128;
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "d must be 256 or 512")) return 7;
  bad = s; bad.n_mel = 82;
  if (saved_bytes(&bad) != 0 || !strstr(last_error(), "n_mel must be a positive multiple of 4")) return 8;
  if (ws_bytes(0) != 0 || !strstr(last_error(), "null argument")) return 9;
  bad = s; bad.n_mel = 20; /* a multiple of 4, but the GEMM dispatch takes Cin only as a multiple of 16 */
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "the Conv1D-as-GEMM dispatch refuses this shape")) return 70;
  if (saved_bytes(&bad) != 0 || !strstr(last_error(), "the Conv1D-as-GEMM dispatch refuses this shape")) return 71;
  if (forward(&bad, &k, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "the Conv1D-as-GEMM dispatch refuses this shape")) return 72;
  if (backward(&bad, &k, 0, 0.f, saved, g, &d, ws, n, 0) == 0 || !strstr(last_error(), "the Conv1D-as-GEMM dispatch refuses this shape")) return 73;
  bad = s; bad.B = 1 << 10; bad.T = 1 << 11; bad.n_mel = 1024; /* B * T * d = 2^29 passes, B * T * n_mel = 2^31 does not */
  if (ws_bytes(&bad) != 0 || !strstr(last_error(), "B * T * n_mel must stay below 2^31")) return 74;
  if (forward(&bad, &k, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "B * T * n_mel must stay below 2^31")) return 75;
  if (backward(&bad, &k, 0, 0.f, saved, g, &d, ws, n, 0) == 0 || !strstr(last_error(), "B * T * n_mel must stay below 2^31")) return 76;
  /* ns_me_forward */
  if (forward(0, &k, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 10;
  if (forward(&s, &k, 0, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 11;
  if (forward(&s, &k, mels, 0, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 12;
  bad = s; bad.B = 0;
  if (forward(&bad, &k, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "must be positive")) return 13;
  bad = s; bad.d = 384;
  if (forward(&bad, &k, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 14;
  bad = s; bad.n_mel = 0;
  if (forward(&bad, &k, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "n_mel must be a positive multiple of 4")) return 15;
  bad = s; bad.B = 1 << 12; bad.T = 1 << 11;
  if (forward(&bad, &k, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "problem too large")) return 16;
  kbad = k; kbad.b1 = 0;
  if (forward(&s, &kbad, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "null weights->b1")) return 17;
  kbad = k; kbad.w2 = (const float*)0x8200004;
  if (forward(&s, &kbad, mels, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "weights->w2 must be 16-byte aligned")) return 18;
  if (forward(&s, &k, mels, pos, 0, 0.2f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "p_drop > 0 needs a keep-mask")) return 19;
  if (forward(&s, &k, mels, pos, keep, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "given although p_drop == 0")) return 20;
  if (forward(&s, &k, mels, pos, keep, 1.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "p_drop must lie in [0, 1)")) return 21;
  if (forward(&s, &k, mels, pos, keep + 4, 0.2f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "keep-mask must be 16-byte aligned")) return 22;
  if (forward(&s, &k, mels + 1, pos, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "mels must be 16-byte aligned")) return 23;
  if (forward(&s, &k, mels, pos + 2, 0, 0.f, y, saved, ws, n, 0) == 0 || !strstr(last_error(), "pos must be 16-byte aligned")) return 24;
  if (forward(&s, &k, mels, pos, 0, 0.f, y, saved, ws, n - 1, 0) == 0 || !strstr(last_error(), "workspace too small (ns_me_ws_bytes)")) return 25;
  /* ns_me_backward */
  if (backward(&s, &k, 0, 0.f, 0, g, &d, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 30;
  if (backward(&s, &k, 0, 0.f, saved, 0, &d, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 31;
  if (backward(&s, &k, 0, 0.f, saved, g, 0, ws, n, 0) == 0 || !strstr(last_error(), "null argument")) return 32;
  dbad = d; dbad.dmels = (float*)0x9000004;
  if (backward(&s, &k, 0, 0.f, saved, g, &dbad, ws, n, 0) == 0 || !strstr(last_error(), "every gradient must be 16-byte aligned")) return 33;
  bad = s; bad.T = -1;
  if (backward(&bad, &k, 0, 0.f, saved, g, &d, ws, n, 0) == 0 || !strstr(last_error(), "must be positive")) return 34;
  if (backward(&s, &k, 0, 0.2f, saved, g, &d, ws, n, 0) == 0 || !strstr(last_error(), "p_drop > 0 needs a keep-mask")) return 35;
  if (backward(&s, &k, 0, 0.f, saved, g + 1, &d, ws, n, 0) == 0 || !strstr(last_error(), "g must be 16-byte aligned")) return 36;
  if (backward(&s, &k, 0, 0.f, saved, g, &d, ws, 0, 0) == 0 || !strstr(last_error(), "workspace too small")) return 37;
  if (backward(&s, &k, 0, 0.f, saved, g, &none, ws, n, 0) != 0 || launches() != 0) return 38; /* nothing wanted: accepted, nothing launched */
  /* the two kernels alone */
  if (drop_pos(0, pos, 0, 0.f, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "null argument")) return 40;
  if (drop_pos(mels, pos, 0, 0.f, 2, 0, 256, y, 0) == 0 || !strstr(last_error(), "must be positive")) return 41;
  if (drop_pos(mels, pos, 0, 0.f, 2, 8, 100, y, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 42;
  if (drop_pos(mels, pos, 0, 0.f, 1 << 12, 1 << 11, 256, y, 0) == 0 || !strstr(last_error(), "problem too large")) return 43;
  if (drop_pos(mels, pos, 0, 0.f, 2, 8, 256, mels, 0) == 0 || !strstr(last_error(), "out of place")) return 44;
  if (drop_pos(mels, pos, 0, 0.5f, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "p_drop > 0 needs a keep-mask")) return 45;
  if (drop_pos(mels, pos + 1, 0, 0.f, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "pos must be 16-byte aligned")) return 46;
  if (gate(0, mels, 0, 0.f, 16, 256, y, pos, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "null argument")) return 50;
  if (gate(g, mels, 0, 0.f, 16, 256, y, pos, 0, 0, 0) == 0 || !strstr(last_error(), "null argument")) return 51;
  if (gate(g, mels, 0, 0.f, 0, 256, y, pos, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "M must be positive")) return 52;
  if (gate(g, mels, 0, 0.f, 16, 128, y, pos, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "d must be 256 or 512")) return 53;
  if (gate(g, mels, 0, 0.f, 1 << 23, 256, y, pos, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "problem too large")) return 54;
  if (gate(g, mels, 0, 0.f, 16, 256, g, pos, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "out of place")) return 55;
  if (gate(g, mels, keep, 0.f, 16, 256, y, pos, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "given although p_drop == 0")) return 56;
  if (gate(g, mels, 0, 0.f, 16, 256, y, pos + 1, ws, 1 << 20, 0) == 0 || !strstr(last_error(), "d_b2 must be 16-byte aligned")) return 57;
  if (gate(g, mels, 0, 0.f, 16, 256, y, pos, ws, 16, 0) == 0 || !strstr(last_error(), "workspace too small")) return 58;
  if (launches() != 0) return 60; /* a refused call launched nothing */
  printf("C caller ok\n");
  return 0;
}
