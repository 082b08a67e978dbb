/* A plain-C caller of the ns_st_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C and every
 * refusal must be reached through dlopen/dlsym without a GPU (validation precedes the first HIP call).  Run by
 * tests/test_stacks_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef int (*embed_pos_fn)(const int64_t*, const float*, const float*, int, int, int, int, float*, void*);
typedef int (*add_pos_fn)(const float*, const float*, int, int, int, float*, void*);
typedef int (*embed_grad_fn)(const float*, const int64_t*, int, int, int, float*, void*);
typedef int (*row_mask_fn)(const float*, const uint8_t*, const int64_t*, int, int, int, float*, void*);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  float* x = (float*)0x1000000; float* y = (float*)0x2000000; float* emb = (float*)0x3000000; float* pos = (float*)0x4000000;
  int64_t* texts = (int64_t*)0x5000000; int64_t* lens = (int64_t*)0x6000000;
  uint8_t* mask = (uint8_t*)0x7000001; /* a byte mask needs no alignment */
  last_error_fn last_error; version_fn version, launches; embed_pos_fn embed_pos; add_pos_fn add_pos; embed_grad_fn embed_grad; row_mask_fn row_mask;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_st_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_st_last_launches");
  *(void**)(&embed_pos) = dlsym(so, "ns_st_op_embed_pos");
  *(void**)(&add_pos) = dlsym(so, "ns_st_op_add_pos");
  *(void**)(&embed_grad) = dlsym(so, "ns_st_op_embed_grad");
  *(void**)(&row_mask) = dlsym(so, "ns_st_op_row_mask");
  if (!last_error || !version || !launches || !embed_pos || !add_pos || !embed_grad || !row_mask) { printf("missing symbol\n"); return 4; }
  if (version() != NS_ST_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  /* ns_st_op_embed_pos */
  if (embed_pos(0, emb, pos, 2, 8, 256, 361, y, 0) == 0 || !strstr(last_error(), "null argument")) return 10;
  if (embed_pos(texts, emb, pos, 2, 8, 256, 361, 0, 0) == 0 || !strstr(last_error(), "null argument")) return 11;
  if (embed_pos(texts, emb, pos, 0, 8, 256, 361, y, 0) == 0 || !strstr(last_error(), "must be positive")) return 12;
  if (embed_pos(texts, emb, pos, 2, 8, 384, 361, y, 0) == 0 || !strstr(last_error(), "D must be 256 or 512")) return 13;
  if (embed_pos(texts, emb, pos, 2, 8, 256, 1, y, 0) == 0 || !strstr(last_error(), "n_vocab must be at least 2")) return 14;
  if (embed_pos(texts, emb, pos, 1 << 11, 1 << 12, 256, 361, y, 0) == 0 || !strstr(last_error(), "problem too large")) return 15;
  if (embed_pos(texts, emb + 1, pos, 2, 8, 256, 361, y, 0) == 0 || !strstr(last_error(), "emb must be 16-byte aligned")) return 16;
  if (embed_pos((const int64_t*)0x5000004, emb, pos, 2, 8, 256, 361, y, 0) == 0 || !strstr(last_error(), "texts must be 8-byte aligned")) return 17;
  /* ns_st_op_add_pos */
  if (add_pos(x, 0, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "null argument")) return 20;
  if (add_pos(x, pos, 2, -1, 256, y, 0) == 0 || !strstr(last_error(), "must be positive")) return 21;
  if (add_pos(x, pos, 2, 8, 128, y, 0) == 0 || !strstr(last_error(), "D must be 256 or 512")) return 22;
  if (add_pos(x, pos, 1 << 11, 1 << 11, 512, y, 0) == 0 || !strstr(last_error(), "problem too large")) return 23;
  if (add_pos(x, pos + 2, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "pos must be 16-byte aligned")) return 24;
  /* ns_st_op_embed_grad */
  if (embed_grad(0, texts, 16, 256, 361, y, 0) == 0 || !strstr(last_error(), "null argument")) return 30;
  if (embed_grad(x, texts, 0, 256, 361, y, 0) == 0 || !strstr(last_error(), "M must be positive")) return 31;
  if (embed_grad(x, texts, 16, 1024, 361, y, 0) == 0 || !strstr(last_error(), "D must be 256 or 512")) return 32;
  if (embed_grad(x, texts, 16, 256, 0, y, 0) == 0 || !strstr(last_error(), "n_vocab must be at least 2")) return 33;
  if (embed_grad(x, texts, 1 << 23, 256, 361, y, 0) == 0 || !strstr(last_error(), "problem too large")) return 34;
  if (embed_grad(x, texts, 16, 256, 361, y + 1, 0) == 0 || !strstr(last_error(), "d_table must be 16-byte aligned")) return 35;
  /* ns_st_op_row_mask */
  if (row_mask(0, mask, lens, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "null argument")) return 40;
  if (row_mask(x, 0, 0, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "neither mask nor lens")) return 41;
  if (row_mask(x, mask, 0, 2, 0, 256, y, 0) == 0 || !strstr(last_error(), "must be positive")) return 42;
  if (row_mask(x, mask, 0, 2, 8, 100, y, 0) == 0 || !strstr(last_error(), "D must be 256 or 512")) return 43;
  if (row_mask(x, mask, 0, 1 << 12, 1 << 11, 256, y, 0) == 0 || !strstr(last_error(), "problem too large")) return 44;
  if (row_mask(x, mask, 0, 2, 8, 256, x, 0) == 0 || !strstr(last_error(), "out of place")) return 45;
  if (row_mask(x, 0, (const int64_t*)0x6000004, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "lens must be 8-byte aligned")) return 46;
  if (row_mask(x + 1, mask, 0, 2, 8, 256, y, 0) == 0 || !strstr(last_error(), "x must be 16-byte aligned")) return 47;
  if (launches() != 0) return 50; /* a refused call launched nothing */
  printf("C caller ok\n");
  return 0;
}
