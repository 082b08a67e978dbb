/* A plain-C caller of the ns_km_* family of include/nar_fs2.h (gcc -std=c99 -pedantic): the header must be usable from C, every refusal
 * must be reached through dlopen/dlsym without a GPU (validation precedes the first HIP call), and the two host entry points
 * (ns_km_op_philox, ns_km_host_draw) must give the known answers.  Run by tests/test_keepmask_host.py. */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "nar_fs2.h"

typedef const char* (*last_error_fn)(void);
typedef int (*version_fn)(void);
typedef int (*threshold_fn)(double, uint32_t*);
typedef size_t (*table_bytes_fn)(int);
typedef int (*plan_fn)(const ns_km_mask*, int, void*, size_t, uint64_t*);
typedef int (*draw_fn)(const void*, int, uint64_t, uint64_t, void*, size_t, void*);
typedef int (*philox_fn)(const uint32_t*, const uint32_t*, uint32_t*);
typedef int (*host_draw_fn)(const void*, int, uint64_t, uint64_t, void*, size_t);

int main(int argc, char** argv) {
  void* so;
  /* made-up device addresses: never dereferenced */
  void* table_dev = (void*)0x1000000; void* arena_dev = (void*)0x2000000;
  static const unsigned char first32[32] = {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1};
  ns_km_mask masks[2], bad[2];
  unsigned char table[3 * NS_KM_TABLE_ROW_BYTES];
  unsigned char arena[32 + 48 + 16];
  uint32_t thr = 0, ctr[4] = {0, 0, 1, 0}, key[2] = {1234, 0}, out[4];
  uint64_t need = 0;
  int i;
  last_error_fn last_error; version_fn version, launches; threshold_fn threshold; table_bytes_fn table_bytes; plan_fn plan; draw_fn draw;
  philox_fn philox; host_draw_fn host_draw;
  if (argc < 2) return 2;
  so = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!so) { printf("dlopen: %s\n", dlerror()); return 3; }
  *(void**)(&last_error) = dlsym(so, "ns_last_error");
  *(void**)(&version) = dlsym(so, "ns_km_abi_version");
  *(void**)(&launches) = dlsym(so, "ns_km_last_launches");
  *(void**)(&threshold) = dlsym(so, "ns_km_threshold");
  *(void**)(&table_bytes) = dlsym(so, "ns_km_table_bytes");
  *(void**)(&plan) = dlsym(so, "ns_km_plan");
  *(void**)(&draw) = dlsym(so, "ns_km_draw");
  *(void**)(&philox) = dlsym(so, "ns_km_op_philox");
  *(void**)(&host_draw) = dlsym(so, "ns_km_host_draw");
  if (!last_error || !version || !launches || !threshold || !table_bytes || !plan || !draw || !philox || !host_draw) { printf("missing symbol\n"); return 4; }
  if (version() != NS_KM_ABI_VERSION) { printf("ABI version mismatch\n"); return 5; }
  /* ns_km_threshold */
  if (threshold(0.2, &thr) != 0 || thr != 3435973836u) return 10;
  if (threshold(0.1, &thr) != 0 || thr != 3865470566u) return 11;
  if (threshold(0.5, &thr) != 0 || thr != 2147483648u) return 12;
  if (threshold(0.2, 0) == 0 || !strstr(last_error(), "null argument")) return 13;
  if (threshold(0.0, &thr) == 0 || !strstr(last_error(), "p must lie in (0, 1)")) return 14;
  if (threshold(1.0, &thr) == 0 || !strstr(last_error(), "p must lie in (0, 1)")) return 15;
  if (threshold(1.0 - 1e-12, &thr) == 0 || !strstr(last_error(), "the threshold would be 0")) return 16;
  if (threshold(1e-30, &thr) == 0 || !strstr(last_error(), "does not fit 32 bits")) return 17;
  /* ns_km_table_bytes, ns_km_plan */
  if (table_bytes(2) != sizeof(table) || table_bytes(NS_KM_MAX_MASKS) != (NS_KM_MAX_MASKS + 1) * NS_KM_TABLE_ROW_BYTES) return 20;
  if (table_bytes(0) != 0 || !strstr(last_error(), "n_masks must lie in [1, 1024]")) return 21;
  if (table_bytes(NS_KM_MAX_MASKS + 1) != 0 || !strstr(last_error(), "n_masks must lie in [1, 1024]")) return 22;
  threshold(0.2, &thr);
  masks[0].n = 32; masks[0].stream = 0; masks[0].thr = thr;
  masks[1].n = 33; masks[1].stream = 1; masks[1].thr = thr;
  if (plan(0, 2, table, sizeof(table), &need) == 0 || !strstr(last_error(), "null argument")) return 23;
  if (plan(masks, 2, 0, sizeof(table), &need) == 0 || !strstr(last_error(), "null argument")) return 24;
  if (plan(masks, 2, table, sizeof(table), 0) == 0 || !strstr(last_error(), "null argument")) return 25;
  if (plan(masks, 0, table, sizeof(table), &need) == 0 || !strstr(last_error(), "n_masks must lie in")) return 26;
  if (plan(masks, NS_KM_MAX_MASKS + 1, table, sizeof(table), &need) == 0 || !strstr(last_error(), "n_masks must lie in")) return 27;
  if (plan(masks, 2, table, sizeof(table) - 1, &need) == 0 || !strstr(last_error(), "table too small (ns_km_table_bytes)")) return 28;
  memcpy(bad, masks, sizeof(masks)); bad[1].n = 0;
  if (plan(bad, 2, table, sizeof(table), &need) == 0 || !strstr(last_error(), "masks[1].n must be positive")) return 29;
  memcpy(bad, masks, sizeof(masks)); bad[0].n = (uint64_t)1 << 34;
  if (plan(bad, 2, table, sizeof(table), &need) == 0 || !strstr(last_error(), "masks[0].n must stay below 2^34")) return 30;
  memcpy(bad, masks, sizeof(masks)); bad[1].thr = 0;
  if (plan(bad, 2, table, sizeof(table), &need) == 0 || !strstr(last_error(), "masks[1].thr must not be 0")) return 31;
  if (plan(masks, 2, table, sizeof(table), &need) != 0 || need != 32 + 48) return 32;
  /* ns_km_draw: every refusal comes before the first HIP call */
  if (draw(0, 2, 1234, 1, arena_dev, 80, 0) == 0 || !strstr(last_error(), "null argument")) return 40;
  if (draw(table_dev, 2, 1234, 1, 0, 80, 0) == 0 || !strstr(last_error(), "null argument")) return 41;
  if (draw(table_dev, 0, 1234, 1, arena_dev, 80, 0) == 0 || !strstr(last_error(), "n_masks must lie in")) return 42;
  if (draw((char*)table_dev + 4, 2, 1234, 1, arena_dev, 80, 0) == 0 || !strstr(last_error(), "the table must be 8-byte aligned")) return 43;
  if (draw(table_dev, 2, 1234, 1, (char*)arena_dev + 8, 80, 0) == 0 || !strstr(last_error(), "the arena must be 16-byte aligned")) return 44;
  if (draw(table_dev, 2, 1234, 1, arena_dev, 31, 0) == 0 || !strstr(last_error(), "arena too small")) return 45;
  if (launches() != 0) return 46; /* a refused call launched nothing */
  /* ns_km_op_philox */
  if (philox(0, key, out) == 0 || !strstr(last_error(), "null argument")) return 50;
  if (philox(ctr, 0, out) == 0 || philox(ctr, key, 0) == 0) return 51;
  if (philox(ctr, key, out) != 0 || out[0] != 0xd115a128u || out[1] != 0x52fc7c75u || out[2] != 0xc7f33f17u || out[3] != 0x0f1539dbu) return 52;
  /* ns_km_host_draw: seed 1234, call 1, stream 0, p 0.2 */
  memset(arena, 0xA5, sizeof(arena));
  if (host_draw(0, 2, 1234, 1, arena, sizeof(arena)) == 0 || !strstr(last_error(), "null argument")) return 60;
  if (host_draw(table, 2, 1234, 1, 0, sizeof(arena)) == 0 || !strstr(last_error(), "null argument")) return 61;
  if (host_draw(table, 2, 1234, 1, arena, 79) == 0 || !strstr(last_error(), "arena too small")) return 62;
  if (host_draw(table, 2, 1234, 1, arena, sizeof(arena)) != 0) return 63;
  if (memcmp(arena, first32, 32) != 0) return 64;
  for (i = 32 + 33; i < 32 + 48; ++i) if (arena[i] != 0) return 65;           /* the tail of the second slot is written as 0 */
  for (i = 32 + 48; i < (int)sizeof(arena); ++i) if (arena[i] != 0xA5) return 66; /* nothing outside a slot is written */
  printf("first 32 bytes of seed 1234, call 1, stream 0, p 0.2 match\n");
  printf("C caller ok\n");
  return 0;
}
