// Dropout keep-masks from a counter-based generator (include/nar_fs2.h ns_km_*): what keepmask.hip (the kernel)
// and keepmask_api.hip (the host entry points, ns_km_op_philox and ns_km_host_draw among them) share.  A mask byte is a pure function
// of (seed, call, stream, element index):
//   block j = e >> 2 of a mask is Philox4x32-10 at counter (j, stream, call & 0xffffffff, call >> 32) and key (seed & 0xffffffff,
//   seed >> 32); element e is word e & 3 of its block; keep = word < thr.
// km_philox4x32_10 and km_draw16 are __host__ __device__: the kernel and the host draw compile this text, so the two cannot drift.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nar_fs2.h"

namespace ns {

constexpr int KM_THREAD_ELEMS = 16;                    // one thread: 16 mask bytes = four Philox blocks = one 16-byte store
constexpr int KM_BLOCK = 256;                          // threads of a workgroup
constexpr int KM_CHUNK = KM_BLOCK * KM_THREAD_ELEMS;   // 4096 elements of one mask per workgroup and turn
constexpr int KM_GRID_CAP = NS_KM_GRID_CAP;            // workgroups of a launch at most; they loop over the chunks beyond
constexpr int KM_MAX_MASKS = NS_KM_MAX_MASKS;

// One row of the table ns_km_plan writes and the kernel reads; row n_masks is the sentinel {arena bytes, 0, 0, 0, chunks of all masks}.
struct KmEntry {
  uint64_t offset;       // of the mask's slot in the arena, in bytes: a multiple of 16
  uint64_t n;            // elements; the slot is ceil(n / 16) * 16 bytes long
  uint32_t stream, thr;
  uint64_t chunk_begin;  // chunks of KM_CHUNK elements of the masks before this one
};
static_assert(sizeof(KmEntry) == NS_KM_TABLE_ROW_BYTES, "KmEntry layout");

struct KmWords { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): ten rounds, the key bumped between them.
__host__ __device__ inline KmWords km_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return KmWords{{c0, c1, c2, c3}};
}

// The 16 mask bytes of the elements [e0, e0 + 16) of one mask (e0 a multiple of 16), byte i in bits [8 (i & 3), 8 (i & 3) + 8) of
// out[i >> 2]: little-endian, so out[] stored as it is puts element e0 + i at byte i.  Elements at or past n give 0.
__host__ __device__ inline void km_draw16(uint64_t e0, uint64_t n, uint32_t stream, uint32_t thr, uint64_t seed, uint64_t call, uint32_t out[4]) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c2 = (uint32_t)call, c3 = (uint32_t)(call >> 32);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint64_t e = e0 + 4 * b;
    const KmWords r = km_philox4x32_10((uint32_t)(e >> 2), stream, c2, c3, k0, k1);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) v |= (uint32_t)(r.w[i] < thr && e + i < n) << (8 * i);
    out[b] = v;
  }
}

// The workgroups a draw of n_masks masks into arena_bytes launches: no plan of that many masks into that arena has more chunks than
// arena_bytes / KM_CHUNK + n_masks (a mask's last chunk is the only partial one), so up to the cap every chunk gets a workgroup of its own.
inline unsigned km_grid(int n_masks, uint64_t arena_bytes) {
  const uint64_t most = arena_bytes / KM_CHUNK + (uint64_t)n_masks;
  return (unsigned)(most < (uint64_t)KM_GRID_CAP ? most : (uint64_t)KM_GRID_CAP);
}

// k_km_draw over the device table: exactly one launch of km_grid workgroups.  The chunk count comes from the table's sentinel on the
// device (no host read); no byte at or past arena + arena_bytes is written whatever the table says.
hipError_t launch_km_draw(const KmEntry* table, int n_masks, uint64_t seed, uint64_t call, uint8_t* arena, uint64_t arena_bytes, hipStream_t st);

}  // namespace ns
