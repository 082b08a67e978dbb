// Dropout keep-mask kernel for gfx950: every mask of a training step in ONE launch, from a device table of
// {arena byte offset, element count, stream, thr, chunk prefix} per mask (keepmask.h KmEntry, written by ns_km_plan).
//   k_km_draw   arena[offset_m + e] = Philox4x32-10 word (e & 3) of block (e >> 2) of mask m < thr_m, for e < n_m; 0 for the bytes of
//               the slot behind element n_m - 1; nothing outside a slot.
// Geometry: a thread produces 16 elements (four Philox blocks, j = 4 t .. 4 t + 3 of its chunk) and makes one 16-byte store; a
// workgroup of 256 threads owns one chunk of 4096 elements of one mask at a time and takes the chunks blockIdx.x, blockIdx.x + gridDim.x,
// ... of the table's chunk order (the grid is capped at KM_GRID_CAP).  The chunk prefix of the table sits in LDS once per workgroup
// (8 bytes per mask), and a chunk finds its mask there by bisection; that is the only LDS.  No atomics, no host read; a mask's bytes do
// not depend on the grid, on the arena or on the masks drawn with it.  Slots start at multiples of 16 bytes and are multiples of 16 long,
// so every store is one whole aligned 16-byte group inside its slot; a store that would end past arena_bytes is not made.
#include "keepmask.h"

namespace ns {

__global__ __launch_bounds__(KM_BLOCK) void k_km_draw(const KmEntry* __restrict__ table, int n_masks, uint64_t seed, uint64_t call,
                                                      uint8_t* __restrict__ arena, uint64_t arena_bytes) {
  __shared__ uint64_t begin[KM_MAX_MASKS + 1];
  for (int i = threadIdx.x; i <= n_masks; i += KM_BLOCK) begin[i] = table[i].chunk_begin;
  __syncthreads();
  const uint64_t total = begin[n_masks];
  for (uint64_t c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = n_masks;  // the mask of chunk c: begin[lo] <= c < begin[lo + 1] (every mask has a chunk: the prefix is strictly increasing)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (begin[mid] <= c) lo = mid; else hi = mid;
    }
    const KmEntry m = table[lo];
    const uint64_t e0 = (c - begin[lo]) * KM_CHUNK + (uint64_t)threadIdx.x * KM_THREAD_ELEMS;
    const uint64_t slot = (m.n + 15) & ~(uint64_t)15;
    if (e0 >= slot || m.offset > arena_bytes || arena_bytes - m.offset < e0 + KM_THREAD_ELEMS) continue;
    uint32_t v[4];
    km_draw16(e0, m.n, m.stream, m.thr, seed, call, v);
    *reinterpret_cast<uint4*>(arena + m.offset + e0) = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

hipError_t launch_km_draw(const KmEntry* table, int n_masks, uint64_t seed, uint64_t call, uint8_t* arena, uint64_t arena_bytes, hipStream_t st) {
  if (n_masks < 1 || n_masks > KM_MAX_MASKS || arena_bytes < 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_km_draw, dim3(km_grid(n_masks, arena_bytes)), dim3(KM_BLOCK), 0, st, table, n_masks, seed, call, arena, arena_bytes);
  return hipGetLastError();
}

}  // namespace ns
