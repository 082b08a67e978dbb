// The tile helpers of the attention backward kernels (attngrad.hip k_ag_*, xattngrad.hip k_xg_*; DESIGN.md sections 22 and 24).
// Device-only, header-only.
//
// The layout trick is attention.hip's: the owner's 32 rows are the B operand, held in registers for the whole sweep (lane (i, h) keeps
// row i's elements 8g + 4h + e), and the swept tile of 32 rows is the A operand, read from LDS.  The product comes out transposed —
// column = the owner's row (lane & 31), the 16 values of a lane = swept rows r(j, h) = (j & 3) + 8 (j >> 2) + 4h — so everything
// per owner row (lse, D, the key mask) is lane-local, and the second contraction takes register j as its B operand as it is:
// MFMA step j / lane half h is DEFINED to be swept row r(j, h), the A operand is tile[r(j, h)][32 db + (lane & 31)], one
// conflict-free ds_read_b32.  The tile is staged through registers (k_pg_wgrad's pattern): the next tile's 16-byte global loads are
// issued before this tile's MFMAs and stored behind them.
#pragma once
#include "kernels.h"

namespace ns {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int AG_ROWS = 32;  // rows of a swept tile

// ------------------------------------------------------------------------------------------------------------------ tile staging
// A tile = AG_ROWS rows x DK floats of a row-major matrix (row stride ld), LDS row stride DK + 4 floats.  Thread t owns the 16-byte
// chunks t + 256 i, i < DK / 32.  Rows at or past `nvalid` are staged as zeros, never read.
template <int DK>
__device__ inline void ag_fetch(const float* __restrict__ base, int ld, int row0, int nvalid, int tid, f32x4 (&r)[DK / 32]) {
#pragma unroll
  for (int i = 0; i < DK / 32; ++i) {
    const int c = tid + 256 * i, row = row0 + c / (DK / 4), col = (c % (DK / 4)) * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    r[i] = zero;
    if (row < nvalid) r[i] = *reinterpret_cast<const f32x4*>(base + (size_t)row * ld + col);
  }
}
template <int DK>
__device__ inline void ag_stash(float* lds, int tid, const f32x4 (&r)[DK / 32]) {
#pragma unroll
  for (int i = 0; i < DK / 32; ++i) {
    const int c = tid + 256 * i;
    *reinterpret_cast<f32x4*>(lds + (c / (DK / 4)) * (DK + 4) + (c % (DK / 4)) * 4) = r[i];
  }
}
// T^T[swept row][owner row] = sum_k tile[swept row][k] own[owner row][k], k = 8g + 4h + e on both sides
template <int DK>
__device__ inline f32x16 ag_cross(const float* tile, int qi, int h, const f32x4 (&own)[DK / 8]) {
  f32x16 s;
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = 0.f;
  const float* tp = tile + qi * (DK + 4) + 4 * h;
#pragma unroll
  for (int g = 0; g < DK / 8; ++g) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(tp + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(t[e], own[g][e], s, 0, 0, 0);
  }
  return s;
}
// acc^T[d][owner row] += sum_j tile[r(j, h)][d] w[j][owner row]
template <int DK>
__device__ inline void ag_accumulate(const float* tile, int qi, int h, const f32x16& w, f32x16 (&acc)[DK / 32]) {
  const float* tp = tile + (4 * h) * (DK + 4) + qi;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* row = tp + ((r & 3) + 8 * (r >> 2)) * (DK + 4);
#pragma unroll
    for (int db = 0; db < DK / 32; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(row[32 * db], w[r], acc[db], 0, 0, 0);
  }
}
// the owner's row as the B operand: lane (i, h) keeps row[8g + 4h .. + 4)
template <int DK>
__device__ inline void ag_own(const float* __restrict__ row, int h, f32x4 (&own)[DK / 8]) {
#pragma unroll
  for (int g = 0; g < DK / 8; ++g) own[g] = *reinterpret_cast<const f32x4*>(row + 8 * g + 4 * h);
}
// acc^T (C/D layout: column = lane & 31 = the owner's row, row d = 32 db + (r & 3) + 8 (r >> 2) + 4h) * scale -> dst[d], 16 bytes a piece
template <int DK>
__device__ inline void ag_store(float* __restrict__ dst, int h, const f32x16 (&acc)[DK / 32], float scale, bool live) {
#pragma unroll
  for (int db = 0; db < DK / 32; ++db)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = live ? acc[db][4 * r4 + j] * scale : 0.f;
      *reinterpret_cast<f32x4*>(dst + 32 * db + 8 * r4 + 4 * h) = o;
    }
}

__device__ inline int ag_len(const long long* lens, int b, int S) {
  const long long l = lens ? lens[b] : (long long)S;
  return (int)(l < 0 ? 0 : (l < S ? l : S));
}

}  // namespace ns
