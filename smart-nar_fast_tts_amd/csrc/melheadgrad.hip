// Mel-head training kernels for gfx950 (model/fastspeech2_align.py:24,83,85):
//   k_mh_pad_colsum  dz [M, 128] = g [M, n_mel] with exact +0.0 in the columns [n_mel, 128): the feed of the weight gradient of
//                    mel_linear at the padded width PN_PAD_N, the narrowest N the plan takes; and, in the same pass, the float64
//                    column partials of g per PG_ROW_BLOCK rows (the bias gradient)
//   k_mh_residual    out = p + x over [M, n_mel]: postnet(output) + output
// Everything else of mel_linear's forward and backward is a kernel the project already has (melheadgrad_api.hip).  The partials take
// k_pn_bias_finish's [blk][n_mel] layout, so that kernel sums them in ascending block order: it takes any multiple of 16 columns,
// k_pg_col_final only multiples of 64.
// Geometry of k_mh_pad_colsum: a workgroup of 4 waves owns the 64 rows [64 blk, 64 blk + 64).  A padded row is 32 16-byte groups, so a
// wave holds two rows: lane l owns group l & 31 of the row slot 2 wave + (l >> 5), and slot s of the 8 takes the rows s, s + 8, ... of
// the block in ascending order.  A lane's float64 column sums live in registers across its rows; the 8 slots are added in slot order
// through LDS.  No atomics, no host reads; every sum has one order that depends on the shape alone (train_rows.h).
#include "kernels.h"
#include "train_rows.h"

namespace ns {

constexpr int MH_SLOTS = 8;  // row slots of a workgroup: 4 waves x 2 rows

// g is autograd's buffer and is only read; dz is the caller's workspace, uninitialised: every float of its M rows is written.
__global__ __launch_bounds__(256) void k_mh_pad_colsum(const float* __restrict__ g, int M, int n_mel, float* __restrict__ dz,
                                                       double* __restrict__ part) {
  __shared__ double red[MH_SLOTS][PN_PAD_N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = 2 * wave + (lane >> 5), col = (lane & 31) * 4;
  const bool live = col < n_mel;  // (n_mel is a multiple of 4: a group is all g or all padding)
  double cs[4] = {0.0, 0.0, 0.0, 0.0};
  for (int rr = slot; rr < PG_ROW_BLOCK; rr += MH_SLOTS) {
    const int m = blockIdx.x * PG_ROW_BLOCK + rr;
    if (m >= M) break;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      v = *reinterpret_cast<const f32x4*>(g + (size_t)m * n_mel + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) cs[e] += (double)v[e];
    }
    *reinterpret_cast<f32x4*>(dz + (size_t)m * PN_PAD_N + col) = v;
  }
  if (!part) return;  // (uniform: no barrier is skipped by a part of the workgroup)
#pragma unroll
  for (int e = 0; e < 4; ++e) red[slot][col + e] = cs[e];
  __syncthreads();
  if ((int)threadIdx.x < n_mel) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < MH_SLOTS; ++k) s += red[k][threadIdx.x];
    part[(size_t)blockIdx.x * n_mel + threadIdx.x] = s;
  }
}

hipError_t launch_mh_pad_colsum(const float* g, int M, int n_mel, float* dz, double* part, hipStream_t st) {
  if (n_mel <= 0 || n_mel % 4 != 0 || n_mel > PN_PAD_N) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mh_pad_colsum, dim3(pg_row_blocks(M)), dim3(256), 0, st, g, M, n_mel, dz, part);
  return hipGetLastError();
}

// One 16-byte group per thread over the M * n_mel / 4 groups of the three dense tensors.  Out of place.
__global__ __launch_bounds__(256) void k_mh_residual(const float* __restrict__ p, const float* __restrict__ x, long long groups,
                                                     float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= groups) return;
  const f32x4 a = *reinterpret_cast<const f32x4*>(p + idx * 4), b = *reinterpret_cast<const f32x4*>(x + idx * 4);
  *reinterpret_cast<f32x4*>(out + idx * 4) = a + b;
}

hipError_t launch_mh_residual(const float* p, const float* x, int M, int n_mel, float* out, hipStream_t st) {
  if (n_mel <= 0 || n_mel % 4 != 0) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  const long long groups = (long long)M * n_mel / 4;
  hipLaunchKernelGGL(k_mh_residual, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, p, x, groups, out);
  return hipGetLastError();
}

}  // namespace ns
