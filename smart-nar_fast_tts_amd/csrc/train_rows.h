// Device helpers of the trainable layers' row kernels (predgrad.hip k_pg_row_*, attngrad.hip k_ag_row_*).
// One wave per row, lane l owns the 16-byte groups (64 i + l) of the row, i < NV = F / 256.  The row statistics and every row-local sum
// are float64 (two-pass variance, xor-shuffle tree: one order), so a stored value is the float64 expression of its fp32 inputs rounded
// once.  The column sums of a row backward live in registers (float64) across a wave's rows; the four waves are added in wave order
// through LDS.  These orders are what makes every gradient bit-reproducible: they are stated here, once.
#pragma once
#include "kernels.h"

namespace ns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr double LN_EPS = 1e-5;  // nn.LayerNorm's default, which the reference keeps

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NV>
__device__ inline void row_stats(const f32x4 (&x)[NV], double* mean, double* rstd) {
  constexpr int F = 256 * NV;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)x[i][e];
  const double mu = wave_sum(s) / F;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) { const double d = (double)x[i][e] - mu; q += d * d; }
  *mean = mu;
  *rstd = 1.0 / sqrt(wave_sum(q) / F + LN_EPS);
}

// keep bytes of this lane's group at `off` as four scale factors (all `scale` without a mask: p = 0 passes scale = 1).  A branch, not
// a default word of ones: both give the same factors, this form leaves the predictor's kernels with the registers they had.
__device__ inline void keep4(const uint8_t* keep, size_t off, float scale, double (&k)[4]) {
  if (keep) {
    const unsigned w = *reinterpret_cast<const unsigned*>(keep + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) k[e] = ((w >> (8 * e)) & 0xffu) ? (double)scale : 0.0;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) k[e] = (double)scale;
  }
}

// ---- column partials of a row backward: cs[slot][i][e] is this lane's running sum of column (64 i + lane) * 4 + e
// Zeroes cs[NS][NV][4].  A macro, so that the loops are unrolled inside the kernel: as a function taking the array by reference they
// are unrolled before they are inlined, the register allocator meets the stores in another order, and k_pg_row_backward<1, false>
// goes from 112 to 93 VGPRs and from 4 to 5 waves per SIMD (profiles/train_core_refactor.md) with no arithmetic changed.
#define NS_COL_ZERO(cs, NS, NV)                  \
  _Pragma("unroll") for (int s = 0; s < NS; ++s) \
  _Pragma("unroll") for (int i = 0; i < NV; ++i) \
  _Pragma("unroll") for (int e = 0; e < 4; ++e) cs[s][i][e] = 0.0

// part[s * F + col] = the four waves' cs[s] of that column, added in wave order; every thread of the 256 calls it
template <int NS, int NV>
__device__ inline void col_flush(const double (&cs)[NS][NV][4], double (&red)[4][256 * NV], double* part) {
  constexpr int F = 256 * NV;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wave][(64 * i + lane) * 4 + e] = cs[s][i][e];
    __syncthreads();
    for (int col = threadIdx.x; col < F; col += 256) part[s * F + col] = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
  }
}

}  // namespace ns
