// MelEncoder training kernels for gfx950 (transformer/Models.py:103-173, transformer/Layers.py:11-26):
//   k_me_drop_pos        y = h2 keep / (1 - p) + pos[m % T]: the Prenet's dropout and the position add (Models.py:151,162) in one pass
//   k_me_drop_relu_gate  dh = (keep != 0 && h2 > 0) ? g / (1 - p) : +0.0, the backward of that dropout and of the second ReLU from the saved
//                        activation, and the float64 column partials of dh per PG_ROW_BLOCK rows (the bias gradient of w_2) in the same pass
// Everything else of the Prenet's forward and backward is a kernel the project already has (melencgrad_api.hip).  The partials take
// k_pg_col_final's [blk][slot][col] layout at F = d with slot 0 alone, so that kernel sums them: no finish of its own.
// No atomics, no host reads; every sum has one order that depends on the shape alone (train_rows.h states it).
#include "kernels.h"
#include "train_rows.h"

namespace ns {

// Workgroup = 4 waves over the rows [64 blk, 64 blk + 64) and the column slab [256 blockIdx.y, 256 blockIdx.y + 256): wave w takes the
// rows w, w + 4, ..., lane l the 16-byte group l of the slab, as the row kernels do at NV = 1.  The product of two fp32 values is exact
// in float64, so the stored value is h2 k + pos rounded to float64 and then to fp32, with or without a contraction.  Out of place.
__global__ __launch_bounds__(256) void k_me_drop_pos(const float* __restrict__ h2, const float* __restrict__ pos, const uint8_t* __restrict__ keep,
                                                     float scale, int M, int T, int F, float* __restrict__ y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.y * 256 + lane * 4;
  for (int rr = wave; rr < PG_ROW_BLOCK; rr += 4) {
    const int m = blockIdx.x * PG_ROW_BLOCK + rr;
    if (m >= M) break;
    const size_t off = (size_t)m * F + col;
    const f32x4 hv = *reinterpret_cast<const f32x4*>(h2 + off);
    const f32x4 pv = *reinterpret_cast<const f32x4*>(pos + (size_t)(m % T) * F + col);
    double k[4];
    keep4(keep, off, scale, k);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)((double)hv[e] * k[e] + (double)pv[e]);
    *reinterpret_cast<f32x4*>(y + off) = o;
  }
}

hipError_t launch_me_drop_pos(const float* h2, const float* pos, const uint8_t* keep, float scale, int M, int T, int F, float* y, hipStream_t st) {
  if (F <= 0 || F % 256 != 0 || F / 256 > 65535 || T <= 0) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_me_drop_pos, dim3(pg_row_blocks(M), F / 256), dim3(256), 0, st, h2, pos, keep, scale, M, T, F, y);
  return hipGetLastError();
}

// The same geometry.  The gate is a select on the keep byte and on the saved activation: a NaN or an infinity of g behind a dropped
// or gated element reaches neither dh nor a sum, and a NaN in h2 gates like a zero.  g is autograd's and is only read; dh is another
// buffer.  keep4's factor is `scale` (> 0) where the byte is nonzero and 0 where it is zero, so the factor itself tells the two apart.
__global__ __launch_bounds__(256) void k_me_drop_relu_gate(const float* __restrict__ g, const float* __restrict__ h2, const uint8_t* __restrict__ keep,
                                                           float scale, int M, int F, float* __restrict__ dh, double* __restrict__ part) {
  __shared__ double red[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.y * 256 + lane * 4;
  double cs[1][1][4];
  NS_COL_ZERO(cs, 1, 1);
  for (int rr = wave; rr < PG_ROW_BLOCK; rr += 4) {
    const int m = blockIdx.x * PG_ROW_BLOCK + rr;
    if (m >= M) break;
    const size_t off = (size_t)m * F + col;
    const f32x4 a = *reinterpret_cast<const f32x4*>(g + off), hv = *reinterpret_cast<const f32x4*>(h2 + off);
    double k[4];
    keep4(keep, off, scale, k);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = (k[e] != 0.0 && hv[e] > 0.f) ? (float)((double)a[e] * k[e]) : 0.f;
      cs[0][0][e] += (double)o[e];
    }
    *reinterpret_cast<f32x4*>(dh + off) = o;
  }
  if (part) col_flush(cs, red, part + (size_t)blockIdx.x * PG_SLOTS * F + blockIdx.y * 256);  // slot 0 of block blk, this slab
}

hipError_t launch_me_drop_relu_gate(const float* g, const float* h2, const uint8_t* keep, float scale, int M, int F, float* dh, double* part,
                                    hipStream_t st) {
  if (F <= 0 || F % 256 != 0 || F / 256 > 65535) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_me_drop_relu_gate, dim3(pg_row_blocks(M), F / 256), dim3(256), 0, st, g, h2, keep, scale, M, F, dh, part);
  return hipGetLastError();
}

}  // namespace ns
