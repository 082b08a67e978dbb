// PositionwiseFeedForward training kernel for gfx950 (transformer/SubLayers.py:62-95):
//   k_fg_relu_gate   the ReLU backward from the saved activation, dh = h > 0 ? da : +0.0, and the float64 column partials of dh per
//                    PG_ROW_BLOCK rows (the bias gradient of w_1) in the same pass
// Everything else of the layer's forward and backward is a kernel the project already has (ffngrad_api.hip).  The partials take
// k_pg_col_final's [blk][slot][col] layout at F = d_inner with slot 0 alone, so that kernel sums them: no finish of its own.
// No atomics, no host reads; every sum has one order that depends on the shape alone (train_rows.h states it).
#include "kernels.h"
#include "train_rows.h"

namespace ns {

// Workgroup = 4 waves over the rows [64 blk, 64 blk + 64) and the column slab [256 blockIdx.y, 256 blockIdx.y + 256): wave w takes the
// rows w, w + 4, ..., lane l the 16-byte group l of the slab, as the row kernels do at NV = 1.  da and dh may be the same buffer (every
// element is read and written by one thread, the read first), so neither is __restrict__.  The gate is a select: a NaN or an infinity of
// da behind h <= 0 reaches neither dh nor a sum, and a NaN in h gates like a zero.
__global__ __launch_bounds__(256) void k_fg_relu_gate(const float* da, const float* __restrict__ h, int M, int F, float* dh,
                                                      double* __restrict__ part) {
  __shared__ double red[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.y * 256 + lane * 4;
  double cs[1][1][4];
  NS_COL_ZERO(cs, 1, 1);
  for (int rr = wave; rr < PG_ROW_BLOCK; rr += 4) {
    const int m = blockIdx.x * PG_ROW_BLOCK + rr;
    if (m >= M) break;
    const size_t off = (size_t)m * F + col;
    const f32x4 a = *reinterpret_cast<const f32x4*>(da + off), hv = *reinterpret_cast<const f32x4*>(h + off);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = hv[e] > 0.f ? a[e] : 0.f;
      cs[0][0][e] += (double)o[e];
    }
    *reinterpret_cast<f32x4*>(dh + off) = o;
  }
  if (part) col_flush(cs, red, part + (size_t)blockIdx.x * PG_SLOTS * F + blockIdx.y * 256);  // slot 0 of block blk, this slab
}

hipError_t launch_fg_relu_gate(const float* da, const float* h, int M, int F, float* dh, double* part, hipStream_t st) {
  if (F <= 0 || F % 256 != 0 || F / 256 > 65535) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fg_relu_gate, dim3(pg_row_blocks(M), F / 256), dim3(256), 0, st, da, h, M, F, dh, part);
  return hipGetLastError();
}

}  // namespace ns
