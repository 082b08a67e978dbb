// PostNet training kernels for gfx950: train-mode BatchNorm1d between the five Conv1d(k = 5) GEMMs (transformer/Layers.py:107-177;
// DESIGN.md section 25):
//   k_pn_stats        column sums of u and u^2 over a block of rows, float64 partials
//   k_pn_finish       the fixed-order sum of the partials: mu and rstd with the running-statistics update (train), mu and rstd from the
//                     running statistics (eval), or d_beta, d_gamma and the two means of the backward
//   k_pn_apply        h = keep * scale * tanh(gamma (u - mu) rstd + beta), elementwise, 16 bytes per thread
//   k_pn_bwd_reduce   column sums of dy and dy * xhat
//   k_pn_bwd_apply    dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)) and the column sums of the unrounded dz (d_bias)
//   k_pn_bias_finish  the fixed-order sum of every layer's d_bias partials, one launch
//   k_pn_copy         the first n_mel rows of the padded last-layer weight gradient
// The normalisation is over all M rows of a column, so nothing here is row-local: all activations are [M, C] with the channels
// contiguous, every kernel reads 16-byte groups along the channels and reduces down the rows.  No atomics; a sum's order depends on
// the shape alone.  Every stored value is the float64 expression of its fp32 inputs rounded once.
#include "kernels.h"
#include "train_rows.h"

namespace ns {

constexpr double BN_EPS = 1e-5, BN_MOMENTUM = 0.1;  // nn.BatchNorm1d's defaults, which the reference keeps

// ------------------------------------------------------------------------------------------------------------------ column reductions
// Thread (r, cg) of a workgroup over `width` columns: the 16-byte column group cg, the rows m0 + r, m0 + r + nr, ... of the block.
struct PnLane {
  int nr, r, col, m0, m1;
  bool on;
  __device__ PnLane(int M, int width) {
    const int ng = width >> 2;
    nr = 256 / ng;
    r = threadIdx.x / ng;
    col = (threadIdx.x - r * ng) * 4;
    on = r < nr;
    m0 = blockIdx.x * PN_ROW_BLOCK;
    m1 = min(M, m0 + PN_ROW_BLOCK);
  }
};

// part[s * C + col] = the row lanes' acc[s] of that column, added in ascending lane order; every thread of the 256 calls it.
// red: 1024 doubles (nr * width <= 1024).
template <int NS>
__device__ inline void pn_flush(const PnLane& l, const double (&acc)[NS][4], double* red, int width, int C, double* part) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    __syncthreads();
    if (l.on) {
#pragma unroll
      for (int e = 0; e < 4; ++e) red[l.r * width + l.col + e] = acc[s][e];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < C; col += 256) {
      double t = 0.0;
      for (int r = 0; r < l.nr; ++r) t += red[r * width + col];
      part[s * C + col] = t;
    }
  }
}

__global__ __launch_bounds__(256) void k_pn_stats(const float* __restrict__ u, int M, int C, double* __restrict__ part) {
  __shared__ double red[1024];
  const PnLane l(M, C);
  double acc[2][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { acc[0][e] = 0.0; acc[1][e] = 0.0; }
  if (l.on) {
    for (int m = l.m0 + l.r; m < l.m1; m += l.nr) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(u + (size_t)m * C + l.col);
#pragma unroll
      for (int e = 0; e < 4; ++e) { const double d = (double)v[e]; acc[0][e] += d; acc[1][e] += d * d; }
    }
  }
  pn_flush<2>(l, acc, red, C, C, part + (size_t)blockIdx.x * 2 * C);
}

hipError_t launch_pn_stats(const float* u, int M, int C, double* part, hipStream_t st) {
  if (C <= 0 || C % 16 != 0 || C > 512) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pn_stats, dim3(pn_row_blocks(M)), dim3(256), 0, st, u, M, C, part);
  return hipGetLastError();
}

// 16 columns x 16 segments of the blocks per workgroup: a thread sums its segment of both slots in ascending order, the segment sums
// are added in segment order.
__global__ __launch_bounds__(256) void k_pn_finish(PnFinish a) {
  __shared__ double seg[2][16][16];
  const int cl = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;  // < C: C is a multiple of 16
  if (a.mode == PN_FIN_EVAL) {
    if (sg == 0) {
      a.stats[col] = (double)a.running_mean[col];
      a.stats[a.C + col] = 1.0 / sqrt((double)a.running_var[col] + BN_EPS);
    }
    return;
  }
  const int per = (a.nblk + 15) / 16, b0 = sg * per, b1 = min(a.nblk, b0 + per);
  const double* p = a.part + col;
  double s0 = 0.0, s1 = 0.0;
  for (int b = b0; b < b1; ++b) {
    s0 += p[(size_t)b * 2 * a.C];
    s1 += p[(size_t)b * 2 * a.C + a.C];
  }
  seg[0][sg][cl] = s0;
  seg[1][sg][cl] = s1;
  __syncthreads();
  if (sg != 0) return;
  s0 = 0.0; s1 = 0.0;
#pragma unroll
  for (int g = 0; g < 16; ++g) { s0 += seg[0][g][cl]; s1 += seg[1][g][cl]; }
  const double inv_m = 1.0 / (double)a.M;
  if (a.mode == PN_FIN_BWD) {
    if (a.out0) a.out0[col] = (float)s0;
    if (a.out1) a.out1[col] = (float)s1;
    if (a.stats) { a.stats[col] = s0 * inv_m; a.stats[a.C + col] = s1 * inv_m; }
    return;
  }
  const double mu = s0 * inv_m;
  double var = s1 * inv_m - mu * mu;
  if (var < 0.0) var = 0.0;
  a.stats[col] = mu;
  a.stats[a.C + col] = 1.0 / sqrt(var + BN_EPS);
  if (a.running_mean) {
    const double unbiased = var * ((double)a.M / (double)(a.M - 1));
    a.running_mean[col] = (float)((1.0 - BN_MOMENTUM) * (double)a.running_mean[col] + BN_MOMENTUM * mu);
    a.running_var[col] = (float)((1.0 - BN_MOMENTUM) * (double)a.running_var[col] + BN_MOMENTUM * unbiased);
    if (col == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
  }
}

hipError_t launch_pn_finish(const PnFinish& a, hipStream_t st) {
  if (a.C <= 0 || a.C % 16 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pn_finish, dim3(a.C / 16), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ forward apply
__global__ __launch_bounds__(256) void k_pn_apply(const float* __restrict__ u, const double* __restrict__ stats, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, const uint8_t* __restrict__ keep, float scale, int last,
                                                  long long groups, int C, float* __restrict__ h) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= groups) return;
  const int col = (int)(idx % (C >> 2)) * 4;
  const f32x4 v = *reinterpret_cast<const f32x4*>(u + idx * 4);
  const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + col), b = *reinterpret_cast<const f32x4*>(beta + col);
  double k[4];
  keep4(keep, (size_t)idx * 4, scale, k);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double n = (double)g[e] * (((double)v[e] - stats[col + e]) * stats[C + col + e]) + (double)b[e];
    o[e] = (float)(k[e] * (last ? n : tanh(n)));
  }
  *reinterpret_cast<f32x4*>(h + idx * 4) = o;
}

hipError_t launch_pn_apply(const float* u, const double* stats, const float* gamma, const float* beta, const uint8_t* keep, float scale, int last,
                           int M, int C, float* h, hipStream_t st) {
  if (C <= 0 || C % 16 != 0) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  const long long groups = (long long)M * (C / 4);
  hipLaunchKernelGGL(k_pn_apply, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, u, stats, gamma, beta, keep, scale, last, groups, C, h);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ backward
// dy and xhat of the four elements at row m, columns col .. col + 3.  Where keep is 0 the gradient is 0; where it is 1, tanh = h / scale:
// no tanh is recomputed.
__device__ inline void pn_dy(const PnBackward& a, int m, int col, const double (&mu)[4], const double (&rs)[4], double (&dy)[4], double (&xh)[4]) {
  const size_t off = (size_t)m * a.C + col;
  const f32x4 d = *reinterpret_cast<const f32x4*>(a.dh + off), v = *reinterpret_cast<const f32x4*>(a.u + off);
  double k[4];
  keep4(a.keep, off, a.scale, k);
  f32x4 hv = {0.f, 0.f, 0.f, 0.f};
  if (!a.last) hv = *reinterpret_cast<const f32x4*>(a.h + off);
  const double inv_scale = 1.0 / (double)a.scale;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    xh[e] = ((double)v[e] - mu[e]) * rs[e];
    const double t = (double)hv[e] * inv_scale;  // 0 on the last layer and where keep is 0 (there k[e] is 0 too)
    dy[e] = (double)d[e] * k[e] * (1.0 - t * t);
  }
}

__global__ __launch_bounds__(256) void k_pn_bwd_reduce(PnBackward a) {
  __shared__ double red[1024];
  const PnLane l(a.M, a.C);
  double acc[2][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { acc[0][e] = 0.0; acc[1][e] = 0.0; }
  if (l.on) {
    double mu[4], rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { mu[e] = a.stats[l.col + e]; rs[e] = a.stats[a.C + l.col + e]; }
    for (int m = l.m0 + l.r; m < l.m1; m += l.nr) {
      double dy[4], xh[4];
      pn_dy(a, m, l.col, mu, rs, dy, xh);
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[0][e] += dy[e]; acc[1][e] += dy[e] * xh[e]; }
    }
  }
  pn_flush<2>(l, acc, red, a.C, a.C, a.part + (size_t)blockIdx.x * 2 * a.C);
}

__global__ __launch_bounds__(256) void k_pn_bwd_apply(PnBackward a) {
  __shared__ double red[1024];
  const PnLane l(a.M, a.ldz);
  const bool real = l.on && l.col < a.C;  // (C and ldz are multiples of 4: a group is all real or all padding)
  double acc[1][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[0][e] = 0.0;
  if (l.on) {
    double mu[4], rs[4], gr[4], m1[4], m2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mu[e] = rs[e] = gr[e] = m1[e] = m2[e] = 0.0;
      if (real) {
        mu[e] = a.stats[l.col + e];
        rs[e] = a.stats[a.C + l.col + e];
        gr[e] = (double)a.gamma[l.col + e] * rs[e];
        if (a.means) { m1[e] = a.means[l.col + e]; m2[e] = a.means[a.C + l.col + e]; }
      }
    }
    for (int m = l.m0 + l.r; m < l.m1; m += l.nr) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (real) {
        double dy[4], xh[4];
        pn_dy(a, m, l.col, mu, rs, dy, xh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double dz = gr[e] * (dy[e] - m1[e] - xh[e] * m2[e]);
          acc[0][e] += dz;
          o[e] = (float)dz;
        }
      }
      *reinterpret_cast<f32x4*>(a.dz + (size_t)m * a.ldz + l.col) = o;
    }
  }
  if (a.bias_part) pn_flush<1>(l, acc, red, a.ldz, a.C, a.bias_part + (size_t)blockIdx.x * a.C);
}

static bool pn_backward_ok(const PnBackward& a) {
  return a.C > 0 && a.C % 16 == 0 && a.C <= 512 && a.ldz >= a.C && a.ldz % 16 == 0 && a.ldz <= 512;
}

hipError_t launch_pn_bwd_reduce(const PnBackward& a, hipStream_t st) {
  if (!pn_backward_ok(a)) return hipErrorInvalidValue;
  if (a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pn_bwd_reduce, dim3(pn_row_blocks(a.M)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pn_bwd_apply(const PnBackward& a, hipStream_t st) {
  if (!pn_backward_ok(a)) return hipErrorInvalidValue;
  if (a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pn_bwd_apply, dim3(pn_row_blocks(a.M)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// blockIdx.y = layer; the segment scheme of k_pn_finish on one slot
__global__ __launch_bounds__(256) void k_pn_bias_finish(PnBiasFinish a) {
  __shared__ double seg[16][16];
  const int layer = blockIdx.y, C = a.C[layer];
  float* out = a.out[layer];
  const int cl = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;
  if (!out || col >= C) return;  // (uniform per workgroup: C is a multiple of 16)
  const int per = (a.nblk + 15) / 16, b0 = sg * per, b1 = min(a.nblk, b0 + per);
  const double* p = a.part[layer] + col;
  double s = 0.0;
  for (int b = b0; b < b1; ++b) s += p[(size_t)b * C];
  seg[sg][cl] = s;
  __syncthreads();
  if (sg != 0) return;
  s = 0.0;
#pragma unroll
  for (int g = 0; g < 16; ++g) s += seg[g][cl];
  out[col] = (float)s;
}

hipError_t launch_pn_bias_finish(const PnBiasFinish& a, hipStream_t st) {
  int cmax = 0;
  for (int i = 0; i < PN_MAX_LAYERS; ++i)
    if (a.out[i]) {
      if (a.C[i] <= 0 || a.C[i] % 16 != 0) return hipErrorInvalidValue;
      cmax = a.C[i] > cmax ? a.C[i] : cmax;
    }
  if (cmax == 0 || a.nblk <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pn_bias_finish, dim3(cmax / 16, PN_MAX_LAYERS), dim3(256), 0, st, a);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_pn_copy(const float* __restrict__ src, float* __restrict__ dst, long long groups) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx < groups) *reinterpret_cast<f32x4*>(dst + idx * 4) = *reinterpret_cast<const f32x4*>(src + idx * 4);
}

hipError_t launch_pn_copy(const float* src, float* dst, long long n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n % 4 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pn_copy, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, src, dst, n / 4);
  return hipGetLastError();
}

}  // namespace ns
