// VarianceAdaptor training kernels for gfx950 (model/modules.py:17-159, 195-230): what the adaptor needs beyond
// the three predictors (predgrad.hip) to carry a gradient from the decoder's input back to the encoder's output.
//   k_va_embed_fwd      y = x + table[bucketize(target, bins)], the index kept as int32; one wave per row
//   k_va_embed_bwd      per (row block, column slab): an n_bins x slab float64 table in LDS, one thread per column walks the block's rows
//                       in order; the block's table goes out as float64 partials
//   k_va_embed_finish   d_table = the partials added in block order, rounded once
//   k_va_duration_scan  cum = inclusive prefix sums of max(d, 0), mel_len = the total; one wave per utterance
//   k_va_lr_bwd         d_x[b, l] = the sum of g[b, t] over the phoneme's frames below T, in t order; one wave per phoneme
// The length regulator's forward gather is rowops.hip's k_length_regulate, unchanged.  No atomics; the order of every sum depends on the
// shape alone, every stored value is the float64 expression of its fp32 inputs rounded once.  The bucket index is rowln.h's
// wave_bucketize, so it equals k_bucketize's bit for bit.  (rowln.h and train_rows.h both define LN_EPS and cannot meet in one file;
// nothing of train_rows.h is needed here.)
#include "kernels.h"
#include "rowln.h"

namespace ns {

// ------------------------------------------------------------------------------------------------------------------ variance embedding
__global__ __launch_bounds__(256) void k_va_embed_fwd(const float* __restrict__ x, const float* __restrict__ target, const float* __restrict__ bins,
                                                       const float* __restrict__ table, int M, int D, int n_edges, float* __restrict__ y,
                                                       int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int k = wave_bucketize(bins, n_edges, target[m], lane);  // in [0, n_edges] = [0, n_bins - 1]
  if (lane == 0) idx[m] = k;
  const float* src = x + (size_t)m * D;
  const float* row = table + (size_t)k * D;
  float* dst = y + (size_t)m * D;
  for (int c = lane * 4; c < D; c += 256)
    *reinterpret_cast<f32x4*>(dst + c) = *reinterpret_cast<const f32x4*>(src + c) + *reinterpret_cast<const f32x4*>(row + c);
}

hipError_t launch_va_embed_fwd(const float* x, const float* target, const float* bins, const float* table, int M, int D, int n_bins, float* y,
                               int32_t* idx, hipStream_t st) {
  if (M <= 0 || D <= 0 || D % 4 != 0 || n_bins < 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_va_embed_fwd, dim3((M + 3) / 4), dim3(256), 0, st, x, target, bins, table, M, D, n_bins - 1, y, idx);
  return hipGetLastError();
}

bool va_plan_embed(int M, int D, int n_bins, VaEmbedPlan* plan) {
  if (M <= 0 || D <= 0 || D % 4 != 0 || n_bins < 2) return false;
  int slab = 64;
  while (slab >= 4 && (long long)n_bins * slab * (long long)sizeof(double) > VA_LDS_LIMIT) slab >>= 1;
  if (slab < 4) return false;
  const int n_slabs = (D + slab - 1) / slab;
  if (n_slabs > 65535) return false;
  plan->row_blocks = (M + VA_ROW_BLOCK - 1) / VA_ROW_BLOCK;
  plan->rows_per_block = VA_ROW_BLOCK;
  plan->slab = slab;
  plan->n_slabs = n_slabs;
  plan->lds_bytes = n_bins * slab * (int)sizeof(double);
  plan->launches = 2;
  plan->ws_bytes = (long long)plan->row_blocks * n_bins * D * (long long)sizeof(double);
  return true;
}

// tab[k * slab + lane] is touched by this lane alone: the read-modify-write needs no atomic, and a lane's additions happen in row order
__global__ __launch_bounds__(64) void k_va_embed_bwd(const float* __restrict__ g, const int32_t* __restrict__ idx, int M, int D, int n_bins,
                                                      int slab, int rows_per_block, double* __restrict__ part) {
  extern __shared__ double tab[];  // [n_bins][slab]
  const int lane = threadIdx.x;
  const int n = n_bins * slab;
  for (int i = lane; i < n; i += 64) tab[i] = 0.0;
  __syncthreads();
  const int col = blockIdx.y * slab + lane;
  const int m0 = blockIdx.x * rows_per_block, m1 = min(M, m0 + rows_per_block);
  if (lane < slab && col < D) {
    const float* gc = g + col;
    double* mine = tab + lane;
    const unsigned nb = (unsigned)n_bins;
    int m = m0;
    for (; m + 4 <= m1; m += 4) {  // four rows' loads in flight; the additions stay in row order
      const int k0 = idx[m], k1 = idx[m + 1], k2 = idx[m + 2], k3 = idx[m + 3];
      const float v0 = gc[(size_t)m * D], v1 = gc[(size_t)(m + 1) * D], v2 = gc[(size_t)(m + 2) * D], v3 = gc[(size_t)(m + 3) * D];
      if ((unsigned)k0 < nb) mine[k0 * slab] += (double)v0;
      if ((unsigned)k1 < nb) mine[k1 * slab] += (double)v1;
      if ((unsigned)k2 < nb) mine[k2 * slab] += (double)v2;
      if ((unsigned)k3 < nb) mine[k3 * slab] += (double)v3;
    }
    for (; m < m1; ++m) {
      const int k = idx[m];
      if ((unsigned)k < nb) mine[k * slab] += (double)gc[(size_t)m * D];
    }
  }
  __syncthreads();
  double* p = part + (size_t)blockIdx.x * n_bins * D;
  const int c0 = blockIdx.y * slab;
  for (int i = lane; i < n; i += 64) {
    const int k = i / slab, c = c0 + (i - k * slab);
    if (c < D) p[(size_t)k * D + c] = tab[i];
  }
}

__global__ __launch_bounds__(256) void k_va_embed_finish(const double* __restrict__ part, int nblk, long long n, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(size_t)b * n + i];
  out[i] = (float)s;
}

hipError_t launch_va_embed_bwd(const float* g, const int32_t* idx, int M, int D, int n_bins, const VaEmbedPlan& plan, double* part, float* d_table,
                               hipStream_t st) {
  if (M <= 0 || plan.row_blocks != (M + plan.rows_per_block - 1) / plan.rows_per_block || plan.lds_bytes > VA_LDS_LIMIT) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_va_embed_bwd, dim3(plan.row_blocks, plan.n_slabs), dim3(64), (size_t)plan.lds_bytes, st, g, idx, M, D, n_bins, plan.slab,
                     plan.rows_per_block, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long n = (long long)n_bins * D;
  hipLaunchKernelGGL(k_va_embed_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, plan.row_blocks, n, d_table);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ length regulator
// Lane j owns the phonemes [j * per, (j + 1) * per): its own sum, an inclusive scan of the 64 sums, then its prefix sums.  Integers: the
// order does not matter.
__global__ __launch_bounds__(64) void k_va_duration_scan(const long long* __restrict__ duration, int L, int32_t* __restrict__ cum,
                                                          long long* __restrict__ mel_len) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const long long* d = duration + (size_t)b * L;
  int32_t* cb = cum + (size_t)b * L;
  const int per = (L + 63) / 64, i0 = min(L, lane * per), i1 = min(L, i0 + per);
  const long long top = 0x7fffffffll;
  long long s = 0;
  for (int i = i0; i < i1; ++i) s += min(max(d[i], 0ll), top);
  long long inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  long long run = inc - s;
  for (int i = i0; i < i1; ++i) {
    run += min(max(d[i], 0ll), top);
    cb[i] = (int32_t)min(run, top);
  }
  if (lane == 63) mel_len[b] = inc;
}

hipError_t launch_va_duration_scan(const long long* duration, int B, int L, int32_t* cum, long long* mel_len, hipStream_t st) {
  if (B <= 0 || L <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_va_duration_scan, dim3(B), dim3(64), 0, st, duration, L, cum, mel_len);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_va_lr_bwd(const float* __restrict__ g, const int32_t* __restrict__ cum, int L, int D, int T, int n_ph,
                                                    float* __restrict__ d_x) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n_ph) return;
  const int b = p / L, l = p - b * L;
  const int32_t* cb = cum + (size_t)b * L;
  const int t0 = max(l ? cb[l - 1] : 0, 0), t1 = min(cb[l], T);  // frames at or past T are dropped; an empty range for duration 0
  const float* gb = g + (size_t)b * T * D;
  float* dst = d_x + (size_t)p * D;
  for (int c = lane * 4; c < D; c += 256) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int t = t0;
    for (; t + 4 <= t1; t += 4) {  // four frames' loads in flight; the additions stay in t order
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(gb + (size_t)t * D + c);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(gb + (size_t)(t + 1) * D + c);
      const f32x4 v2 = *reinterpret_cast<const f32x4*>(gb + (size_t)(t + 2) * D + c);
      const f32x4 v3 = *reinterpret_cast<const f32x4*>(gb + (size_t)(t + 3) * D + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = (((a[e] + (double)v0[e]) + (double)v1[e]) + (double)v2[e]) + (double)v3[e];
    }
    for (; t < t1; ++t) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(gb + (size_t)t * D + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += (double)v[e];
    }
    *reinterpret_cast<f32x4*>(dst + c) = f32x4{(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
  }
}

hipError_t launch_va_lr_bwd(const float* g, const int32_t* cum, int B, int L, int D, int T, float* d_x, hipStream_t st) {
  if (B <= 0 || L <= 0 || T <= 0 || D <= 0 || D % 4 != 0) return hipErrorInvalidValue;
  const int n_ph = B * L;
  hipLaunchKernelGGL(k_va_lr_bwd, dim3((n_ph + 3) / 4), dim3(256), 0, st, g, cum, L, D, T, n_ph, d_x);
  return hipGetLastError();
}

}  // namespace ns
