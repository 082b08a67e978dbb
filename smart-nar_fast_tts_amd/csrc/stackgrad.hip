// TxtEncoder / MelDecoder training kernels for gfx950 (transformer/Models.py:33-100, 176-244):
//   k_st_embed_grad  the gradient of the word-embedding table, d_table[v, :] = the sum of g[m, :] over the rows with texts[m] == v
//   k_st_row_mask    masked_fill(mask.unsqueeze(-1), 0) of [B, S, D] rows (transformer/Layers.py:43,46), forward and backward
// The forward's embedding + position add, the decoder's position add and the regenerated table are rowops.hip's kernels, called as
// they are (stackgrad_api.hip).  No atomics, no LDS, no host reads; every sum has one order that depends on the tokens alone.
#include "kernels.h"
#include "train_rows.h"

namespace ns {

// One wave owns one (token id v, 256-column slab): lane l the 16-byte group l of the slab, four float64 accumulators.  A workgroup of
// four waves holds the ids [4 blockIdx.x, 4 blockIdx.x + 4); blockIdx.y is the slab.  The wave walks the M tokens 64 at a time: each
// lane loads one, the ballot of tok == v is the 64-bit hit mask, and its set bits are visited lowest first, so a column's sum is
// accumulated in ascending m in float64 and rounded once.  Row 0 (PAD, padding_idx = 0) is written as +0.0 without a scan, so g at a PAD
// row is never read; an id no row carries gives +0.0; a token outside [0, n_vocab) equals no v and contributes nowhere.
__global__ __launch_bounds__(256) void k_st_embed_grad(const float* __restrict__ g, const long long* __restrict__ texts, int M, int D, int n_vocab,
                                                       float* __restrict__ d_table) {
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n_vocab) return;
  const int col = blockIdx.y * 256 + lane * 4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (v != 0) {
    for (int base = 0; base < M; base += 64) {
      const int m = base + lane;
      const long long tok = m < M ? texts[m] : 0ll;  // (0 never equals v here)
      unsigned long long hits = __ballot(tok == (long long)v);
      while (hits) {
        const int m_hit = base + (__ffsll(hits) - 1);
        hits &= hits - 1;
        const f32x4 a = *reinterpret_cast<const f32x4*>(g + (size_t)m_hit * D + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (double)a[e];
      }
    }
  }
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (float)acc[e];
  *reinterpret_cast<f32x4*>(d_table + (size_t)v * D + col) = o;
}

hipError_t launch_st_embed_grad(const float* g, const long long* texts, int M, int D, int n_vocab, float* d_table, hipStream_t st) {
  if (D <= 0 || D % 256 != 0 || D / 256 > 65535 || n_vocab <= 0) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_st_embed_grad, dim3((n_vocab + 3) / 4, D / 256), dim3(256), 0, st, g, texts, M, D, n_vocab, d_table);
  return hipGetLastError();
}

// Workgroup = 4 waves over the rows [64 blk, 64 blk + 64) and the column slab [256 blockIdx.y, 256 blockIdx.y + 256): wave w takes the
// rows w, w + 4, ..., lane l the 16-byte group l of the slab, as the row kernels do at NV = 1.  padded(m) is mask[m] != 0 when a mask
// is given, else m % S >= lens[m / S].  A select, never a multiply: a NaN or an infinity in a padded row of x reaches nothing, and x
// there is not read at all.  Out of place (x and y are different buffers).
__global__ __launch_bounds__(256) void k_st_row_mask(const float* __restrict__ x, const uint8_t* __restrict__ mask, const long long* __restrict__ lens,
                                                     int M, int S, int D, float* __restrict__ y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.y * 256 + lane * 4;
  for (int rr = wave; rr < PG_ROW_BLOCK; rr += 4) {
    const int m = blockIdx.x * PG_ROW_BLOCK + rr;
    if (m >= M) break;
    const bool padded = mask ? mask[m] != 0 : (long long)(m % S) >= lens[m / S];
    const size_t off = (size_t)m * D + col;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (!padded) o = *reinterpret_cast<const f32x4*>(x + off);
    *reinterpret_cast<f32x4*>(y + off) = o;
  }
}

hipError_t launch_st_row_mask(const float* x, const uint8_t* mask, const long long* lens, int M, int S, int D, float* y, hipStream_t st) {
  if (D <= 0 || D % 256 != 0 || D / 256 > 65535 || S <= 0 || (!mask && !lens)) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_st_row_mask, dim3(pg_row_blocks(M), D / 256), dim3(256), 0, st, x, mask, lens, M, S, D, y);
  return hipGetLastError();
}

}  // namespace ns
