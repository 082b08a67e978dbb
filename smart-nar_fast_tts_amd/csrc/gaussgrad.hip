// The Gaussian length regulator's training side for gfx950 (model/modules.py:162-192).  The forward is
// rowops.hip's launch_gaussian_upsampling, unchanged; these are the three kernels around it:
//   k_gu_prepare        duration [B, L] int64 -> the fp32 durations max(d, 0) the forward launch reads, mel_len [B] int64 (the uncropped
//                       total) and the centres [B, L] the backward keeps — k_gauss_centers' own serial fp32 scan, so the same bits
//   k_gu_denominators   S [B, T] for t < lim_b in k_gauss_upsample's own order: eight strided partial sums, the three-level tree, + 1e-20f
//   k_gu_bwd            d_x[b, l] = sum_{t < lim_b} w_lt g[b, t] with w_lt = expf(-0.01f (t - c_l)^2) / S_t generated on the fly: the
//                       forward's launch transposed.  One workgroup = 32 consecutive phonemes of one utterance x 128 channels (one
//                       32-channel tile per wave); the weights of a chunk of GB_TC frames are staged in LDS at the forward's padded
//                       row stride (the A-fragment read — 32 phonemes at one frame — hits 32 banks), g[t, n0 + lane] comes from
//                       global memory, and v_mfma_f32_32x32x2_f32 walks t upwards: a k-ordered fmaf chain, so d_x is the serial
//                       acc = fmaf(w[t], g[t], acc) bit for bit.
// The frame band.  The centres of a tile are nondecreasing (c_{l+1} - c_l = (d_l + d_{l+1}) / 2 >= 0), and for |t - c_l| >= 102 the
// argument 0.01f (t - c_l)^2 is at least 104.03 > 150 ln 2 = 103.98: expf returns exactly +0.0, with or without denormals.  A workgroup
// therefore walks only the frames of [floor(c_first) - 102, ceil(c_last) + 102] cut to [0, lim_b); a skipped frame would have added
// fmaf(+0.0, g, acc) = acc.  The bounds are uniform per workgroup; a frame outside them is never read.
// No atomics, no host read: every sum runs in one order that depends on the shape and the durations alone.
#include "kernels.h"

namespace ns {

typedef float f32x16g __attribute__((ext_vector_type(16)));
constexpr int GB_TC = 256;        // frames staged per LDS chunk (the forward's GU_LC: row stride GB_TC + 1)
constexpr int GB_REACH = 102;     // frames past which a weight is exactly +0.0

// lim_b = min(max(own_len[b], 0), T); own_len == nullptr: every row below T is live
__device__ __forceinline__ int gu_row_limit(const long long* own_len, int b, int T) {
  if (!own_len) return T;
  const long long n = own_len[b];
  return n < 0 ? 0 : n < (long long)T ? (int)n : T;
}

__global__ __launch_bounds__(64) void k_gu_prepare(const long long* __restrict__ duration, int L, float* __restrict__ dur_f,
                                                    float* __restrict__ centres, long long* __restrict__ mel_len) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long* d = duration + (size_t)b * L;
  long long total = 0;
  for (int l = lane; l < L; l += 64) {
    const long long v = d[l] > 0 ? d[l] : 0;
    dur_f[(size_t)b * L + l] = (float)v;
    total += v;
  }
  for (int o = 32; o > 0; o >>= 1) total += __shfl_down(total, o, 64);  // integers: the order does not matter
  if (lane != 0) return;
  mel_len[b] = total;
  // the serial fp32 scan of k_gauss_centers, from the same fp32 durations
  float e = 0.f;
  for (int l = 0; l < L; ++l) {
    const float dl = (float)(d[l] > 0 ? d[l] : 0);
    e += dl;
    centres[(size_t)b * L + l] = e - 0.5f * dl;
  }
}

__global__ __launch_bounds__(256) void k_gu_denominators(const float* __restrict__ centres, const long long* __restrict__ own_len, int L,
                                                          int T, float* __restrict__ S) {
  __shared__ float p8[32 * 9];
  const int b = blockIdx.y, t0 = blockIdx.x * 32, tid = threadIdx.x;
  const int lim = gu_row_limit(own_len, b, T);
  if (t0 >= lim) return;
  const int tt = tid & 31, sub = tid >> 5;
  const float* cb = centres + (size_t)b * L;
  const float tf = (float)(t0 + tt);
  float part = 0.f;
  for (int l = sub; l < L; l += 8) {
    const float df = tf - cb[l];
    part += expf(-0.01f * (df * df));
  }
  p8[tt * 9 + sub] = part;
  __syncthreads();
  if (tid < 32 && t0 + tid < lim) {
    const float* p = p8 + tid * 9;
    S[(size_t)b * T + t0 + tid] = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) + 1e-20f;
  }
}

// grid (ceil(L / 32), B, ceil(D / 128)); band == 0 walks every frame below lim_b (the bench's comparison: the same bits for finite g)
__global__ __launch_bounds__(256) void k_gu_bwd(const float* __restrict__ g, const float* __restrict__ centres, const float* __restrict__ S,
                                                 const long long* __restrict__ own_len, int L, int D, int T, int band,
                                                 float* __restrict__ d_x, float* __restrict__ w_out) {
#if defined(__HIP_DEVICE_COMPILE__)  // the MFMA builtin does not exist in the host pass; it only needs the stub
  __shared__ float wt[32 * (GB_TC + 1)];
  const int b = blockIdx.y, l0 = blockIdx.x * 32, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ll = tid & 31, sub = tid >> 5;  // phoneme of this thread inside the tile, and which eighth of a chunk's frames it makes
  const float* cb = centres + (size_t)b * L;
  const int lim = gu_row_limit(own_len, b, T);
  int t_lo = 0, t_hi = lim;
  if (band) {
    // (clamped before the casts: a centre may be anything once the durations are)
    const float top = (float)T + (float)(GB_REACH + 2);
    const float c_first = fminf(fmaxf(cb[l0], 0.f), top), c_last = fminf(fmaxf(cb[min(l0 + 31, L - 1)], 0.f), top);
    t_lo = max(0, (int)floorf(c_first) - GB_REACH);
    t_hi = min(lim, (int)ceilf(c_last) + GB_REACH + 1);
  }
  const bool live = l0 + ll < L;
  const float c = live ? cb[l0 + ll] : 0.f;
  const float* gb = g + (size_t)b * T * D;
  const float* Sb = S + (size_t)b * T;
  const int col = (blockIdx.z * 4 + wv) * 32 + (lane & 31);  // this lane's channel
  const bool col_in = col < D;
  const bool wr = w_out != nullptr && blockIdx.z == 0 && live;
  float* wrow = wr ? w_out + ((size_t)b * L + l0 + ll) * T : nullptr;
  if (wr) {  // the test output: a frame the band skips, or at or past lim_b, had the weight +0.0
    for (int t = sub; t < T; t += 8)
      if (t < t_lo || t >= t_hi) wrow[t] = 0.f;
  }
  f32x16g acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int tc = t_lo; tc < t_hi; tc += GB_TC) {
    const int n = min(GB_TC, t_hi - tc), npad = (n + 1) & ~1;
    for (int j = sub; j < npad; j += 8) {
      float w = 0.f;
      if (j < n && live) {
        const float df = (float)(tc + j) - c;
        w = expf(-0.01f * (df * df)) / Sb[tc + j];
        if (wr) wrow[tc + j] = w;
      }
      wt[ll * (GB_TC + 1) + j] = w;
    }
    __syncthreads();
    const float* arow = wt + (lane & 31) * (GB_TC + 1) + (lane >> 5);
    const float* grow = gb + (size_t)(tc + (lane >> 5)) * D + col;
    for (int j2 = 0; j2 < npad; j2 += 2) {
      const float av = arow[j2];
      const float bv = (col_in && j2 + (lane >> 5) < n) ? grow[(size_t)j2 * D] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (!col_in) return;
  const int lb = l0 + 4 * (lane >> 5);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int l = lb + (r & 3) + 8 * (r >> 2);
    if (l < L) d_x[((size_t)b * L + l) * D + col] = acc[r];
  }
#endif
}

hipError_t launch_gu_prepare(const long long* duration, int B, int L, float* dur_f, float* centres, long long* mel_len, hipStream_t st) {
  if (B <= 0 || L <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gu_prepare, dim3(B), dim3(64), 0, st, duration, L, dur_f, centres, mel_len);
  return hipGetLastError();
}

hipError_t launch_gu_denominators(const float* centres, const long long* own_len, int B, int L, int T, float* S, hipStream_t st) {
  if (B <= 0 || L <= 0 || T <= 0 || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gu_denominators, dim3((T + 31) / 32, B), dim3(256), 0, st, centres, own_len, L, T, S);
  return hipGetLastError();
}

hipError_t launch_gu_bwd(const float* g, const float* centres, const float* S, const long long* own_len, int B, int L, int D, int T, bool band,
                         float* d_x, float* w_out, hipStream_t st) {
  if (B <= 0 || L <= 0 || D <= 0 || T <= 0 || B > 65535 || (D + 127) / 128 > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gu_bwd, dim3((L + 31) / 32, B, (D + 127) / 128), dim3(256), 0, st, g, centres, S, own_len, L, D, T, band ? 1 : 0, d_x,
                     w_out);
  return hipGetLastError();
}

}  // namespace ns
