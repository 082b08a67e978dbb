// Wave-to-mel front end (kernels.h launch_mel_*): the two row kernels around the STFT GEMM of the reference's
// TacotronSTFT.mel_spectrogram (audio/stft.py:52-81,159-178) behind get_mel_from_wav's clip (audio/tools.py:9).
//   k_mel_frame_rows  wave -> clipped, reflect-padded samples laid out as rows of hop samples (the GEMM's [rows, Cin] operand)
//   k_mel_project     packed spectrum row -> magnitude (staged once in LDS) -> energy, band-form mel basis, clamp + log
// Both are bandwidth-shaped: a frame costs hop samples of reads in the first and filter_length floats (4 KB) in the second.
#include "kernels.h"

namespace ns {

// One float4 (four consecutive padded samples) per thread; blockIdx.y = utterance.  Padded sample p comes from source sample
// p - fl/2, mirrored at both ends without repeating the edge sample (torch "reflect", stft.py:60-64).  For p < n + fl and n > fl/2
// the mirrored index lies in [0, n): left |src| <= fl/2 <= n - 1, right 2(n-1) - src >= n - 1 - fl/2 >= 0.
// CLIP = false is the Griffin-Lim loop's transform (stft.py:52-81 pads but does not clip; griffinlim_api.hip): pure data movement.
template <bool CLIP>
__global__ __launch_bounds__(256) void k_mel_frame_rows(const float* __restrict__ wav, long long ld, const long long* __restrict__ wav_lens,
                                                        long long n_max, int fl, int hop, long long row_floats, float* __restrict__ rows,
                                                        long long* __restrict__ mel_lens_out) {
  const int b = blockIdx.y;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long p0 = q * 4;
  if (p0 >= row_floats) return;
  long long n = wav_lens[b];
  n = n < 0 ? 0 : (n > n_max ? n_max : n);
  const int half = fl >> 1;
  const bool ok = n > half;  // the reference's reflect pad refuses anything shorter: zero frames
  if (q == 0 && mel_lens_out) mel_lens_out[b] = ok ? n / hop + 1 : 0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (ok && p0 < n + fl) {
    const float* w = wav + (long long)b * ld;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long p = p0 + e;
      if (p < n + fl) {
        long long s = p - half;
        if (s < 0) s = -s;
        if (s >= n) s = 2 * (n - 1) - s;
        const float x = w[s];
        v[e] = !CLIP ? x : (x < -1.f ? -1.f : (x > 1.f ? 1.f : x));  // torch.clip: a NaN fails both comparisons and stays
      }
    }
  }
  *reinterpret_cast<float4*>(rows + (long long)b * row_floats + p0) = make_float4(v[0], v[1], v[2], v[3]);
}

hipError_t launch_mel_frame_rows(const float* wav, long long ld, const long long* wav_lens, int B, long long n_max, int fl, int hop, int S,
                                 float* rows, long long* mel_lens_out, hipStream_t st, bool clip) {
  if (B <= 0 || S <= 0) return hipSuccess;
  if (B > 65535 || (hop & 3) || (fl & 1)) return hipErrorInvalidValue;
  const long long row_floats = (long long)S * hop;
  const long long blocks = (row_floats / 4 + 255) / 256;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  if (clip)
    hipLaunchKernelGGL(k_mel_frame_rows<true>, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, wav, ld, wav_lens, n_max, fl, hop, row_floats,
                       rows, mel_lens_out);
  else
    hipLaunchKernelGGL(k_mel_frame_rows<false>, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, wav, ld, wav_lens, n_max, fl, hop, row_floats,
                       rows, mel_lens_out);
  return hipGetLastError();
}

// One wave per frame, four frames per workgroup.  A lane reads float4 i = lane, lane + 64, ... of the frame's spectrum row: bins 2i
// and 2i + 1 as (re, im) pairs, except float4 0 whose first pair is (re_0, re_{fl/2}).  Magnitudes go to the wave's LDS row; the
// energy is the lanes' partial sums of mag^2 (each in bin order) folded by a fixed butterfly; filter m = lane, lane + 64, ... then
// sums its band in bin order.  Nothing depends on which workgroup or wave a frame lands on, so equal frames give equal bits.
constexpr int MEL_FRAMES_PER_WG = 4;

__global__ __launch_bounds__(64 * MEL_FRAMES_PER_WG) void k_mel_project(const float* __restrict__ spec, const long long* __restrict__ wav_lens,
                                                                        int B, int S, long long n_max, int T, int fl, int hop, int n_mel,
                                                                        float clip, const int* __restrict__ band, const float* __restrict__ bw,
                                                                        float* __restrict__ mel, float* __restrict__ energy) {
  extern __shared__ float mel_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int half = fl >> 1, stride = half + 4;
  float* mag = mel_lds + wv * stride;
  const long long f = (long long)blockIdx.x * MEL_FRAMES_PER_WG + wv;
  const bool valid = f < (long long)B * T;
  const int b = valid ? (int)(f / T) : 0, t = valid ? (int)(f % T) : 0;
  bool live = false;
  if (valid) {
    long long n = wav_lens[b];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long long frames = n > half ? n / hop + 1 : 0;
    live = t < frames && t < S - fl / hop + 1;
  }
  float esum = 0.f;
  if (live) {
    const float4* row = reinterpret_cast<const float4*>(spec + ((long long)b * S + t) * fl);
    for (int i = lane; i < fl / 4; i += 64) {
      const float4 c = row[i];
      float m0, m1;
      if (i == 0) {
        m0 = sqrtf(c.x * c.x);  // bins 0 and fl/2: the imaginary part is identically zero (sqrt(re^2 + 0), stft.py:78)
        const float mn = sqrtf(c.y * c.y);
        mag[half] = mn;
        esum += m0 * m0;
        esum += mn * mn;
      } else {
        m0 = sqrtf(c.x * c.x + c.y * c.y);
        esum += m0 * m0;
      }
      m1 = sqrtf(c.z * c.z + c.w * c.w);
      esum += m1 * m1;
      mag[2 * i] = m0;
      mag[2 * i + 1] = m1;
    }
  }
  __syncthreads();  // every wave arrives: the loops above hold no barrier
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) esum += __shfl_xor(esum, off, 64);
  if (!valid) return;
  if (lane == 0) energy[f] = live ? sqrtf(esum) : 0.f;
  for (int m = lane; m < n_mel; m += 64) {
    float out = 0.f;
    if (live) {
      const int k0 = band[3 * m], nk = band[3 * m + 1];
      const float* w = bw + band[3 * m + 2];
      float acc = 0.f;
      for (int i = 0; i < nk; ++i) acc += w[i] * mag[k0 + i];
      const float c = acc < clip ? clip : acc;  // torch.clamp(min): a NaN fails the comparison and stays
      // the logarithm in double, rounded once: the device's logf was measured 1.6 ulp off at log(1e-5), the reference's torch.log
      // (CPU) rounds within an ulp; n_mel logarithms per 4 KB frame cost nothing next to the reads
      out = (float)log((double)c);
    }
    mel[f * n_mel + m] = out;
  }
}

hipError_t launch_mel_project(const float* spec, const long long* wav_lens, int B, int S, long long n_max, int T, int fl, int hop, int n_mel,
                              float clip, const int* band, const float* bw, float* mel, float* energy, hipStream_t st) {
  if (B <= 0 || T <= 0) return hipSuccess;
  if (fl > MEL_MAX_FILTER || (fl & 3) || hop <= 0 || fl % hop || S < fl / hop) return hipErrorInvalidValue;
  const long long frames = (long long)B * T;
  const long long blocks = (frames + MEL_FRAMES_PER_WG - 1) / MEL_FRAMES_PER_WG;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  const size_t lds = (size_t)MEL_FRAMES_PER_WG * (fl / 2 + 4) * sizeof(float);  // <= 32.1 KB at MEL_MAX_FILTER
  hipLaunchKernelGGL(k_mel_project, dim3((unsigned)blocks), dim3(64 * MEL_FRAMES_PER_WG), lds, st, spec, wav_lens, B, S, n_max, T, fl, hop, n_mel,
                     clip, band, bw, mel, energy);
  return hipGetLastError();
}

}  // namespace ns
