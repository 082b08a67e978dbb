// Griffin-Lim mel-to-wave (kernels.h launch_gl_*): the row-local kernels around the two fp32 GEMMs of one iteration of the reference's
// griffin_lim (audio/audio_processing.py:66-82) over STFT.inverse / STFT.transform (audio/stft.py:52-122) and inv_mel_spec's mel
// inversion (audio/tools.py:18-29).
//   k_gl_mel_to_mag    log-mel frame -> expf (staged in LDS) -> dense n_mel-term dot with mel_basis^T, * scaling
//   k_gl_recombine     mag, angles -> packed (mag cos, mag sin): the loop's start, the only place a cosine or sine is evaluated
//   k_gl_rephase       packed spectrum Y, mag -> packed mag * Y / |Y|: the loop's phase step without an angle
//   k_gl_overlap_add   frames -> wave: gather in ascending t, / window_sum, * fl / hop, trim
//   k_gl_polar         packed spectrum -> magnitude, atan2f phase (STFT.transform for users of the class; never in the loop)
// All are bandwidth-shaped; the packed rows move as float4.  No atomics: every sum's order is a function of the shapes alone.
#include <cfloat>

#include "kernels.h"

namespace ns {

// frames of utterance b: clamp(lens[b] - drop, 0, Tg), and none when hop (t - 1) <= fl / 2 (the reflect pad of the loop's transform,
// stft.py:60-64, refuses such a signal)
__device__ __forceinline__ int gl_frames(const long long* __restrict__ lens, int b, int drop, int Tg, int fl, int hop) {
  long long t = lens[b] - drop;
  t = t < 0 ? 0 : (t > Tg ? Tg : t);
  return (t - 1) * hop <= (fl >> 1) ? 0 : (int)t;
}

// ---- mel -> magnitude (tools.py:20-25,28).  GL_MAG_FRAMES frames per workgroup share every mel_basis load; thread = bin.
constexpr int GL_MAG_FRAMES = 4;

__global__ __launch_bounds__(256) void k_gl_mel_to_mag(const float* __restrict__ mel, const long long* __restrict__ lens, int drop, int T_mel, int Tg,
                                                       int fl, int hop, int n_mel, float scaling, const float* __restrict__ mb,
                                                       float* __restrict__ mag) {
  extern __shared__ float gl_e[];  // [GL_MAG_FRAMES][n_mel]
  const int b = blockIdx.y, t0 = blockIdx.x * GL_MAG_FRAMES, bins = (fl >> 1) + 1;
  const int tg = gl_frames(lens, b, drop, Tg, fl, hop);
  for (int i = threadIdx.x; i < GL_MAG_FRAMES * n_mel; i += 256) {
    const int f = i / n_mel, m = i - f * n_mel;
    gl_e[i] = t0 + f < tg ? expf(mel[((long long)b * T_mel + t0 + f) * n_mel + m]) : 0.f;  // torch.exp, audio_processing.py:100
  }
  __syncthreads();
  for (int k = threadIdx.x; k < bins; k += 256) {
    float acc[GL_MAG_FRAMES] = {0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < n_mel; ++m) {
      const float w = mb[(long long)m * bins + k];
#pragma unroll
      for (int f = 0; f < GL_MAG_FRAMES; ++f) acc[f] += gl_e[f * n_mel + m] * w;
    }
#pragma unroll
    for (int f = 0; f < GL_MAG_FRAMES; ++f)
      if (t0 + f < Tg) mag[((long long)b * Tg + t0 + f) * bins + k] = t0 + f < tg ? acc[f] * scaling : 0.f;
  }
}

hipError_t launch_gl_mel_to_mag(const float* mel, const long long* lens, int drop, int B, int T_mel, int Tg, int fl, int hop, int n_mel,
                                float scaling, const float* mel_basis, float* mag, hipStream_t st) {
  if (B <= 0 || Tg <= 0) return hipSuccess;
  if (B > 65535 || n_mel < 1 || n_mel > 2048 || T_mel < Tg) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gl_mel_to_mag, dim3((unsigned)((Tg + GL_MAG_FRAMES - 1) / GL_MAG_FRAMES), (unsigned)B), dim3(256),
                     (size_t)GL_MAG_FRAMES * n_mel * sizeof(float), st, mel, lens, drop, T_mel, Tg, fl, hop, n_mel, scaling, mel_basis, mag);
  return hipGetLastError();
}

// ---- packed rows: one float4 (bins 2i and 2i + 1; float4 0 = re_0, re_{fl/2}, re_1, im_1) per thread, blockIdx.y = utterance.
// The magnitude rows are fl / 2 + 1 floats long, an odd count, so their two values per thread are 4-byte loads (neighbouring lanes
// read neighbouring pairs: whole cache lines are used); the packed rows are 16-byte accesses.
__global__ __launch_bounds__(256) void k_gl_recombine(const float* __restrict__ mag, const float* __restrict__ ang, const long long* __restrict__ lens,
                                                      int drop, int Tg, int fl, int hop, float* __restrict__ X) {
  const int b = blockIdx.y, q4 = fl >> 2, half = fl >> 1;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Tg * q4) return;
  const int t = (int)(idx / q4), i = (int)(idx - (long long)t * q4);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < gl_frames(lens, b, drop, Tg, fl, hop)) {
    const long long r = ((long long)b * Tg + t) * (half + 1);
    const float m1 = mag[r + 2 * i + 1], a1 = ang[r + 2 * i + 1];
    o.z = m1 * cosf(a1);
    o.w = m1 * sinf(a1);
    if (i == 0) {  // the sine rows of bins 0 and fl / 2 of the inverse basis are zero: their products are dropped
      o.x = mag[r] * cosf(ang[r]);
      o.y = mag[r + half] * cosf(ang[r + half]);
    } else {
      const float m0 = mag[r + 2 * i], a0 = ang[r + 2 * i];
      o.x = m0 * cosf(a0);
      o.y = m0 * sinf(a0);
    }
  }
  *reinterpret_cast<float4*>(X + ((long long)b * Tg + t) * fl + 4 * i) = o;
}

hipError_t launch_gl_recombine(const float* mag, const float* angles, const long long* lens, int drop, int B, int Tg, int fl, int hop,
                               float* X, hipStream_t st) {
  if (B <= 0 || Tg <= 0) return hipSuccess;
  if (B > 65535 || (fl & 3)) return hipErrorInvalidValue;
  const long long blocks = ((long long)Tg * (fl >> 2) + 255) / 256;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gl_recombine, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, mag, angles, lens, drop, Tg, fl, hop, X);
  return hipGetLastError();
}

// mag * (re, im) / |(re, im)| = mag (cos, sin)(atan2(im, re)) (stft.py:79,84-86) without the angle.  The pair is scaled by its larger
// component first, so no square under- or overflows; (0, 0) gives (mag, 0) because atan2(0, 0) = 0.  A NaN in either component makes
// both outputs of the bin NaN (fmaxf alone would drop it: (NaN, 0) would read as (0, 0)).
__device__ __forceinline__ float2 gl_unit(float re, float im, float m) {
  if (re != re || im != im) return make_float2(re + im, re + im);
  const float s = fmaxf(fabsf(re), fabsf(im));
  if (s == 0.f) return make_float2(m, 0.f);
  const float a = re / s, c = im / s;
  const float inv = 1.f / sqrtf(a * a + c * c);
  return make_float2(m * (a * inv), m * (c * inv));
}

__global__ __launch_bounds__(256) void k_gl_rephase(const float* __restrict__ Y, const float* __restrict__ mag, const long long* __restrict__ lens,
                                                    int drop, int Tg, int S, int fl, int hop, float* __restrict__ X) {
  const int b = blockIdx.y, q4 = fl >> 2, half = fl >> 1;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Tg * q4) return;
  const int t = (int)(idx / q4), i = (int)(idx - (long long)t * q4);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < gl_frames(lens, b, drop, Tg, fl, hop)) {
    const float4 y = *reinterpret_cast<const float4*>(Y + ((long long)b * S + t) * fl + 4 * i);
    const long long r = ((long long)b * Tg + t) * (half + 1);
    const float2 hi = gl_unit(y.z, y.w, mag[r + 2 * i + 1]);
    o.z = hi.x; o.w = hi.y;
    if (i == 0) {  // bins 0 and fl / 2: the imaginary part is +0
      o.x = gl_unit(y.x, 0.f, mag[r]).x;
      o.y = gl_unit(y.y, 0.f, mag[r + half]).x;
    } else {
      const float2 lo = gl_unit(y.x, y.y, mag[r + 2 * i]);
      o.x = lo.x; o.y = lo.y;
    }
  }
  *reinterpret_cast<float4*>(X + ((long long)b * Tg + t) * fl + 4 * i) = o;
}

hipError_t launch_gl_rephase(const float* Y, const float* mag, const long long* lens, int drop, int B, int Tg, int S, int fl, int hop,
                             float* X, hipStream_t st) {
  if (B <= 0 || Tg <= 0) return hipSuccess;
  if (B > 65535 || (fl & 3) || S < Tg) return hipErrorInvalidValue;
  const long long blocks = ((long long)Tg * (fl >> 2) + 255) / 256;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gl_rephase, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, Y, mag, lens, drop, Tg, S, fl, hop, X);
  return hipGetLastError();
}

// ---- overlap-add (F.conv_transpose1d's scatter as a gather, stft.py:88-93; window_sumsquare, audio_processing.py:51-63; stft.py:95-120).
// Four consecutive output samples per thread.  hop % 32 == 0 and fl / 2 % 16 == 0, so the four share their frames and each frame's
// contribution is one aligned float4.  Padded position p = s + fl / 2 lies in frame t at offset p - t hop for t in
// [max(0, (p - fl) / hop + 1), min(Tg_b - 1, p / hop)]: at most fl / hop terms, ascending.  window_sum restates the reference's fp32
// accumulator: every += adds a float64 squared-window value and rounds once to fp32, frames in ascending order.
__global__ __launch_bounds__(256) void k_gl_overlap_add(const float* __restrict__ frames, const long long* __restrict__ lens, int drop, int Tg, int fl,
                                                        int hop, const double* __restrict__ wsq, float* __restrict__ wave, long long ld,
                                                        long long* __restrict__ wave_lens_out) {
  const int b = blockIdx.y;
  const long long s0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  const int tg = gl_frames(lens, b, drop, Tg, fl, hop);
  const long long n = tg ? (long long)hop * (tg - 1) : 0;
  if (s0 == 0 && wave_lens_out) wave_lens_out[b] = n;
  if (s0 >= ld) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (s0 < n) {
    const long long p0 = s0 + (fl >> 1);
    const int t_lo = p0 < fl ? 0 : (int)((p0 - fl) / hop) + 1;
    int t_hi = (int)(p0 / hop);
    t_hi = t_hi > tg - 1 ? tg - 1 : t_hi;
    float ws[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = t_lo; t <= t_hi; ++t) {
      const int off = (int)(p0 - (long long)t * hop);
      const float4 v = *reinterpret_cast<const float4*>(frames + ((long long)b * Tg + t) * fl + off);
      acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
#pragma unroll
      for (int e = 0; e < 4; ++e) ws[e] = (float)((double)ws[e] + wsq[off + e]);
    }
    const float scale = (float)fl / (float)hop;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (ws[e] > FLT_MIN) acc[e] /= ws[e];  // tiny(window_sum), stft.py:105-114
      acc[e] = s0 + e < n ? acc[e] * scale : 0.f;
    }
  }
  *reinterpret_cast<float4*>(wave + (long long)b * ld + s0) = make_float4(acc[0], acc[1], acc[2], acc[3]);  // ld % 4 == 0: s0 + 4 <= ld
}

hipError_t launch_gl_overlap_add(const float* frames, const long long* lens, int drop, int B, int Tg, int fl, int hop, const double* wsq,
                                 float* wave, long long ld, long long* wave_lens_out, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (B > 65535 || Tg < 0 || hop <= 0 || (hop & 31) || fl % hop || ((fl >> 1) & 3) || ld < 0 || (ld & 3)) return hipErrorInvalidValue;
  long long blocks = ((ld + 3) / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;  // wave_lens_out is written even for ld == 0
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gl_overlap_add, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, frames, lens, drop, Tg, fl, hop, wsq, wave, ld,
                     wave_lens_out);
  return hipGetLastError();
}

__global__ __launch_bounds__(64) void k_gl_wave_lens(const long long* __restrict__ lens, int drop, int B, int Tg, int fl, int hop,
                                                     long long* __restrict__ wave_lens_out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int tg = gl_frames(lens, b, drop, Tg, fl, hop);
  wave_lens_out[b] = tg ? (long long)hop * (tg - 1) : 0;
}

hipError_t launch_gl_wave_lens(const long long* lens, int drop, int B, int Tg, int fl, int hop, long long* wave_lens_out, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gl_wave_lens, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, lens, drop, B, Tg, fl, hop, wave_lens_out);
  return hipGetLastError();
}

// ---- STFT.transform's outputs (stft.py:74-81): thread = bin, blockIdx.y = utterance
__global__ __launch_bounds__(256) void k_gl_polar(const float* __restrict__ Y, const long long* __restrict__ wav_lens, long long n_max, int S, int T,
                                                  int fl, int hop, float* __restrict__ magnitude, float* __restrict__ phase) {
  const int b = blockIdx.y, half = fl >> 1, bins = half + 1;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)T * bins) return;
  const int t = (int)(idx / bins), k = (int)(idx - (long long)t * bins);
  long long n = wav_lens[b];
  n = n < 0 ? 0 : (n > n_max ? n_max : n);
  const long long frames = n > half ? n / hop + 1 : 0;
  float m = 0.f, ph = 0.f;
  if (t < frames && t < S - fl / hop + 1) {
    const float* row = Y + ((long long)b * S + t) * fl;
    const float re = k == 0 ? row[0] : (k == half ? row[1] : row[2 * k]);
    const float im = (k == 0 || k == half) ? 0.f : row[2 * k + 1];
    m = sqrtf(re * re + im * im);
    ph = atan2f(im, re);
  }
  magnitude[((long long)b * T + t) * bins + k] = m;
  phase[((long long)b * T + t) * bins + k] = ph;
}

hipError_t launch_gl_polar(const float* Y, const long long* wav_lens, long long n_max, int B, int S, int T, int fl, int hop, float* magnitude,
                           float* phase, hipStream_t st) {
  if (B <= 0 || T <= 0) return hipSuccess;
  if (B > 65535 || hop <= 0 || fl % hop || S < fl / hop) return hipErrorInvalidValue;
  const long long blocks = ((long long)T * ((fl >> 1) + 1) + 255) / 256;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gl_polar, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, Y, wav_lens, n_max, S, T, fl, hop, magnitude, phase);
  return hipGetLastError();
}

}  // namespace ns
