// FastSpeech2Loss backward (train.py:88 through model/loss.py:149-250): the gradient of sum_i g[i] * out7[i] with respect to the five
// predictions and the four alignment maps, in one launch with no host read, no atomic and no LDS.
//   k_lossg_backward  one launch over a flat work list of three segments, as k_loss_partial — frame rows (d_mel, d_postnet, and
//                     d_pitch / d_energy at frame_level), phoneme rows (d_log_d, and d_pitch / d_energy at phoneme_level), the
//                     elements of the maps (d_attn[0..3]).  A workgroup owns a fixed run of one segment's flat element indices and
//                     writes every element of it in every wanted tensor: zeros where a mask hides the element.
// Selection, not multiplication: a masked-out prediction is never read and its gradient is the constant +0.0f, so NaN behind a mask
// (an utterance with src_lens == 0) cannot leak — masked_select's backward, not 0 * NaN.  A part whose selection is
// empty has a NaN or infinite coefficient (count 0) and no selected element: the coefficient is never applied.
// Coefficients: g7 (autograd's grad_output, [7] fp32) and the record (the forward's three int64 counts, k_loss_final) are read here,
// on the device; (g[0] + g[i]) / count is formed in float64 and rounded to fp32 once.  The maps' gradient does not depend on the maps:
// ALPHA * (g[0] + g[6]) / n_attn * W[t, l] on head 0 inside {t < olen_b, l < ilen_b}, W = guide() of the forward, computed once per
// element and stored to the four maps.
// Stores are 16-byte vectors at multiples of four of the tensor's flat element index (every output is 16-byte aligned), the last
// one to three elements of a tensor one by one; L, T and B * H * T * L need not be multiples of four.
#include "kernels.h"
#include "loss_guide.h"

namespace ns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int LOSSG_THREADS = 256;
static_assert(LOSSG_PHONEME_ROWS == 4 * LOSSG_THREADS && LOSSG_ATTN_ELEMS % (4 * LOSSG_THREADS) == 0 && LOSSG_FRAME_ROWS % 4 == 0 &&
              LOSSG_FRAME_ROWS / 4 <= LOSSG_THREADS, "work list geometry");

// (g[0] + g[i]) / count, times `scale`, in float64, rounded once
__device__ __forceinline__ float coef(const float* __restrict__ g, int i, double scale, long long count) {
  return (float)(scale * ((double)g[0] + (double)g[i]) / (double)count);
}

// four consecutive elements m0 .. m0 + 3 of a [M] tensor: one 16-byte store, or the tensor's last one to three elements one by one
__device__ __forceinline__ void store4(float* __restrict__ out, long long m0, long long M, const float (&v)[4]) {
  if (m0 + 3 < M) {
    f32x4 q;
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3];
    *reinterpret_cast<f32x4*>(out + m0) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (m0 + j < M) out[m0 + j] = v[j];
  }
}

// 2 * c * (x - y) of four rows of a per-row scalar (pitch, energy): c2 = 2 * c
__device__ __forceinline__ void mse4(const float* __restrict__ x, const float* __restrict__ y, const unsigned char* __restrict__ masks, float c2,
                                     float* __restrict__ out, long long m0, long long M) {
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long m = m0 + j;
    v[j] = (m < M && !masks[m]) ? c2 * (x[m] - y[m]) : 0.f;
  }
  store4(out, m0, M, v);
}
}  // namespace

__global__ __launch_bounds__(LOSSG_THREADS) void k_lossg_backward(LossArgs a, LossGrads d, const long long* __restrict__ record,
                                                                  const float* __restrict__ g, int n_frame_wgs, int n_phoneme_wgs) {
  const int tid = threadIdx.x;
  int wg = blockIdx.x;
  const long long n_frames = record[0], n_phonemes = record[1], n_attn = record[2];

  if (wg < n_frame_wgs) {
    // ---- frame rows: LOSSG_FRAME_ROWS rows x n_mel / 4 vectors, flat over the workgroup's lanes as in k_loss_partial
    const long long M = (long long)a.B * a.T;
    const long long r0 = (long long)wg * LOSSG_FRAME_ROWS;
    const int rows = (int)(M - r0 < LOSSG_FRAME_ROWS ? M - r0 : LOSSG_FRAME_ROWS);
    if (d.mel || d.postnet) {
      const float c_mel = coef(g, 1, 1.0, n_frames * a.n_mel), c_post = coef(g, 2, 1.0, n_frames * a.n_mel);
      const int C4 = a.n_mel >> 2;
      const int nvec = rows * C4;
      for (int v = tid; v < nvec; v += LOSSG_THREADS) {
        const int r = v / C4, c = v - r * C4;
        const long long m = r0 + r;
        f32x4 dx = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
        if (!a.mel_masks[m]) {  // a padded frame is not read (model/loss.py:189,219-224)
          const long long b = m / a.T, t = m - b * a.T;
          const f32x4 y = reinterpret_cast<const f32x4*>(a.mel_targets + b * a.mel_targets_stride + t * a.n_mel)[c];
          if (d.mel) {
            const f32x4 x = reinterpret_cast<const f32x4*>(a.mel + m * a.n_mel)[c];
#pragma unroll
            for (int j = 0; j < 4; ++j)  // c * sign(x - y), sign(0) = 0 (torch's abs backward); x - y is 0 in fp32 only for x == y
              dx[j] = c_mel * (float)((x[j] > y[j]) - (x[j] < y[j]));
          }
          if (d.postnet) {
            const f32x4 p = reinterpret_cast<const f32x4*>(a.postnet + m * a.n_mel)[c];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              dp[j] = c_post * (float)((p[j] > y[j]) - (p[j] < y[j]));
          }
        }
        if (d.mel) reinterpret_cast<f32x4*>(d.mel + m * a.n_mel)[c] = dx;
        if (d.postnet) reinterpret_cast<f32x4*>(d.postnet + m * a.n_mel)[c] = dp;
      }
    }
    // the per-frame scalars: r0 is a multiple of four, a thread owns four rows
    const bool pitch = a.pitch_frame_level && d.pitch, energy = a.energy_frame_level && d.energy;
    if ((pitch || energy) && 4 * tid < rows) {
      const long long m0 = r0 + 4 * tid;
      if (pitch) mse4(a.pitch, a.pitch_targets, a.mel_masks, coef(g, 3, 2.0, n_frames), d.pitch, m0, M);
      if (energy) mse4(a.energy, a.energy_targets, a.mel_masks, coef(g, 4, 2.0, n_frames), d.energy, m0, M);
    }
  } else if ((wg -= n_frame_wgs) < n_phoneme_wgs) {
    // ---- phoneme rows: four per thread
    const long long M = (long long)a.B * a.L;
    const long long m0 = (long long)wg * LOSSG_PHONEME_ROWS + 4 * tid;
    if (m0 < M) {
      if (d.log_d) {
        const float c2 = coef(g, 5, 2.0, n_phonemes);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long m = m0 + j;
          v[j] = 0.f;
          if (m < M && !a.src_masks[m]) {
            const long long b = m / a.L, l = m - b * a.L;
            // log(duration_targets.float() + 1) (model/loss.py:190): the fp32 argument of k_loss_partial, its logarithm taken in
            // float64 and rounded once.  The device logf is one ulp off the correctly rounded value at some arguments (12.0f is
            // one) where the host's is not, and one ulp of a target near 2.5 is more than a gradient's whole allowance.
            const float tgt = (float)log((double)((float)a.d_targets[b * a.d_targets_stride + l] + 1.0f));
            v[j] = c2 * (a.log_d[m] - tgt);
          }
        }
        store4(d.log_d, m0, M, v);
      }
      if (!a.pitch_frame_level && d.pitch) mse4(a.pitch, a.pitch_targets, a.src_masks, coef(g, 3, 2.0, n_phonemes), d.pitch, m0, M);
      if (!a.energy_frame_level && d.energy) mse4(a.energy, a.energy_targets, a.src_masks, coef(g, 4, 2.0, n_phonemes), d.energy, m0, M);
    }
  } else {
    // ---- the maps: LOSSG_ATTN_ELEMS consecutive elements of [B, H, T, L], the same run in the four maps.  One 64-bit division
    // finds the workgroup's first (row, column); a thread's groups lie less than LOSSG_ATTN_ELEMS + L < 2^27 behind it, and the
    // rows B * H * T fit 31 bits (ns_lossg_backward), so the rest is 32-bit.
    wg -= n_phoneme_wgs;
    const long long N = (long long)a.B * a.H * a.T * a.L;
    const long long e0 = (long long)wg * LOSSG_ATTN_ELEMS;
    const long long row0 = e0 / a.L;
    const unsigned l0 = (unsigned)(e0 - row0 * a.L);
    const float c = coef(g, 6, GA_ALPHA, n_attn);
#pragma unroll 1
    for (int i = 0; i < LOSSG_ATTN_ELEMS / (4 * LOSSG_THREADS); ++i) {
      const unsigned off = 4u * (unsigned)(i * LOSSG_THREADS + tid);
      const long long e = e0 + off;
      if (e >= N) break;
      const unsigned col = l0 + off, q = col / (unsigned)a.L;
      unsigned row = (unsigned)row0 + q;
      int l = (int)(col - q * (unsigned)a.L);
      float v[4];
      int t = 0, ilen = 0;  // ilen == 0: nothing selected in this row
      float fi = 0.f, fo = 0.f;
      bool fresh = true;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (fresh) {  // a new row: (b, h, t) and the utterance's lengths
          const unsigned bh = row / (unsigned)a.T;
          t = (int)(row - bh * (unsigned)a.T);
          const unsigned b = bh / (unsigned)a.H;
          ilen = 0;
          if (bh - b * (unsigned)a.H == 0 && b < (unsigned)a.B) {  // head 0 only (model/loss.py:233-236); b == B: behind the tensor's end
            const int olen = clamp_len(a.mel_lens[b], a.T);
            if (t < olen) {
              ilen = clamp_len(a.src_lens[b], a.L);
              fi = (float)ilen; fo = (float)olen;
            }
          }
          fresh = false;
        }
        v[j] = l < ilen ? c * guide(t, l, fi, fo) : 0.f;
        if (++l == a.L) { l = 0; ++row; fresh = true; }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (d.attn[k]) store4(d.attn[k], e, N, v);
    }
  }
}

long long lossg_wgs(const LossArgs& a, const LossGrads& d, int* n_frame_wgs, int* n_phoneme_wgs) {
  const bool p = d.pitch != nullptr, e = d.energy != nullptr;
  const bool frame = d.mel || d.postnet || (p && a.pitch_frame_level) || (e && a.energy_frame_level);
  const bool phoneme = d.log_d || (p && !a.pitch_frame_level) || (e && !a.energy_frame_level);
  const bool maps = d.attn[0] || d.attn[1] || d.attn[2] || d.attn[3];
  const long long nf = frame ? ((long long)a.B * a.T + LOSSG_FRAME_ROWS - 1) / LOSSG_FRAME_ROWS : 0;
  const long long np = phoneme ? ((long long)a.B * a.L + LOSSG_PHONEME_ROWS - 1) / LOSSG_PHONEME_ROWS : 0;
  const long long na = maps ? ((long long)a.B * a.H * a.T * a.L + LOSSG_ATTN_ELEMS - 1) / LOSSG_ATTN_ELEMS : 0;
  if (n_frame_wgs) *n_frame_wgs = (int)nf;
  if (n_phoneme_wgs) *n_phoneme_wgs = (int)np;
  return nf + np + na;
}

hipError_t launch_lossg(const LossArgs& a, const long long* record, const float* g7, const LossGrads& d, hipStream_t st) {
  int nf = 0, np = 0;
  const long long wgs = lossg_wgs(a, d, &nf, &np);
  if (wgs >= (1ll << 31)) return hipErrorInvalidValue;
  if (wgs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_lossg_backward, dim3((unsigned)wgs), dim3(LOSSG_THREADS), 0, st, a, d, record, g7, nf, np);
  return hipGetLastError();
}

}  // namespace ns
