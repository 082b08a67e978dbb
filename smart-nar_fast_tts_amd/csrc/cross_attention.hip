// Cross attention of the reference-mel aligner (MelEncoder, transformer/Models.py:103-173; FFTBlock2, transformer/Layers.py:51-70):
// mel-frame queries against phoneme keys, and — unlike attention.hip's flash-style kernels — the attention PROBABILITIES are an
// output (the reference returns them as tgt_alignment, transformer/SubLayers.py:47-49), so the softmax is a true multi-pass one
// whose stored values are final.  Also here: the aligner's input copy (frame 0 replaced by zeros, Models.py:145-146) and the
// duration count over the last layer's alignment (an extension beyond the reference, include/nar_fs2.h).
//
// k_cross_attention<DK>: one workgroup of two waves per (utterance, head, block of 64 queries); a wave owns 32 query rows and walks
// the keys in strips of 32.  Both contractions run on v_mfma_f32_32x32x2_f32:
//   pass A  S = Q K^T per strip (A = Q: lane l holds row l & 31; B = K: lane l holds key l & 31; the contraction index of a lane's
//           e-th MFMA is channel (l >> 5) * DK / 2 + e, so both fragments are contiguous float4 reads of a row), divided by
//           sqrt(dk), keys >= src_len set to -inf, stored RAW into the attn buffer; running row maximum per lane
//   pass B  re-reads the lane's own raw scores, sums exp(s - max)
//   pass C  re-reads them once more, stores p = exp(s - max) / sum (final: masked keys exactly 0, an utterance with src_len == 0
//           is NaN like torch's softmax over a row of -inf), transposes the strip through LDS into the A fragment and accumulates
//           O += P V (B = V: lane l holds channel l & 31 of key (l >> 5) * 16 + e of the strip: coalesced row reads)
// A lane only ever re-reads addresses it wrote itself, so the passes need no fence.  Every output element is one fixed-order sum:
// replicas of an utterance inside a batch carry the same bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include "kernels.h"

namespace ns {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int XA_QW = 32;      // query rows per wave
constexpr int XA_WAVES = 2;    // waves per workgroup
constexpr int XA_KS = 32;      // keys per strip

template <int DK>
__global__ __launch_bounds__(64 * XA_WAVES) void k_cross_attention(const float* __restrict__ q, const float* __restrict__ kv,
                                                                   const long long* __restrict__ src_lens, int T, int L, int H,
                                                                   float* __restrict__ ctx, float* attn) {
  constexpr int HALF = DK / 2, NDB = DK / 32;
  __shared__ float pl[XA_WAVES][32][33];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 31, g = lane >> 5;
  const int nqb = (T + XA_QW * XA_WAVES - 1) / (XA_QW * XA_WAVES);
  int blk = blockIdx.x;
  const int qb = blk % nqb; blk /= nqb;
  const int h = blk % H, b = blk / H;
  const int d = H * DK;
  const int q0 = (qb * XA_WAVES + w) * XA_QW;
  const long long sl = src_lens[b];
  const int slen = sl < 0 ? 0 : (sl > L ? L : (int)sl);
  const float temperature = sqrtf((float)DK);  // transformer/SubLayers.py:22, Modules.py:16-17: attn = bmm(q, k^T) / temperature
  const float NEG_INF = -INFINITY;

  float qf[HALF];
  {
    const int tq = q0 + r;
    const bool ok = tq < T;
    const float* qp = q + ((size_t)b * T + (ok ? tq : 0)) * d + h * DK + g * HALF;
#pragma unroll
    for (int i = 0; i < HALF / 4; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (ok) v = *reinterpret_cast<const f32x4*>(qp + 4 * i);
      qf[4 * i] = v[0]; qf[4 * i + 1] = v[1]; qf[4 * i + 2] = v[2]; qf[4 * i + 3] = v[3];
    }
  }
  // accumulator register e of a 32x32 tile: row (e & 3) + 8 * (e >> 2) + 4 * g, column r
  float* arow = attn + (((size_t)b * H + h) * T) * (size_t)L;
  auto at = [&](int e, int key) -> float* { return arow + (size_t)(q0 + (e & 3) + 8 * (e >> 2) + 4 * g) * L + key; };
  auto row_ok = [&](int e) { return q0 + (e & 3) + 8 * (e >> 2) + 4 * g < T; };

  // ---- pass A: raw scores, row maximum
  float mx[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) mx[e] = NEG_INF;
  for (int k0 = 0; k0 < L; k0 += XA_KS) {
    const int key = k0 + r;
    const bool kok = key < L;
    const float* kp = kv + ((size_t)b * L + (kok ? key : 0)) * (size_t)(2 * d) + h * DK + g * HALF;
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
    for (int i = 0; i < HALF / 4; ++i) {
      f32x4 kk = {0.f, 0.f, 0.f, 0.f};
      if (kok) kk = *reinterpret_cast<const f32x4*>(kp + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[4 * i + e], kk[e], s, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float v = key < slen ? s[e] / temperature : NEG_INF;
      mx[e] = fmaxf(mx[e], v);
      if (kok && row_ok(e)) *at(e, key) = v;
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e)
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) mx[e] = fmaxf(mx[e], __shfl_xor(mx[e], off));

  // ---- pass B: sum of exp(s - max)
  float sum[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) sum[e] = 0.f;
  for (int k0 = 0; k0 < L; k0 += XA_KS) {
    const int key = k0 + r;
    if (key < L) {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (row_ok(e)) sum[e] += expf(*at(e, key) - mx[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e)
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) sum[e] += __shfl_xor(sum[e], off);

  // ---- pass C: final probabilities, O = P V
  f32x16 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  for (int k0 = 0; k0 < L; k0 += XA_KS) {
    const int key = k0 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float p = 0.f;
      if (key < L && row_ok(e)) {
        float* a = at(e, key);
        p = expf(*a - mx[e]) / sum[e];
        *a = p;
      }
      pl[w][(e & 3) + 8 * (e >> 2) + 4 * g][r] = p;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
      const int kx = k0 + g * 16 + j;
      const bool vok = kx < L;
      const float a = pl[w][r][g * 16 + j];
      const float* vp = kv + ((size_t)b * L + (vok ? kx : 0)) * (size_t)(2 * d) + d + h * DK + r;
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const float vv = vok ? vp[db * 32] : 0.f;
        o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, vv, o[db], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // merged heads: ctx [B*T, H*dk], head h at column h * dk (transformer/SubLayers.py:51-54)
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (!row_ok(e)) continue;
    float* cp = ctx + ((size_t)b * T + q0 + (e & 3) + 8 * (e >> 2) + 4 * g) * d + h * DK + r;
#pragma unroll
    for (int db = 0; db < NDB; ++db) cp[db * 32] = o[db][e];
  }
}

bool cross_attention_ok(int H, int dk) { return H > 0 && (dk == 64 || dk == 128); }

hipError_t launch_cross_attention(const float* q, const float* kv, const long long* src_lens, int B, int T, int L, int H, int dk,
                                  float* ctx, float* attn, hipStream_t st) {
  if (B <= 0 || T <= 0) return hipSuccess;
  if (L <= 0 || !cross_attention_ok(H, dk)) return hipErrorInvalidValue;
  if (((uintptr_t)q | (uintptr_t)kv) & 15) return hipErrorInvalidValue;  // float4 fragment reads
  const long long nqb = (T + XA_QW * XA_WAVES - 1) / (XA_QW * XA_WAVES);
  const long long wgs = (long long)B * H * nqb;
  if (wgs >= (1ll << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)wgs), block(64 * XA_WAVES);
  if (dk == 128) hipLaunchKernelGGL(k_cross_attention<128>, grid, block, 0, st, q, kv, src_lens, T, L, H, ctx, attn);
  else hipLaunchKernelGGL(k_cross_attention<64>, grid, block, 0, st, q, kv, src_lens, T, L, H, ctx, attn);
  return hipGetLastError();
}

// x[m, :] = mels[m, :], rows at frame 0 of an utterance zero (transformer/Models.py:145-146: a replacement, not a shift).
__global__ __launch_bounds__(256) void k_aln_input(const float* __restrict__ mels, float* __restrict__ x, long long n4, int T, int C4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long long m = i / C4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (m % T != 0) v = reinterpret_cast<const f32x4*>(mels)[i];
  reinterpret_cast<f32x4*>(x)[i] = v;
}
hipError_t launch_aln_input(const float* mels, float* x, int B, int T, int C, hipStream_t st) {
  if (B <= 0 || T <= 0) return hipSuccess;
  if ((C & 3) || (((uintptr_t)mels | (uintptr_t)x) & 15)) return hipErrorInvalidValue;
  const long long n4 = (long long)B * T * (C / 4);
  hipLaunchKernelGGL(k_aln_input, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, mels, x, n4, T, C / 4);
  return hipGetLastError();
}

// durations[b, i] = #{t < mel_len[b] : argmax_{l < src_len[b]} sum_h attn[b, h, t, l] == i}; heads summed in head order in fp32,
// ties to the lowest l.  One wave per (utterance, frame); `out` [B, L] int64 must be zero on entry.
__global__ __launch_bounds__(256) void k_aln_durations(const float* __restrict__ attn, const long long* __restrict__ src_lens,
                                                       const long long* __restrict__ mel_lens, int B, int H, int T, int L,
                                                       unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= (long long)B * T) return;
  const int b = (int)(gw / T), t = (int)(gw % T);
  const long long sl = src_lens[b], ml = mel_lens[b];
  const int slen = sl < 0 ? 0 : (sl > L ? L : (int)sl);
  if (slen == 0 || (long long)t >= ml) return;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int l = lane; l < slen; l += 64) {
    float a = attn[(((size_t)b * H) * T + t) * (size_t)L + l];
    for (int h = 1; h < H; ++h) a = a + attn[(((size_t)b * H + h) * T + t) * (size_t)L + l];
    if (a > best || bi == 0x7fffffff) { best = a; bi = l; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int oi = __shfl_xor(bi, off);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
  }
  if (lane == 0 && bi < slen) atomicAdd(out + (size_t)b * L + bi, 1ull);
}
hipError_t launch_aln_durations(const float* attn_last, const long long* src_lens, const long long* mel_lens, int B, int H, int T, int L,
                                long long* out, hipStream_t st) {
  if (B <= 0 || L <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)B * L * sizeof(long long), st);
  if (e != hipSuccess || T <= 0) return e;
  const long long waves = (long long)B * T;
  hipLaunchKernelGGL(k_aln_durations, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, attn_last, src_lens, mel_lens, B, H, T, L,
                     reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}

}  // namespace ns
