// FastSpeech2Loss.forward in eval() (model/loss.py:149-250): the six masked means of a teacher-forced batch and their total, in two
// launches on one stream with no host read and no float atomic.
//   k_loss_partial  one launch over a flat work list of three segments — frame rows, phoneme rows, guided-attention row blocks; a
//                   workgroup owns a fixed slice of one segment and writes its partial sums into its own workspace slot
//   k_loss_final    one workgroup: sums the slots in a fixed order in float64, derives the counts as int64, divides, writes 7 floats
//                   (and, where the caller passes a record, the three counts: what the backward of lossgrad.hip divides by)
// Selection, not multiplication: a masked-out element never enters the arithmetic (`cond ? term : 0`).  Padded positions may
// hold NaN (an utterance with src_lens == 0); masked_select drops them, 0 * NaN would not.
// Reduction order: per-thread fp32 over a short fixed run, wave64 shuffle tree in fp32, the four waves of a workgroup added in
// wave order in float64.  Which element lands in which (thread, slot) depends on (B, L, T, H, n_mel, feature levels) only — not on
// pointer alignment, not on the stream, not on what the workspace held — so equal inputs give equal bits.
#include "kernels.h"
#include "loss_guide.h"

namespace ns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int LOSS_THREADS = 256;
// slot words: 0 sum|mel - tgt|, 1 sum|postnet - tgt|, 2 sum (pitch err)^2, 3 sum (energy err)^2, 4 sum (log-duration err)^2,
// 5 sum_k sum W * attn_k (doubles); 6 unmasked frames, 7 unmasked phonemes (int64)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// every word of the slot is written, so the workspace needs no initialisation
__device__ __forceinline__ void write_slot(const float (&acc)[LOSS_SLOT_SUMS], int n_frames, int n_phonemes, void* slot) {
  __shared__ double part[LOSS_THREADS / 64][LOSS_SLOT_SUMS];
  __shared__ int cnt[LOSS_THREADS / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < LOSS_SLOT_SUMS; ++q) {
    const float s = wave_sum(acc[q]);
    if (lane == 0) part[wave][q] = (double)s;
  }
  const int nf = wave_sum(n_frames), np = wave_sum(n_phonemes);
  if (lane == 0) { cnt[wave][0] = nf; cnt[wave][1] = np; }
  __syncthreads();
  if (threadIdx.x < LOSS_SLOT_WORDS) {
    const int q = threadIdx.x;
    if (q < LOSS_SLOT_SUMS) {
      double s = part[0][q];
#pragma unroll
      for (int w = 1; w < LOSS_THREADS / 64; ++w) s += part[w][q];
      reinterpret_cast<double*>(slot)[q] = s;
    } else {
      long long c = 0;
#pragma unroll
      for (int w = 0; w < LOSS_THREADS / 64; ++w) c += cnt[w][q - LOSS_SLOT_SUMS];
      reinterpret_cast<long long*>(slot)[q] = c;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(LOSS_THREADS) void k_loss_partial(LossArgs a, int n_frame_wgs, int n_phoneme_wgs, char* __restrict__ ws) {
  const int tid = threadIdx.x;
  int wg = blockIdx.x;
  float acc[LOSS_SLOT_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int n_frames = 0, n_phonemes = 0;
  void* slot = ws + (size_t)wg * LOSS_SLOT_BYTES;

  if (wg < n_frame_wgs) {
    // ---- frame rows: LOSS_FRAME_ROWS rows x n_mel / 4 vectors, flat over the workgroup's lanes (n_mel = 80 is 20 float4: a
    // wave per row would idle 44 lanes); the row is recovered per vector
    const long long M = (long long)a.B * a.T;
    const long long r0 = (long long)wg * LOSS_FRAME_ROWS;
    const int C4 = a.n_mel >> 2;
    const int rows = (int)(M - r0 < LOSS_FRAME_ROWS ? M - r0 : LOSS_FRAME_ROWS);
    const int nvec = rows * C4;
    for (int v = tid; v < nvec; v += LOSS_THREADS) {
      const int r = v / C4, c = v - r * C4;
      const long long m = r0 + r;
      if (a.mel_masks[m]) continue;  // padded frame: not read (model/loss.py:189,219-224)
      const long long b = m / a.T, t = m - b * a.T;
      const f32x4 x = reinterpret_cast<const f32x4*>(a.mel + m * a.n_mel)[c];
      const f32x4 p = reinterpret_cast<const f32x4*>(a.postnet + m * a.n_mel)[c];
      const f32x4 y = reinterpret_cast<const f32x4*>(a.mel_targets + b * a.mel_targets_stride + t * a.n_mel)[c];  // mel_targets[:, :T] (loss.py:191)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[0] += fabsf(x[j] - y[j]);
        acc[1] += fabsf(p[j] - y[j]);
      }
    }
    if (tid < rows) {
      const long long m = r0 + tid;
      if (!a.mel_masks[m]) {
        n_frames = 1;
        if (a.pitch_frame_level) { const float d = a.pitch[m] - a.pitch_targets[m]; acc[2] = d * d; }
        if (a.energy_frame_level) { const float d = a.energy[m] - a.energy_targets[m]; acc[3] = d * d; }
      }
    }
  } else if ((wg -= n_frame_wgs) < n_phoneme_wgs) {
    // ---- phoneme rows: the log-duration error, and pitch / energy at phoneme_level
    const long long M = (long long)a.B * a.L;
    const long long r0 = (long long)wg * LOSS_PHONEME_ROWS;
#pragma unroll
    for (int i = 0; i < LOSS_PHONEME_ROWS / LOSS_THREADS; ++i) {
      const long long m = r0 + i * LOSS_THREADS + tid;
      if (m >= M || a.src_masks[m]) continue;
      const long long b = m / a.L, l = m - b * a.L;
      n_phonemes += 1;
      // log(duration_targets.float() + 1) (model/loss.py:190), columns past L never read (:214-216)
      const float tgt = logf((float)a.d_targets[b * a.d_targets_stride + l] + 1.0f);
      const float d = a.log_d[m] - tgt;
      acc[4] += d * d;
      if (!a.pitch_frame_level) { const float e = a.pitch[m] - a.pitch_targets[m]; acc[2] += e * e; }
      if (!a.energy_frame_level) { const float e = a.energy[m] - a.energy_targets[m]; acc[3] += e * e; }
    }
  } else {
    // ---- guided attention: LOSS_ATTN_ROWS query rows of head 0 of one utterance, all four maps.  Head 0's rows t0 .. t0 + rows
    // are one contiguous run of rows * L floats inside [B, H, T, L]; it is cut into groups of four at multiples of four of the
    // TENSOR's element index (the same cut for the four maps: W is computed once per element), a group is one 16-byte load when
    // the map's base pointer is 16-byte aligned and four 4-byte loads otherwise, and the elements before the first and after the
    // last group boundary are read one by one.  L need not be a multiple of four and no row is rounded.
    wg -= n_phoneme_wgs;
    const int chunks = (a.T + LOSS_ATTN_ROWS - 1) / LOSS_ATTN_ROWS;
    const int b = wg / chunks, t0 = (wg - b * chunks) * LOSS_ATTN_ROWS;
    const int ilen = clamp_len(a.src_lens[b], a.L), olen = clamp_len(a.mel_lens[b], a.T);
    const int rows = (olen - t0 < LOSS_ATTN_ROWS ? olen - t0 : LOSS_ATTN_ROWS);  // rows at t >= olen are not read
    if (rows > 0 && ilen > 0) {
      const float fi = (float)ilen, fo = (float)olen;
      const size_t o = (((size_t)b * a.H) * a.T + t0) * (size_t)a.L;
      const int n = rows * a.L;
      int head = (int)((4 - (o & 3)) & 3);
      head = head < n ? head : n;
      const int groups = (n - head) >> 2;
      const int tail0 = head + 4 * groups;
      bool vec[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) vec[k] = ((uintptr_t)a.attn[k] & 15) == 0;
      float s = 0.f;
      for (int g = tid; g < groups; g += LOSS_THREADS) {
        const int rel = head + 4 * g;
        int r = rel / a.L, l = rel - r * a.L;
        float w[4];
        bool sel[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sel[j] = l < ilen;  // (t0 + r < olen by the choice of rows)
          any |= sel[j];
          w[j] = sel[j] ? guide(t0 + r, l, fi, fo) : 0.f;
          if (++l == a.L) { l = 0; ++r; }
        }
        if (!any) continue;  // four padded keys: not read
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float* p = a.attn[k] + o + rel;
          f32x4 v;
          if (vec[k]) v = *reinterpret_cast<const f32x4*>(p);
          else { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3]; }
#pragma unroll
          for (int j = 0; j < 4; ++j) s += sel[j] ? w[j] * v[j] : 0.f;
        }
      }
      // the up to three elements in front of the first group (threads 0-2) and behind the last one (threads 4-6)
      const int edge = tid < 4 ? tid : tail0 + (tid - 4);
      if ((tid < 4 && tid < head) || (tid >= 4 && tid < 8 && edge < n)) {
        const int r = edge / a.L, l = edge - r * a.L;
        if (l < ilen) {
          const float w = guide(t0 + r, l, fi, fo);
#pragma unroll
          for (int k = 0; k < 4; ++k) s += w * a.attn[k][o + edge];
        }
      }
      acc[5] = s;
    }
  }
  write_slot(acc, n_frames, n_phonemes, slot);
}

// out7 = total, mel, postnet, pitch, energy, duration, attn (model/loss.py:242-250).  A zero count divides 0 by 0: NaN, what
// torch.mean of an empty selection gives, and the total is then NaN too.
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_final(LossArgs a, int n_slots, const char* __restrict__ ws, float* __restrict__ out7,
                                                               long long* __restrict__ record) {
  __shared__ double part[LOSS_THREADS][LOSS_SLOT_SUMS];
  __shared__ long long cnt[LOSS_THREADS][3];
  const int tid = threadIdx.x;
  double s[LOSS_SLOT_SUMS] = {0, 0, 0, 0, 0, 0};
  long long c[3] = {0, 0, 0};
  for (int i = tid; i < n_slots; i += LOSS_THREADS) {  // thread i: slots i, i + 256, ... in slot order
    const double* d = reinterpret_cast<const double*>(ws + (size_t)i * LOSS_SLOT_BYTES);
#pragma unroll
    for (int q = 0; q < LOSS_SLOT_SUMS; ++q) s[q] += d[q];
    c[0] += reinterpret_cast<const long long*>(d)[6];
    c[1] += reinterpret_cast<const long long*>(d)[7];
  }
  for (int b = tid; b < a.B; b += LOSS_THREADS)  // the selected attention cells: sum_b ilen_b * olen_b (model/loss.py:144-146)
    c[2] += (long long)clamp_len(a.src_lens[b], a.L) * (long long)clamp_len(a.mel_lens[b], a.T);
#pragma unroll
  for (int q = 0; q < LOSS_SLOT_SUMS; ++q) part[tid][q] = s[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) cnt[tid][q] = c[q];
  __syncthreads();
  for (int w = LOSS_THREADS / 2; w >= 1; w >>= 1) {  // a fixed tree: thread i adds thread i + w
    if (tid < w) {
#pragma unroll
      for (int q = 0; q < LOSS_SLOT_SUMS; ++q) part[tid][q] += part[tid + w][q];
#pragma unroll
      for (int q = 0; q < 3; ++q) cnt[tid][q] += cnt[tid + w][q];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double nf = (double)cnt[0][0], np = (double)cnt[0][1], na = (double)cnt[0][2];
    const float mel = (float)(part[0][0] / ((double)a.n_mel * nf));
    const float post = (float)(part[0][1] / ((double)a.n_mel * nf));
    const float pitch = (float)(part[0][2] / (a.pitch_frame_level ? nf : np));
    const float energy = (float)(part[0][3] / (a.energy_frame_level ? nf : np));
    const float dur = (float)(part[0][4] / np);
    const float attn = (float)(GA_ALPHA * part[0][5] / na);
    out7[0] = mel + post + dur + pitch + energy + attn;  // the reference's order (model/loss.py:238-240)
    out7[1] = mel; out7[2] = post; out7[3] = pitch; out7[4] = energy; out7[5] = dur; out7[6] = attn;
    if (record) {  // what the backward divides by (lossgrad.hip): the caller's own words, not the shared workspace
      record[0] = cnt[0][0]; record[1] = cnt[0][1]; record[2] = cnt[0][2]; record[3] = 0;
    }
  }
}

long long loss_slots(int B, int L, int T, int* n_frame_wgs, int* n_phoneme_wgs) {
  const long long nf = ((long long)B * T + LOSS_FRAME_ROWS - 1) / LOSS_FRAME_ROWS;
  const long long np = ((long long)B * L + LOSS_PHONEME_ROWS - 1) / LOSS_PHONEME_ROWS;
  const long long na = (long long)B * ((T + LOSS_ATTN_ROWS - 1) / LOSS_ATTN_ROWS);
  if (n_frame_wgs) *n_frame_wgs = (int)nf;
  if (n_phoneme_wgs) *n_phoneme_wgs = (int)np;
  return nf + np + na;
}

hipError_t launch_loss(const LossArgs& a, void* ws, float* out7, hipStream_t st, long long* record) {
  int nf = 0, np = 0;
  const long long slots = loss_slots(a.B, a.L, a.T, &nf, &np);
  if (slots >= (1ll << 31)) return hipErrorInvalidValue;
  if (slots > 0) {
    hipLaunchKernelGGL(k_loss_partial, dim3((unsigned)slots), dim3(LOSS_THREADS), 0, st, a, nf, np, (char*)ws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(LOSS_THREADS), 0, st, a, (int)slots, (const char*)ws, out7, record);
  return hipGetLastError();
}

}  // namespace ns
