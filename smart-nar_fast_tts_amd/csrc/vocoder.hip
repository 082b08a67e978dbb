// HiFi-GAN generator (the reference's vocoder, utils/model.py:38-88) on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Activations are time-major [B, S, C] like the rest of the library, so no layer needs a transpose.  Two kernels do the work:
//
// k_voc_gemm — one implicit GEMM for every convolution of the generator except conv_pre (gemm_conv.hip) and conv_post (below):
//   * the ResBlock1 convolutions, "same" Conv1d with dilation d: grid row t of utterance b reads input rows t + off0 + j d,
//     j < KW, off0 = -d (KW - 1) / 2, zero outside the utterance's [0, S);
//   * the ConvTranspose1d(k = 2u, stride u, padding u / 2) upsamplers as a POLYPHASE GEMM: grid row q in [0, S_in] is a 2-tap
//     conv over (x[q - 1], x[q]) with N = u * Cout columns ordered (r, co):
//         y[q u + r - p, co] = x[q] . W[:, co, r] + x[q - 1] . W[:, co, r + u],   p = u / 2
//     in time-major layout row q's u * Cout outputs are one contiguous run starting at output row q u - p, so the store is a
//     plain GEMM store shifted by -p rows and clipped to the utterance.
//   The input leaky ReLU (slope 0.1) is applied to the A operand as it is staged (lrelu(0) = 0 keeps the zero padding valid), so
//   no activated copy of a tensor is ever written.  Epilogues: + bias, then optionally lrelu(0.1) (c1), + residual (c2), and the
//   multi-receptive-field sum of the last c2 of a resblock: store / += / (xs + v) / n_kernels, in the reference's order.
//   Accumulation is chunked: each BK = 32 slice of K is summed by the MFMAs from zero and then added into a running total, so
//   the matrix cores round against short partial sums at every contraction length (K reaches 2816 at stage 0).
//   Staging is register-based (global float4 -> VGPR -> lrelu -> LDS, next slice prefetched while the MFMAs run on this one);
//   LDS rows are padded to 36 floats so the fragment reads (ds_read_b128, lane-half h holds k = 8g + 4h .. +3) are conflict-free.
//
// k_voc_post — conv_post (Cout = 1, K = 7 * 32): a bandwidth-bound VALU kernel, lrelu(0.01) on load, bias, tanhf, one sample
//   per thread from an LDS window of the input rows.
#include "kernels.h"

namespace ns {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

static constexpr int VBK = 32;       // k values per staged slice (every channel count of the generator is a multiple of 32)
static constexpr int VLDK = VBK + 4; // LDS row stride in floats

static __device__ __forceinline__ float lrelu(float v, float s) { return v > 0.f ? v : v * s; }

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN) void k_voc_gemm(VocGemm p) {
  constexpr int NT = 64 * WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
  constexpr int AU = BM * VBK / 4 / NT, BU = BN * VBK / 4 / NT;  // float4 staging units per thread
  static_assert(TM >= 1 && TN >= 1 && WM % 32 == 0 && WN % 32 == 0, "wave tile");
  static_assert(AU >= 1 && BU >= 1 && AU * NT * 4 == BM * VBK && BU * NT * 4 == BN * VBK, "staging units");
  __shared__ __attribute__((aligned(16))) float As[BM * VLDK];
  __shared__ __attribute__((aligned(16))) float Bs[BN * VLDK];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ntn = (p.N + BN - 1) / BN;
  const long long tile_m = blockIdx.x / ntn;
  const int tile_n = blockIdx.x % ntn;
  const long long m0 = tile_m * BM;
  const int n0 = tile_n * BN;
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const long long M = (long long)p.B * p.Sg;
  const int K = p.KW * p.Cin, cpj = p.Cin / VBK, nch = p.KW * cpj;

  // this thread's A staging rows: unit u = tid + i NT -> tile row u / 8, float4 column u % 8
  const int c4 = tid & 7;
  long long a_row[AU];  // input row (b S_in + t + off0) of tap 0 (0 for grid rows past M, whose a_t keeps every tap out of range)
  int a_t[AU];          // t + off0
#pragma unroll
  for (int i = 0; i < AU; ++i) {
    const long long m = m0 + (tid >> 3) + i * (NT / 8);
    if (m < M) {
      const long long b = m / p.Sg;
      const int t = (int)(m - b * p.Sg);
      a_t[i] = t + p.off0;
      a_row[i] = b * p.S_in + t + p.off0;
    } else {
      a_t[i] = -(1 << 30);
      a_row[i] = 0;
    }
  }
  v4f ra[AU], rb[BU];
  auto load = [&](int ch) {
    const int j = ch / cpj, cc = ch - j * cpj;
    const int sh = j * p.dil;
#pragma unroll
    for (int i = 0; i < AU; ++i) {
      const int src = a_t[i] + sh;
      v4f v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)src < (unsigned)p.S_in) v = *reinterpret_cast<const v4f*>(p.X + (size_t)(a_row[i] + sh) * p.Cin + cc * VBK + c4 * 4);
      if (p.in_act) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = lrelu(v[e], p.in_slope);
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < BU; ++i) {
      const int n = n0 + (tid >> 3) + i * (NT / 8);
      rb[i] = n < p.N ? *reinterpret_cast<const v4f*>(p.W + (size_t)n * K + (size_t)ch * VBK + c4 * 4) : v4f{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < AU; ++i) *reinterpret_cast<v4f*>(&As[((tid >> 3) + i * (NT / 8)) * VLDK + c4 * 4]) = ra[i];
#pragma unroll
    for (int i = 0; i < BU; ++i) *reinterpret_cast<v4f*>(&Bs[((tid >> 3) + i * (NT / 8)) * VLDK + c4 * 4]) = rb[i];
  };

  v16f tot[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) tot[mi][ni][r] = 0.f;

  const int frow = lane & 31, fh = lane >> 5;
  load(0);
  for (int ch = 0; ch < nch; ++ch) {
    stash();
    __syncthreads();
    if (ch + 1 < nch) load(ch + 1);  // in flight while the MFMAs run
    v16f acc[TM][TN];
#pragma unroll
    for (int g = 0; g < VBK / 8; ++g) {
      v4f a[TM], b[TN];
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) a[mi] = *reinterpret_cast<const v4f*>(&As[(wm0 + mi * 32 + frow) * VLDK + 8 * g + 4 * fh]);
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) b[ni] = *reinterpret_cast<const v4f*>(&Bs[(wn0 + ni * 32 + frow) * VLDK + 8 * g + 4 * fh]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][e], b[ni][e], (g == 0 && e == 0) ? v16f{} : acc[mi][ni], 0, 0, 0);
    }
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) tot[mi][ni] += acc[mi][ni];
    __syncthreads();
  }

  // C/D layout of the 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int ni = 0; ni < TN; ++ni) {
    const int n = n0 + wn0 + ni * 32 + (lane & 31);
    if (n >= p.N) continue;
    const float bv = p.bias[n % p.Cb];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long m = m0 + wm0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= M) continue;
        const long long b = m / p.Sg;
        const long long o = (m - b * p.Sg) * p.N + n - p.out_shift;
        if (o < 0 || o >= p.out_ustride) continue;
        const size_t at = (size_t)(b * p.out_ustride + o);
        float v = tot[mi][ni][r] + bv;
        if (p.out_act) v = lrelu(v, p.out_slope);
        if (p.R) v = v + p.R[at];
        if (p.mrf == 1) v = p.Y[at] + v;
        else if (p.mrf == 2) v = (p.Y[at] + v) / p.mrf_div;
        p.Y[at] = v;
      }
    }
  }
}

// conv_post: wav[b, t] = tanh(bias + sum_j sum_c lrelu(x[b, t + j - P, c], slope) w[j, c]), one sample per thread; the block's
// input window (256 + KW - 1 rows x C channels) is staged once in LDS with a row stride of C + 1 floats (conflict-free column reads).
static constexpr int POST_T = 256;
__global__ __launch_bounds__(POST_T) void k_voc_post(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ wav, int S, int C, int KW, float slope) {
  extern __shared__ float sm[];
  const int P = (KW - 1) / 2, R = POST_T + KW - 1, LD = C + 1;
  float* win = sm;
  float* ws = sm + R * LD;
  const int tiles = (S + POST_T - 1) / POST_T;
  const int b = blockIdx.x / tiles, s0 = (blockIdx.x % tiles) * POST_T;
  const int tid = threadIdx.x, c4n = C / 4;
  for (int u = tid; u < R * c4n; u += POST_T) {
    const int row = u / c4n, c4 = u % c4n, t = s0 - P + row;
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0 && t < S) v = *reinterpret_cast<const v4f*>(x + ((size_t)b * S + t) * C + c4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) win[row * LD + c4 * 4 + e] = lrelu(v[e], slope);
  }
  for (int u = tid; u < KW * C; u += POST_T) ws[u] = w[u];
  __syncthreads();
  const int t = s0 + tid;
  if (t >= S) return;
  float tot = 0.f;
  for (int j = 0; j < KW; ++j) {  // one partial sum per tap, added into the total (short sums, like the GEMM's chunks)
    const float* xr = win + (tid + j) * LD;
    const float* wr = ws + j * C;
    float part = 0.f;
    for (int c = 0; c < C; ++c) part = fmaf(xr[c], wr[c], part);
    tot += part;
  }
  wav[(size_t)b * S + t] = tanhf(tot + bias[0]);
}

// [B, C, T] (channel-major mel) -> [B, T, C] through a 32 x 32 LDS tile
__global__ __launch_bounds__(256) void k_voc_transpose(const float* __restrict__ src, float* __restrict__ dst, int C, int T) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < T) ? src[((size_t)b * C + c) * T + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (c < C && t < T) dst[((size_t)b * T + t) * C + c] = tile[tx][i];
  }
}

template <int BM, int BN, int WGM, int WGN>
static hipError_t voc_launch(const VocGemm& p, hipStream_t st) {
  const long long M = (long long)p.B * p.Sg;
  const long long blocks = ((M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_voc_gemm<BM, BN, WGM, WGN>), dim3((unsigned)blocks), dim3(64 * WGM * WGN), 0, st, p);
  return hipGetLastError();
}

bool voc_gemm_ok(const VocGemm& p) {
  return p.X && p.W && p.bias && p.Y && p.B > 0 && p.S_in > 0 && p.Sg > 0 && p.Cin > 0 && p.Cin % VBK == 0 && p.KW > 0 && p.dil > 0 &&
         p.N > 0 && p.N % 32 == 0 && p.Cb > 0 && p.N % p.Cb == 0 && (p.mrf == 0 || p.mrf == 1 || p.mrf == 2) &&
         ((uintptr_t)p.X & 15) == 0 && ((uintptr_t)p.W & 15) == 0;
}

hipError_t launch_voc_gemm(const VocGemm& p, hipStream_t st) {
  if (!voc_gemm_ok(p)) return hipErrorInvalidValue;
  if (p.N % 128 == 0) return voc_launch<128, 128, 2, 2>(p, st);
  if (p.N % 64 == 0) return voc_launch<128, 64, 4, 1>(p, st);
  return voc_launch<128, 32, 4, 1>(p, st);
}

size_t voc_post_lds_bytes(int C, int KW) { return ((size_t)(POST_T + KW - 1) * (C + 1) + (size_t)KW * C) * sizeof(float); }

hipError_t launch_voc_post(const float* x, const float* w, const float* bias, float* wav, int B, int S, int C, int KW, float slope, hipStream_t st) {
  if (B <= 0 || S <= 0) return hipSuccess;
  if (C % 4 || ((uintptr_t)x & 15) || !(KW & 1) || voc_post_lds_bytes(C, KW) > 65536) return hipErrorInvalidValue;
  const long long blocks = (long long)B * ((S + POST_T - 1) / POST_T);
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_voc_post, dim3((unsigned)blocks), dim3(POST_T), voc_post_lds_bytes(C, KW), st, x, w, bias, wav, S, C, KW, slope);
  return hipGetLastError();
}

hipError_t launch_voc_transpose(const float* src, float* dst, int B, int C, int T, hipStream_t st) {
  if (B <= 0 || T <= 0 || C <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_voc_transpose, dim3((T + 31) / 32, (C + 31) / 32, B), dim3(256), 0, st, src, dst, C, T);
  return hipGetLastError();
}

}  // namespace ns
