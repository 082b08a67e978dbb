// OPT-IN "bf16" matmul mode of the HiFi-GAN generator (ns_voc_set_matmul(v, 1); never the default): the implicit GEMM of
// k_voc_gemm (vocoder.hip) — every ResBlock1 convs1 / convs2 and every polyphase ConvTranspose1d upsampler — on the bf16 matrix
// cores (v_mfma_f32_32x32x16_bf16, 16x the fp32 MFMA rate).  Same forms, same launch record (VocGemm), same epilogues.
//
// Numerics:
//   * A operand: the input leaky ReLU is computed in fp32 exactly as in k_voc_gemm, then rounded to bf16 with round to nearest
//     even by the plain cast (v_cvt_pk_bf16_f32: a NaN stays a NaN).  Zero padding stays zero.
//   * B operand: the folded fp32 weights rounded to bf16 (RNE) once, at ns_voc_finalize_weights, into a bf16 plane of the arena
//     (VocGemm::Wbf) in the same packed layouts as the fp32 image ([N][KW][Cin], the polyphase [u Cout][2 Cin]).
//   * Products accumulate in fp32 (bf16 x bf16 products are exact in fp32).  Bias, the c1 output leaky ReLU, the residual, the
//     multi-receptive-field sum / mean and every stored activation stay fp32.
//   * Every output element is ONE fp32 accumulator chain over the 16-wide k steps in one fixed order (tap major, 32-channel
//     block, then the two 16-wide halves), whatever tile the launch picks: replicas of an utterance in a batch give the same
//     bits, and a layer's bits do not depend on B.  No K split, no fp32 fallback at any size.
//
// Staging is register-based like k_voc_gemm: each thread loads 8 consecutive fp32 activations (two float4) of one row of the
// next 32-channel slice while the MFMAs run on this one, then applies the leaky ReLU, converts to bf16 and writes 16 B to LDS;
// the weights come as 16-B bf16 pieces.  Two LDS buffers, one barrier per slice.  LDS rows are 40 bf16 (80 B): the fragment
// reads (ds_read_b128, lane (row = lane & 31, h = lane >> 5) of k step s holds k = 16 s + 8 h + [0, 8)) are conflict-free.
#include "kernels.h"

namespace ns {

typedef float vb_f4 __attribute__((ext_vector_type(4)));
typedef float vb_f8 __attribute__((ext_vector_type(8)));
typedef float vb_f16 __attribute__((ext_vector_type(16)));
typedef unsigned vb_u4 __attribute__((ext_vector_type(4)));
typedef __bf16 vb_bf8 __attribute__((ext_vector_type(8)));

static constexpr int QBK = 32;       // k values per staged slice (every channel count of the generator is a multiple of 32)
static constexpr int QLD = QBK + 8;  // LDS row stride in bf16 (80 B)

static __device__ __forceinline__ float lrelu_b(float v, float s) { return v > 0.f ? v : v * s; }

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN) void k_voc_gemm_bf16(VocGemm p) {
  constexpr int NT = 64 * WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
  constexpr int AUN = BM * QBK / 8, BUN = BN * QBK / 8;                   // 8-element staging units per slice
  constexpr int AU = AUN / NT, BU = BUN >= NT ? BUN / NT : 1;            // per thread
  static_assert(TM >= 1 && TN >= 1 && WM % 32 == 0 && WN % 32 == 0, "wave tile");
  static_assert(AU >= 1 && AU * NT == AUN && (BUN < NT || BU * NT == BUN), "staging units");
  __shared__ __attribute__((aligned(16))) unsigned short As[2][BM * QLD];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[2][BN * QLD];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ntn = (p.N + BN - 1) / BN;
  const long long tile_m = blockIdx.x / ntn;
  const int tile_n = blockIdx.x % ntn;
  const long long m0 = tile_m * BM;
  const int n0 = tile_n * BN;
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const long long M = (long long)p.B * p.Sg;
  const int K = p.KW * p.Cin, cpj = p.Cin / QBK, nch = p.KW * cpj;
  const bool b_loader = BUN >= NT || tid < BUN;

  // unit u = tid + i NT -> tile row u / 4, 8-element slot u % 4
  const int slot = tid & 3;
  long long a_row[AU];  // input row (b S_in + t + off0) of tap 0 (0 for grid rows past M, whose a_t keeps every tap out of range)
  int a_t[AU];          // t + off0
#pragma unroll
  for (int i = 0; i < AU; ++i) {
    const long long m = m0 + (tid >> 2) + i * (NT / 4);
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
  vb_f4 ra[AU][2];
  vb_u4 rb[BU];
  auto load = [&](int ch) {
    const int j = ch / cpj, cc = ch - j * cpj;
    const int sh = j * p.dil;
#pragma unroll
    for (int i = 0; i < AU; ++i) {
      const int src = a_t[i] + sh;
      ra[i][0] = ra[i][1] = vb_f4{0.f, 0.f, 0.f, 0.f};
      if ((unsigned)src < (unsigned)p.S_in) {
        const vb_f4* g = reinterpret_cast<const vb_f4*>(p.X + (size_t)(a_row[i] + sh) * p.Cin + cc * QBK + slot * 8);
        ra[i][0] = g[0];
        ra[i][1] = g[1];
      }
    }
    if (b_loader) {
#pragma unroll
      for (int i = 0; i < BU; ++i) {
        const int n = n0 + (tid >> 2) + i * (NT / 4);
        rb[i] = n < p.N ? *reinterpret_cast<const vb_u4*>(p.Wbf + (size_t)n * K + (size_t)ch * QBK + slot * 8) : vb_u4{0u, 0u, 0u, 0u};
      }
    }
  };
  // lrelu in fp32, then one RNE cast per 8 values, 16 B into LDS
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AU; ++i) {
      vb_f8 x = {ra[i][0][0], ra[i][0][1], ra[i][0][2], ra[i][0][3], ra[i][1][0], ra[i][1][1], ra[i][1][2], ra[i][1][3]};
      if (p.in_act) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = lrelu_b(x[e], p.in_slope);
      }
      const vb_bf8 h = __builtin_convertvector(x, vb_bf8);
      *reinterpret_cast<vb_u4*>(&As[buf][((tid >> 2) + i * (NT / 4)) * QLD + slot * 8]) = __builtin_bit_cast(vb_u4, h);
    }
    if (b_loader) {
#pragma unroll
      for (int i = 0; i < BU; ++i) *reinterpret_cast<vb_u4*>(&Bs[buf][((tid >> 2) + i * (NT / 4)) * QLD + slot * 8]) = rb[i];
    }
  };

  vb_f16 acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int frow = lane & 31, fh = lane >> 5;
  auto compute = [&](int buf) {
#pragma unroll
    for (int s = 0; s < QBK / 16; ++s) {
      vb_bf8 a[TM], b[TN];
#pragma unroll
      for (int mi = 0; mi < TM; ++mi)
        a[mi] = __builtin_bit_cast(vb_bf8, *reinterpret_cast<const vb_u4*>(&As[buf][(wm0 + mi * 32 + frow) * QLD + 16 * s + 8 * fh]));
#pragma unroll
      for (int ni = 0; ni < TN; ++ni)
        b[ni] = __builtin_bit_cast(vb_bf8, *reinterpret_cast<const vb_u4*>(&Bs[buf][(wn0 + ni * 32 + frow) * QLD + 16 * s + 8 * fh]));
#pragma unroll
      for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
  };

  load(0);
  stash(0);
  __syncthreads();
  for (int ch = 0; ch < nch; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < nch) load(ch + 1);  // in flight while the MFMAs run
    compute(buf);
    if (ch + 1 < nch) stash(buf ^ 1);  // the other buffer was last read before the previous barrier
    __syncthreads();
  }

  // C/D layout of the 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); the arithmetic of k_voc_gemm's
  // epilogue.  The (utterance, position) of a row comes from ONE division per 32-row block and lane half, stepped forward for
  // its 16 rows: a 64-bit division per element costs more VALU time than a short contraction's MFMAs.
  long long mf[TM], bfst[TM];  // first row of this lane's 32-row block mi (r = 0) and its utterance
  int tfst[TM];                // its position in the utterance
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
    mf[mi] = m0 + wm0 + mi * 32 + 4 * (lane >> 5);
    bfst[mi] = mf[mi] / p.Sg;
    tfst[mi] = (int)(mf[mi] - bfst[mi] * p.Sg);
  }
#pragma unroll
  for (int ni = 0; ni < TN; ++ni) {
    const int n = n0 + wn0 + ni * 32 + (lane & 31);
    if (n >= p.N) continue;
    const float bv = p.bias[n % p.Cb];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      long long b = bfst[mi];
      int t = tfst[mi], prev = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = (r & 3) + 8 * (r >> 2);
        t += off - prev;
        prev = off;
        while (t >= p.Sg) {  // at most once when Sg >= 28
          t -= p.Sg;
          ++b;
        }
        if (mf[mi] + off >= M) continue;
        const long long o = (long long)t * p.N + n - p.out_shift;
        if (o < 0 || o >= p.out_ustride) continue;
        const size_t at = (size_t)(b * p.out_ustride + o);
        float v = acc[mi][ni][r] + bv;
        if (p.out_act) v = lrelu_b(v, p.out_slope);
        if (p.R) v = v + p.R[at];
        if (p.mrf == 1) v = p.Y[at] + v;
        else if (p.mrf == 2) v = (p.Y[at] + v) / p.mrf_div;
        p.Y[at] = v;
      }
    }
  }
}

template <int BM, int BN, int WGM, int WGN>
static hipError_t voc_launch_bf16(const VocGemm& p, hipStream_t st) {
  const long long M = (long long)p.B * p.Sg;
  const long long blocks = ((M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_voc_gemm_bf16<BM, BN, WGM, WGN>), dim3((unsigned)blocks), dim3(64 * WGM * WGN), 0, st, p);
  return hipGetLastError();
}

// The tile by output width: 256 rows tall everywhere (the narrow stages stage fp32 activation rows, so tall tiles keep the
// MFMA work per staged byte up), as wide as N allows up to 256.  Any tile gives the same bits.
hipError_t launch_voc_gemm_bf16(const VocGemm& p, hipStream_t st) {
  if (!voc_gemm_ok(p) || !p.Wbf || ((uintptr_t)p.Wbf & 15)) return hipErrorInvalidValue;
  if (p.N % 256 == 0) return voc_launch_bf16<256, 256, 4, 2>(p, st);
  if (p.N % 128 == 0) return voc_launch_bf16<256, 128, 4, 2>(p, st);
  if (p.N % 64 == 0) return voc_launch_bf16<256, 64, 4, 1>(p, st);
  return voc_launch_bf16<256, 32, 4, 1>(p, st);
}

}  // namespace ns
