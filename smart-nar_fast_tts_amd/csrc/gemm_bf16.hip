// OPT-IN precision mode "bf16" (ns_config.matmul_bf16x3 == 2; never the default): the Conv1D-as-GEMM contraction of
// gemm_conv.hip with both operands rounded to bf16 (round to nearest even, the plain cast: v_cvt_pk_bf16_f32, a NaN stays a
// NaN) and the products accumulated in fp32 on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, 16x the fp32 MFMA rate).
// Used for every contraction downstream of the last discrete decision (decoder, mel_linear, PostNet: api.hip); bias,
// activation, residual and the LayerNorm row epilogue stay fp32.
//
// Weights: ONE bf16 plane per covered weight, rounded once at load (api.hip), laid out [N][KW][Cinp] with the channel axis
// padded with zeros to Cinp = Cin rounded up to 32 (the PostNet's 80-channel input).  Activations stay fp32 in HBM, are
// staged by LDS-DMA exactly like gemm_conv.hip (same zero padding / halo rule, packed rows through RowMap, same XOR swizzle;
// channels >= Cin of a padded chunk read as zero) and are rounded to bf16 in registers after the fragment read.
//
// Every output element is one fp32 sum over the 16-wide k steps in the same order (channel block major, tap minor, the same
// MFMA shape) whatever the tile: all tiles give the same bits per row, so a plan may pick any of them and replicas of an
// utterance stay bit-identical.  No K split, no fp32 fallback: a launch of one row gets the precision of a launch of 16 000.
#include <cstring>

#include "rowln.h"

namespace ns {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_bf_t;

[[maybe_unused]] constexpr int OOR_BF = (int)0x80000000;

template <int BM, int BN, int WGM, int WGN, bool ROWEPI = false>
__global__ __launch_bounds__(64 * WGM * WGN) void k_conv_gemm_bf16(ConvGemm p, int ntn) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BK = 32, NW = WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN, TN = WN / 32;
  static_assert(WM == 32 && TN >= 1 && BM % 8 == 0 && BN % 16 == 0, "wave strip is 32 rows x TN 32-column tiles");
  constexpr int TOTA = BM / 8;   // DMA instructions per A chunk (8 rows of 128 B each)
  constexpr int TOTB = BN / 16;  // per weight chunk (16 rows of 64 B each)
  static_assert(TOTA % NW == 0 && TOTB % NW == 0, "DMA work divides evenly over the waves (no branch around a DMA)");
  static_assert(!ROWEPI || (BM == 64 && BN % 256 == 0 && BM % NW == 0), "row epilogue: 64-row full-row tile");
  constexpr int IA = TOTA / NW, IB = TOTB / NW;
  // the row epilogue parks the BM x BN fp32 tile, 32 rows per weight buffer
  constexpr int BSZ = ROWEPI ? 32 * BN * 2 : BN * BK;

  __shared__ __attribute__((aligned(16))) float As0[BM * BK];
  __shared__ __attribute__((aligned(16))) float As1[BM * BK];
  __shared__ __attribute__((aligned(16))) unsigned short Bs0[BSZ];
  __shared__ __attribute__((aligned(16))) unsigned short Bs1[BSZ];

  // XCD-aware bijective remap, as in gemm_conv.hip: an XCD keeps a contiguous group of activation rows in its L2
  const int nblk = gridDim.x, bid = blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7;
  int pos = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int ntm = nblk / ntn, mq = ntm >> 3, mr = ntm & 7;
  int tile_m = 0, tile_n = 0, mstart = 0;
  for (int x = 0; x < 8; ++x) {
    const int gm = mq + (x < mr ? 1 : 0), gsz = gm * ntn;
    if (pos < gsz) {
      tile_n = pos / gm;
      tile_m = mstart + pos % gm;
      break;
    }
    pos -= gsz;
    mstart += gm;
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const int Cinp = (p.Cin + BK - 1) / BK * BK, cpj = Cinp / BK, nch = p.KW * cpj;
  const int Kt = p.KW * Cinp;  // weight row length (padded channels)

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.X + ((ptrdiff_t)m0 - p.pad) * p.ldx), (short)0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.Wbf + (size_t)n0 * Kt), (short)0, 0x7FFFFFFF, 0x00020000);

  // A: 8 lanes per 128-B row, source-side swizzle f(r) = (r>>1)&7 on the 16-B slot (gemm_conv.hip, BK = 32); per entry the
  // byte offset without the tap shift, the range of taps that stay inside the utterance's window, and the first channel of
  // the 16-B source slot (a slot at or past Cin, in the last chunk of a padded channel axis, reads zero)
  int a_base[IA], a_ch[IA];
  unsigned a_jlo[IA], a_jn[IA];
#pragma unroll
  for (int i = 0; i < IA; ++i) {
    const int r = (wid * IA + i) * 8 + (lane >> 3), m = m0 + r;
    int t = -1, sw = p.S;  // position in the utterance and its window (packed rows: kernels.h RowMap)
    if (m < p.M) {
      if (p.rm.row_t) { t = p.rm.row_t[m]; sw = p.rm.row_w[m]; }
      else t = m % p.S;
    }
    const int slot = (lane & 7) ^ ((r >> 1) & 7);
    a_base[i] = (r * p.ldx + slot * 4) * 4;
    a_ch[i] = slot * 4;
    const int jlo = max(0, p.pad - t), jhi = min(p.KW, sw + p.pad - t);
    a_jlo[i] = (unsigned)jlo;
    a_jn[i] = (t >= 0 && jhi > jlo) ? (unsigned)(jhi - jlo) : 0u;
  }
  // B: 4 lanes per 64-B row (32 bf16), swizzle f(r) = (r>>2)&3 on the 16-B slot (the 64-B-row rule of gemm_conv.hip)
  int vb[IB];
#pragma unroll
  for (int i = 0; i < IB; ++i) {
    const int r = (wid * IB + i) * 16 + (lane >> 2);
    vb[i] = (n0 + r < p.N) ? (r * Kt + ((lane & 3) ^ ((r >> 2) & 3)) * 8) * 2 : OOR_BF;
  }
  auto dma_chunk = [&](float* As, unsigned short* Bs, int ch) {
    const int cc = ch / p.KW, j = ch - cc * p.KW;  // channel-block major, tap minor (L2 reuse of the activation lines)
    const int soA = (cc * BK + j * p.ldx) * 4;
    const int soB = (j * Cinp + cc * BK) * 2;
    const int chl = p.Cin - cc * BK;  // channels of this block that exist
#pragma unroll
    for (int i = 0; i < IA; ++i) {
      const int va = ((unsigned)j - a_jlo[i] < a_jn[i] && a_ch[i] < chl) ? a_base[i] : OOR_BF;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr_bf_t)&As[(wid * IA + i) * 8 * BK], 16, va, soA, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < IB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr_bf_t)&Bs[(wid * IB + i) * 16 * BK], 16, vb[i], soB, 0, 0);
  };

  f32x16 acc[TN];
#pragma unroll
  for (int ni = 0; ni < TN; ++ni)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;

  // fragment offsets: lane (row = lane&31, h = lane>>5) of K-step t holds k = 16t + 8h + [0,8)
  const int frow = lane & 31, fh = lane >> 5;
  int aoff[2][2], boff[2];  // floats / ushorts
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int ar = wm0 + frow;
#pragma unroll
    for (int s = 0; s < 2; ++s) aoff[t][s] = ar * BK + (((4 * t + 2 * fh + s) ^ ((ar >> 1) & 7)) * 4);
    boff[t] = frow * BK + (((2 * t + fh) ^ ((frow >> 2) & 3)) * 8);  // + (wn0 + ni*32) * BK: those rows keep (row>>2)&3 of frow
  }

  auto compute = [&](const float* Ac, const unsigned short* Bc) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(Ac + aoff[t][0]);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(Ac + aoff[t][1]);
      const f32x8 x = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      const bf16x8 A = __builtin_convertvector(x, bf16x8);  // round to nearest even (v_cvt_pk_bf16_f32)
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const unsigned short* bp = Bc + (wn0 + ni * 32) * BK + boff[t];
        const bf16x8 B = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(bp));
        acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, B, acc[ni], 0, 0, 0);
      }
    }
  };

  dma_chunk(As0, Bs0, 0);
  __syncthreads();
  auto step = [&](int ch, const float* Ac, const unsigned short* Bc, float* An, unsigned short* Bn) {
    if (ch + 1 < nch) dma_chunk(An, Bn, ch + 1);
    compute(Ac, Bc);
    __syncthreads();
  };
  for (int ch = 0; ch < nch; ch += 2) {
    step(ch, As0, Bs0, As1, Bs1);
    if (ch + 1 < nch) step(ch + 1, As1, Bs1, As0, Bs0);
  }

  // epilogue: C/D layout col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5); bias / act / residual as gemm_conv.hip
  const int ecol = lane & 31, erow = (lane >> 5) * 4;
  if constexpr (ROWEPI) {
    // full-row tile (BN == N): the row epilogue of gemm_conv.hip (rowln.h) — LayerNorm (+ mask) of act(acc + bias) + residual,
    // one row per wave64; rows [0,32) of the tile are parked in Bs0, [32,64) in Bs1
    auto trow = [&](int ml) -> float* { return reinterpret_cast<float*>(ml < 32 ? Bs0 : Bs1) + (ml & 31) * BN; };
    constexpr int NV = BN / 256, RPW = BM / NW;
    f32x4 rv[RPW][NV];
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      const int m = m0 + wid * RPW + rr;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        rv[rr][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.resid && m < p.M) rv[rr][i] = *reinterpret_cast<const f32x4*>(p.resid + (size_t)m * p.ldr + lane * 4 + i * 256);
      }
    }
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      const int nl = wn0 + ni * 32 + ecol;
      const float bv = p.bias ? p.bias[n0 + nl] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = wm0 + (r & 3) + 8 * (r >> 2) + erow;
        float v = acc[ni][r] + bv;
        if (p.act == ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (p.act == ACT_TANH) v = tanhf(v);
        trow(ml)[nl] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      const int ml = wid * RPW + rr, m = m0 + ml;
      if (m < p.M) {
        int b, t;
        if (p.e.row_b) { b = p.e.row_b[m]; t = p.e.row_t[m]; }
        else { b = m / p.S; t = m - b * p.S; }
        const bool masked = p.e.lens && (long long)t >= p.e.lens[b];
        if (masked) {
#pragma unroll
          for (int i = 0; i < NV; ++i) *reinterpret_cast<f32x4*>(p.Y + (size_t)m * p.ldy + lane * 4 + i * 256) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
          f32x4 v[NV];
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            v[i] = *reinterpret_cast<const f32x4*>(trow(ml) + lane * 4 + i * 256);
            if (p.resid) v[i] += rv[rr][i];
          }
          float mean, rstd;
          ln_moments<NV>(v, BN, lane, mean, rstd);
          ln_store<NV>(v, BN, lane, mean, rstd, p.e.ln_g, p.e.ln_b, p.Y + (size_t)m * p.ldy);
        }
      }
    }
  } else {
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      const int n = n0 + wn0 + ni * 32 + ecol;
      if (n >= p.N) continue;
      const float bv = p.bias ? p.bias[n] : 0.f;
      float rs[16];  // residual values first, all loads in flight together (see gemm_conv.hip)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + (r & 3) + 8 * (r >> 2) + erow;
        rs[r] = (p.resid && m < p.M) ? p.resid[(size_t)m * p.ldr + n] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + (r & 3) + 8 * (r >> 2) + erow;
        if (m >= p.M) continue;
        float v = acc[ni][r] + bv;
        if (p.act == ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (p.act == ACT_TANH) v = tanhf(v);
        if (p.resid) v += rs[r];
        p.Y[(size_t)m * p.ldy + n] = v;
      }
    }
  }
#endif
}

static int cin_padded(int Cin) { return (Cin + 31) / 32 * 32; }

bool conv_gemm_bf16_ok(int M, int N, int Cin, int KW, int epi) {
  if (M <= 0 || Cin % 16 != 0 || N % 16 != 0 || 2ll * N * KW * cin_padded(Cin) >= (1ll << 31)) return false;
  // LayerNorm epilogue: the 64 x 256 full-row tile, taken once the launch has about a workgroup per CU (below that the caller
  // runs the plain GEMM and k_layernorm)
  if (epi == EPI_LN) return N == 256 && (M + 63) / 64 >= 200;
  return epi == EPI_NONE;
}

// the tile of a plain launch: the tallest / widest one that still gives about a workgroup per CU (256-wide tiles only for
// N > 128: the 80-column mel_linear / last PostNet layer would waste two thirds of them).  Any choice gives the same bits.
void conv_gemm_bf16_plan(int M, int N, int* bm, int* bn) {
  const long long ntn256 = (N + 255) / 256, ntn128 = (N + 127) / 128;
  if (N > 128 && (long long)((M + 255) / 256) * ntn256 >= 240) { *bm = 256; *bn = 256; return; }
  if (N > 128 && (long long)((M + 127) / 128) * ntn256 >= 200) { *bm = 128; *bn = 256; return; }
  if ((long long)((M + 63) / 64) * ntn128 >= 200) { *bm = 64; *bn = 128; return; }
  *bm = 64; *bn = 64;
}

hipError_t launch_conv_gemm_bf16(const ConvGemm& p, hipStream_t st) {
  if (p.M <= 0 || p.N <= 0) return hipSuccess;
  if (!p.Wbf || !conv_gemm_bf16_ok(p.M, p.N, p.Cin, p.KW, p.epi) || (p.ldx & 3) || p.m_base != 0) return hipErrorInvalidValue;
  if ((long long)(256 + p.KW) * p.ldx >= (1ll << 29)) return hipErrorInvalidValue;
  if (p.epi == EPI_LN) {
    if ((p.ldy & 3) || (p.resid && (p.ldr & 3))) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_conv_gemm_bf16<64, 256, 2, 4, true>), dim3((p.M + 63) / 64), dim3(512), 0, st, p, 1);
    return hipGetLastError();
  }
  int bm, bn;
  conv_gemm_bf16_plan(p.M, p.N, &bm, &bn);
  const int ntn = (p.N + bn - 1) / bn, ntm = (p.M + bm - 1) / bm;
  const dim3 grid(ntm * ntn);
  if (bm == 256) hipLaunchKernelGGL((k_conv_gemm_bf16<256, 256, 8, 2>), grid, dim3(1024), 0, st, p, ntn);
  else if (bm == 128) hipLaunchKernelGGL((k_conv_gemm_bf16<128, 256, 4, 4>), grid, dim3(1024), 0, st, p, ntn);
  else if (bn == 128) hipLaunchKernelGGL((k_conv_gemm_bf16<64, 128, 2, 2>), grid, dim3(256), 0, st, p, ntn);
  else hipLaunchKernelGGL((k_conv_gemm_bf16<64, 64, 2, 2>), grid, dim3(256), 0, st, p, ntn);
  return hipGetLastError();
}

// host-side: an fp32 weight matrix [N][KW][Cin] (packed, api.hip) -> one bf16 plane [N][KW][Cinp], rounded to nearest even
// like the device's cast, channels [Cin, Cinp) zero
static unsigned short bf16_rne(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);  // NaN stays a (quiet) NaN
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
size_t bf16_plane_elems(int N, int KW, int Cin) { return (size_t)N * KW * cin_padded(Cin); }
void round_weights_bf16(const float* w, int N, int KW, int Cin, unsigned short* dst) {
  const int Cinp = cin_padded(Cin);
  for (size_t r = 0; r < (size_t)N * KW; ++r)
    for (int c = 0; c < Cinp; ++c) dst[r * Cinp + c] = c < Cin ? bf16_rne(w[r * Cin + c]) : (unsigned short)0;
}

}  // namespace ns
