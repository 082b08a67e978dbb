// OPT-IN "bf16" matmul mode of the PositionwiseFeedForward training layer (never the default):
//   k_fg_pack_bf16    the live torch-layout fp32 weights -> the bf16 planes k_conv_gemm_bf16 (gemm_bf16.hip) reads through
//                     ConvGemm::Wbf: the forward's [N][KW][Cin] and the data gradient's transposed, tap-flipped [Cin][KW][N]
//   k_fg_wgrad_bf16   the weight gradient of a "same"-padded Conv1d with both operands rounded to bf16 (round to nearest even, the
//                     plain cast: v_cvt_pk_bf16_f32, a NaN stays a NaN) and fp32 accumulation on v_mfma_f32_32x32x16_bf16, split
//                     over row ranges exactly as k_pg_wgrad (predgrad.hip) is; k_pg_wgrad_reduce finishes it unchanged
// No atomics, no host reads; every sum has one order that depends on the shape alone.
#include "kernels.h"

namespace ns {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;

// ------------------------------------------------------------------------------------------------------------------ weight gradient
// Workgroup = 4 waves as 2 x 2 over a 128 (n) x 128 (kk = j*Cin + c) output tile, each wave 2 x 2 MFMA tiles of 32 x 32, as k_pg_wgrad.
// One stage holds FGB_STAGE = 32 rows of m (two 16-deep k steps) of both operands: 16-byte fp32 global loads of dz[m][n0 .. n0+128) and
// X[m + j - pad][c] for the tile's 128 kk (eight consecutive kk share a tap, Cin being a multiple of 32), rounded to bf16 in registers
// and stored as 16-byte chunks into an LDS image of bf16 rows [m][128] (256 bytes a row).  Both MFMA operands want, per lane, eight
// consecutive m of ONE column (A[n = l & 31][k = 8 (l >> 5) + e], B[k][kk = l & 31]): a transposed read, two ds_read_b64_tr_b16 per
// fragment (rows 8h .. 8h+3 and 8h+4 .. 8h+7 of the k step).  The image is the XOR one for plain 256-byte rows,
//   off(row, ch) = 256 row + 16 (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))),    ch = the 16-byte chunk (8 columns) of the row,
// stored and read through the same function: lane 4q + p of a 16-lane group supplies row r0 + q, chunk c0 + (p >> 1), half p & 1 of
// the group's 4 x 16 block.  Every lane address is 8-byte aligned, every transposed read is made with EXEC all ones (the tile is padded
// with zeros, no lane is masked, no wave leaves before the loop ends).  A tap that leaves the utterance's [0, S) rows, a row past the
// range's end and a column past KW*Cin are staged as zeros, never read.  Staging goes through registers: the next stage's global
// loads are issued before this stage's MFMAs and stored behind them; one barrier per stage.  Accumulation in chunks as k_pg_wgrad:
// `acc` takes fl stages from zero, then is added into `tot`.
__device__ __forceinline__ int fgb_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

__global__ __launch_bounds__(256) void k_fg_wgrad_bf16(const float* __restrict__ dz, const float* __restrict__ X, int M, int S, int N, int Cin,
                                                       int KW, int rows, int tiles_c, int fl, float* __restrict__ partial) {
  constexpr int IMG = FGB_STAGE * 256;  // bytes of one operand's stage
  __shared__ __attribute__((aligned(16))) unsigned char As[2 * IMG];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2 * IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, range = blockIdx.y;
  const int n0 = (tile / tiles_c) * PG_TILE_N, c0 = (tile % tiles_c) * PG_TILE_C;
  const int KC = KW * Cin, pad = (KW - 1) / 2;
  const int mbeg = range * rows, mend = min(M, mbeg + rows);
  const int nsteps = (mend - mbeg + FGB_STAGE - 1) / FGB_STAGE;

  // this thread's two staging rows (r0, r0 + 16) and its 16-byte chunk (8 columns) of both operands
  const int r0 = tid >> 4, ch = tid & 15;
  const int kk = c0 + ch * 8;
  const bool kk_ok = kk < KC;
  const int j = kk_ok ? kk / Cin : 0, c = kk_ok ? kk - j * Cin : 0;
  f32x8 ra[2], rb[2];
  auto fetch = [&](int st) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mbeg + st * FGB_STAGE + r0 + 16 * i;
      const f32x8 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      ra[i] = zero; rb[i] = zero;
      if (m < mend) {
        const float* pa = dz + (size_t)m * N + n0 + ch * 8;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(pa), a1 = *reinterpret_cast<const f32x4*>(pa + 4);
        ra[i] = f32x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        const int t = m % S + j - pad;
        if (kk_ok && t >= 0 && t < S) {
          const float* pb = X + (size_t)(m + j - pad) * Cin + c;
          const f32x4 b0 = *reinterpret_cast<const f32x4*>(pb), b1 = *reinterpret_cast<const f32x4*>(pb + 4);
          rb[i] = f32x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
        }
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = buf * IMG + fgb_off(r0 + 16 * i, ch);
      *reinterpret_cast<u32x4*>(&As[o]) = __builtin_bit_cast(u32x4, __builtin_convertvector(ra[i], bf16x8));  // round to nearest even
      *reinterpret_cast<u32x4*>(&Bs[o]) = __builtin_bit_cast(u32x4, __builtin_convertvector(rb[i], bf16x8));
    }
  };

  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[a][b][r] = 0.f; tot[a][b][r] = 0.f; }

  // transposed-read addresses of k step 0 of buffer 0: group g = lane >> 4 takes the columns 16 (g & 1) .. + 15 of a 32-column MFMA
  // tile and the k rows 8 (g >> 1) + 4 s .. + 3 (s = 0, 1: the fragment's elements 4 s .. 4 s + 3)
  const int wn = (wave >> 1) * 64, wc = (wave & 1) * 64;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  int aoff[2][2], boff[2][2];  // [MFMA tile][s], bytes
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int row = 8 * (g >> 1) + 4 * s + q;
      aoff[i][s] = fgb_off(row, (wn + 32 * i + 16 * (g & 1)) / 8 + (p >> 1)) + 8 * (p & 1);
      boff[i][s] = fgb_off(row, (wc + 32 * i + 16 * (g & 1)) / 8 + (p >> 1)) + 8 * (p & 1);
    }
  auto frag = [&](const unsigned char* img, const int (&off)[2]) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(img + off[0]));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(img + off[1]));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  if (nsteps > 0) { fetch(0); stash(0); }
  __syncthreads();
  int due = fl;
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    if (st + 1 < nsteps) fetch(st + 1);
#pragma unroll
    for (int t = 0; t < FGB_STAGE / 16; ++t) {
      // (rows 16 t + r keep (r & 3) and ((r >> 2) & 3) of r: the XOR term of k step t is that of k step 0)
      const unsigned char* as = As + buf * IMG + t * 16 * 256;
      const unsigned char* bs = Bs + buf * IMG + t * 16 * 256;
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) { a[i] = frag(as, aoff[i]); b[i] = frag(bs, boff[i]); }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    if (fl > 0 && --due == 0 && st + 1 < nsteps) {
      due = fl;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          tot[mi][ni] += acc[mi][ni];
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        }
    }
    if (st + 1 < nsteps) stash(buf ^ 1);
    __syncthreads();
  }
  // C/D layout of the 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int l31 = lane & 31, lh = lane >> 5;
  float* out = partial + (size_t)range * N * KC;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int col = c0 + wc + 32 * ni + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (n < N && col < KC) out[(size_t)n * KC + col] = tot[mi][ni][r] + acc[mi][ni][r];
      }
    }
}

// pg_plan_wgrad's rule at FGB_STAGE rows per stage; Cin a multiple of 32 (eight consecutive kk share a tap, 32-byte fp32 loads)
bool fg_plan_wgrad_bf16(int M, int N, int Cin, int KW, PgWgradPlan* out) {
  if (M <= 0 || N <= 0 || N % PG_TILE_N != 0 || Cin <= 0 || Cin % 32 != 0 || KW <= 0 || KW % 2 == 0) return false;
  const long long KC = (long long)KW * Cin;
  if (KC >= (1 << 20) || (long long)M * N >= (1ll << 31) || (long long)M * Cin >= (1ll << 31)) return false;
  const int tiles_c = (int)((KC + PG_TILE_C - 1) / PG_TILE_C);
  const int tiles = (N / PG_TILE_N) * tiles_c;
  // ranges: enough for about one workgroup per CU, never shorter than two stages of rows
  long long want = (PG_WG_TARGET + tiles - 1) / tiles;
  const long long most = ((long long)M + 2 * FGB_STAGE - 1) / (2 * FGB_STAGE);
  if (want > most) want = most;
  if (want < 1) want = 1;
  long long rows = ((long long)M + want - 1) / want;
  rows = (rows + FGB_STAGE - 1) / FGB_STAGE * FGB_STAGE;
  const long long ranges = ((long long)M + rows - 1) / rows;
  const long long floats = ranges * N * KC;
  if (floats >= (1ll << 31) || ranges > 65535) return false;
  out->tile_n = PG_TILE_N; out->tile_c = PG_TILE_C; out->rows = (int)rows; out->ranges = (int)ranges; out->tiles = tiles;
  out->chunk = conv_gemm_acc_chunk() / FGB_STAGE * FGB_STAGE;
  out->ws_floats = floats;
  return true;
}

hipError_t launch_fg_wgrad_bf16(const float* dz, const float* X, int M, int S, int N, int Cin, int KW, const PgWgradPlan& pl, float* partial,
                                float* dW, hipStream_t st) {
  if (S <= 0 || M % S != 0 || Cin % 32 != 0 || N % PG_TILE_N != 0 || pl.rows % FGB_STAGE != 0) return hipErrorInvalidValue;
  const int tiles_c = pl.tiles / (N / PG_TILE_N);
  hipLaunchKernelGGL(k_fg_wgrad_bf16, dim3(pl.tiles, pl.ranges), dim3(256), 0, st, dz, X, M, S, N, Cin, KW, pl.rows, tiles_c, pl.chunk / FGB_STAGE,
                     partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long n = (long long)N * Cin;
  hipLaunchKernelGGL(k_pg_wgrad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partial, pl.ranges, N, Cin, KW, dW);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ weight pack
// One thread per pair of neighbouring plane elements, stored as one 4-byte word: wp[n][j][c], wp[n][j][c + 1] and wt[c'][j][n'],
// wt[c'][j][n' + 1] = bf(w[n'][c'][KW - 1 - j]), w[n' + 1][c'][KW - 1 - j] (N and Cin are even).  Both planes have N KW Cin / 2 pairs.
__global__ __launch_bounds__(256) void k_fg_pack_bf16(FgPackBf a, FgPackBf b) {
  const FgPackBf p = blockIdx.y ? b : a;
  if (!p.w) return;
  const int hc = p.Cin / 2, hn = p.N / 2;
  const long long pairs = (long long)p.N * p.KW * hc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (long long)gridDim.x * 256) {
    if (p.wp) {
      const int c = 2 * (int)(i % hc);
      const long long nj = i / hc;
      const int j = (int)(nj % p.KW), n = (int)(nj / p.KW);
      const float* s = p.w + ((size_t)n * p.Cin + c) * p.KW + j;
      const f32x2 v = {s[0], s[p.KW]};
      reinterpret_cast<unsigned*>(p.wp)[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    }
    if (p.wt) {
      const int n = 2 * (int)(i % hn);
      const long long cj = i / hn;
      const int j = (int)(cj % p.KW), c = (int)(cj / p.KW);
      const float* s = p.w + ((size_t)n * p.Cin + c) * p.KW + (p.KW - 1 - j);
      const f32x2 v = {s[0], s[(size_t)p.Cin * p.KW]};
      reinterpret_cast<unsigned*>(p.wt)[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    }
  }
}

hipError_t launch_fg_pack_bf16(const FgPackBf& a, const FgPackBf& b, hipStream_t st) {
  long long n = 0;
  for (const FgPackBf* p : {&a, &b}) {
    if (!p->w) continue;
    if (p->N <= 0 || p->Cin <= 0 || p->KW <= 0 || p->N % 2 != 0 || p->Cin % 2 != 0) return hipErrorInvalidValue;
    const long long pairs = (long long)p->N * p->KW * (p->Cin / 2);
    if (pairs >= (1ll << 31)) return hipErrorInvalidValue;
    if (pairs > n) n = pairs;
  }
  if (n == 0) return hipSuccess;
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_fg_pack_bf16, dim3((unsigned)blocks, 2), dim3(256), 0, st, a, b);
  return hipGetLastError();
}

}  // namespace ns
