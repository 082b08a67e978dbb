// VariancePredictor training kernels for gfx950 (model/modules.py:233-286):
//   k_pg_wgrad / k_pg_wgrad_reduce   the weight gradient of a "same"-padded Conv1d, a GEMM contracted over the M activation rows on
//                                    the fp32 matrix cores (v_mfma_f32_32x32x2_f32), split over row ranges, summed in a fixed order
//   k_pg_pack                        the live torch-layout weights -> the forward's [n][j*Cin + c] and the data gradient's
//                                    transposed, tap-flipped [c][j*N + n] (both feed launch_conv_gemm, gemm_conv.hip)
//   k_pg_row_forward                 LayerNorm * keep / (1 - p) of a row, and the Linear(F, 1) + masked_fill of the tail
//   k_pg_row_backward                LayerNorm + ReLU backward of a row, per-workgroup column partials in float64
//   k_pg_colsum / k_pg_col_final     column sums of a matrix alone, of 1 to PG_SLOTS column parts per row (a bias gradient here, the
//                                    thirds of dqkv in attngrad_api.hip, dQ and dK | dV in xattngrad_api.hip); the fixed-order sum of
//                                    the partials
// No atomics, no host reads; every sum has one order that depends on the shape alone.  The row kernels' float64 helpers (wave_sum,
// row_stats, keep4, the column-partial flush) are train_rows.h's, shared with attngrad.hip's row kernels.
#include "kernels.h"
#include "train_rows.h"

namespace ns {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------------------------ weight gradient
// Workgroup = 4 waves as 2 x 2 over a 128 (n) x 128 (kk = j*Cin + c) output tile, each wave 2 x 2 MFMA tiles of 32 x 32.  One stage
// holds 16 rows of m of both operands, m-major — dz[m][n0 .. n0+128) and X[m + j - pad][c] for the tile's 128 kk — so lane l of an
// MFMA reads A[n = l & 31][k = l >> 5] and B[k][kk = l & 31] as consecutive floats of one LDS row: conflict-free ds_read_b32 without a
// transpose.  (Row stride 160 floats: the two lane halves, one row apart, land 32 banks apart.)  Staging goes through registers: the
// next stage's 16-byte global loads are issued before this stage's MFMAs and stored behind them; one barrier per stage.
// A tap that leaves the utterance's [0, S) rows is staged as zeros, never read.  Accumulation in chunks as gemm_conv.hip ACC2:
// `acc` takes fl stages from zero, then is added into `tot`.
constexpr int PG_LD = 160;

__global__ __launch_bounds__(256) void k_pg_wgrad(const float* __restrict__ dz, const float* __restrict__ X, int M, int S, int N, int Cin,
                                                  int KW, int rows, int tiles_c, int fl, float* __restrict__ partial, int ldz) {
  __shared__ __attribute__((aligned(16))) float As[2][PG_STEP_ROWS * PG_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][PG_STEP_ROWS * PG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, range = blockIdx.y;
  const int n0 = (tile / tiles_c) * PG_TILE_N, c0 = (tile % tiles_c) * PG_TILE_C;
  const int KC = KW * Cin, pad = (KW - 1) / 2;
  const int mbeg = range * rows, mend = min(M, mbeg + rows);
  const int nsteps = (mend - mbeg + PG_STEP_ROWS - 1) / PG_STEP_ROWS;

  // this thread's two staging rows (r0, r0 + 8) and its 16-byte column group of both operands
  const int r0 = tid >> 5, cg = (tid & 31) * 4;
  const int kk = c0 + cg;
  const bool kk_ok = kk < KC;
  const int j = kk_ok ? kk / Cin : 0, c = kk_ok ? kk - j * Cin : 0;
  const bool n_ok = n0 + cg < N;
  f32x4 ra[2], rb[2];
  auto fetch = [&](int st) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mbeg + st * PG_STEP_ROWS + r0 + 8 * i;
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      ra[i] = zero; rb[i] = zero;
      if (m < mend) {
        if (n_ok) ra[i] = *reinterpret_cast<const f32x4*>(dz + (size_t)m * ldz + n0 + cg);
        const int t = m % S + j - pad;
        if (kk_ok && t >= 0 && t < S) rb[i] = *reinterpret_cast<const f32x4*>(X + (size_t)(m + j - pad) * Cin + c);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<f32x4*>(&As[buf][(r0 + 8 * i) * PG_LD + cg]) = ra[i];
      *reinterpret_cast<f32x4*>(&Bs[buf][(r0 + 8 * i) * PG_LD + cg]) = rb[i];
    }
  };

  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[a][b][r] = 0.f; tot[a][b][r] = 0.f; }

  const int wn = (wave >> 1) * 64, wc = (wave & 1) * 64;
  const int l31 = lane & 31, lh = lane >> 5;
  if (nsteps > 0) { fetch(0); stash(0); }
  __syncthreads();
  int due = fl;
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    if (st + 1 < nsteps) fetch(st + 1);
    const float* as = &As[buf][wn + l31];
    const float* bs = &Bs[buf][wc + l31];
#pragma unroll
    for (int kp = 0; kp < PG_STEP_ROWS / 2; ++kp) {
      const int k = 2 * kp + lh;
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) { a[i] = as[k * PG_LD + 32 * i]; b[i] = bs[k * PG_LD + 32 * i]; }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
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

// dW[n][c][j] = sum over ranges, ascending, in float64, rounded once; one thread per (n, c), its KW taps stored side by side
__global__ __launch_bounds__(256) void k_pg_wgrad_reduce(const float* __restrict__ partial, int ranges, int N, int Cin, int KW,
                                                         float* __restrict__ dW) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * Cin) return;
  const int n = (int)(idx / Cin), c = (int)(idx - (long long)n * Cin);
  const size_t KC = (size_t)KW * Cin, plane = (size_t)N * KC;
  for (int j = 0; j < KW; ++j) {
    const float* p = partial + (size_t)n * KC + (size_t)j * Cin + c;
    double s = 0.0;
    for (int r = 0; r < ranges; ++r) s += (double)p[(size_t)r * plane];
    dW[(size_t)idx * KW + j] = (float)s;
  }
}

bool pg_plan_wgrad(int M, int N, int Cin, int KW, PgWgradPlan* out) {
  if (M <= 0 || N <= 0 || N % PG_TILE_N != 0 || Cin <= 0 || Cin % 4 != 0 || KW <= 0 || KW % 2 == 0) return false;
  const long long KC = (long long)KW * Cin;
  if (KC >= (1 << 20) || (long long)M * N >= (1ll << 31) || (long long)M * Cin >= (1ll << 31)) return false;
  const int tiles_c = (int)((KC + PG_TILE_C - 1) / PG_TILE_C);
  const int tiles = (N / PG_TILE_N) * tiles_c;
  // ranges: enough for about one workgroup per CU, never shorter than two stages of rows
  long long want = (PG_WG_TARGET + tiles - 1) / tiles;
  const long long most = ((long long)M + 2 * PG_STEP_ROWS - 1) / (2 * PG_STEP_ROWS);
  if (want > most) want = most;
  if (want < 1) want = 1;
  long long rows = ((long long)M + want - 1) / want;
  rows = (rows + PG_STEP_ROWS - 1) / PG_STEP_ROWS * PG_STEP_ROWS;
  const long long ranges = ((long long)M + rows - 1) / rows;
  const long long floats = ranges * N * KC;
  if (floats >= (1ll << 31) || ranges > 65535) return false;
  out->tile_n = PG_TILE_N; out->tile_c = PG_TILE_C; out->rows = (int)rows; out->ranges = (int)ranges; out->tiles = tiles;
  out->chunk = conv_gemm_acc_chunk() / PG_STEP_ROWS * PG_STEP_ROWS;
  out->ws_floats = floats;
  return true;
}

hipError_t launch_pg_wgrad(const float* dz, const float* X, int M, int S, int N, int Cin, int KW, const PgWgradPlan& pl, float* partial,
                           float* dW, hipStream_t st, int ldz) {
  const int tiles_c = pl.tiles / (N / PG_TILE_N);
  hipLaunchKernelGGL(k_pg_wgrad, dim3(pl.tiles, pl.ranges), dim3(256), 0, st, dz, X, M, S, N, Cin, KW, pl.rows, tiles_c, pl.chunk / PG_STEP_ROWS,
                     partial, ldz > 0 ? ldz : N);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long n = (long long)N * Cin;
  hipLaunchKernelGGL(k_pg_wgrad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partial, pl.ranges, N, Cin, KW, dW);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ weight pack
__global__ __launch_bounds__(256) void k_pg_pack(PgPack a, PgPack b) {
  const PgPack p = blockIdx.y ? b : a;
  if (!p.w) return;
  const long long n_el = (long long)p.N * p.Cin * p.KW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long long)gridDim.x * 256) {
    const int j = (int)(i % p.KW);
    const long long nc = i / p.KW;
    const int c = (int)(nc % p.Cin), n = (int)(nc / p.Cin);
    const float v = p.w[i];
    if (p.wp) p.wp[((size_t)n * p.KW + j) * p.Cin + c] = v;
    if (p.wt) p.wt[((size_t)c * p.KW + (p.KW - 1 - j)) * p.N + n] = v;
  }
}

hipError_t launch_pg_pack(const PgPack& a, const PgPack& b, hipStream_t st) {
  const long long na = a.w ? (long long)a.N * a.Cin * a.KW : 0, nb = b.w ? (long long)b.N * b.Cin * b.KW : 0;
  const long long n = na > nb ? na : nb;
  if (n == 0) return hipSuccess;
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_pg_pack, dim3((unsigned)blocks, 2), dim3(256), 0, st, a, b);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ row kernels
// One wave per row; the lane layout, the float64 row statistics, keep4 and the column-partial flush are train_rows.h's.
template <int NV>
__global__ __launch_bounds__(256) void k_pg_row_forward(const float* __restrict__ v, const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                        const uint8_t* __restrict__ keep, float scale, float* __restrict__ h,
                                                        const float* __restrict__ wlin, const float* __restrict__ blin,
                                                        const uint8_t* __restrict__ mask, float* __restrict__ pred, int M) {
  constexpr int F = 256 * NV;
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  f32x4 x[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) x[i] = *reinterpret_cast<const f32x4*>(v + (size_t)m * F + (64 * i + lane) * 4);
  double mu, rs;
  row_stats<NV>(x, &mu, &rs);
  double dot = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (64 * i + lane) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(ln_g + col), b = *reinterpret_cast<const f32x4*>(ln_b + col);
    double k[4];
    keep4(keep, (size_t)m * F + col, scale, k);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (float)((((double)x[i][e] - mu) * rs * (double)g[e] + (double)b[e]) * k[e]);
    if (h) *reinterpret_cast<f32x4*>(h + (size_t)m * F + col) = y;
    if (wlin) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(wlin + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) dot += (double)y[e] * (double)w[e];
    }
  }
  if (wlin) {
    dot = wave_sum(dot);
    if (lane == 0) pred[m] = (mask && mask[m]) ? 0.f : (float)(dot + (double)blin[0]);
  }
}

hipError_t launch_pg_row_forward(const float* v, const float* ln_g, const float* ln_b, const uint8_t* keep, float scale, float* h,
                                 const float* wlin, const float* blin, const uint8_t* mask, float* pred, int M, int F, hipStream_t st) {
  if (F != 256 && F != 512) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  const dim3 grid((M + 3) / 4), block(256);
  if (F == 256) hipLaunchKernelGGL(k_pg_row_forward<1>, grid, block, 0, st, v, ln_g, ln_b, keep, scale, h, wlin, blin, mask, pred, M);
  else hipLaunchKernelGGL(k_pg_row_forward<2>, grid, block, 0, st, v, ln_g, ln_b, keep, scale, h, wlin, blin, mask, pred, M);
  return hipGetLastError();
}

// Rows [64 blk, 64 blk + 64) of one workgroup, wave w the rows w, w + 4, ...; the column sums live in registers (float64) across the
// wave's rows and the four waves are added in wave order through LDS: part[blk][slot][col].
template <int NV, bool TAIL>
__global__ __launch_bounds__(256) void k_pg_row_backward(PgRowBackward a) {
  constexpr int F = 256 * NV;
  constexpr int NS = TAIL ? 4 : 3;
  __shared__ double red[4][F];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double cs[NS][NV][4];
  NS_COL_ZERO(cs, NS, NV);
  double sum_dp = 0.0;
  f32x4 g4[NV], b4[NV], w4[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (64 * i + lane) * 4;
    g4[i] = *reinterpret_cast<const f32x4*>(a.ln_g + col);
    if (TAIL) { b4[i] = *reinterpret_cast<const f32x4*>(a.ln_b + col); w4[i] = *reinterpret_cast<const f32x4*>(a.wlin + col); }
  }
  for (int rr = wave; rr < PG_ROW_BLOCK; rr += 4) {
    const int m = blockIdx.x * PG_ROW_BLOCK + rr;
    if (m >= a.M) break;
    f32x4 x[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) x[i] = *reinterpret_cast<const f32x4*>(a.v + (size_t)m * F + (64 * i + lane) * 4);
    double mu, rs;
    row_stats<NV>(x, &mu, &rs);
    double dp = 0.0;
    if (TAIL) {
      float gm = 0.f;
      if (!(a.mask && a.mask[m])) gm = a.g[m];  // selection: g behind the mask is not read
      dp = (double)gm;
      sum_dp += dp;
    }
    double xh[NV][4], dyh[NV][4], s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int col = (64 * i + lane) * 4;
      double k[4];
      keep4(a.keep, (size_t)m * F + col, a.scale, k);
      f32x4 up;
      if (!TAIL) up = *reinterpret_cast<const f32x4*>(a.dy + (size_t)m * F + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xh[i][e] = ((double)x[i][e] - mu) * rs;
        const double dy = (TAIL ? dp * (double)w4[i][e] : (double)up[e]) * k[e];
        cs[0][i][e] += dy * xh[i][e];
        cs[1][i][e] += dy;
        if (TAIL) cs[3][i][e] += dp * ((xh[i][e] * (double)g4[i][e] + (double)b4[i][e]) * k[e]);
        dyh[i][e] = dy * (double)g4[i][e];
        s1 += dyh[i][e];
        s2 += dyh[i][e] * xh[i][e];
      }
    }
    const double m1 = wave_sum(s1) / F, m2 = wave_sum(s2) / F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = x[i][e] > 0.f ? (float)(rs * (dyh[i][e] - m1 - xh[i][e] * m2)) : 0.f;
        cs[2][i][e] += (double)o[e];
      }
      *reinterpret_cast<f32x4*>(a.dz + (size_t)m * F + (64 * i + lane) * 4) = o;
    }
  }
  double* part = a.part + (size_t)blockIdx.x * PG_SLOTS * F;
  col_flush(cs, red, part);
  if (TAIL) {
    __syncthreads();
    if (lane == 0) red[wave][0] = sum_dp;
    __syncthreads();
    if (threadIdx.x == 0) part[4 * F] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
  }
}

hipError_t launch_pg_row_backward(const PgRowBackward& a, hipStream_t st) {
  if (a.F != 256 && a.F != 512) return hipErrorInvalidValue;
  if (a.M <= 0) return hipSuccess;
  const dim3 grid(pg_row_blocks(a.M)), block(256);
  if (a.F == 256) {
    if (a.tail) hipLaunchKernelGGL((k_pg_row_backward<1, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_pg_row_backward<1, false>), grid, block, 0, st, a);
  } else {
    if (a.tail) hipLaunchKernelGGL((k_pg_row_backward<2, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_pg_row_backward<2, false>), grid, block, 0, st, a);
  }
  return hipGetLastError();
}

// part[blk][slot][col] = sum of rows [64 blk, 64 blk + 64) of src[:, slot * F + col] (rows of `parts * F` floats), ascending
__global__ __launch_bounds__(256) void k_pg_colsum(const float* __restrict__ src, int M, int F, int parts, double* __restrict__ part) {
  const int m0 = blockIdx.x * PG_ROW_BLOCK, m1 = min(M, m0 + PG_ROW_BLOCK), slot = blockIdx.y;
  for (int col = threadIdx.x; col < F; col += 256) {
    double s = 0.0;
    for (int m = m0; m < m1; ++m) s += (double)src[(size_t)m * parts * F + slot * F + col];
    part[((size_t)blockIdx.x * PG_SLOTS + slot) * F + col] = s;
  }
}

hipError_t launch_pg_colsum(const float* src, int M, int F, int parts, double* part, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  if (parts < 1 || parts > PG_SLOTS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pg_colsum, dim3(pg_row_blocks(M), parts), dim3(256), 0, st, src, M, F, parts, part);
  return hipGetLastError();
}

// 64 columns x 4 segments of the blocks per workgroup: a thread sums its segment in ascending order, the four segment sums are
// added in segment order.  blockIdx.y = stage * PG_SLOTS + slot.
__global__ __launch_bounds__(256) void k_pg_col_final(const double* __restrict__ part, int nblk, int F, PgColFinal o) {
  __shared__ double seg[4][64];
  float* out = o.out[blockIdx.y];
  if (!out) return;
  const int stage = blockIdx.y / PG_SLOTS, slot = blockIdx.y % PG_SLOTS;
  const int cl = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const bool live = col < (slot == 4 ? 1 : F);
  const int per = (nblk + 3) / 4, b0 = sg * per, b1 = min(nblk, b0 + per);
  const double* p = part + ((size_t)stage * nblk * PG_SLOTS + slot) * F + col;
  double s = 0.0;
  if (live)
    for (int b = b0; b < b1; ++b) s += p[(size_t)b * PG_SLOTS * F];
  seg[sg][cl] = s;
  __syncthreads();
  if (sg == 0 && live) out[col] = (float)(((seg[0][cl] + seg[1][cl]) + seg[2][cl]) + seg[3][cl]);
}

hipError_t launch_pg_col_final(const double* part, int nblk, int F, const PgColFinal& o, hipStream_t st) {
  bool any = false;
  for (int i = 0; i < 2 * PG_SLOTS; ++i) any = any || o.out[i];
  if (!any || nblk <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pg_col_final, dim3(F / 64, 2 * PG_SLOTS), dim3(256), 0, st, part, nblk, F, o);
  return hipGetLastError();
}

}  // namespace ns
