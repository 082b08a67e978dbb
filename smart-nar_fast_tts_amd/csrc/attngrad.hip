// MultiHeadAttention training kernels for gfx950 (transformer/SubLayers.py:8-59, self-attention):
//   k_ag_lse            lse[b, h, i] = log sum_{j < lens[b]} exp(c q_i . k_j): one sweep of Q K^T with a running row maximum
//   k_ag_bwd_q          owns 128 queries of one (b, h), sweeps the key tiles: D[i] = dctx_i . ctx_i (float64, rounded once) and dQ
//   k_ag_bwd_kv         owns 128 keys of one (b, h), sweeps the query tiles: dK and dV; reads the D that k_ag_bwd_q left
//   k_ag_row_forward    z = u * keep / (1 - p) + x, y = LayerNorm(z)  (row kernels over train_rows.h, as predgrad.hip's)
//   k_ag_row_backward   LayerNorm backward from z: dz, du = dz * keep / (1 - p), float64 column partials (d_ln_g, d_ln_b, d_bfc)
//   k_ag_pack           Wq | Wk | Wv -> one [3d][d] weight + [3d] bias (forward) and the transposed forms the data gradients read
// Both backward kernels recompute S = Q K^T and dP = dO V^T for their own tiles on the fp32 matrix cores (v_mfma_f32_32x32x2_f32);
// the [S, S] matrices never reach memory.  No atomics, no host reads; every sum has one order that depends on the shape alone.
//
// The tile helpers and the layout trick they share with xattngrad.hip are ag_tiles.h's.
#include "ag_tiles.h"
#include "train_rows.h"

namespace ns {

constexpr float AG_LOG2E = 1.4426950408889634f, AG_LN2 = 0.6931471805599453f;

// ------------------------------------------------------------------------------------------------------------------ row log-sum-exp
// Workgroup = 4 waves = 128 queries of one (b, h), each wave 32 queries; the 32-key tiles of K are swept once.  A lane keeps a running
// (maximum, sum) over its 16 keys of every tile; the two halves of a query are merged at the end.  Natural-log domain throughout:
// t = c s, exp(t - m) as exp2((t - m) log2 e), lse = m + ln 2 * log2(sum).  lens[b] == 0 gives -inf.
template <int DK>
__global__ __launch_bounds__(256) void k_ag_lse(const float* __restrict__ qkv, const long long* __restrict__ lens, int S, int d, int H, float c,
                                               float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float Ks[AG_ROWS * (DK + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, qi = lane & 31;
  const int b = blockIdx.z, hd = blockIdx.y;
  const int q = blockIdx.x * 128 + wid * 32 + qi, qc = q < S ? q : S - 1;
  const int ld = 3 * d, len = ag_len(lens, b, S), nkt = (len + AG_ROWS - 1) / AG_ROWS;
  const float* base = qkv + (size_t)b * S * ld + hd * DK;
  f32x4 qreg[DK / 8], kr[DK / 32];
  ag_own<DK>(base + (size_t)qc * ld, h, qreg);
  float m_run = -INFINITY, l_run = 0.f;
  if (nkt > 0) ag_fetch<DK>(base + d, ld, 0, len, tid, kr);
  for (int kt = 0; kt < nkt; ++kt) {
    ag_stash<DK>(Ks, tid, kr);
    __syncthreads();
    if (kt + 1 < nkt) ag_fetch<DK>(base + d, ld, (kt + 1) * AG_ROWS, len, tid, kr);
    f32x16 s = ag_cross<DK>(Ks, qi, h, qreg);
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * AG_ROWS + 4 * h + (r & 3) + 8 * (r >> 2);
      s[r] = key < len ? s[r] * c : -INFINITY;
      mt = fmaxf(mt, s[r]);
    }
    const float m_new = fmaxf(m_run, mt), m_use = m_new == -INFINITY ? 0.f : m_new;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f((s[r] - m_use) * AG_LOG2E);
    l_run = l_run * __builtin_amdgcn_exp2f((m_run - m_use) * AG_LOG2E) + sum;
    m_run = m_new;
    __syncthreads();
  }
  const float m_o = __shfl_xor(m_run, 32, 64), l_o = __shfl_xor(l_run, 32, 64);
  const float m = fmaxf(m_run, m_o), mu = m == -INFINITY ? 0.f : m;
  const float a = l_run * __builtin_amdgcn_exp2f((m_run - mu) * AG_LOG2E), bb = l_o * __builtin_amdgcn_exp2f((m_o - mu) * AG_LOG2E);
  const float l = h == 0 ? a + bb : bb + a;  // the two halves add the same two numbers
  if (h == 0 && q < S) lse[((size_t)b * H + hd) * S + q] = m + AG_LN2 * __builtin_amdgcn_logf(l);
}

hipError_t launch_ag_lse(const float* qkv, const long long* lens, int B, int S, int H, int dk, float* lse, hipStream_t st) {
  if (dk != 32 && dk != 64 && dk != 128) return hipErrorInvalidValue;
  if (B <= 0 || S <= 0) return hipSuccess;
  const dim3 grid((S + 127) / 128, H, B), block(256);
  const float c = 1.f / sqrtf((float)dk);
  const int d = H * dk;
  if (dk == 32) hipLaunchKernelGGL(k_ag_lse<32>, grid, block, 0, st, qkv, lens, S, d, H, c, lse);
  else if (dk == 64) hipLaunchKernelGGL(k_ag_lse<64>, grid, block, 0, st, qkv, lens, S, d, H, c, lse);
  else hipLaunchKernelGGL(k_ag_lse<128>, grid, block, 0, st, qkv, lens, S, d, H, c, lse);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ attention backward
// P[key][q] = exp(c s - lse[q]) for key < len, else exactly 0 (a select, so nothing a padded key holds can reach a sum)
__device__ inline float ag_prob(float s, float c, float lse, bool live) { return live ? __builtin_amdgcn_exp2f((s * c - lse) * AG_LOG2E) : 0.f; }

// dQ: wave = 32 queries (Q^T and dO^T in registers), sweep of the key tiles below lens[b]; K and V rows at or past lens[b] are staged
// as zeros.  dS^T[key][q] = P (dP - D[q]) is the B operand of dQ^T += K^T dS^T as it stands.  dQ = c * the sum.
template <int DK>
__global__ __launch_bounds__(256) void k_ag_bwd_q(const float* __restrict__ qkv, const float* __restrict__ ctx, const float* __restrict__ lse,
                                                 const float* __restrict__ dctx, const long long* __restrict__ lens, int S, int d, int H, float c,
                                                 float* __restrict__ Dout, float* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) float Ks[AG_ROWS * (DK + 4)];
  __shared__ __attribute__((aligned(16))) float Vs[AG_ROWS * (DK + 4)];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, qi = lane & 31;
  const int b = blockIdx.z, hd = blockIdx.y;
  const int q = blockIdx.x * 128 + wid * 32 + qi, qc = q < S ? q : S - 1;
  const int ld = 3 * d, len = ag_len(lens, b, S), nkt = (len + AG_ROWS - 1) / AG_ROWS;
  const float* base = qkv + (size_t)b * S * ld + hd * DK;
  const size_t row = (size_t)b * S + qc, stat = ((size_t)b * H + hd) * S + qc;
  f32x4 qreg[DK / 8], doreg[DK / 8], kr[DK / 32], vr[DK / 32];
  if (nkt > 0) {
    ag_fetch<DK>(base + d, ld, 0, len, tid, kr);
    ag_fetch<DK>(base + 2 * d, ld, 0, len, tid, vr);
  }
  ag_own<DK>(base + (size_t)qc * ld, h, qreg);
  ag_own<DK>(dctx + row * d + hd * DK, h, doreg);
  float Dq;
  {
    f32x4 o[DK / 8];
    ag_own<DK>(ctx + row * d + hd * DK, h, o);
    double part = 0.0;
#pragma unroll
    for (int g = 0; g < DK / 8; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) part += (double)doreg[g][e] * (double)o[g][e];
    const double other = __shfl_xor(part, 32, 64);
    Dq = (float)(h == 0 ? part + other : other + part);
    if (h == 0 && q < S) Dout[stat] = Dq;
  }
  const float lq = lse[stat];
  f32x16 acc[DK / 32];
#pragma unroll
  for (int db = 0; db < DK / 32; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
  for (int kt = 0; kt < nkt; ++kt) {
    ag_stash<DK>(Ks, tid, kr);
    ag_stash<DK>(Vs, tid, vr);
    __syncthreads();
    if (kt + 1 < nkt) {
      ag_fetch<DK>(base + d, ld, (kt + 1) * AG_ROWS, len, tid, kr);
      ag_fetch<DK>(base + 2 * d, ld, (kt + 1) * AG_ROWS, len, tid, vr);
    }
    f32x16 s = ag_cross<DK>(Ks, qi, h, qreg);
    f32x16 dp = ag_cross<DK>(Vs, qi, h, doreg);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * AG_ROWS + 4 * h + (r & 3) + 8 * (r >> 2);
      const float p = ag_prob(s[r], c, lq, key < len);
      dp[r] = p * (dp[r] - Dq);
    }
    ag_accumulate<DK>(Ks, qi, h, dp, acc);
    __syncthreads();
  }
  if (q < S) ag_store<DK>(dqkv + ((size_t)b * S + q) * ld + hd * DK, h, acc, c, true);
}

// dK and dV: wave = 32 keys (K and V in registers; a key at or past lens[b] holds zeros and its P is 0 by select), sweep of EVERY query
// tile (padded query rows are computed like any other).  Rows past S of the swept tile are zeros with lse = +inf (P = 0) and D = 0.
// dV^T += dO^T P, dK^T += Q^T dS; dK = c * the sum.  Keys at or past lens[b] are written as +0.0; a workgroup wholly past lens[b]
// only writes its zeros.
template <int DK>
__global__ __launch_bounds__(256) void k_ag_bwd_kv(const float* __restrict__ qkv, const float* __restrict__ lse, const float* __restrict__ Dws,
                                                  const float* __restrict__ dctx, const long long* __restrict__ lens, int S, int d, int H, float c,
                                                  float* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) float Qs[AG_ROWS * (DK + 4)];
  __shared__ __attribute__((aligned(16))) float Os[AG_ROWS * (DK + 4)];
  __shared__ __attribute__((aligned(16))) float Ls[AG_ROWS];
  __shared__ __attribute__((aligned(16))) float Ds[AG_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, qi = lane & 31;
  const int b = blockIdx.z, hd = blockIdx.y;
  const int key = blockIdx.x * 128 + wid * 32 + qi, kc = key < S ? key : S - 1;
  const int ld = 3 * d, len = ag_len(lens, b, S);
  const bool live = key < len;
  const float* base = qkv + (size_t)b * S * ld + hd * DK;
  float* out = dqkv + ((size_t)b * S + kc) * ld + hd * DK;
  f32x16 accK[DK / 32], accV[DK / 32];
#pragma unroll
  for (int db = 0; db < DK / 32; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) { accK[db][r] = 0.f; accV[db][r] = 0.f; }
  if (blockIdx.x * 128 >= len) {  // (workgroup-uniform)
    if (key < S) { ag_store<DK>(out + d, h, accK, 0.f, false); ag_store<DK>(out + 2 * d, h, accV, 0.f, false); }
    return;
  }
  const float* dO = dctx + (size_t)b * S * d + hd * DK;
  const float* lrow = lse + ((size_t)b * H + hd) * S;
  const float* drow = Dws + ((size_t)b * H + hd) * S;
  f32x4 kreg[DK / 8], vreg[DK / 8], qr[DK / 32], orr[DK / 32];
  float lr = 0.f, dr = 0.f;
  auto fetch = [&](int qt) {
    ag_fetch<DK>(base, ld, qt * AG_ROWS, S, tid, qr);
    ag_fetch<DK>(dO, d, qt * AG_ROWS, S, tid, orr);
    if (tid < AG_ROWS) {
      const int qq = qt * AG_ROWS + tid;
      lr = qq < S ? lrow[qq] : INFINITY;
      dr = qq < S ? drow[qq] : 0.f;
    }
  };
  fetch(0);
  ag_own<DK>(base + d + (size_t)kc * ld, h, kreg);
  ag_own<DK>(base + 2 * d + (size_t)kc * ld, h, vreg);
#pragma unroll
  for (int g = 0; g < DK / 8; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) { kreg[g][e] = live ? kreg[g][e] : 0.f; vreg[g][e] = live ? vreg[g][e] : 0.f; }
  const int nqt = (S + AG_ROWS - 1) / AG_ROWS;
  for (int qt = 0; qt < nqt; ++qt) {
    ag_stash<DK>(Qs, tid, qr);
    ag_stash<DK>(Os, tid, orr);
    if (tid < AG_ROWS) { Ls[tid] = lr; Ds[tid] = dr; }
    __syncthreads();
    if (qt + 1 < nqt) fetch(qt + 1);
    f32x16 s = ag_cross<DK>(Qs, qi, h, kreg);
    f32x16 dp = ag_cross<DK>(Os, qi, h, vreg);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(&Ls[8 * r4 + 4 * h]), d4 = *reinterpret_cast<const f32x4*>(&Ds[8 * r4 + 4 * h]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * r4 + j;
        s[r] = ag_prob(s[r], c, l4[j], live);
        dp[r] = s[r] * (dp[r] - d4[j]);
      }
    }
    ag_accumulate<DK>(Os, qi, h, s, accV);
    ag_accumulate<DK>(Qs, qi, h, dp, accK);
    __syncthreads();
  }
  if (key < S) { ag_store<DK>(out + d, h, accK, c, live); ag_store<DK>(out + 2 * d, h, accV, 1.f, live); }
}

hipError_t launch_ag_attention_backward(const float* qkv, const float* ctx, const float* lse, const float* dctx, const long long* lens, int B,
                                        int S, int H, int dk, float* D, float* dqkv, hipStream_t st) {
  if (dk != 32 && dk != 64 && dk != 128) return hipErrorInvalidValue;
  if (B <= 0 || S <= 0) return hipSuccess;
  const dim3 grid((S + 127) / 128, H, B), block(256);
  const float c = 1.f / sqrtf((float)dk);
  const int d = H * dk;
#define NS_AG_BWD(DK)                                                                                              \
  hipLaunchKernelGGL(k_ag_bwd_q<DK>, grid, block, 0, st, qkv, ctx, lse, dctx, lens, S, d, H, c, D, dqkv);          \
  hipLaunchKernelGGL(k_ag_bwd_kv<DK>, grid, block, 0, st, qkv, lse, (const float*)D, dctx, lens, S, d, H, c, dqkv)
  if (dk == 32) { NS_AG_BWD(32); }
  else if (dk == 64) { NS_AG_BWD(64); }
  else { NS_AG_BWD(128); }
#undef NS_AG_BWD
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ row kernels
// One wave per row; the lane layout, the float64 row statistics, keep4 and the column-partial flush are train_rows.h's.
template <int NV>
__global__ __launch_bounds__(256) void k_ag_row_forward(const float* __restrict__ u, const float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                       float scale, const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                       float* __restrict__ z, float* __restrict__ y, int M) {
  constexpr int F = 256 * NV;
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  f32x4 zr[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const size_t off = (size_t)m * F + (64 * i + lane) * 4;
    const f32x4 uu = *reinterpret_cast<const f32x4*>(u + off), xx = *reinterpret_cast<const f32x4*>(x + off);
    double k[4];
    keep4(keep, off, scale, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) zr[i][e] = (float)((double)uu[e] * k[e] + (double)xx[e]);
    if (z) *reinterpret_cast<f32x4*>(z + off) = zr[i];
  }
  double mu, rs;
  row_stats<NV>(zr, &mu, &rs);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int col = (64 * i + lane) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(ln_g + col), bb = *reinterpret_cast<const f32x4*>(ln_b + col);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)(((double)zr[i][e] - mu) * rs * (double)g[e] + (double)bb[e]);
    *reinterpret_cast<f32x4*>(y + (size_t)m * F + col) = o;
  }
}

hipError_t launch_ag_row_forward(const float* u, const float* x, const uint8_t* keep, float scale, const float* ln_g, const float* ln_b, float* z,
                                 float* y, int M, int F, hipStream_t st) {
  if (F != 256 && F != 512) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  const dim3 grid((M + 3) / 4), block(256);
  if (F == 256) hipLaunchKernelGGL(k_ag_row_forward<1>, grid, block, 0, st, u, x, keep, scale, ln_g, ln_b, z, y, M);
  else hipLaunchKernelGGL(k_ag_row_forward<2>, grid, block, 0, st, u, x, keep, scale, ln_g, ln_b, z, y, M);
  return hipGetLastError();
}

// Rows [64 blk, 64 blk + 64) of one workgroup, wave w the rows w, w + 4, ...; column partials part[blk][slot][col] in the layout of
// k_pg_row_backward (slot 0 d_ln_g, 1 d_ln_b, 2 the column sums of du), summed by k_pg_col_final.
template <int NV>
__global__ __launch_bounds__(256) void k_ag_row_backward(AgRowBackward a) {
  constexpr int F = 256 * NV;
  __shared__ double red[4][F];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double cs[3][NV][4];
  NS_COL_ZERO(cs, 3, NV);
  f32x4 g4[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) g4[i] = *reinterpret_cast<const f32x4*>(a.ln_g + (64 * i + lane) * 4);
  for (int rr = wave; rr < PG_ROW_BLOCK; rr += 4) {
    const int m = blockIdx.x * PG_ROW_BLOCK + rr;
    if (m >= a.M) break;
    f32x4 x[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) x[i] = *reinterpret_cast<const f32x4*>(a.z + (size_t)m * F + (64 * i + lane) * 4);
    double mu, rs;
    row_stats<NV>(x, &mu, &rs);
    double xh[NV][4], dyh[NV][4], s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const f32x4 up = *reinterpret_cast<const f32x4*>(a.dy + (size_t)m * F + (64 * i + lane) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xh[i][e] = ((double)x[i][e] - mu) * rs;
        const double dy = (double)up[e];
        cs[0][i][e] += dy * xh[i][e];
        cs[1][i][e] += dy;
        dyh[i][e] = dy * (double)g4[i][e];
        s1 += dyh[i][e];
        s2 += dyh[i][e] * xh[i][e];
      }
    }
    const double m1 = wave_sum(s1) / F, m2 = wave_sum(s2) / F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const size_t off = (size_t)m * F + (64 * i + lane) * 4;
      double k[4];
      keep4(a.keep, off, a.scale, k);
      f32x4 o, w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (float)(rs * (dyh[i][e] - m1 - xh[i][e] * m2));
        w[e] = (float)((double)o[e] * k[e]);
        cs[2][i][e] += (double)w[e];
      }
      *reinterpret_cast<f32x4*>(a.dz + off) = o;
      *reinterpret_cast<f32x4*>(a.du + off) = w;
    }
  }
  double* part = a.part + (size_t)blockIdx.x * PG_SLOTS * F;
  col_flush(cs, red, part);
}

hipError_t launch_ag_row_backward(const AgRowBackward& a, hipStream_t st) {
  if (a.F != 256 && a.F != 512) return hipErrorInvalidValue;
  if (a.M <= 0) return hipSuccess;
  const dim3 grid(pg_row_blocks(a.M)), block(256);
  if (a.F == 256) hipLaunchKernelGGL(k_ag_row_backward<1>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_ag_row_backward<2>, grid, block, 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ weight pack
__global__ __launch_bounds__(256) void k_ag_pack(AgPack p) {
  const long long dd = (long long)p.d * p.d, step = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p.wp || p.wt)
    for (long long i = first; i < 3 * dd; i += step) {
      const int n = (int)(i / p.d), c = (int)(i - (long long)n * p.d), third = n / p.d;
      const float* w = third == 0 ? p.wq : (third == 1 ? p.wk : p.wv);
      const float v = w[i - third * dd];
      if (p.wp) p.wp[i] = v;
      if (p.wt) p.wt[(size_t)c * 3 * p.d + n] = v;
    }
  if (p.wfct)
    for (long long i = first; i < dd; i += step) {
      const int n = (int)(i / p.d), c = (int)(i - (long long)n * p.d);
      p.wfct[(size_t)c * p.d + n] = p.wfc[i];
    }
  if (p.bp)
    for (long long i = first; i < 3 * p.d; i += step) {
      const int third = (int)(i / p.d);
      const float* bsrc = third == 0 ? p.bq : (third == 1 ? p.bk : p.bv);
      p.bp[i] = bsrc[i - third * p.d];
    }
}

hipError_t launch_ag_pack(const AgPack& p, hipStream_t st) {
  if (!p.wp && !p.wt && !p.wfct && !p.bp) return hipSuccess;
  hipLaunchKernelGGL(k_ag_pack, dim3(1024), dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace ns
