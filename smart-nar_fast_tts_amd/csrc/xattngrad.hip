// Cross-attention training kernels for gfx950 (transformer/SubLayers.py:8-59 as FFTBlock2.crs_attn):
//   k_xg_bwd_q          owns 128 queries of one (b, h), sweeps the key tiles below src_lens[b]: D and dQ
//   k_xg_bwd_kv         owns 128 keys of one (b, h) and one part of the query tiles: dK and dV (or their partial sums)
//   k_xg_kv_reduce      the fixed-order sum of the parts, +0.0 at keys >= src_lens[b]; only launched when there is more than one part
//   k_xg_pack           Wk | Wv -> one [2d][d] weight + [2d] bias (forward) and the transposed forms the data gradients read
// Unlike attngrad.hip nothing is recomputed: the probabilities A [B, H, T, L] are the module's own output (k_cross_attention wrote the
// final values, exact 0 at masked keys) and carry an upstream gradient dA of their own (nullable), so both kernels READ their tile of A
// and dA instead of forming exp(c S - lse):
//   dP = dO V^T + dA,   D_i = dO_i . O_i + sum_{l < len} A_il dA_il (float64, rounded once),   dS = A (dP - D)
//   dQ = c dS K,   dK = c dS^T Q,   dV = A^T dO
// dA is selected away (never reaches a sum) at keys >= src_lens[b], and so are K and V rows there.  Exact fp32 on
// v_mfma_f32_32x32x2_f32; no atomics, no host reads; every sum has one order that depends on (B, H, T, L, the number of parts) alone.
//
// A map tile is staged through registers into LDS like every other tile, because L is arbitrary: a row of the map is 16-byte aligned
// only when L % 4 == 0.  Then a thread moves 16-byte chunks; otherwise it moves single floats, consecutive lanes consecutive
// addresses.  Both forms leave the same values in the same LDS places, so the sums do not depend on which one ran.
#include "ag_tiles.h"

namespace ns {

constexpr int XG_MAP_LD = 36;     // LDS row stride of the query-owning kernel's map tile: 128 query rows x 32 keys
constexpr int XG_MAPT_LD = 132;   // LDS row stride of the key-owning kernel's map tile: 32 query rows x 128 keys

// ------------------------------------------------------------------------------------------------------------------ map tiles
// ROWS x COLS floats of one [T, L] plane starting at (row0, col0); COLS = 32 or 128, ROWS * COLS = 4096 = 16 floats per thread.
// Elements at rows >= nrows or columns >= ncols (ncols <= L) are staged as +0.0 and never loaded.
template <int COLS>
__device__ inline void xg_fetch_map(const float* __restrict__ plane, int L, int row0, int nrows, int col0, int ncols, bool vec, int tid,
                                    float (&r)[16]) {
  if (vec) {  // (workgroup-uniform) L % 4 == 0: chunk c = tid + 256 i covers 4 consecutive columns, all of them below L when the first is
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i, row = row0 + c / (COLS / 4), col = col0 + (c % (COLS / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < nrows && col < ncols) v = *reinterpret_cast<const f32x4*>(plane + (size_t)row * L + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[4 * i + e] = col + e < ncols ? v[e] : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int f = tid + 256 * j, row = row0 + f / COLS, col = col0 + f % COLS;
      r[j] = 0.f;
      if (row < nrows && col < ncols) r[j] = plane[(size_t)row * L + col];
    }
  }
}
template <int COLS, int LD>
__device__ inline void xg_stash_map(float* lds, bool vec, int tid, const float (&r)[16]) {
  if (vec) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      const f32x4 v = {r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
      *reinterpret_cast<f32x4*>(lds + (c / (COLS / 4)) * LD + (c % (COLS / 4)) * 4) = v;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int f = tid + 256 * j;
      lds[(f / COLS) * LD + f % COLS] = r[j];
    }
  }
}
// the query-owning kernel's view: lane (qi, h) of wave w owns query row 32 w + qi; register j = key 4h + 8 (j >> 2) + (j & 3) of the tile
__device__ inline f32x16 xg_read_map(const float* lds, int wrow, int h) {
  f32x16 a;
  const float* p = lds + wrow * XG_MAP_LD + 4 * h;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[4 * g + e] = v[e];
  }
  return a;
}
// the key-owning kernel's view: lane (ki, h) of wave w owns key column 32 w + ki; register j = swept query row r(j, h) of the tile
__device__ inline f32x16 xg_read_mapt(const float* lds, int wcol, int h) {
  f32x16 a;
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = lds[((j & 3) + 8 * (j >> 2) + 4 * h) * XG_MAPT_LD + wcol];
  return a;
}

// dP^T[swept row][owner row] = sum_k tile[swept row][k] own[owner row][k] in ag_cross's layout, but as partial sums of 8 products (4
// MFMA steps) that are added up in float64, in ascending k: where the probabilities are peaked dS = A (dP + dA - D) is a difference of
// nearly equal numbers (with one key it is zero), so dP is kept to about the precision D has; it is rounded once, inside dS.
template <int DK>
__device__ inline void xg_cross(const float* tile, int qi, int h, const f32x4 (&own)[DK / 8], double (&tot)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] = 0.0;
  const float* tp = tile + qi * (DK + 4) + 4 * h;
#pragma unroll
  for (int g = 0; g < DK / 8; ++g) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const f32x4 t = *reinterpret_cast<const f32x4*>(tp + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(t[e], own[g][e], s, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] += (double)s[r];
  }
}

// ------------------------------------------------------------------------------------------------------------------ dQ and D
// Workgroup = 4 waves = 128 queries of one (b, h); wave = 32 queries with dO^T in registers.  First one sweep of the map rows for
// sum_l A dA (skipped without dA), then the sweep of the key tiles: K and V rows at or past src_lens[b] are staged as zeros, and so
// are A and dA there.  dS^T[key][q] = A (dP + dA - D[q]), the bracket formed in float64 and rounded once, is the B operand of
// dQ^T += K^T dS^T as it stands.  dQ = c * the sum.
template <int DK>
__global__ __launch_bounds__(256) void k_xg_bwd_q(const float* __restrict__ kv, const float* __restrict__ ctx, const float* __restrict__ attn,
                                                 const float* __restrict__ dctx, const float* __restrict__ dattn,
                                                 const long long* __restrict__ lens, int T, int L, int d, int H, float c,
                                                 float* __restrict__ Dout, float* __restrict__ dq) {
  __shared__ __attribute__((aligned(16))) float Ks[AG_ROWS * (DK + 4)];
  __shared__ __attribute__((aligned(16))) float Vs[AG_ROWS * (DK + 4)];
  __shared__ __attribute__((aligned(16))) float As[128 * XG_MAP_LD];
  __shared__ __attribute__((aligned(16))) float Gs[128 * XG_MAP_LD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, qi = lane & 31;
  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * 128;
  const int q = q0 + wid * 32 + qi, qc = q < T ? q : T - 1;
  const int ld = 2 * d, len = ag_len(lens, b, L), nkt = (len + AG_ROWS - 1) / AG_ROWS;
  const bool vec = (L & 3) == 0;
  const float* base = kv + (size_t)b * L * ld + hd * DK;
  const size_t row = (size_t)b * T + qc, stat = ((size_t)b * H + hd) * T + qc;
  const float* aplane = attn + ((size_t)b * H + hd) * T * (size_t)L;
  const float* gplane = dattn ? dattn + ((size_t)b * H + hd) * T * (size_t)L : nullptr;
  f32x4 doreg[DK / 8], kr[DK / 32], vr[DK / 32];
  float ar[16], gr[16];
  ag_own<DK>(dctx + row * d + hd * DK, h, doreg);
  double part = 0.0;
  {
    f32x4 o[DK / 8];
    ag_own<DK>(ctx + row * d + hd * DK, h, o);
#pragma unroll
    for (int g = 0; g < DK / 8; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) part += (double)doreg[g][e] * (double)o[g][e];
  }
  if (gplane) {  // (workgroup-uniform)
    for (int kt = 0; kt < nkt; ++kt) {
      xg_fetch_map<32>(aplane, L, q0, T, kt * AG_ROWS, len, vec, tid, ar);
      xg_fetch_map<32>(gplane, L, q0, T, kt * AG_ROWS, len, vec, tid, gr);
      xg_stash_map<32, XG_MAP_LD>(As, vec, tid, ar);
      xg_stash_map<32, XG_MAP_LD>(Gs, vec, tid, gr);
      __syncthreads();
      const f32x16 a = xg_read_map(As, wid * 32 + qi, h), g = xg_read_map(Gs, wid * 32 + qi, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) part += (double)a[r] * (double)g[r];
      __syncthreads();
    }
  }
  float Dq;
  {
    const double other = __shfl_xor(part, 32, 64);
    Dq = (float)(h == 0 ? part + other : other + part);
    if (h == 0 && q < T) Dout[stat] = Dq;
  }
  f32x16 acc[DK / 32];
#pragma unroll
  for (int db = 0; db < DK / 32; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
  auto fetch = [&](int kt) {
    ag_fetch<DK>(base, ld, kt * AG_ROWS, len, tid, kr);
    ag_fetch<DK>(base + d, ld, kt * AG_ROWS, len, tid, vr);
    xg_fetch_map<32>(aplane, L, q0, T, kt * AG_ROWS, len, vec, tid, ar);
    if (gplane) xg_fetch_map<32>(gplane, L, q0, T, kt * AG_ROWS, len, vec, tid, gr);
  };
  if (nkt > 0) fetch(0);
  for (int kt = 0; kt < nkt; ++kt) {
    ag_stash<DK>(Ks, tid, kr);
    ag_stash<DK>(Vs, tid, vr);
    xg_stash_map<32, XG_MAP_LD>(As, vec, tid, ar);
    if (gplane) xg_stash_map<32, XG_MAP_LD>(Gs, vec, tid, gr);
    __syncthreads();
    if (kt + 1 < nkt) fetch(kt + 1);
    const f32x16 a = xg_read_map(As, wid * 32 + qi, h);
    double dp64[16];
    xg_cross<DK>(Vs, qi, h, doreg, dp64);
    if (gplane) {
      const f32x16 g = xg_read_map(Gs, wid * 32 + qi, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) dp64[r] += (double)g[r];
    }
    f32x16 dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = a[r] * (float)(dp64[r] - (double)Dq);
    ag_accumulate<DK>(Ks, qi, h, dp, acc);
    __syncthreads();
  }
  if (q < T) ag_store<DK>(dq + ((size_t)b * T + q) * d + hd * DK, h, acc, c, true);
}

// ------------------------------------------------------------------------------------------------------------------ dK and dV
// Workgroup = 4 waves = 128 keys of one (b, h) and the query tiles [part * per, part * per + per) of ceil(T / 32); wave = 32 keys with
// V in registers (a key at or past src_lens[b] holds zeros, and its column of A and dA is staged as zeros).  Rows past T of a swept
// tile are zeros everywhere.  dV^T += dO^T A, dK^T += Q^T dS.  out rows have `ldo` floats, K at 0 and V at d: the final dK | dV when
// there is one part (keys at or past src_lens[b] written as +0.0, a workgroup wholly past it only writes its zeros), else this part's
// slab of the partial sums (a workgroup wholly past src_lens[b] writes nothing: k_xg_kv_reduce never reads those rows).
template <int DK>
__global__ __launch_bounds__(256) void k_xg_bwd_kv(const float* __restrict__ qm, const float* __restrict__ kv, const float* __restrict__ attn,
                                                  const float* __restrict__ dctx, const float* __restrict__ dattn,
                                                  const float* __restrict__ Dws, const long long* __restrict__ lens, int T, int L, int d, int H,
                                                  int nsplit, int per, float c, float* __restrict__ outbase, size_t slab) {
  __shared__ __attribute__((aligned(16))) float Qs[AG_ROWS * (DK + 4)];
  __shared__ __attribute__((aligned(16))) float Os[AG_ROWS * (DK + 4)];
  __shared__ __attribute__((aligned(16))) float As[AG_ROWS * XG_MAPT_LD];
  __shared__ __attribute__((aligned(16))) float Gs[AG_ROWS * XG_MAPT_LD];
  __shared__ __attribute__((aligned(16))) float Ds[AG_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, qi = lane & 31;
  const int b = blockIdx.z / nsplit, sp = blockIdx.z % nsplit, hd = blockIdx.y, k0 = blockIdx.x * 128;
  const int key = k0 + wid * 32 + qi, kc = key < L ? key : L - 1;
  const int ld = 2 * d, len = ag_len(lens, b, L);
  const bool live = key < len, vec = (L & 3) == 0;
  float* out = outbase + (size_t)sp * slab + ((size_t)b * L + kc) * ld + hd * DK;
  f32x16 accK[DK / 32], accV[DK / 32];
#pragma unroll
  for (int db = 0; db < DK / 32; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) { accK[db][r] = 0.f; accV[db][r] = 0.f; }
  if (k0 >= len) {  // (workgroup-uniform)
    if (nsplit == 1 && key < L) { ag_store<DK>(out, h, accK, 0.f, false); ag_store<DK>(out + d, h, accV, 0.f, false); }
    return;
  }
  const float* Q = qm + (size_t)b * T * d + hd * DK;
  const float* dO = dctx + (size_t)b * T * d + hd * DK;
  const float* drow = Dws + ((size_t)b * H + hd) * T;
  const float* aplane = attn + ((size_t)b * H + hd) * T * (size_t)L;
  const float* gplane = dattn ? dattn + ((size_t)b * H + hd) * T * (size_t)L : nullptr;
  f32x4 vreg[DK / 8], qr[DK / 32], orr[DK / 32];
  float ar[16], gr[16], dr = 0.f;
  auto fetch = [&](int qt) {
    ag_fetch<DK>(Q, d, qt * AG_ROWS, T, tid, qr);
    ag_fetch<DK>(dO, d, qt * AG_ROWS, T, tid, orr);
    xg_fetch_map<128>(aplane, L, qt * AG_ROWS, T, k0, len, vec, tid, ar);
    if (gplane) xg_fetch_map<128>(gplane, L, qt * AG_ROWS, T, k0, len, vec, tid, gr);
    if (tid < AG_ROWS) {
      const int qq = qt * AG_ROWS + tid;
      dr = qq < T ? drow[qq] : 0.f;
    }
  };
  const int nqt = (T + AG_ROWS - 1) / AG_ROWS, qt0 = sp * per, qt1 = min(nqt, qt0 + per);
  if (qt0 < qt1) fetch(qt0);
  ag_own<DK>(kv + ((size_t)b * L + kc) * ld + d + hd * DK, h, vreg);
#pragma unroll
  for (int g = 0; g < DK / 8; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) vreg[g][e] = live ? vreg[g][e] : 0.f;
  for (int qt = qt0; qt < qt1; ++qt) {
    ag_stash<DK>(Qs, tid, qr);
    ag_stash<DK>(Os, tid, orr);
    xg_stash_map<128, XG_MAPT_LD>(As, vec, tid, ar);
    if (gplane) xg_stash_map<128, XG_MAPT_LD>(Gs, vec, tid, gr);
    if (tid < AG_ROWS) Ds[tid] = dr;
    __syncthreads();
    if (qt + 1 < qt1) fetch(qt + 1);
    const f32x16 a = xg_read_mapt(As, wid * 32 + qi, h);
    double dp64[16];
    xg_cross<DK>(Os, qi, h, vreg, dp64);
    if (gplane) {
      const f32x16 g = xg_read_mapt(Gs, wid * 32 + qi, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) dp64[r] += (double)g[r];
    }
    f32x16 dp;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(&Ds[8 * r4 + 4 * h]);
#pragma unroll
      for (int j = 0; j < 4; ++j) dp[4 * r4 + j] = a[4 * r4 + j] * (float)(dp64[4 * r4 + j] - (double)d4[j]);
    }
    ag_accumulate<DK>(Os, qi, h, a, accV);
    ag_accumulate<DK>(Qs, qi, h, dp, accK);
    __syncthreads();
  }
  if (key < L) { ag_store<DK>(out, h, accK, c, live); ag_store<DK>(out + d, h, accV, 1.f, live); }
}

// dkv[row][:] = sum over the parts, ascending, of part[p][row][:] for a key row below src_lens[b], else +0.0 (the partial is not read)
__global__ __launch_bounds__(256) void k_xg_kv_reduce(const float* __restrict__ part, const long long* __restrict__ lens, int L, int w4, int nsplit,
                                                     long long n4, float* __restrict__ dkv) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long long rowi = i / w4;
  const int b = (int)(rowi / L), key = (int)(rowi % L);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (key < ag_len(lens, b, L)) {
    s = reinterpret_cast<const f32x4*>(part)[i];
    for (int p = 1; p < nsplit; ++p) {
      const f32x4 v = reinterpret_cast<const f32x4*>(part)[(size_t)p * n4 + i];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += v[e];
    }
  }
  reinterpret_cast<f32x4*>(dkv)[i] = s;
}

// The number of query parts of the key-owning kernel: a function of (B, H, T, L) alone (include/nar_fs2.h ns_xg_kv_splits).  Doubled
// while the grid stays under one workgroup per CU and every part keeps at least 4 query tiles; at most 8.
int xg_kv_splits(int B, int H, int T, int L) {
  const long long wgs = (long long)((L + 127) / 128) * H * B;
  const int nqt = (T + AG_ROWS - 1) / AG_ROWS;
  int n = 1;
  while (n < 8 && wgs * n < PG_WG_TARGET && nqt / (2 * n) >= 4) n *= 2;
  return n;
}

hipError_t launch_xg_attention_backward(const float* q, const float* kv, const float* ctx, const float* attn, const float* dctx, const float* dattn,
                                        const long long* lens, int B, int T, int L, int H, int dk, int nsplit, float* D, float* partial, float* dq,
                                        float* dkv, hipStream_t st) {
  if (dk != 64 && dk != 128) return hipErrorInvalidValue;
  if (nsplit < 1 || nsplit > 8 || (nsplit > 1 && dkv && !partial)) return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || L <= 0) return hipSuccess;
  if ((long long)B * nsplit > 65535 || H > 65535) return hipErrorInvalidValue;  // grid.z, grid.y
  const dim3 gq((T + 127) / 128, H, B), gk((L + 127) / 128, H, B * nsplit), block(256);
  const float c = 1.f / sqrtf((float)dk);
  const int d = H * dk, nqt = (T + AG_ROWS - 1) / AG_ROWS, per = (nqt + nsplit - 1) / nsplit;
  const size_t slab = (size_t)B * L * 2 * d;
  float* out = nsplit > 1 ? partial : dkv;
#define NS_XG_BWD(DK)                                                                                                            \
  hipLaunchKernelGGL(k_xg_bwd_q<DK>, gq, block, 0, st, kv, ctx, attn, dctx, dattn, lens, T, L, d, H, c, D, dq);                  \
  if (dkv)                                                                                                                       \
  hipLaunchKernelGGL(k_xg_bwd_kv<DK>, gk, block, 0, st, q, kv, attn, dctx, dattn, (const float*)D, lens, T, L, d, H, nsplit, per, c, out, slab)
  if (dk == 64) { NS_XG_BWD(64); }
  else { NS_XG_BWD(128); }
#undef NS_XG_BWD
  if (dkv && nsplit > 1) {
    const long long n4 = (long long)(slab / 4);
    hipLaunchKernelGGL(k_xg_kv_reduce, dim3((unsigned)((n4 + 255) / 256)), block, 0, st, (const float*)partial, lens, L, 2 * d / 4, nsplit, n4, dkv);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ weight pack
__global__ __launch_bounds__(256) void k_xg_pack(XgPack p) {
  const long long dd = (long long)p.d * p.d, step = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p.wkv || p.wkvt)
    for (long long i = first; i < 2 * dd; i += step) {
      const int n = (int)(i / p.d), c = (int)(i - (long long)n * p.d), half = n / p.d;
      const float v = (half == 0 ? p.wk : p.wv)[i - half * dd];
      if (p.wkv) p.wkv[i] = v;
      if (p.wkvt) p.wkvt[(size_t)c * 2 * p.d + n] = v;
    }
  if (p.wqt || p.wfct)
    for (long long i = first; i < dd; i += step) {
      const int n = (int)(i / p.d), c = (int)(i - (long long)n * p.d);
      if (p.wqt) p.wqt[(size_t)c * p.d + n] = p.wq[i];
      if (p.wfct) p.wfct[(size_t)c * p.d + n] = p.wfc[i];
    }
  if (p.bkv)
    for (long long i = first; i < 2 * p.d; i += step) p.bkv[i] = i < p.d ? p.bk[i] : p.bv[i - p.d];
}

hipError_t launch_xg_pack(const XgPack& p, hipStream_t st) {
  if (!p.wkv && !p.bkv && !p.wkvt && !p.wqt && !p.wfct) return hipSuccess;
  hipLaunchKernelGGL(k_xg_pack, dim3(1024), dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace ns
