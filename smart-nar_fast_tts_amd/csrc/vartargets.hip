// Pitch / energy variance targets and dataset statistics: the tail of Preprocessor.process_utterance and build_from_path /
// remove_outlier / normalize (preprocessor/preprocessor.py:188-227, 61-133, 289-310) on device tensors, with no host read and no
// float atomic.
//   k_vt_targets       one workgroup per (utterance, feature): n_b = min(T, sum of durations), the voiced flag, then either the
//                      frame-level copy or the per-phoneme float64 mean — for pitch over the contour interpolated across unvoiced
//                      frames (previous / next voiced index by a forward max-scan and a backward min-scan over 256-frame tiles)
//   k_vt_fit_partial   one workgroup per (utterance, feature): bitonic sort in LDS, numpy's linear p25 / p75, the strict outlier
//                      filter, (count, mean, M2) in float64 into the utterance's slot
//   k_vt_fit_merge     one workgroup: Chan's update over the slots in utterance order into the caller's state
//   k_vt_normalize     one workgroup per (utterance, feature): (x - mean) / std in place, float64 min / max into its slot
//   k_vt_minmax_merge  one workgroup: the slots folded into the state in utterance order
// Selection, not multiplication: frames at t >= n_b and phonemes at i >= src_lens[b] are never read (they may hold NaN).
// Reduction order: integer sums are exact in any order; a phoneme's mean is one thread's left-to-right float64 sum; the fit's sums
// are per-thread strided runs over the SORTED values followed by a fixed LDS tree — functions of the shapes and values only, not
// of pointer alignment, the stream, or what the workspace held.
#include <cfloat>
#include <climits>

#include "kernels.h"

namespace ns {

namespace {
constexpr int VT_THREADS = 256;
constexpr int VT_WAVES = VT_THREADS / 64;

__device__ __forceinline__ int clamp_len(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }
// max(d, 0), capped so that 2^26 of them cannot overflow an int64
__device__ __forceinline__ long long clamp_dur(long long d) { return d > 0 ? (d < 0x7fffffffll ? d : 0x7fffffffll) : 0; }

// exact (integer) sum over the workgroup; sh [VT_WAVES]
__device__ __forceinline__ long long block_sum(long long v, long long* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();  // sh may still be read from the previous call
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = sh[0];
#pragma unroll
  for (int w = 1; w < VT_WAVES; ++w) s += sh[w];
  return s;
}

// a fixed tree over the workgroup's 256 values: thread i adds thread i + w; red [VT_THREADS]
template <class Op>
__device__ __forceinline__ double block_tree(double v, double* red, Op op) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = VT_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  return red[0];
}
struct OpAdd { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };
}  // namespace

__global__ __launch_bounds__(VT_THREADS) void k_vt_targets(VtArgs a, double* __restrict__ contour_ws, int* __restrict__ next_ws) {
  __shared__ long long lsum[VT_WAVES];
  __shared__ long long lcarry;
  __shared__ int iw[VT_WAVES];
  __shared__ int icarry;
  const int b = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int L = a.L, T = a.T;
  const int Ls = clamp_len(a.src_lens[b], L);
  const long long* dur = a.durations + (size_t)b * a.durations_stride;
  const float* pitch = a.pitch + (size_t)b * T;
  const bool frame_level = (f ? a.energy_frame_level : a.pitch_frame_level) != 0;
  const float* x = f ? a.energy + (size_t)b * T : pitch;
  const int n_out = frame_level ? T : L;
  float* out = (f ? a.energy_targets : a.pitch_targets) + (size_t)b * n_out;

  // ---- n_b = min(T, sum_{i < Ls} max(d_i, 0)) (preprocessor.py:188,194-195) and the voiced count (:189)
  long long part = 0;
  for (int i = tid; i < Ls; i += VT_THREADS) part += clamp_dur(dur[i]);
  const long long total = block_sum(part, lsum);
  const int nb = total < (long long)T ? (int)total : T;
  long long voiced = 0;
  for (int t = tid; t < nb; t += VT_THREADS) voiced += pitch[t] != 0.0f ? 1 : 0;
  const bool valid = block_sum(voiced, lsum) > 1;
  if (f == 0 && tid == 0) {
    a.frame_lens[b] = nb;
    a.valid[b] = valid ? 1 : 0;
  }
  if (!valid) {  // the reference drops the utterance (:190)
    for (int i = tid; i < n_out; i += VT_THREADS) out[i] = 0.0f;
    return;
  }
  if (frame_level) {
    for (int t = tid; t < T; t += VT_THREADS) out[t] = t < nb ? x[t] : 0.0f;
    return;
  }

  double* contour = contour_ws + (size_t)b * T;
  if (f == 0) {
    // ---- the interpolated contour (:199-206).  Backward: next[t] = smallest voiced index >= t, INT_MAX when there is none.
    int* next = next_ws + (size_t)b * T;
    const int tiles = (nb + VT_THREADS - 1) / VT_THREADS;
    if (tid == 0) icarry = INT_MAX;
    __syncthreads();
    for (int k = tiles - 1; k >= 0; --k) {
      const int t = k * VT_THREADS + tid;
      int v = (t < nb && pitch[t] != 0.0f) ? t : INT_MAX;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_down(v, o);
        if (lane + o < 64) v = n < v ? n : v;
      }
      if (lane == 0) iw[wid] = v;
      __syncthreads();
      int off = icarry;
      for (int w = wid + 1; w < VT_WAVES; ++w) off = iw[w] < off ? iw[w] : off;
      v = off < v ? off : v;
      if (t < nb) next[t] = v;  // read back below by this same thread
      __syncthreads();
      if (tid == 0) icarry = v;
      __syncthreads();
    }
    // Forward: prev = largest voiced index <= t, -1 when there is none; then the contour in float64.
    if (tid == 0) icarry = -1;
    __syncthreads();
    for (int k = 0; k < tiles; ++k) {
      const int t = k * VT_THREADS + tid;
      int v = (t < nb && pitch[t] != 0.0f) ? t : -1;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o);
        if (lane >= o) v = n > v ? n : v;
      }
      if (lane == 63) iw[wid] = v;
      __syncthreads();
      int off = icarry;
      for (int w = 0; w < wid; ++w) off = iw[w] > off ? iw[w] : off;
      v = off > v ? off : v;
      if (t < nb) {
        const int x0 = v, x1 = next[t];  // valid: at least two voiced frames below nb, so one of the two exists
        double y;
        if (x0 == t) y = (double)pitch[t];
        else if (x0 < 0) y = (double)pitch[x1];          // before the first voiced frame: fill_value[0]
        else if (x1 == INT_MAX) y = (double)pitch[x0];   // after the last one: fill_value[1]
        else {
          const double y0 = (double)pitch[x0], y1 = (double)pitch[x1];
          const double slope = (y1 - y0) / (double)(x1 - x0);
          y = slope * (double)(t - x0) + y0;
        }
        contour[t] = y;
      }
      __syncthreads();
      if (tid == VT_THREADS - 1) icarry = v;
      __syncthreads();
    }
    __threadfence_block();
    __syncthreads();  // the contour is read by other threads of this workgroup below
  }

  // ---- per-phoneme mean over [c_i - d_i, c_i) within [0, nb), c the inclusive prefix sum (:208-216, 219-227): durations
  // walked 256 at a time, wave64 shuffle scan plus carry (rowops.hip k_duration_scan)
  if (tid == 0) lcarry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < L; i0 += VT_THREADS) {
    const int i = i0 + tid;
    const long long d = i < Ls ? clamp_dur(dur[i]) : 0;
    long long inc = d;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long n = __shfl_up(inc, o);
      if (lane >= o) inc += n;
    }
    if (lane == 63) lsum[wid] = inc;
    __syncthreads();
    long long c = lcarry + inc;
    for (int w = 0; w < wid; ++w) c += lsum[w];
    if (i < L) {
      float y = 0.0f;
      if (d > 0) {
        const long long s = c - d;
        const int lo = s < (long long)nb ? (int)s : nb, hi = c < (long long)nb ? (int)c : nb;
        if (hi > lo) {
          double sum = 0.0;
          if (f == 0) for (int t = lo; t < hi; ++t) sum += contour[t];
          else for (int t = lo; t < hi; ++t) sum += (double)x[t];
          y = (float)(sum / (double)(hi - lo));
        }
      }
      out[i] = y;
    }
    __syncthreads();
    if (tid == VT_THREADS - 1) lcarry = c;
    __syncthreads();
  }
}

// n values of one (utterance, feature): valid ? (frame_level ? frame_lens : src_lens) : 0, clamped to the tensor
__device__ __forceinline__ int vt_count(const VtArgs& a, int b, bool frame_level) {
  if (a.valid && !a.valid[b]) return 0;
  return frame_level ? clamp_len(a.frame_lens[b], a.T) : clamp_len(a.src_lens[b], a.L);
}

// numpy.percentile's default (linear) method at virtual index q (n - 1), its _lerp form, on the sorted values
__device__ __forceinline__ double vt_percentile(const float* s, int n, double q) {
  const double idx = (double)(n - 1) * q;
  const int lo = (int)idx;
  const int hi = lo + 1 < n ? lo + 1 : n - 1;
  const double g = idx - (double)lo, A = (double)s[lo], Bv = (double)s[hi], diff = Bv - A;
  return g >= 0.5 ? Bv - diff * (1.0 - g) : A + diff * g;
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_fit_partial(VtArgs a, double* __restrict__ slots) {
  __shared__ float s[VT_SORT_CAPACITY];
  __shared__ double red[VT_THREADS];
  const int b = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const bool frame_level = (f ? a.energy_frame_level : a.pitch_frame_level) != 0;
  int n = vt_count(a, b, frame_level);
  n = n < VT_SORT_CAPACITY ? n : VT_SORT_CAPACITY;  // (the host refuses a larger T / L)
  double* slot = slots + ((size_t)b * 2 + f) * (VT_SLOT_BYTES / 8);
  if (n < 2) {  // n == 1: the strict comparison keeps nothing (lower == upper == the value)
    if (tid < VT_SLOT_BYTES / 8) slot[tid] = 0.0;
    return;
  }
  const float* x = (f ? a.energy_targets : a.pitch_targets) + (size_t)b * (frame_level ? a.T : a.L);
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += VT_THREADS) s[i] = i < n ? x[i] : INFINITY;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < (P >> 1); p += VT_THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
        const bool up = (i & k) == 0;
        const float u = s[i], v = s[q];
        if ((u > v) == up) { s[i] = v; s[q] = u; }
      }
      __syncthreads();
    }
  const double p25 = vt_percentile(s, n, 0.25), p75 = vt_percentile(s, n, 0.75);
  const double lower = p25 - 1.5 * (p75 - p25), upper = p75 + 1.5 * (p75 - p25);
  double cnt = 0.0, sum = 0.0;
  for (int i = tid; i < n; i += VT_THREADS) {
    const double v = (double)s[i];
    if (v > lower && v < upper) { cnt += 1.0; sum += v; }
  }
  cnt = block_tree(cnt, red, OpAdd());
  sum = block_tree(sum, red, OpAdd());
  const double mean = cnt > 0.0 ? sum / cnt : 0.0;
  double m2 = 0.0;
  for (int i = tid; i < n; i += VT_THREADS) {
    const double v = (double)s[i];
    if (v > lower && v < upper) m2 += (v - mean) * (v - mean);
  }
  m2 = block_tree(m2, red, OpAdd());
  if (tid == 0) { slot[0] = cnt; slot[1] = mean; slot[2] = cnt > 0.0 ? m2 : 0.0; slot[3] = 0.0; }
}

// Chan's update, slot after slot in utterance order: thread f owns feature f
__global__ __launch_bounds__(64) void k_vt_fit_merge(int B, const double* __restrict__ slots, VtState* __restrict__ st) {
  const int f = threadIdx.x;
  if (f >= 2) return;
  double n = st->count[f], mean = st->mean[f], m2 = st->m2[f];
  for (int b = 0; b < B; ++b) {
    const double* slot = slots + ((size_t)b * 2 + f) * (VT_SLOT_BYTES / 8);
    const double nb = slot[0];
    if (!(nb > 0.0)) continue;
    const double delta = slot[1] - mean, tot = n + nb;
    mean += delta * (nb / tot);
    m2 += slot[2] + delta * delta * (n * nb / tot);
    n = tot;
  }
  st->count[f] = n; st->mean[f] = mean; st->m2[f] = m2;
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_normalize(VtArgs a, const VtState* __restrict__ st, double* __restrict__ slots) {
  __shared__ double red[VT_THREADS];
  const int b = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const bool frame_level = (f ? a.energy_frame_level : a.pitch_frame_level) != 0;
  const int n = vt_count(a, b, frame_level);
  double mean = 0.0, sd = 1.0;  // "a numerical trick to avoid normalization" (preprocessor.py:96-105)
  if ((f ? a.energy_normalization : a.pitch_normalization) && st->count[f] > 0.0) {
    mean = st->mean[f];
    sd = sqrt(st->m2[f] / st->count[f]);  // StandardScaler.scale_: the population std, 1 for a constant feature
    if (sd == 0.0) sd = 1.0;
  }
  float* x = (f ? a.energy_targets : a.pitch_targets) + (size_t)b * (frame_level ? a.T : a.L);
  double mn = DBL_MAX, mx = -DBL_MAX;
  for (int i = tid; i < n; i += VT_THREADS) {
    const double y = ((double)x[i] - mean) / sd;
    x[i] = (float)y;
    mn = fmin(mn, y);
    mx = fmax(mx, y);
  }
  mn = block_tree(mn, red, OpMin());
  mx = block_tree(mx, red, OpMax());
  if (tid == 0) {
    double* slot = slots + ((size_t)b * 2 + f) * (VT_SLOT_BYTES / 8);
    slot[0] = mn; slot[1] = mx; slot[2] = 0.0; slot[3] = 0.0;
  }
}

__global__ __launch_bounds__(64) void k_vt_minmax_merge(int B, const double* __restrict__ slots, VtState* __restrict__ st) {
  const int f = threadIdx.x;
  if (f >= 2) return;
  double mn = st->min[f], mx = st->max[f];
  for (int b = 0; b < B; ++b) {
    const double* slot = slots + ((size_t)b * 2 + f) * (VT_SLOT_BYTES / 8);
    mn = fmin(mn, slot[0]);
    mx = fmax(mx, slot[1]);
  }
  st->min[f] = mn; st->max[f] = mx;
}

__global__ __launch_bounds__(64) void k_vt_state_init(VtState* __restrict__ st) {
  const int f = threadIdx.x;
  if (f >= 2) return;
  st->count[f] = 0.0; st->mean[f] = 0.0; st->m2[f] = 0.0;
  st->min[f] = DBL_MAX; st->max[f] = -DBL_MAX;  // np.finfo(np.float64).max / .min (preprocessor.py:300-301)
}

namespace {
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
}

size_t vt_ws_bytes(int B, int L, int T) {
  (void)L;
  const size_t b = B > 0 ? (size_t)B : 0, t = T > 0 ? (size_t)T : 0;
  return 256 + up256(b * t * sizeof(double)) + up256(b * t * sizeof(int)) + up256(b * 2 * VT_SLOT_BYTES);
}

hipError_t launch_vt_state_init(VtState* state, hipStream_t st) {
  hipLaunchKernelGGL(k_vt_state_init, dim3(1), dim3(64), 0, st, state);
  return hipGetLastError();
}

hipError_t launch_vt_targets(const VtArgs& a, void* ws, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  double* contour = (double*)ws;
  int* next = (int*)((char*)ws + up256((size_t)a.B * a.T * sizeof(double)));
  hipLaunchKernelGGL(k_vt_targets, dim3(a.B, 2), dim3(VT_THREADS), 0, st, a, contour, next);
  return hipGetLastError();
}

hipError_t launch_vt_fit(const VtArgs& a, VtState* state, void* ws, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vt_fit_partial, dim3(a.B, 2), dim3(VT_THREADS), 0, st, a, (double*)ws);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_vt_fit_merge, dim3(1), dim3(64), 0, st, a.B, (const double*)ws, state);
  return hipGetLastError();
}

hipError_t launch_vt_normalize(const VtArgs& a, VtState* state, void* ws, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_vt_normalize, dim3(a.B, 2), dim3(VT_THREADS), 0, st, a, (const VtState*)state, (double*)ws);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_vt_minmax_merge, dim3(1), dim3(64), 0, st, a.B, (const double*)ws, state);
  return hipGetLastError();
}

}  // namespace ns
