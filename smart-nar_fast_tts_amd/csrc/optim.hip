// The optimiser half of the reference's training step: clip_grad_norm_, ScheduledOptim.step_and_update_lr's Adam.step() and
// zero_grad() (train.py:91-95, model/optimizer.py:10-15,24,28) over ~300 tensors as a fixed handful of launches, no host read, no
// float atomic.  The learning-rate schedule itself is host arithmetic (optim.py); lr arrives as a kernel argument.
//   k_opt_sumsq       one slot per chunk: the sum of squares of the chunk's gradient elements (0 for a skipped tensor)
//   k_opt_norm_final  one workgroup: adds the slots in a fixed order in float64, writes (norm64, total_norm, clip_coef)
//   k_opt_scale       g *= clip_coef                                         (the stand-alone clip_grad_norm_)
//   k_opt_adam        torch's _single_tensor_adam per element, optionally with the clip in front and zero_grad behind
//   k_opt_zero        g = 0                                                  (the stand-alone zero_grad)
// Chunk table: tensor i owns max(1, ceil(numel_i / OPT_CHUNK)) consecutive chunks; a workgroup takes chunks blockIdx.x,
// blockIdx.x + gridDim.x, ... and finds a chunk's tensor by bisecting the per-tensor prefix `chunk_begin` (wave-uniform: scalar
// loads), so no launch depends on the number of tensors.  Inside a chunk thread t owns the 16-byte groups t, t + 256, t + 512,
// t + 768 (elements 4 (t + 256 k) .. + 4): the same elements whether a tensor's pointer is 16-byte aligned (one vector access per
// group) or not (four scalar ones), so alignment changes no bit.  A group that crosses numel is accessed element by element.
// Reduction order of the norm: every square is exact in float64 (24 x 24 bits), a thread adds its <= 16 squares in element order,
// the wave adds in a wave64 shuffle tree, the four waves are added in wave order, then the slots in a fixed tree — float64
// throughout.  fp32 partial sums were tried first and left: on the tiny fixture the fp32 norm then sat one ulp from the correctly
// rounded one, the clip coefficient carried that into every g * coef, and exp_avg / exp_avg_sq of the one- to five-element tensors
// left their gates (shares 1.11 and 1.24).  The kernel is bound by its one read of g; the float64 adds cost nothing visible.
// A slot depends on its chunk alone — not on the grid, the stream or what the workspace held — so equal inputs give equal bits.
// Contraction is OFF for the whole file: every product is rounded before it is added, as the unfused tensor ops of torch round
// every intermediate.  That is also what makes the fused clip bitwise equal to k_opt_scale followed by the plain update: g * coef
// is rounded to the fp32 value k_opt_scale would have stored.
#include "kernels.h"

#pragma clang fp contract(off)

namespace ns {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the largest i >= lo with chunk_begin[i] <= c; chunk_begin is strictly increasing and chunk_begin[0] == 0
__device__ __forceinline__ int find_tensor(const OptTensor* __restrict__ table, int n_tensors, int c, int lo) {
  int hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].chunk_begin <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ f32x4 load4(const float* p, bool vec, int nvalid) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec && nvalid == 4) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nvalid) v[j] = p[j];
  return v;
}
__device__ __forceinline__ void store4(float* p, bool vec, int nvalid, f32x4 v) {
  if (vec && nvalid == 4) { *reinterpret_cast<f32x4*>(p) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nvalid) p[j] = v[j];
}
__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// elements of chunk c of tensor t, and its first element
__device__ __forceinline__ int chunk_extent(const OptTensor& t, int c, long long* e0) {
  *e0 = (long long)(c - t.chunk_begin) * OPT_CHUNK;
  const long long left = t.numel - *e0;
  return left < OPT_CHUNK ? (left < 0 ? 0 : (int)left) : OPT_CHUNK;
}

// b ** t for an integer t >= 1 by squaring, float64 (within a few float64 ulps of pow(); the result is rounded to fp32 afterwards)
__device__ __forceinline__ double ipow(double b, long long t) {
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}
}  // namespace

__global__ __launch_bounds__(OPT_THREADS) void k_opt_sumsq(const OptTensor* __restrict__ table, int n_tensors, int n_chunks,
                                                            double* __restrict__ slots) {
  __shared__ double part[OPT_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ti = 0;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    ti = find_tensor(table, n_tensors, c, ti);
    const OptTensor t = table[ti];
    double acc = 0.0;
    if (t.g) {
      long long e0;
      const int n = chunk_extent(t, c, &e0);
      const bool vec = aligned16(t.g);
#pragma unroll
      for (int k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); ++k) {
        const int i = 4 * (tid + OPT_THREADS * k);
        if (i >= n) break;
        const f32x4 g = load4(t.g + e0 + i, vec, n - i < 4 ? n - i : 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)g[j] * (double)g[j];
      }
    }
    const double s = wave_sum(acc);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) slots[c] = ((part[0] + part[1]) + part[2]) + part[3];  // every slot is written: the workspace needs no initialisation
    __syncthreads();
  }
}

// total_norm = sqrt(sum), clip_coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 as torch.nn.utils.clip_grad_norm_ computes it
// (clamp(max=1.0): a NaN norm gives a NaN coefficient, an infinite one gives 0)
__global__ __launch_bounds__(OPT_THREADS) void k_opt_norm_final(const double* __restrict__ slots, int n_chunks, float max_norm,
                                                                 OptRecord* __restrict__ record) {
  __shared__ double part[OPT_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n_chunks; i += OPT_THREADS) s += slots[i];  // thread i: slots i, i + 256, ... in slot order
  part[tid] = s;
  __syncthreads();
  for (int w = OPT_THREADS / 2; w >= 1; w >>= 1) {  // a fixed tree: thread i adds thread i + w
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const double norm = sqrt(part[0]);
    const float total = (float)norm;
    const float c = max_norm / (total + 1e-6f);
    record->norm64 = norm;
    record->total_norm = total;
    record->clip_coef = c > 1.0f ? 1.0f : c;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void k_opt_scale(const OptTensor* __restrict__ table, int n_tensors, int n_chunks,
                                                            const OptRecord* __restrict__ record) {
  const int tid = threadIdx.x;
  const float coef = record->clip_coef;
  int ti = 0;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    ti = find_tensor(table, n_tensors, c, ti);
    const OptTensor t = table[ti];
    if (!t.g) continue;
    long long e0;
    const int n = chunk_extent(t, c, &e0);
    const bool vec = aligned16(t.g);
#pragma unroll
    for (int k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); ++k) {
      const int i = 4 * (tid + OPT_THREADS * k);
      if (i >= n) break;
      const int nv = n - i < 4 ? n - i : 4;
      f32x4 g = load4(t.g + e0 + i, vec, nv);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = g[j] * coef;  // multiplied even when coef == 1, as torch does
      store4(t.g + e0 + i, vec, nv, g);
    }
  }
}

__global__ __launch_bounds__(OPT_THREADS) void k_opt_zero(const OptTensor* __restrict__ table, int n_tensors, int n_chunks) {
  const int tid = threadIdx.x;
  int ti = 0;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    ti = find_tensor(table, n_tensors, c, ti);
    const OptTensor t = table[ti];
    if (!t.g) continue;
    long long e0;
    const int n = chunk_extent(t, c, &e0);
    const bool vec = aligned16(t.g);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); ++k) {
      const int i = 4 * (tid + OPT_THREADS * k);
      if (i >= n) break;
      store4(t.g + e0 + i, vec, n - i < 4 ? n - i : 4, z);
    }
  }
}

// torch/optim/adam.py _single_tensor_adam, the non-capturable branch, per element:
//   grad = grad.add(param, alpha=weight_decay)                      (weight_decay != 0)
//   exp_avg.lerp_(grad, 1 - beta1)                                  m + (1 - beta1) * (g - m)   (weight < 0.5; else g - (g - m) * (1 - weight))
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)    v * beta2 + ((1 - beta2) * g) * g
//   step_size = lr / (1 - beta1 ** step)                            float64 scalars, rounded to fp32 where they meet the tensor
//   denom = (exp_avg_sq.sqrt() / (1 - beta2 ** step) ** 0.5).add_(eps)
//   param.addcdiv_(exp_avg, denom, value=-step_size)                p - (step_size * m) / denom
__global__ __launch_bounds__(OPT_THREADS) void k_opt_adam(const OptTensor* __restrict__ table, int n_tensors, int n_chunks, OptHyper h,
                                                           float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                           const OptRecord* __restrict__ record) {
  const int tid = threadIdx.x;
  const float coef = h.fuse_clip ? record->clip_coef : 1.0f;
  const float w1 = (float)(1.0 - h.beta1), b2 = (float)h.beta2, w2 = (float)(1.0 - h.beta2);
  const float eps = (float)h.eps, wd = (float)h.weight_decay;
  const bool lerp_low = w1 < 0.5f;
  const float w1c = 1.0f - w1;
  int ti = 0;
  long long step_of = -1;
  float step_size = 0.f, bc2_sqrt = 1.f;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    ti = find_tensor(table, n_tensors, c, ti);
    const OptTensor t = table[ti];
    if (!t.g) continue;
    long long e0;
    const int n = chunk_extent(t, c, &e0);
    long long step = h.global_step - t.lag;  // the tensor's own step count (torch keeps `step` per parameter)
    step = step < 1 ? 1 : step;
    if (step != step_of) {  // once per workgroup while the step count does not change
      step_of = step;
      step_size = (float)(h.lr / (1.0 - ipow(h.beta1, step)));
      bc2_sqrt = (float)sqrt(1.0 - ipow(h.beta2, step));
    }
    const bool vec_p = aligned16(t.p), vec_g = aligned16(t.g);
    float* mp = exp_avg + t.state_off + e0;
    float* vp = exp_avg_sq + t.state_off + e0;
#pragma unroll
    for (int k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); ++k) {
      const int i = 4 * (tid + OPT_THREADS * k);
      if (i >= n) break;
      const int nv = n - i < 4 ? n - i : 4;
      f32x4 p = load4(t.p + e0 + i, vec_p, nv);
      f32x4 g = load4(t.g + e0 + i, vec_g, nv);
      f32x4 m = load4(mp + i, true, nv);  // the arenas pad every tensor to a multiple of 4 floats
      f32x4 v = load4(vp + i, true, nv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gj = g[j];
        if (h.fuse_clip) gj = gj * coef;
        if (wd != 0.f) gj = gj + wd * p[j];
        const float d = gj - m[j];
        m[j] = lerp_low ? m[j] + w1 * d : gj - d * w1c;
        v[j] = v[j] * b2 + (w2 * gj) * gj;
        const float denom = sqrtf(v[j]) / bc2_sqrt + eps;
        p[j] = p[j] - (step_size * m[j]) / denom;
      }
      store4(t.p + e0 + i, vec_p, nv, p);
      store4(mp + i, true, nv, m);
      store4(vp + i, true, nv, v);
      if (h.zero_grads) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        store4(t.g + e0 + i, vec_g, nv, z);
      }
    }
  }
}

namespace {
inline unsigned opt_grid(int n_chunks) { return (unsigned)(n_chunks < OPT_MAX_GRID ? n_chunks : OPT_MAX_GRID); }
}  // namespace

hipError_t launch_opt_grad_norm(const OptTensor* table, int n_tensors, int n_chunks, float max_norm, double* slots, OptRecord* record,
                                hipStream_t st) {
  hipLaunchKernelGGL(k_opt_sumsq, dim3(opt_grid(n_chunks)), dim3(OPT_THREADS), 0, st, table, n_tensors, n_chunks, slots);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_opt_norm_final, dim3(1), dim3(OPT_THREADS), 0, st, (const double*)slots, n_chunks, max_norm, record);
  return hipGetLastError();
}

hipError_t launch_opt_scale(const OptTensor* table, int n_tensors, int n_chunks, const OptRecord* record, hipStream_t st) {
  hipLaunchKernelGGL(k_opt_scale, dim3(opt_grid(n_chunks)), dim3(OPT_THREADS), 0, st, table, n_tensors, n_chunks, record);
  return hipGetLastError();
}

hipError_t launch_opt_adam(const OptTensor* table, int n_tensors, int n_chunks, const OptHyper& h, float* exp_avg, float* exp_avg_sq,
                           const OptRecord* record, hipStream_t st) {
  hipLaunchKernelGGL(k_opt_adam, dim3(opt_grid(n_chunks)), dim3(OPT_THREADS), 0, st, table, n_tensors, n_chunks, h, exp_avg, exp_avg_sq, record);
  return hipGetLastError();
}

hipError_t launch_opt_zero(const OptTensor* table, int n_tensors, int n_chunks, hipStream_t st) {
  hipLaunchKernelGGL(k_opt_zero, dim3(opt_grid(n_chunks)), dim3(OPT_THREADS), 0, st, table, n_tensors, n_chunks);
  return hipGetLastError();
}

}  // namespace ns
