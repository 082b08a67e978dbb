// The guided-attention weight of FastSpeech2Loss (model/loss.py:19,60-65,104-108), shared by the forward (loss.hip) and the backward
// (lossgrad.hip): one definition, so both see the same W bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace ns {

constexpr float GA_TWO_SIGMA_SQ = 0.08f;  // 2 * sigma ** 2, sigma = 0.2 (model/loss.py:19,107); torch divides the fp32 tensor by this scalar
constexpr double GA_ALPHA = 10.0;         // model/loss.py:19,65

__device__ __forceinline__ int clamp_len(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// W[t, l] = 1 - exp(-((l / ilen - t / olen) ** 2) / (2 * sigma ** 2)), fp32, the reference's operation order (model/loss.py:104-108)
__device__ __forceinline__ float guide(int t, int l, float ilen, float olen) {
  const float d = (float)l / ilen - (float)t / olen;
  return 1.0f - expf(-(d * d) / GA_TWO_SIGMA_SQ);
}

}  // namespace ns
