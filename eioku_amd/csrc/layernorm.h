// The wave-per-row LayerNorm of the transformer models (K20 Whisper, K25 TimeSformer, K26 CLIP, K27 nomic-embed-text).
// Included by whisper.hip, actions.hip, clip.hip, nomic.hip and sounds.hip; everything here has internal linkage.
#pragma once

#include "gemm_f16.h"

namespace {

// the sum of v over the wave's 64 lanes, the same value in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct RowStats { float mean, inv; };

// mean and 1 / sqrt(variance + eps) of the d values x(0) .. x(d - 1), by one wave: lane-strided sums joined by wave_sum, the
// mean first, then the centred sum of squares
template <class Load>
__device__ __forceinline__ RowStats row_stats(int lane, int d, float eps, Load x) {
  float s = 0.f;
  for (int i = lane; i < d; i += 64) s += x(i);
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float c = x(i) - mean;
    q += c * c;
  }
  return {mean, 1.f / sqrtf(wave_sum(q) / (float)d + eps)};
}

// LayerNorm: fp32 row -> OUT (fp16 or fp32), one wave per row; pick != nullptr: output row r is the norm of x row pick[r]
template <typename OUT>
__global__ __launch_bounds__(256) void k_ln(const float* __restrict__ x, int M, int d, const float* __restrict__ g,
                                            const float* __restrict__ b, float eps, const int* __restrict__ pick, OUT* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (size_t)(pick ? pick[row] : row) * d;
  const RowStats st = row_stats(lane, d, eps, [&](int i) { return xr[i]; });
  for (int i = lane; i < d; i += 64) out[(size_t)row * d + i] = (OUT)((xr[i] - st.mean) * st.inv * g[i] + b[i]);
}

}  // namespace
