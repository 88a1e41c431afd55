// The wave-per-row LayerNorm of the transformer models (K20 Whisper, K25 TimeSformer, K26 CLIP, K27 nomic-embed-text, K29 AST),
// and the workgroup arg-max of the two classifier heads.  Included by whisper.hip, nomic.hip and probe/transformer_probe.hip,
// and through encoder.h by actions.hip, clip.hip and sounds.hip; everything here has internal linkage.
#pragma once

#include "gemm_f16.h"

namespace {

// the sum of v over the wave's 64 lanes, the same value in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Best { float v; int i; };

// The largest of s[0 .. n) and its index over a workgroup of 256 threads, the smaller index among equal values, the same pair
// in every thread: a strided scan per thread from (floor, 0x7fffffff), lanes joined by xor shuffles, the four waves through
// s_f / s_i [4].  Values below the floor and NaN are never picked; with nothing to pick the index stays 0x7fffffff.  The
// caller's next barrier frees s_f / s_i for the next call.
__device__ __forceinline__ Best block_argmax_256(const float* s, int n, float floor, float* s_f, int* s_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float bv = floor;
  int bi = 0x7fffffff;
  for (int j = threadIdx.x; j < n; j += 256) {
    const float v = s[j];
    if (v > bv || (v == bv && j < bi)) bv = v, bi = j;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
  }
  if (lane == 0) s_f[wave] = bv, s_i[wave] = bi;
  __syncthreads();
  bv = s_f[0], bi = s_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (s_f[w] > bv || (s_f[w] == bv && s_i[w] < bi)) bv = s_f[w], bi = s_i[w];
  return {bv, bi};
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
