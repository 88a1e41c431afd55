// The fp16 GEMM of the transformer models (K20 Whisper, K25 TimeSformer, K26 CLIP, K27 nomic-embed-text, K29 AST): C = A . W^T
// on v_mfma_f32_16x16x32_f16 with fused epilogues, and its one launcher.  The models' other shared parts sit next to it:
// layernorm.h (the wave-per-row LayerNorm), attn_f16.h (the tiled MFMA attention and its sequence policies), tensors.h (the
// named-tensor table behind *_num_tensors / *_tensor_info / *_set_tensor) and encoder.h (the pre-LN layer's host side).
// Included by whisper.hip, nomic.hip and probe/transformer_probe.hip, and through encoder.h by actions.hip, clip.hip and
// sounds.hip; everything here has internal linkage.
#pragma once

#include "common.h"

#include <cstddef>
#include <cstdint>

namespace {

typedef _Float16 h16;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

// ---- GEMM ---------------------------------------------------------------------------------------------------------------
enum { EPI_F16 = 0, EPI_GELU_F16 = 1, EPI_RESID = 2, EPI_GELU_POS = 3, EPI_F32 = 4, EPI_POS = 5, EPI_QGELU_F16 = 6, EPI_ROPE_F16 = 7,
       EPI_SWIGLU_F16 = 8 };

__device__ __forceinline__ float gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float quick_gelu(float v) { return v / (1.f + expf(-1.702f * v)); }  // v * sigmoid(1.702 v)

// out[m][n] = epi(sum_k A[m][k] W[n][k] + bias[n]).  grid (ceil(N / 64), ceil(M / (16 MT))), 4 waves: wave w owns weight
// rows n0 = 64 bx + 16 w .. + 15.  MFMA 16x16x32: A operand = weight rows (lane (r, u): row r, k 8u .. 8u + 7), B operand =
// activation rows; lane holds D[n0 + 4u + t][m0 + r].  K % 32 == 0, lda / ldw % 8 == 0.  Each output element is one
// k-ordered sum whatever M is, so a lane's result does not depend on the batch around it.
//   EPI_F16      out fp16 [m * ldc + n]            EPI_GELU_F16  the same after GELU
//   EPI_RESID    out fp32 [m * ldc + n] += value   EPI_GELU_POS  out fp32 = GELU(value) + pos[m % pos_rows][n]
//   EPI_F32      out fp32 [m * ldc + n] = value    EPI_POS       out fp32 = value + pos[m % pos_rows][n]
//   EPI_QGELU_F16  out fp16 after v * sigmoid(1.702 v) (CLIP's quick_gelu)
// The two pair epilogues work on the four consecutive weight rows n .. n + 3 a lane holds (N % 16 == 0, ldc % 4 == 0, no bias),
// which the caller has stored so that rows 2p and 2p + 1 belong together; row_pos is read by EPI_ROPE_F16 alone (else NULL):
//   EPI_ROPE_F16   packed q | k | v, N = 3 d: within each 64-row head of q and k, stored row 2j is the head's dimension j and
//                  stored row 2j + 1 its dimension j + 32, the two partners of rotate_half.  Rows n < 2 N / 3 are rotated in
//                  fp32 by the angle of (row_pos[m], j): pos is a [pos_rows][64] table, cos in columns 0 .. 31 and sin in 32 ..
//                  63; out fp16 [m * ldc + n] in the stored order (q . k does not depend on a permutation both carry), one
//                  rounding.  Rows n >= 2 N / 3 (v) are written as EPI_F16 writes them.
//   EPI_SWIGLU_F16 N = 2 F: stored row 2i is gate row i, 2i + 1 up row i; out fp16 [m * ldc + i] = silu(gate) * up, in fp32
template <int MT, int EPI>
__global__ __launch_bounds__(256) void k_gemm(const h16* __restrict__ A, int lda, const h16* __restrict__ W, int ldw,
                                              const float* __restrict__ bias, int M, int N, int K, void* __restrict__ out,
                                              long long ldc, const float* __restrict__ pos, int pos_rows,
                                              const int* __restrict__ row_pos) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, u = lane >> 4;
  const int n0 = (blockIdx.x * 4 + wave) * 16, m0 = blockIdx.y * 16 * MT;
  if (n0 >= N) return;
  const bool wl = n0 + r < N;
  const h16* wr = W + (size_t)(wl ? n0 + r : 0) * ldw + 8 * u;
  const h16* ar[MT];
  bool al[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int mm = m0 + 16 * i + r;
    al[i] = mm < M;
    ar[i] = A + (size_t)(al[i] ? mm : 0) * lda + 8 * u;
  }
  float4v acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = float4v{0.f, 0.f, 0.f, 0.f};
  const half8 zero = {};
  for (int k = 0; k < K; k += 32) {
    const half8 w = wl ? __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(wr + k)) : zero;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const half8 a = al[i] ? __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(ar[i] + k)) : zero;
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, a, acc[i], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int mm = m0 + 16 * i + r;
    if (mm >= M) continue;
    if (EPI == EPI_ROPE_F16) {  // n0 and 2 N / 3 are multiples of 16: a wave is all q / k or all v
      const int n = n0 + 4 * u;
      float4v v = acc[i];
      if (n0 < N / 3 * 2) {
        const float* cs = pos + (size_t)row_pos[mm] * 64 + ((n & 63) >> 1);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const float c = cs[p], s = cs[32 + p], lo = acc[i][2 * p], hi = acc[i][2 * p + 1];
          v[2 * p] = lo * c - hi * s;
          v[2 * p + 1] = hi * c + lo * s;
        }
      }
      typedef _Float16 half4 __attribute__((ext_vector_type(4)));
      const half4 h = {(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
      *reinterpret_cast<half4*>(reinterpret_cast<h16*>(out) + (size_t)mm * (size_t)ldc + n) = h;
      continue;
    }
    if (EPI == EPI_SWIGLU_F16) {
      typedef _Float16 half2v __attribute__((ext_vector_type(2)));
      half2v h;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float g = acc[i][2 * p];
        h[p] = (h16)(g / (1.f + expf(-g)) * acc[i][2 * p + 1]);
      }
      *reinterpret_cast<half2v*>(reinterpret_cast<h16*>(out) + (size_t)mm * (size_t)ldc + ((n0 + 4 * u) >> 1)) = h;
      continue;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + 4 * u + t;
      if (n >= N) continue;
      const float v = acc[i][t] + (bias ? bias[n] : 0.f);
      const size_t o = (size_t)mm * (size_t)ldc + n;
      if (EPI == EPI_F16) reinterpret_cast<h16*>(out)[o] = (h16)v;
      if (EPI == EPI_GELU_F16) reinterpret_cast<h16*>(out)[o] = (h16)gelu(v);
      if (EPI == EPI_RESID) reinterpret_cast<float*>(out)[o] += v;
      if (EPI == EPI_GELU_POS) reinterpret_cast<float*>(out)[o] = gelu(v) + pos[(size_t)(mm % pos_rows) * N + n];
      if (EPI == EPI_F32) reinterpret_cast<float*>(out)[o] = v;
      if (EPI == EPI_POS) reinterpret_cast<float*>(out)[o] = v + pos[(size_t)(mm % pos_rows) * N + n];
      if (EPI == EPI_QGELU_F16) reinterpret_cast<h16*>(out)[o] = (h16)quick_gelu(v);
    }
  }
}

// The launch of k_gemm<MT, EPI> with the alignment the kernel assumes checked; *flops grows by 2 M N K.  M == 0 launches nothing.
template <int MT, int EPI>
int launch_gemm(hipStream_t st, const h16* A, int lda, const h16* W, int ldw, const float* bias, int M, int N, int K, void* out,
                long long ldc, const float* pos, int pos_rows, const int* row_pos, double* flops) {
  EIOKU_REQUIRE(K % 32 == 0 && lda % 8 == 0 && ldw % 8 == 0, "GEMM K %d / lda %d / ldw %d misaligned", K, lda, ldw);
  if (EPI == EPI_ROPE_F16 || EPI == EPI_SWIGLU_F16)
    EIOKU_REQUIRE(N % 16 == 0 && ldc % 4 == 0, "GEMM K %d / N %d / ldc %lld misaligned", K, N, ldc);
  if (M == 0) return EIOKU_OK;
  const dim3 grid((N + 63) / 64, (M + 16 * MT - 1) / (16 * MT));
  hipLaunchKernelGGL((k_gemm<MT, EPI>), grid, dim3(256), 0, st, A, lda, W, ldw, bias, M, N, K, out, ldc, pos, pos_rows, row_pos);
  *flops += 2.0 * M * N * K;
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // namespace
