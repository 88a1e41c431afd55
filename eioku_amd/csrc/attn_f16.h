// The tiled MFMA attention of the transformer models with 64-wide heads (K25 TimeSformer's spatial attention, K26 CLIP, K27
// nomic-embed-text, K29 AST): one kernel, and per model a policy that says which rows of qkv form a sequence and where its
// outputs go.  Included by nomic.hip and probe/transformer_probe.hip, and through encoder.h by actions.hip, clip.hip and
// sounds.hip; everything here has internal linkage.
#pragma once

#include "common.h"
#include "gemm_f16.h"

#include <cmath>

namespace {

constexpr int kKC = 128;           // keys per LDS stage
constexpr int kKStride = 72;       // halfs per staged key row (64 + 8: 144 B, 16-byte aligned, spreads the banks)
constexpr int kVStride = kKC + 2;  // halfs per staged value column (65 words: a column starts one bank after its neighbour)

// ---- sequence policies --------------------------------------------------------------------------------------------------
// A policy is passed to the kernel by value and answers for the workgroup's sequence blockIdx.z: n() its number of tokens,
// row(tok) the token's row in qkv, out(q) the output row of query q (d = 64 heads halfs).

// sequence z = rows z n .. z n + n - 1; out [. n][d]
struct DenseSeq {
  int len, d;
  h16* o;
  __device__ int n() const { return len; }
  __device__ size_t row(int tok) const { return (size_t)blockIdx.z * len + tok; }
  __device__ h16* out(int q) const { return o + row(q) * d; }
};

// packed sequences: sequence z = rows cu[z] .. cu[z + 1] - 1; out [T][d].  A query tile starts at a multiple of 64 of its OWN
// sequence, so it never straddles two.
struct RaggedSeq {
  const int* cu;
  int d;
  h16* o;
  __device__ int n() const { return cu[blockIdx.z + 1] - cu[blockIdx.z]; }
  __device__ size_t row(int tok) const { return (size_t)cu[blockIdx.z] + tok; }
  __device__ h16* out(int q) const { return o + row(q) * d; }
};

// TimeSformer's stream order, problem z = (clip b, frame t) = (z / T, z % T): token 0 is the clip's CLS row B P T + b, token
// 1 + p the patch row (b P + p) T + t.  Patch outputs go to out_patch [B P T][d], the CLS output of frame t to out_cls [b T + t][d].
struct SpaceTimeSeq {
  int B, P, T, d;
  h16 *out_patch, *out_cls;
  __device__ int n() const { return 1 + P; }
  __device__ size_t row(int tok) const {
    const int b = blockIdx.z / T, t = blockIdx.z % T;
    return tok == 0 ? (size_t)B * P * T + b : ((size_t)b * P + tok - 1) * T + t;
  }
  __device__ h16* out(int q) const { return q == 0 ? out_cls + (size_t)blockIdx.z * d : out_patch + row(q) * d; }  // z = b T + t
};

// ---- the kernel -----------------------------------------------------------------------------------------------------------
// qkv [rows][3 d] fp16 (q | k | v, head h in columns 64 h .. 64 h + 63 of each third).  grid (ceil(longest n / 64), heads,
// sequences), 4 waves of 16 queries; a workgroup whose first query is at or past its sequence's length leaves before any
// barrier.  Keys and values go through LDS kKC at a time (keys [key][72], values transposed [dim][kKC + 2]); the workgroup
// stages keys up to its last query (CAUSAL) or n.  Per 32 keys and wave: S^T = K Q^T in two 16-key MFMA tiles (lane (r, u):
// query r, keys 4u .. 4u + 3 of each tile), the online softmax per query across the lanes r, r + 16, r + 32, r + 48, then O^T
// += V^T P^T with the 32 keys in the order the lanes already hold them (slot 8u + t: key 4u + t of the first tile, slot 8u + 4
// + t: of the second), p = exp(s - max) rounded to fp16.  Keys at or past the end score -inf before the running maximum; groups
// start at multiples of 32 below the end, so every visited 32-key group holds a live key.  CAUSAL: key > query scores -inf
// too, and a wave stops after the 32-key group that holds its last query's key.  A wave's queries start at a multiple of 16
// and groups at multiples of 32, so every group a wave visits starts at or before each of its queries: no query ever sees a
// group of masked keys only.
template <class Seq, bool CAUSAL>
__global__ __launch_bounds__(256) void k_attn_tiles(const h16* __restrict__ qkv, Seq seq, int heads) {
  __shared__ __align__(16) h16 sk[kKC * kKStride];
  __shared__ __align__(16) h16 svt[64 * kVStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, u = lane >> 4;
  const int head = blockIdx.y;
  const int d = heads * 64, n = seq.n();
  const size_t ld = (size_t)3 * d;
  if ((int)blockIdx.x * 64 >= n) return;
  const int q = blockIdx.x * 64 + wave * 16 + r;  // this lane's query token
  half8 q0 = {}, q1 = {};
  if (q < n) {
    const h16* qr = qkv + seq.row(q) * ld + head * 64 + 8 * u;
    q0 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(qr));
    q1 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(qr + 32));
  }
  int kend_wg = n, kend_wave = n;  // one past the last key the workgroup stages / this wave scores
  if (CAUSAL) {
    const int last_wg = blockIdx.x * 64 + 63, last_wave = blockIdx.x * 64 + wave * 16 + 15;
    kend_wg = last_wg < n - 1 ? last_wg + 1 : n;
    kend_wave = last_wave < n - 1 ? last_wave + 1 : n;
  }
  float4v acc[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc[f] = float4v{0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, sum = 0.f;  // sum: this lane's share, joined over u at the end
  for (int k0 = 0; k0 < kend_wg; k0 += kKC) {
    const int nk = kend_wg - k0 < kKC ? kend_wg - k0 : kKC, nk32 = (nk + 31) & ~31;
    __syncthreads();  // the previous stage has been read
    for (int i = threadIdx.x; i < nk32 * 8; i += 256) {
      const int piece = i & 7, key = i >> 3;
      uint4 kv = {0, 0, 0, 0}, vv = {0, 0, 0, 0};  // keys past the end: zeros (masked below; 0 * value adds nothing)
      if (key < nk) {
        const h16* row = qkv + seq.row(k0 + key) * ld + head * 64 + piece * 8;
        kv = *reinterpret_cast<const uint4*>(row + d);
        vv = *reinterpret_cast<const uint4*>(row + 2 * d);
      }
      *reinterpret_cast<uint4*>(sk + key * kKStride + piece * 8) = kv;
      const half8 vh = __builtin_bit_cast(half8, vv);
#pragma unroll
      for (int e = 0; e < 8; ++e) svt[(piece * 8 + e) * kVStride + key] = vh[e];
    }
    __syncthreads();
    for (int j0 = 0; j0 < nk32 && (!CAUSAL || k0 + j0 < kend_wave); j0 += 32) {
      float4v s[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const h16* kr = sk + (j0 + 16 * e + r) * kKStride + 8 * u;
        const half8 ka = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(kr));
        const half8 kb = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(kr + 32));
        s[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, q0, float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        s[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kb, q1, s[e], 0, 0, 0);
      }
      float m_new = mx;
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = j0 + 16 * e + 4 * u + i;
          const bool seen = key < nk && (!CAUSAL || k0 + key <= q);
          s[e][i] = seen ? s[e][i] * 0.125f : -INFINITY;
          m_new = fmaxf(m_new, s[e][i]);
        }
      m_new = fmaxf(m_new, __shfl_xor(m_new, 16, 64));
      m_new = fmaxf(m_new, __shfl_xor(m_new, 32, 64));  // finite from the first 32 keys on: key 0 is never masked
      const float alpha = expf(mx - m_new);
      mx = m_new;
      half8 p;
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const h16 ph = (h16)expf(s[e][i] - m_new);
          p[4 * e + i] = ph;
          ps += (float)ph;
        }
      sum = sum * alpha + ps;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const h16* vr = svt + (16 * f + r) * kVStride + j0 + 4 * u;
        const unsigned* va = reinterpret_cast<const unsigned*>(vr);  // 4-byte aligned: kVStride, j0 and 4u are even
        const uint4 v4 = {va[0], va[1], va[8], va[9]};
        acc[f] = acc[f] * alpha;
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, v4), p, acc[f], 0, 0, 0);
      }
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (q >= n) return;
  h16* o = seq.out(q) + head * 64 + 4 * u;
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[16 * f + i] = (h16)(acc[f][i] / sum);
}

// `sequences` problems of at most `longest` tokens each
template <bool CAUSAL, class Seq>
int launch_attn(hipStream_t st, const h16* qkv, const Seq& seq, int longest, int heads, int sequences) {
  hipLaunchKernelGGL((k_attn_tiles<Seq, CAUSAL>), dim3((longest + 63) / 64, heads, sequences), dim3(256), 0, st, qkv, seq, heads);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // namespace
