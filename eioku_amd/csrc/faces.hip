// K13 / K14: face clustering - ArcFace (insightface arcface_torch IResNet) embeddings and cosine DBSCAN.
//
// Fills the "cluster_id" field that face detection returns (eioku_amd/faces.py, ModelManager.detect_faces with
// cluster_faces).  On the device:
//   k_face_crop      K13a: a square of side max(w, h, 1) centred on each box, bilinear to 112 x 112 at pixel centres,
//                    outside-frame samples 0.  Tap positions / weights come from the host (float64, 11-bit fixed
//                    point); the kernel is integer only (u8 result, rounded), then arcface_torch's (v / 255 - 0.5) / 0.5
//                    in fp32 -> fp16 NHWC8 (R, G, B, 5 zero channels)
//   k_face_warp      K13c: the aligned crop - cv2.warpAffine(frame, M, (112, 112), INTER_LINEAR, borderValue = 0) in
//                    OpenCV's fixed point (M inverted in float64 without FMA contraction, coordinates in 1/1024 rounded
//                    to 1/32, four taps with 5-bit weights), then K13a's normalisation and output format.  M is the
//                    similarity transform of the detector's five landmarks onto ArcFace's template (faces.py)
//   the IBasicBlocks K13b: K4's 3x3 kernels (conv.hip) with BatchNorm folded into each conv that precedes it; the 1x1 / s2
//                    downsample as the centre tap of a 3x3 / s2 (as resnet.hip).  Two things do not fold: the block's
//                    leading bn1 sits before a zero-padded conv (folding its shift is wrong on the border), and PReLU
//                    has per-channel slopes - both run in k_chan_ops (the stem's PReLU and block 0's bn1 in one pass)
//   k_face_fc        bn2 -> flatten -> fc -> features (BatchNorm1d), folded on the host into one fp16-weight GEMM
//                    (weight columns in NHWC order) on v_mfma_f32_16x16x32_f16, split over K in fixed slices
//   k_face_norm      the K slices summed in slice order + bias, L2 normalisation -> fp32 [m][512]
//   k_gram_bits      K14: f32 Gram tiles on v_mfma_f32_32x32x2_f32 (fixed summation order: bit-stable), neighbour
//                    bitmask of 1 - e_i.e_j <= eps (a point is always its own neighbour)
//   k_row_counts ... k_border   core flags, connected components of the core-core graph by lock-free union-find
//                    (hooks always point to the smaller index, so a component's root is its smallest core index),
//                    a one-workgroup prefix sum numbers the roots in index order, border points take the smallest
//                    label among their core neighbours - scikit-learn's DBSCAN labels exactly
// Numerics of the embedder: fp16 storage, fp32 accumulation (the detector's arithmetic, as K11).
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "convnet.h"

using namespace eioku;

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float16v __attribute__((ext_vector_type(16)));

constexpr int kCrop = 112;
constexpr int kTapBits = 11;  // bilinear weights in 1/2048: w0 + w1 = 2048, products 2^22
constexpr int kFeat = 512;
constexpr int kFcK = 7 * 7 * 512;
constexpr int kFcSplit = 16;                // K slices of the head GEMM: 25088 = 16 x 49 x 32
constexpr int kFcSlice = kFcK / kFcSplit;   // 1568
constexpr int kChunk = 256;                 // faces per network pass (activations: ~8 MB per face)

// ---- K13a: crop + resample + normalise ----------------------------------------------------------------------------
// taps [m][2][112][2] int32: (first source index, weight of the second tap in 1/2048) for x then y; slot [m]
__global__ __launch_bounds__(256) void k_face_crop(const uint8_t* __restrict__ bgr, int h, int w, const int* __restrict__ slot,
                                                   const int* __restrict__ taps, int m, __half* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)m * kCrop * kCrop) return;
  const int ox = (int)(i % kCrop), oy = (int)((i / kCrop) % kCrop), c = (int)(i / (kCrop * kCrop));
  const int* tx = taps + (size_t)c * 4 * kCrop;
  const int* ty = tx + 2 * kCrop;
  const int x0 = tx[2 * ox], wx1 = tx[2 * ox + 1], y0 = ty[2 * oy], wy1 = ty[2 * oy + 1];
  const uint8_t* f = bgr + (size_t)slot[c] * h * w * 3;
  int acc0 = 1 << (2 * kTapBits - 1), acc1 = acc0, acc2 = acc0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int yy = y0 + dy, wy = dy ? wy1 : (1 << kTapBits) - wy1;
    if ((unsigned)yy >= (unsigned)h || wy == 0) continue;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int xx = x0 + dx, wx = dx ? wx1 : (1 << kTapBits) - wx1;
      if ((unsigned)xx >= (unsigned)w || wx == 0) continue;
      const uint8_t* p = f + ((size_t)yy * w + xx) * 3;
      const int k = wy * wx;
      acc0 += k * p[0];
      acc1 += k * p[1];
      acc2 += k * p[2];
    }
  }
  const int b = acc0 >> (2 * kTapBits), g = acc1 >> (2 * kTapBits), r = acc2 >> (2 * kTapBits);
  half8 v;
  v[0] = (_Float16)(((float)r / 255.0f - 0.5f) / 0.5f);
  v[1] = (_Float16)(((float)g / 255.0f - 0.5f) / 0.5f);
  v[2] = (_Float16)(((float)b / 255.0f - 0.5f) / 0.5f);
#pragma unroll
  for (int j = 3; j < 8; ++j) v[j] = (_Float16)0.f;
  *reinterpret_cast<uint4*>(out + (size_t)i * 8) = __builtin_bit_cast(uint4, v);
}

// ---- K13c: warpAffine onto the 112 x 112 template + normalise --------------------------------------------------------
// round-half-to-even to int32, saturating; NaN -> 0 (defined for every double, and restated so by the oracle)
__device__ __forceinline__ int rne_i32(double v) {
  v = rint(v);
  if (!(v == v)) return 0;
  return (int)fmin(fmax(v, -2147483648.0), 2147483647.0);
}

// OpenCV's own inversion of the 2 x 3 matrix (imgproc/imgwarp.cpp, warpAffine without WARP_INVERSE_MAP): every product
// and sum is rounded on its own.  The pragma takes the `contract` flag off the operations of this function, so they stay
// separate v_mul_f64 / v_add_f64 wherever it is inlined (hipcc's default is -ffp-contract=fast).
__device__ __forceinline__ void warp_invert(const double* __restrict__ m, double* __restrict__ o) {
#pragma clang fp contract(off)
  double M0 = m[0], M1 = m[1], M2 = m[2], M3 = m[3], M4 = m[4], M5 = m[5];
  double D = M0 * M4 - M1 * M3;
  D = D != 0 ? 1.0 / D : 0.0;
  const double A11 = M4 * D, A22 = M0 * D;
  M0 = A11;
  M1 *= -D;
  M3 *= -D;
  M4 = A22;
  const double b1 = -M0 * M2 - M1 * M5, b2 = -M3 * M2 - M4 * M5;
  o[0] = M0; o[1] = M1; o[2] = b1; o[3] = M3; o[4] = M4; o[5] = b2;
}

// source position of output pixel (x, y) in 1/32 pixels: (X0 + adelta[x]) >> 5 of OpenCV's WarpAffineInvoker
__device__ __forceinline__ void warp_coord(const double* __restrict__ inv, int x, int y, long long* X, long long* Y) {
#pragma clang fp contract(off)
  const int adelta = rne_i32(inv[0] * x * 1024.0), bdelta = rne_i32(inv[3] * x * 1024.0);
  const int X0 = rne_i32((inv[1] * y + inv[2]) * 1024.0), Y0 = rne_i32((inv[4] * y + inv[5]) * 1024.0);
  *X = ((long long)X0 + 16 + adelta) >> 5;
  *Y = ((long long)Y0 + 16 + bdelta) >> 5;
}

// grid (ceil(112 * 112 / 256), m): one grid row per face, so the face's slot, flag and matrix are uniform in a workgroup.
// mats [m][6] float64 (the forward matrix M: frame -> crop); use_box (optional) [m]: non-zero = this face keeps the crop
// K13a wrote
__global__ __launch_bounds__(256) void k_face_warp(const uint8_t* __restrict__ bgr, int h, int w, const int* __restrict__ slot,
                                                   const double* __restrict__ mats, const int* __restrict__ use_box,
                                                   __half* __restrict__ out) {
  const int c = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= kCrop * kCrop || (use_box && use_box[c])) return;
  const int ox = p % kCrop, oy = p / kCrop;
  double inv[6];
  warp_invert(mats + (size_t)6 * c, inv);
  long long X, Y;
  warp_coord(inv, ox, oy, &X, &Y);
  const int sx = (int)min(max(X >> 5, -32768ll), 32767ll), sy = (int)min(max(Y >> 5, -32768ll), 32767ll);
  const int fx = (int)(X & 31), fy = (int)(Y & 31);
  const uint8_t* f = bgr + (size_t)slot[c] * h * w * 3;
  int acc0 = 512, acc1 = 512, acc2 = 512;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int yy = sy + dy, wy = dy ? fy : 32 - fy;
    if ((unsigned)yy >= (unsigned)h) continue;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int xx = sx + dx, wx = dx ? fx : 32 - fx;
      if ((unsigned)xx >= (unsigned)w) continue;
      const uint8_t* q = f + ((size_t)yy * w + xx) * 3;
      const int k = wy * wx;
      acc0 += k * q[0];
      acc1 += k * q[1];
      acc2 += k * q[2];
    }
  }
  const int b = acc0 >> 10, g = acc1 >> 10, r = acc2 >> 10;
  half8 v;
  v[0] = (_Float16)(((float)r / 255.0f - 0.5f) / 0.5f);
  v[1] = (_Float16)(((float)g / 255.0f - 0.5f) / 0.5f);
  v[2] = (_Float16)(((float)b / 255.0f - 0.5f) / 0.5f);
#pragma unroll
  for (int j = 3; j < 8; ++j) v[j] = (_Float16)0.f;
  *reinterpret_cast<uint4*>(out + ((size_t)c * kCrop * kCrop + p) * 8) = __builtin_bit_cast(uint4, v);
}

// ---- per-channel passes over NHWC fp16 (C % 8 == 0) -----------------------------------------------------------------
// v = in; with `slope`: v = PReLU(v) -> fp16 -> out_act (may alias in); with `scale`: fp16(fp16(v) * scale + shift) -> out_bn
__global__ __launch_bounds__(256) void k_chan_ops(const __half* in, long long pixels, int C, const float* __restrict__ slope,
                                                  __half* out_act, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, __half* __restrict__ out_bn) {
  const int C8 = C / 8;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels * C8) return;
  const int c0 = (int)(i % C8) * 8;
  const uint4 raw = *reinterpret_cast<const uint4*>(in + (size_t)i * 8);
  half8 v = __builtin_bit_cast(half8, raw);
  if (slope) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = (float)v[j];
      float p = x * slope[c0 + j];
      // The product stays an fp32 value of its own.  Left to itself the compiler selects v_fma_mixlo_f16 (x * slope + 0.0 rounded
      // to fp16) for the multiply and the conversion together: the added +0 turns a -0 product into +0, and the sum is rounded
      // once, not to fp32 and then to fp16 (tests/test_convnet_glue_gpu.py found both).
      asm volatile("" : "+v"(p));
      v[j] = (_Float16)(x > 0.f ? x : p);
    }
    if (out_act) *reinterpret_cast<uint4*>(out_act + (size_t)i * 8) = __builtin_bit_cast(uint4, v);
  }
  if (out_bn) {
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)((float)v[j] * scale[c0 + j] + shift[c0 + j]);
    *reinterpret_cast<uint4*>(out_bn + (size_t)i * 8) = __builtin_bit_cast(uint4, o);
  }
}

// ---- head: partial[s][face][o] = sum over K slice s of W[o][k] * X[face][k] ------------------------------------------
// grid (512 / 64, ceil(m / 16), kFcSplit), 4 waves: wave w owns outputs 64 bx + 16 w .. + 15 for faces 16 by .. + 15.
// MFMA 16x16x32: A = weight rows (lane (r, u): row r, k 8u .. 8u + 7), B = face rows; lane holds D[4u + t][r].
__global__ __launch_bounds__(256) void k_face_fc(const __half* __restrict__ x, int m, const __half* __restrict__ wt,
                                                 float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, u = lane >> 4;
  const int o0 = blockIdx.x * 64 + wave * 16, f0 = blockIdx.y * 16, s = blockIdx.z;
  const int face = f0 + r;
  const bool live = face < m;
  const __half* wr = wt + (size_t)(o0 + r) * kFcK + (size_t)s * kFcSlice + 8 * u;
  const __half* xr = x + (size_t)(live ? face : 0) * kFcK + (size_t)s * kFcSlice + 8 * u;
  float4v acc = {0.f, 0.f, 0.f, 0.f};
  const half8 zero = {};
#pragma unroll 7
  for (int k = 0; k < kFcSlice; k += 32) {
    const half8 a = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(wr + k));
    const half8 b = live ? __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(xr + k)) : zero;
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
  }
  if (live)
    *reinterpret_cast<float4*>(partial + ((size_t)s * m + face) * kFeat + o0 + 4 * u) = float4{acc[0], acc[1], acc[2], acc[3]};
}

// one workgroup per face: slices summed in order, + bias, / max(||v||, 1e-12)
__global__ __launch_bounds__(256) void k_face_norm(const float* __restrict__ partial, int m, const float* __restrict__ bias,
                                                   float* __restrict__ out) {
  __shared__ float red[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  float v[2];
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int o = tid + 256 * t;
    float a = 0.f;
    for (int s = 0; s < kFcSplit; ++s) a += partial[((size_t)s * m + f) * kFeat + o];
    v[t] = a + bias[o];
    ss += v[t] * v[t];
  }
  ss = wave_reduce_add(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float nrm = fmaxf(sqrtf((red[0] + red[1]) + (red[2] + red[3])), 1e-12f);
#pragma unroll
  for (int t = 0; t < 2; ++t) out[(size_t)f * kFeat + tid + 256 * t] = v[t] / nrm;
}

// ---- K14: DBSCAN -------------------------------------------------------------------------------------------------
// Gram tile 128 x 128 per workgroup (4 waves in 2 x 2, each 64 x 64 = 2 x 2 blocks of 32 x 32), K in chunks of 32 through
// LDS.  MFMA 32x32x2 f32: lane l supplies A[l & 31][l >> 5], B[l >> 5][l & 31]; accumulator t of lane l is
// D[8 (t / 4) + 4 (l / 32) + t % 4][l & 31].  A ballot over a register gives two 32-bit words of the bitmask: rows
// i and i + 4 of one 32-column block.  adj [n][words] u32, bit j % 32 of word j / 32.
constexpr int kGT = 128, kGK = 32, kGP = kGK + 1;
__global__ __launch_bounds__(256) void k_gram_bits(const float* __restrict__ e, int n, int d, float eps, int words,
                                                   unsigned* __restrict__ adj) {
  __shared__ float sa[kGT * kGP];
  __shared__ float sb[kGT * kGP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int row0 = blockIdx.y * kGT, col0 = blockIdx.x * kGT;
  float16v acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[a][b][t] = 0.f;
  for (int k0 = 0; k0 < d; k0 += kGK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q, rr = idx >> 3, c4 = (idx & 7) * 4;
      float4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (row0 + rr < n) va = *reinterpret_cast<const float4*>(e + (size_t)(row0 + rr) * d + k0 + c4);
      if (col0 + rr < n) vb = *reinterpret_cast<const float4*>(e + (size_t)(col0 + rr) * d + k0 + c4);
      float* pa = sa + rr * kGP + c4;
      float* pb = sb + rr * kGP + c4;
      pa[0] = va.x; pa[1] = va.y; pa[2] = va.z; pa[3] = va.w;
      pb[0] = vb.x; pb[1] = vb.y; pb[2] = vb.z; pb[3] = vb.w;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kGK; k += 2) {
      float fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) fa[a] = sa[(wr * 64 + a * 32 + (lane & 31)) * kGP + k + (lane >> 5)];
#pragma unroll
      for (int b = 0; b < 2; ++b) fb[b] = sb[(wc * 64 + b * 32 + (lane & 31)) * kGP + k + (lane >> 5)];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int cblk = col0 + wc * 64 + b * 32;  // first column of the 32-column block
    if (cblk >= n) continue;
    const int j = cblk + (lane & 31);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int i = row0 + wr * 64 + a * 32 + 8 * (t >> 2) + 4 * (lane >> 5) + (t & 3);
        const bool nb = j < n && (i == j || 1.0f - acc[a][b][t] <= eps);
        const unsigned long long bits = __builtin_amdgcn_ballot_w64(nb);
        if (lane == 0) {
          const int ia = i;  // lane 0: l / 32 = 0; the upper half of the ballot is row ia + 4
          if (ia < n) adj[(size_t)ia * words + (cblk >> 5)] = (unsigned)bits;
          if (ia + 4 < n) adj[(size_t)(ia + 4) * words + (cblk >> 5)] = (unsigned)(bits >> 32);
        }
      }
  }
}

// one wave per row: neighbour count -> core flag
__global__ __launch_bounds__(256) void k_row_counts(const unsigned* __restrict__ adj, int n, int words, int min_samples,
                                                    int* __restrict__ core) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  int c = 0;
  for (int w = lane; w < words; w += 64) c += __popc(adj[(size_t)row * words + w]);
  c = wave_reduce_add(c);
  if (lane == 0) core[row] = c >= min_samples ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_core_bits(const int* __restrict__ core, int n, int words, unsigned* __restrict__ cbits,
                                                   int* __restrict__ parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = i;
  if (i >= words) return;
  unsigned v = 0;
  for (int b = 0; b < 32; ++b)
    if (i * 32 + b < n && core[i * 32 + b]) v |= 1u << b;
  cbits[i] = v;
}

__device__ __forceinline__ int ld(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// parent[v] <= v always: finds terminate, roots are the smallest index of their tree.  Path halving stores an ancestor.
__device__ int uf_find(int* parent, int x) {
  int curr = ld(parent + x);
  if (curr != x) {
    int prev = x, next;
    while (curr > (next = ld(parent + curr))) {
      __atomic_store_n(parent + prev, next, __ATOMIC_RELAXED);
      prev = curr;
      curr = next;
    }
  }
  return curr;
}

__device__ void uf_unite(int* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(parent + b, b, a) == b) return;  // hook the larger root under the smaller one
  }
}

// core-core edges (i < j) of the bitmask: thread per (row, word), grid-stride
__global__ __launch_bounds__(256) void k_union(const unsigned* __restrict__ adj, int n, int words, const int* __restrict__ core,
                                               const unsigned* __restrict__ cbits, int* parent) {
  const long long total = (long long)n * words;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
    const int i = (int)(q / words), w = (int)(q % words);
    if (w < (i >> 5) || !core[i]) continue;
    unsigned bits = adj[q] & cbits[w];
    if (w == (i >> 5)) bits &= (i & 31) == 31 ? 0u : ~0u << ((i & 31) + 1);  // j > i only
    while (bits) {
      const int j = w * 32 + __builtin_ctz(bits);
      bits &= bits - 1;
      uf_unite(parent, i, j);
    }
  }
}

// read-only finds after every union: root of each core point (no path halving here - it would race the stores)
__global__ __launch_bounds__(256) void k_roots(const int* __restrict__ parent, int n, const int* __restrict__ core,
                                               int* __restrict__ root, int* __restrict__ is_root) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int r = -1;
  if (core[i]) {
    r = i;
    while (parent[r] != r) r = parent[r];
  }
  root[i] = r;
  is_root[i] = core[i] && r == i ? 1 : 0;
}

// exclusive prefix sum of is_root (one workgroup of 1024, n <= 65536: 64 consecutive entries per thread) -> rank
__global__ __launch_bounds__(1024) void k_rank(const int* __restrict__ is_root, int n, int* __restrict__ rank) {
  __shared__ int s[1024];
  const int tid = threadIdx.x, per = (n + 1023) / 1024, lo = tid * per;
  int c = 0;
  for (int i = lo; i < lo + per && i < n; ++i) c += is_root[i];
  s[tid] = c;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const int v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  int run = s[tid] - c;
  for (int i = lo; i < lo + per && i < n; ++i) {
    rank[i] = run;
    run += is_root[i];
  }
}

__global__ __launch_bounds__(256) void k_core_labels(const int* __restrict__ root, const int* __restrict__ rank, int n,
                                                     int* __restrict__ labels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) labels[i] = root[i] >= 0 ? rank[root[i]] : -1;
}

// one wave per non-core row: the smallest label among its core neighbours, else -1
__global__ __launch_bounds__(256) void k_border(const unsigned* __restrict__ adj, int n, int words, const int* __restrict__ core,
                                                const unsigned* __restrict__ cbits, int* labels) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n || core[row]) return;
  int best = INT_MAX;
  for (int w = lane; w < words; w += 64) {
    unsigned bits = adj[(size_t)row * words + w] & cbits[w];
    while (bits) {
      const int j = w * 32 + __builtin_ctz(bits);
      bits &= bits - 1;
      best = min(best, labels[j]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
  if (lane == 0) labels[row] = best == INT_MAX ? -1 : best;
}

struct Block {
  int conv1, conv2, down;  // layer indices (down = -1: identity shortcut)
  int cin, cout, stride;
  std::string name;        // "layer<L>.<b>"
};

}  // namespace

struct eioku_iresnet {
  int depths[4] = {};
  ConvStack convs;
  std::vector<Block> blocks;
  std::vector<DevBuf<float>> prelu;  // [1 + blocks]: the stem's, then each block's (cout floats)
  std::vector<DevBuf<float>> bn;     // [blocks] x (scale | shift) of each block's leading bn1 (2 x cin floats)
  DevBuf<__half> fc_w;               // [512][25088] fp16, NHWC column order
  DevBuf<float> fc_b;
  // activations, grown to the most faces seen in one pass
  DevBuf<__half> crop;               // [m][112][112][8]
  DevBuf<__half> buf[5];             // [m][112][112][64] each
  DevBuf<float> partial;             // [kFcSplit][m][512]
  DevBuf<float> emb;                 // [m][512] (host outputs)
  DevBuf<uint8_t> src;               // staged host frames
  DevBuf<int> taps;                  // [m][2][112][2] + slot [m]
  DevBuf<double> mats;               // K13c: [m][6] forward matrices
  DevBuf<int> warp_ix;               // K13c: slot [m] + box flag [m]
  std::vector<int> htaps;
  std::vector<int32_t> hslots;       // K13c: the slots of an embed_aligned call (kept until its copy has run)
  double flops_last = 0;
};

namespace {

int ensure_cap(eioku_iresnet* r, int m) {
  EIOKU_TRY(r->crop.grow((size_t)m * kCrop * kCrop * 8));
  for (auto& b : r->buf) EIOKU_TRY(b.grow((size_t)m * kCrop * kCrop * 64));
  EIOKU_TRY(r->partial.grow((size_t)kFcSplit * m * kFeat));
  return r->emb.grow((size_t)m * kFeat);
}

int chan_ops(const __half* in, long long pixels, int C, const float* slope, __half* out_act, const float* bn, __half* out_bn,
             hipStream_t stream) {
  const long long work = pixels * (C / 8);
  if (work == 0) return EIOKU_OK;
  hipLaunchKernelGGL(k_chan_ops, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, in, pixels, C, slope, out_act,
                     bn, bn ? bn + C : nullptr, out_bn);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

int pick(int a, int b = -1, int c = -1) {
  for (int i = 0; i < 5; ++i)
    if (i != a && i != b && i != c) return i;
  return -1;
}

// the network on r->crop ([m][112][112][8]) -> emb_out [m][512] fp32 (device).  upto_block >= 0: stop after that block
// and copy its output (NHWC fp16) to act_out instead.
int run_iresnet(eioku_iresnet* r, int m, int upto_block, void* act_out, float* emb_out, hipStream_t stream) {
  EIOKU_TRY(r->convs.all_set());
  const auto& W = r->convs.w;
  for (size_t i = 0; i < r->prelu.size(); ++i) EIOKU_REQUIRE(r->prelu[i], "PReLU %zu has no slopes", i);
  for (size_t i = 0; i < r->bn.size(); ++i) EIOKU_REQUIRE(r->bn[i], "%s.bn1 has no parameters", r->blocks[i].name.c_str());
  EIOKU_REQUIRE(r->fc_w, "head has no weights");
  double flops = 0;
  int H = kCrop;
  int rc = conv_forward(W[0], Slice{r->crop, 8, 0}, m, H, H, Slice{r->buf[0], 64, 0}, nullptr, Slice{}, kActNone, stream);
  if (rc) return rc;
  flops += 2.0 * 64 * 3 * 9 * H * H * m;
  rc = chan_ops(r->buf[0], (long long)m * H * H, 64, r->prelu[0], r->buf[0], r->bn[0], r->buf[1], stream);
  if (rc) return rc;
  int x = 0, t = 1;
  for (size_t bi = 0; bi < r->blocks.size(); ++bi) {
    const Block& b = r->blocks[bi];
    const int Ho = conv_out_dim(H, 3, b.stride);
    const int u = pick(x, t);
    rc = conv_forward(W[b.conv1], Slice{r->buf[t], b.cin, 0}, m, H, H, Slice{r->buf[u], b.cout, 0}, nullptr, Slice{}, kActNone,
                      stream);
    if (rc) return rc;
    flops += W[b.conv1].flops_per_pixel() * m * H * H;
    rc = chan_ops(r->buf[u], (long long)m * H * H, b.cout, r->prelu[bi + 1], r->buf[u], nullptr, nullptr, stream);
    if (rc) return rc;
    int res = x;
    if (b.down >= 0) {
      res = pick(x, u);
      rc = conv_forward(W[b.down], Slice{r->buf[x], b.cin, 0}, m, H, H, Slice{r->buf[res], b.cout, 0}, nullptr, Slice{},
                        kActNone, stream);
      if (rc) return rc;
      flops += 2.0 * b.cout * b.cin * m * Ho * Ho;  // algorithmic: a 1x1
    }
    const int y = pick(x, u, res);
    rc = conv_forward(W[b.conv2], Slice{r->buf[u], b.cout, 0}, m, H, H, Slice{r->buf[y], b.cout, 0}, nullptr,
                      Slice{r->buf[res], b.cout, 0}, kActNone, stream);
    if (rc) return rc;
    flops += W[b.conv2].flops_per_pixel() * m * Ho * Ho;
    x = y;
    H = Ho;
    if ((int)bi == upto_block) {
      EIOKU_HIP_CHECK(hipMemcpyAsync(act_out, r->buf[x], (size_t)m * H * H * b.cout * 2, hipMemcpyDeviceToDevice, stream));
      r->flops_last = flops;
      return EIOKU_OK;
    }
    if (bi + 1 < r->blocks.size()) {
      t = pick(x);
      rc = chan_ops(r->buf[x], (long long)m * H * H, b.cout, nullptr, nullptr, r->bn[bi + 1], r->buf[t], stream);
      if (rc) return rc;
    }
  }
  hipLaunchKernelGGL(k_face_fc, dim3(kFeat / 64, (unsigned)((m + 15) / 16), kFcSplit), dim3(256), 0, stream, r->buf[x].p, m, r->fc_w.p,
                     r->partial.p);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_face_norm, dim3((unsigned)m), dim3(256), 0, stream, r->partial.p, m, r->fc_b.p, emb_out);
  EIOKU_LAUNCH_CHECK();
  flops += 2.0 * kFcK * kFeat * m;
  r->flops_last = flops;
  return EIOKU_OK;
}

// Host taps of one box (float64, then 11-bit fixed point): a square of side max(w, h, 1) centred on the box, sampled at
// the centres of 112 x 112 output pixels.  First source index clamped to [-2, size] (both taps stay outside the frame
// where they were).  Mirrored by eioku_amd/faces.py crop_taps.
void axis_taps(double lo, double hi, double side, int size, int* out) {
  const double left = (lo + hi) * 0.5 - side * 0.5, step = side / kCrop;
  for (int i = 0; i < kCrop; ++i) {
    const double src = left + (i + 0.5) * step - 0.5;
    const double f = std::floor(src);
    long long x0 = (long long)f;
    int w1 = (int)std::floor((src - f) * (1 << kTapBits) + 0.5);
    if (w1 == (1 << kTapBits)) {
      ++x0;
      w1 = 0;
    }
    x0 = std::min<long long>(std::max<long long>(x0, -2), size);
    out[2 * i] = (int)x0;
    out[2 * i + 1] = w1;
  }
}

int upload_taps(eioku_iresnet* r, int n, int h, int w, const float* boxes, int m, hipStream_t stream, int** d_taps, int** d_slot) {
  const size_t per = (size_t)4 * kCrop;
  r->htaps.assign(per * m + m, 0);
  for (int i = 0; i < m; ++i) {
    const float* b = boxes + (size_t)5 * i;
    for (int k = 0; k < 5; ++k) EIOKU_REQUIRE(std::isfinite(b[k]), "box %d has a non-finite value", i);
    const int slot = (int)b[0];
    EIOKU_REQUIRE(slot >= 0 && slot < n && (float)slot == b[0], "box %d: frame slot %g outside [0, %d)", i, (double)b[0], n);
    for (int k = 1; k < 5; ++k)
      EIOKU_REQUIRE(std::fabs(b[k]) <= 1e7f, "box %d: coordinate %g out of range", i, (double)b[k]);
    const double x1 = b[1], y1 = b[2], x2 = b[3], y2 = b[4];
    const double side = std::max(std::max(x2 - x1, y2 - y1), 1.0);
    axis_taps(x1, x2, side, w, r->htaps.data() + per * i);
    axis_taps(y1, y2, side, h, r->htaps.data() + per * i + 2 * kCrop);
    r->htaps[per * m + i] = slot;
  }
  const size_t tb = r->htaps.size() * 4;
  EIOKU_TRY(r->taps.grow(r->htaps.size()));
  EIOKU_HIP_CHECK(hipMemcpyAsync(r->taps, r->htaps.data(), tb, hipMemcpyHostToDevice, stream));
  *d_taps = r->taps;
  *d_slot = r->taps + per * m;
  return EIOKU_OK;
}

int launch_crop(const uint8_t* d_src, int h, int w, const int* d_slot, const int* d_taps, int mc, __half* out, hipStream_t stream) {
  const long long work = (long long)mc * kCrop * kCrop;
  hipLaunchKernelGGL(k_face_crop, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, d_src, h, w, d_slot, d_taps, mc, out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// K13c's per-face inputs -> device: slots (checked against n) and matrices (finite wherever the face is warped)
int upload_warp(eioku_iresnet* r, int n, const int32_t* slots, const double* M, const int32_t* use_box, int m, hipStream_t stream) {
  for (int i = 0; i < m; ++i) {
    EIOKU_REQUIRE(slots[i] >= 0 && slots[i] < n, "face %d: frame slot %d outside [0, %d)", i, slots[i], n);
    if (use_box && use_box[i]) continue;
    for (int k = 0; k < 6; ++k) EIOKU_REQUIRE(std::isfinite(M[(size_t)6 * i + k]), "face %d: matrix entry %d is not finite", i, k);
  }
  EIOKU_TRY(r->mats.grow((size_t)6 * m));
  EIOKU_TRY(r->warp_ix.grow((size_t)2 * m));
  EIOKU_HIP_CHECK(hipMemcpyAsync(r->mats, M, (size_t)6 * m * sizeof(double), hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(r->warp_ix, slots, (size_t)m * 4, hipMemcpyHostToDevice, stream));
  if (use_box) EIOKU_HIP_CHECK(hipMemcpyAsync(r->warp_ix + m, use_box, (size_t)m * 4, hipMemcpyHostToDevice, stream));
  return EIOKU_OK;
}

// faces [c0, c0 + mc) of the uploaded lists -> out rows 0 .. mc - 1
int launch_warp(eioku_iresnet* r, const uint8_t* d_src, int h, int w, int m, int c0, int mc, bool flags, __half* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_face_warp, dim3((kCrop * kCrop + 255) / 256, (unsigned)mc), dim3(256), 0, stream, d_src, h, w,
                     r->warp_ix.p + c0, r->mats.p + (size_t)6 * c0, flags ? r->warp_ix.p + m + c0 : nullptr, out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// eioku_iresnet_embed / _embed_aligned: M == nullptr is the box-crop path, launch for launch what it always was
int embed_faces(eioku_iresnet* r, const uint8_t* bgr, int n, int h, int w, const float* boxes, const double* M,
                const int32_t* use_box, int m, float* out, int mem, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && n >= 0 && h > 0 && w > 0 && m >= 0, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr && boxes && out && n > 0, "NULL buffer");
  int *d_taps, *d_slot;
  int rc = upload_taps(r, n, h, w, boxes, m, stream, &d_taps, &d_slot);
  if (rc) return rc;
  if (M) {
    r->hslots.resize((size_t)m);
    for (int i = 0; i < m; ++i) r->hslots[i] = (int32_t)boxes[(size_t)5 * i];  // (upload_taps has checked them)
    rc = upload_warp(r, n, r->hslots.data(), M, use_box, m, stream);
    if (rc) return rc;
  }
  const uint8_t* d_src;
  rc = stage_host(r->src, bgr, (size_t)n * h * w * 3, mem, stream, &d_src);
  if (rc) return rc;
  rc = ensure_cap(r, std::min(m, kChunk));
  if (rc) return rc;
  double flops = 0;
  for (int c0 = 0; c0 < m; c0 += kChunk) {
    const int mc = std::min(kChunk, m - c0);
    bool any_box = !M, any_warp = false;
    for (int i = c0; M && i < c0 + mc; ++i) (use_box[i] ? any_box : any_warp) = true;
    if (any_box) {
      rc = launch_crop(d_src, h, w, d_slot + c0, d_taps + (size_t)c0 * 4 * kCrop, mc, r->crop, stream);
      if (rc) return rc;
    }
    if (any_warp) {  // after K13a on the same stream: the warped faces' rows are overwritten whole
      rc = launch_warp(r, d_src, h, w, m, c0, mc, true, r->crop, stream);
      if (rc) return rc;
    }
    float* dst = mem == EIOKU_MEM_HOST ? r->emb : out + (size_t)c0 * kFeat;
    rc = run_iresnet(r, mc, -1, nullptr, dst, stream);
    if (rc) return rc;
    flops += r->flops_last;
    if (mem == EIOKU_MEM_HOST) {
      EIOKU_HIP_CHECK(hipMemcpyAsync(out + (size_t)c0 * kFeat, r->emb, (size_t)mc * kFeat * 4, hipMemcpyDeviceToHost, stream));
      EIOKU_HIP_CHECK(hipStreamSynchronize(stream));  // r->emb is reused by the next pass
    }
  }
  r->flops_last = flops;
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// DBSCAN workspace: one per process, grown on demand (the 65,536-point bitmask is 512 MiB); calls are serialised.  A raw
// pointer on purpose: it lives as long as the process, and a static destructor would free it after the runtime is gone
std::mutex g_db_mu;
void* g_db_ws = nullptr;
size_t g_db_bytes = 0;

}  // namespace

extern "C" {

int eioku_iresnet_create(const int* depths, eioku_iresnet_t** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out && depths, "NULL argument");
  for (int s = 0; s < 4; ++s) EIOKU_REQUIRE(depths[s] >= 1 && depths[s] <= 64, "stage %d depth %d outside [1, 64]", s + 1, depths[s]);
  auto* r = new eioku_iresnet();
  ConvStack& cs = r->convs;
  cs.add({"conv1", 64, 3, 3, 1});
  const int widths[4] = {64, 128, 256, 512};
  int inplanes = 64;
  for (int s = 0; s < 4; ++s) {
    r->depths[s] = depths[s];
    const int planes = widths[s];
    for (int b = 0; b < depths[s]; ++b) {
      const std::string p = "layer" + std::to_string(s + 1) + "." + std::to_string(b);
      const int cin = b == 0 ? inplanes : planes, stride = b == 0 ? 2 : 1;
      Block blk{cs.size(), cs.size() + 1, -1, cin, planes, stride, p};
      cs.add({p + ".conv1", planes, cin, 3, 1});
      cs.add({p + ".conv2", planes, planes, 3, stride});
      if (b == 0) blk.down = cs.add({p + ".downsample.0", planes, cin, 1, 2});  // every stage opens with a stride 2
      r->blocks.push_back(blk);
    }
    inplanes = planes;
  }
  r->prelu.resize(r->blocks.size() + 1);
  r->bn.resize(r->blocks.size());
  *out = r;
  return EIOKU_OK;
}

void eioku_iresnet_destroy(eioku_iresnet_t* r) {
  if (!r) return;
  (void)hipDeviceSynchronize();
  delete r;
}

int eioku_iresnet_num_convs(const eioku_iresnet_t* r) { return r ? r->convs.size() : 0; }

int eioku_iresnet_num_blocks(const eioku_iresnet_t* r) { return r ? (int)r->blocks.size() : 0; }

int eioku_iresnet_conv_info(const eioku_iresnet_t* r, int idx, char* name, size_t cap, int* cout, int* cin, int* ksize,
                            int* stride) {
  EIOKU_REQUIRE(r, "bad convolution index %d", idx);
  return r->convs.info(idx, name, cap, cout, cin, ksize, stride);
}

// weight HOST fp32 [cout][cin][k][k] with the following BatchNorm folded in, bias HOST fp32 [cout]
int eioku_iresnet_set_conv(eioku_iresnet_t* r, int idx, const float* w, const float* b) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && idx >= 0 && idx < r->convs.size() && w && b, "bad argument");
  const ConvLayer& l = r->convs.layers[idx];
  ConvWeights* cw = &r->convs.w[idx];
  // the stem reads the crop's 8 channels; a stride-2 1x1 runs as a 3x3 / s2 with the weights on the centre tap
  return r->convs.mark(idx, idx == 0   ? conv_weights_create_cin8(cw, l.cout, l.cin, l.k, l.stride, w, b)
                            : l.k == 1 ? conv_weights_create_centre(cw, l.cout, l.cin, l.stride, w, b)
                                       : conv_weights_create(cw, l.cout, l.cin, l.k, l.stride, w, b));
}

// unit 0: the stem's PReLU (64 slopes); unit 1 + b: block b's PReLU (its cout slopes).  HOST fp32.
int eioku_iresnet_set_prelu(eioku_iresnet_t* r, int unit, const float* slope) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && slope && unit >= 0 && unit <= (int)r->blocks.size(), "bad PReLU unit %d", unit);
  const int c = unit == 0 ? 64 : r->blocks[unit - 1].cout;
  return r->prelu[unit].upload(slope, (size_t)c);
}

// block b's leading bn1 as y = x * scale + shift per input channel (HOST fp32, cin each)
int eioku_iresnet_set_bn(eioku_iresnet_t* r, int block, const float* scale, const float* shift) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && scale && shift && block >= 0 && block < (int)r->blocks.size(), "bad block %d", block);
  const int c = r->blocks[block].cin;
  EIOKU_TRY(r->bn[block].grow((size_t)c * 2));
  EIOKU_HIP_CHECK(hipMemcpy(r->bn[block], scale, (size_t)c * 4, hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(r->bn[block] + c, shift, (size_t)c * 4, hipMemcpyHostToDevice));
  return EIOKU_OK;
}

// head: bn2 -> flatten -> fc -> features folded into weight HOST fp32 [512][25088] (columns in NHWC order (y, x, c)) and
// bias HOST fp32 [512]
int eioku_iresnet_set_head(eioku_iresnet_t* r, const float* w, const float* b) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && w && b, "bad argument");
  std::vector<_Float16> hw((size_t)kFeat * kFcK);
  for (size_t i = 0; i < hw.size(); ++i) hw[i] = (_Float16)w[i];
  EIOKU_TRY(r->fc_w.upload(reinterpret_cast<const __half*>(hw.data()), hw.size()));
  return r->fc_b.upload(b, kFeat);
}

// K13a alone (parity helper): n BGR u8 frames (h x w; host or device per mem), boxes HOST fp32 [m][5] = (frame slot, x1,
// y1, x2, y2) -> out_f16 [m][112][112][8] fp16 (device).  Synchronous.
int eioku_iresnet_crop(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const float* boxes, int m, void* out_f16,
                       int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && n >= 0 && h > 0 && w > 0 && m >= 0, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr && boxes && out_f16 && n > 0, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  int *d_taps, *d_slot;
  int rc = upload_taps(r, n, h, w, boxes, m, stream, &d_taps, &d_slot);
  if (rc) return rc;
  const uint8_t* d_src;
  rc = stage_host(r->src, bgr, (size_t)n * h * w * 3, mem, stream, &d_src);
  if (rc) return rc;
  rc = launch_crop(d_src, h, w, d_slot, d_taps, m, (__half*)out_f16, stream);
  if (rc) return rc;
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// The raw network on crops in_f16 [m][112][112][8] (device) -> emb_out [m][512] fp32 (device); upto_block >= 0 stops after
// that block and writes its NHWC fp16 output to act_out (device) instead.  Synchronous.
int eioku_iresnet_forward(eioku_iresnet_t* r, const void* in_f16, int m, int upto_block, void* act_out, float* emb_out,
                          void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && m >= 0 && upto_block < (int)r->blocks.size(), "bad argument");
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(in_f16 && (upto_block >= 0 ? act_out != nullptr : emb_out != nullptr), "NULL buffer");
  EIOKU_REQUIRE(m <= kChunk, "at most %d faces per forward", kChunk);
  hipStream_t stream = (hipStream_t)stream_;
  int rc = ensure_cap(r, m);
  if (rc) return rc;
  EIOKU_HIP_CHECK(hipMemcpyAsync(r->crop, in_f16, (size_t)m * kCrop * kCrop * 8 * 2, hipMemcpyDeviceToDevice, stream));
  rc = run_iresnet(r, m, upto_block, act_out, emb_out, stream);
  if (rc) return rc;
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// Crop + network for m boxes on n BGR frames (host or device per mem; boxes HOST fp32 [m][5] = (frame slot, x1, y1, x2,
// y2)) -> out [m][512] fp32 unit vectors (HOST when mem == EIOKU_MEM_HOST, else device).  Faces run in passes of 256.
// Synchronous.
int eioku_iresnet_embed(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const float* boxes, int m, float* out,
                        int mem, void* stream_) {
  return embed_faces(r, bgr, n, h, w, boxes, nullptr, nullptr, m, out, mem, (hipStream_t)stream_);
}

// K13c alone (parity helper): faces warped by M HOST float64 [m][6] (frame -> 112 x 112 crop, cv2.warpAffine's M) from
// frame slots HOST int32 [m] -> out_f16 [m][112][112][8] fp16 (device).  Synchronous.
int eioku_iresnet_crop_aligned(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const int32_t* slots, const double* M,
                               int m, void* out_f16, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && n >= 0 && h > 0 && w > 0 && m >= 0, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr && slots && M && out_f16 && n > 0, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  EIOKU_TRY(upload_warp(r, n, slots, M, nullptr, m, stream));
  const uint8_t* d_src;
  EIOKU_TRY(stage_host(r->src, bgr, (size_t)n * h * w * 3, mem, stream, &d_src));
  for (int c0 = 0; c0 < m; c0 += 32768)  // a grid's y extent is 65535
    EIOKU_TRY(launch_warp(r, d_src, h, w, m, c0, std::min(32768, m - c0), false, (__half*)out_f16 + (size_t)c0 * kCrop * kCrop * 8, stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// eioku_iresnet_embed with aligned crops: face i is warped by M[i] (K13c) unless use_box[i] != 0 (HOST int32 [m]), which
// keeps the box crop of boxes[i] (K13a) - the fallback for faces whose landmarks give no usable transform.  The frame
// slot of every face is boxes[i][0].  Same passes of 256, same outputs.  Synchronous.
int eioku_iresnet_embed_aligned(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const float* boxes, const double* M,
                                const int32_t* use_box, int m, float* out, int mem, void* stream_) {
  EIOKU_REQUIRE(m <= 0 || (M && use_box), "NULL buffer");
  return embed_faces(r, bgr, n, h, w, boxes, M, use_box, m, out, mem, (hipStream_t)stream_);
}

int eioku_iresnet_last_flops(const eioku_iresnet_t* r, double* flops) {
  EIOKU_REQUIRE(r && flops, "NULL argument");
  *flops = r->flops_last;
  return EIOKU_OK;
}

// scikit-learn DBSCAN(metric="cosine") on unit-norm rows: emb [n][d] fp32 (host or device per mem), d % 32 == 0,
// n <= 65536, eps in [0, 2], min_samples >= 1 -> labels_out [n] int32 (same side): clusters 0, 1, ... by smallest core
// index, -1 = noise.  Synchronous.
int eioku_dbscan_cosine(const float* emb, int n, int d, float eps, int min_samples, int32_t* labels_out, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(n >= 0 && n <= 65536, "n = %d outside [0, 65536]", n);
  EIOKU_REQUIRE(d > 0 && d % 32 == 0, "d = %d must be a positive multiple of 32", d);
  EIOKU_REQUIRE(eps >= 0.f && eps <= 2.f, "eps = %g outside [0, 2]", (double)eps);
  EIOKU_REQUIRE(min_samples >= 1, "min_samples = %d must be >= 1", min_samples);
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(emb && labels_out, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> lock(g_db_mu);
  const int words = (n + 31) / 32;
  const size_t adj_b = ((size_t)n * words * 4 + 255) / 256 * 256, vec = ((size_t)n * 4 + 255) / 256 * 256, wv = ((size_t)words * 4 + 255) / 256 * 256;
  const size_t emb_b = mem == EIOKU_MEM_HOST ? ((size_t)n * d * 4 + 255) / 256 * 256 : 0;
  const size_t need = adj_b + 6 * vec + wv + emb_b;
  if (g_db_bytes < need) {
    if (g_db_ws) (void)hipFree(g_db_ws);
    g_db_ws = nullptr;
    g_db_bytes = 0;
    EIOKU_HIP_CHECK(hipMalloc(&g_db_ws, need));
    g_db_bytes = need;
  }
  char* p = (char*)g_db_ws;
  unsigned* adj = (unsigned*)p;
  p += adj_b;
  int* core = (int*)p;
  int* parent = (int*)(p + vec);
  int* root = (int*)(p + 2 * vec);
  int* is_root = (int*)(p + 3 * vec);
  int* rank = (int*)(p + 4 * vec);
  int* labels = (int*)(p + 5 * vec);
  unsigned* cbits = (unsigned*)(p + 6 * vec);
  const float* d_emb = emb;
  if (mem == EIOKU_MEM_HOST) {
    float* e = (float*)(p + 6 * vec + wv);
    EIOKU_HIP_CHECK(hipMemcpyAsync(e, emb, (size_t)n * d * 4, hipMemcpyHostToDevice, stream));
    d_emb = e;
  }
  const unsigned tiles = (unsigned)((n + kGT - 1) / kGT), rows4 = (unsigned)((n + 3) / 4), lin = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_gram_bits, dim3(tiles, tiles), dim3(256), 0, stream, d_emb, n, d, eps, words, adj);
  hipLaunchKernelGGL(k_row_counts, dim3(rows4), dim3(256), 0, stream, adj, n, words, min_samples, core);
  hipLaunchKernelGGL(k_core_bits, dim3((unsigned)((std::max(n, words) + 255) / 256)), dim3(256), 0, stream, core, n, words, cbits,
                     parent);
  const long long items = (long long)n * words;
  hipLaunchKernelGGL(k_union, dim3((unsigned)std::min<long long>((items + 255) / 256, 65536)), dim3(256), 0, stream, adj, n, words,
                     core, cbits, parent);
  hipLaunchKernelGGL(k_roots, dim3(lin), dim3(256), 0, stream, parent, n, core, root, is_root);
  hipLaunchKernelGGL(k_rank, dim3(1), dim3(1024), 0, stream, is_root, n, rank);
  hipLaunchKernelGGL(k_core_labels, dim3(lin), dim3(256), 0, stream, root, rank, n, labels);
  hipLaunchKernelGGL(k_border, dim3(rows4), dim3(256), 0, stream, adj, n, words, core, cbits, labels);
  EIOKU_LAUNCH_CHECK();
  EIOKU_HIP_CHECK(hipMemcpyAsync(labels_out, labels, (size_t)n * 4,
                                 mem == EIOKU_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

}  // extern "C"
