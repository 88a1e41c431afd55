// K15 / K16: OCR - EasyOCR's CRAFT text detector and its `english_g2` CRNN recogniser.
//
// Fills ModelManager.extract_ocr (eioku_amd/ocr.py holds the host logic: boxes, crops, CTC decode).  On the device:
//   k_craft_prep     K15 input: BGR u8 frame -> the CRAFT canvas as NHWC8 fp16 in one pass.  Either a copy (long side
//                    <= canvas) or OpenCV INTER_LINEAR with host-made 11-bit taps; pad to a multiple of 32 with zeros,
//                    THEN normalise (ImageNet RGB mean / std applied to B, G, R in that order, as EasyOCR does on the
//                    BGR array): the pad holds -mean / std.  The fp32 canvas is never written.
//   VGG16-BN + U-Net the convolutions on K4 (conv.hip) with every BatchNorm folded into its conv.  The basenet's slices
//                    end at a BN output and slices 2-4 open with torchvision's ReLU(inplace=True), which rewrites the
//                    tensor CRAFT kept for its skip: relu2_2, relu3_2 and relu4_3 are ReLU'd (written so by their
//                    convs, straight into the concat slices); relu5_3 is not (slice5 opens with a max pool).  New here:
//   k_maxpool        kh x kw / (sh, sw) / pad max pool over an NHWC slice
//   k_im2col_dil     fc6 (3x3, dilation 6, pad 6, 512 -> 1024 at 1/16) as a 4608-channel im2col + K4's 1x1
//   k_up2x           F.interpolate(bilinear, align_corners=False) to exactly twice the size, into a concat slice
//   k_craft_maps     conv_cls's fp32 (text, link) pixels -> text / link maps + (text > low_text) | (link > link_thr) u8
//   K16 (CRNN): crops as NHWC8 fp16 (grey value in channel 0) on K4's convs; (2, 1) pools on k_maxpool; the 2x2 valid
//                    conv as a 3x3 whose bottom-right 2x2 holds the weights (last row / column dropped)
//   k_row_mean       AdaptiveAvgPool over the 3 remaining rows -> packed sequences [sum T][256] fp32
//   k_gemm_f32       C = A W^T + bias on the exact-fp32 matrix pipe (v_mfma_f32_16x16x4_f32): the BiLSTMs' input
//                    projection (all steps, both directions: one GEMM), their Linear(512, 256) and Prediction
//   k_lstm           one BiLSTM recurrence: one workgroup per (tile of 4 sequences, direction), h in LDS, c in registers,
//                    W_hh (fp32, [k][4 * 256]) streamed from L2 each step, per-sequence lengths (the reverse direction
//                    starts at each sequence's own end); no cross-workgroup waits
//   k_ctc_probs      softmax over the classes, ignored classes zeroed and renormalised, argmax + max probability
// Numerics: CRAFT and the recogniser's VGG store fp16 activations and weights (K4), accumulate in fp32; from the row mean
// on, the recogniser is fp32 throughout (sequences, GEMM operands, recurrence, hidden states, logits).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "convnet.h"

using namespace eioku;

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int kTapBits = 11;  // OpenCV INTER_RESIZE_COEF_BITS
constexpr int kHid = 256;     // english_g2 BiLSTM hidden size
constexpr int kSeqTile = 4;   // sequences per k_lstm workgroup

// ---- K15 input -----------------------------------------------------------------------------------------------------
// taps: x [tw][3] then y [th][3] = (first source index, weight 0, weight 1) in 1/2048; copy: th == h and tw == w
__global__ __launch_bounds__(256) void k_craft_prep(const uint8_t* __restrict__ bgr, int n, int h, int w, int th, int tw, int H,
                                                    int W, const int* __restrict__ taps, int copy, __half* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * H * W) return;
  const int x = (int)(i % W), y = (int)((i / W) % H), f = (int)(i / ((long long)W * H));
  float v[3] = {0.f, 0.f, 0.f};
  if (y < th && x < tw) {
    const uint8_t* fr = bgr + (size_t)f * h * w * 3;
    if (copy) {
      const uint8_t* p = fr + ((size_t)y * w + x) * 3;
      v[0] = p[0];
      v[1] = p[1];
      v[2] = p[2];
    } else {
      const int* tx = taps + 3 * x;
      const int* ty = taps + 3 * tw + 3 * y;
      const int x0 = tx[0], x1 = min(x0 + 1, w - 1), y0 = ty[0], y1 = min(y0 + 1, h - 1);
      const uint8_t* r0 = fr + (size_t)y0 * w * 3;
      const uint8_t* r1 = fr + (size_t)y1 * w * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int s0 = tx[1] * r0[x0 * 3 + c] + tx[2] * r0[x1 * 3 + c];
        const int s1 = tx[1] * r1[x0 * 3 + c] + tx[2] * r1[x1 * 3 + c];
        const int acc = ty[1] * s0 + ty[2] * s1 + (1 << (2 * kTapBits - 1));
        v[c] = (float)min(max(acc >> (2 * kTapBits), 0), 255);
      }
    }
  }
  // normalizeMeanVariance in float32: (v - mean * 255) / (std * 255), constants rounded to float32 first
  const float mean[3] = {(float)(0.485 * 255.0), (float)(0.456 * 255.0), (float)(0.406 * 255.0)};
  const float sd[3] = {(float)(0.229 * 255.0), (float)(0.224 * 255.0), (float)(0.225 * 255.0)};
  half8 o = {};
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (_Float16)((v[c] - mean[c]) / sd[c]);
  *reinterpret_cast<uint4*>(out + (size_t)i * 8) = __builtin_bit_cast(uint4, o);
}

// ---- pooling / elementwise over NHWC fp16 slices (C % 8 == 0, slices 8-channel aligned) ----------------------------
__global__ __launch_bounds__(256) void k_maxpool(const __half* __restrict__ in, int in_cs, int N, int H, int W, int C, int kh,
                                                 int kw, int sh, int sw, int ph, int pw, int Ho, int Wo,
                                                 __half* __restrict__ out, int out_cs) {
  const int C8 = C / 8;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * Ho * Wo * C8) return;
  const int c0 = (int)(i % C8) * 8;
  const long long p = i / C8;
  const int xo = (int)(p % Wo), yo = (int)((p / Wo) % Ho), nb = (int)(p / ((long long)Wo * Ho));
  float m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
  for (int dy = 0; dy < kh; ++dy) {
    const int yy = yo * sh - ph + dy;
    if ((unsigned)yy >= (unsigned)H) continue;
    for (int dx = 0; dx < kw; ++dx) {
      const int xx = xo * sw - pw + dx;
      if ((unsigned)xx >= (unsigned)W) continue;
      const half8 v = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(in + (((size_t)nb * H + yy) * W + xx) * in_cs + c0));
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], (float)v[j]);
    }
  }
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (_Float16)m[j];
  *reinterpret_cast<uint4*>(out + (size_t)p * out_cs + c0) = __builtin_bit_cast(uint4, o);
}

// dense [N][H][W][C] -> [N*H*W][9][C]: tap (ky, kx) of pixel (y, x) = in[y + d (ky - 1)][x + d (kx - 1)], zero outside
__global__ __launch_bounds__(256) void k_im2col_dil(const __half* __restrict__ in, int N, int H, int W, int C, int d,
                                                    __half* __restrict__ out) {
  const int C8 = C / 8;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * H * W * 9 * C8) return;
  const int c0 = (int)(i % C8) * 8;
  const int tap = (int)((i / C8) % 9);
  const long long p = i / ((long long)C8 * 9);
  const int x = (int)(p % W), y = (int)((p / W) % H), nb = (int)(p / ((long long)W * H));
  const int yy = y + d * (tap / 3 - 1), xx = x + d * (tap % 3 - 1);
  uint4 v = {0u, 0u, 0u, 0u};
  if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
    v = *reinterpret_cast<const uint4*>(in + (((size_t)nb * H + yy) * W + xx) * C + c0);
  *reinterpret_cast<uint4*>(out + (size_t)i * 8) = v;
}

// bilinear, align_corners=False, h x w -> 2h x 2w: even outputs 0.25 in[i - 1] + 0.75 in[i], odd 0.75 in[i] + 0.25
// in[i + 1], indices clamped (PyTorch's upsample_bilinear2d source index and lambdas for a scale of exactly 1/2)
__global__ __launch_bounds__(256) void k_up2x(const __half* __restrict__ in, int N, int h, int w, int C,
                                              __half* __restrict__ out, int out_cs) {
  const int C8 = C / 8, H = 2 * h, W = 2 * w;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * H * W * C8) return;
  const int c0 = (int)(i % C8) * 8;
  const long long p = i / C8;
  const int x = (int)(p % W), y = (int)((p / W) % H), nb = (int)(p / ((long long)W * H));
  // source coordinate max(0, (o + 0.5) / 2 - 0.5): i0 = floor, i1 = min(i0 + 1, n - 1), lambda1 = coord - i0
  const float sy = fmaxf(0.f, (y + 0.5f) * 0.5f - 0.5f), sx = fmaxf(0.f, (x + 0.5f) * 0.5f - 0.5f);
  const int y0 = (int)sy, x0 = (int)sx, y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  const float ly1 = sy - y0, ly0 = 1.f - ly1, lx1 = sx - x0, lx0 = 1.f - lx1;
  const __half* b = in + (size_t)nb * h * w * C + c0;
  const half8 a00 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(b + ((size_t)y0 * w + x0) * C));
  const half8 a01 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(b + ((size_t)y0 * w + x1) * C));
  const half8 a10 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(b + ((size_t)y1 * w + x0) * C));
  const half8 a11 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(b + ((size_t)y1 * w + x1) * C));
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    o[j] = (_Float16)(ly0 * (lx0 * (float)a00[j] + lx1 * (float)a01[j]) + ly1 * (lx0 * (float)a10[j] + lx1 * (float)a11[j]));
  *reinterpret_cast<uint4*>(out + (size_t)p * out_cs + c0) = __builtin_bit_cast(uint4, o);
}

// y [pixels][2] fp32 (text, link) -> text [pixels], link [pixels], bin [pixels]
__global__ __launch_bounds__(256) void k_craft_maps(const float* __restrict__ y, long long pixels, float low_text, float link_thr,
                                                    float* __restrict__ text, float* __restrict__ link,
                                                    uint8_t* __restrict__ bin) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const float2 v = *reinterpret_cast<const float2*>(y + 2 * i);
  if (text) text[i] = v.x;
  if (link) link[i] = v.y;
  if (bin) bin[i] = (uint8_t)((v.x > low_text) | (v.y > link_thr));
}

// ---- K16 -----------------------------------------------------------------------------------------------------------
// x dense [m][4][wq][C] (the 3x3-as-2x2 conv's output; rows 0..2 and columns 0..wq-2 valid) -> seq[off[s] + t][C]
__global__ __launch_bounds__(256) void k_row_mean(const __half* __restrict__ x, int m, int wq, int C, const int* __restrict__ off,
                                                  float* __restrict__ seq) {
  const int T = wq - 1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)m * T * C) return;
  const int c = (int)(i % C), t = (int)((i / C) % T), s = (int)(i / ((long long)C * T));
  const __half* b = x + ((size_t)s * 4 * wq + t) * C + c;
  const float v = ((float)b[0] + (float)b[(size_t)wq * C]) + (float)b[(size_t)2 * wq * C];
  seq[((size_t)off[s] + t) * C + c] = v / 3.f;
}

typedef float float4v __attribute__((ext_vector_type(4)));

// C [M][N] = A [M][K] . W [N][K]^T + bias [N], all fp32, K % 4 == 0.  grid (ceil(N / 64), ceil(M / 16)), 4 waves: wave w
// owns columns 64 bx + 16 w .. + 15 of rows 16 by .. + 15.  MFMA 16x16x4 f32: lane (r, u) supplies A[m0 + r][k + u] and
// W[n0 + r][k + u]; it holds D[4u + t][r], i.e. C[m0 + 4u + t][n0 + r].
__global__ __launch_bounds__(256) void k_gemm_f32(const float* __restrict__ A, int M, int K, const float* __restrict__ W, int N,
                                                  const float* __restrict__ bias, float* __restrict__ Cout) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, u = lane >> 4;
  const int n0 = blockIdx.x * 64 + wave * 16, m0 = blockIdx.y * 16;
  if (n0 >= N) return;  // wave-uniform
  const int m = m0 + r, n = n0 + r;
  const float* ar = A + (size_t)min(m, M - 1) * K + u;
  const float* wr = W + (size_t)min(n, N - 1) * K + u;
  float4v acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; k += 4) {
    const float a = m < M ? ar[k] : 0.f;
    const float b = n < N ? wr[k] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  if (n >= N) return;
  const float bn = bias[n];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = m0 + 4 * u + t;
    if (row < M) Cout[(size_t)row * N + n] = acc[t] + bn;
  }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// grid (ceil(nseq / kSeqTile), 2 directions), 256 threads: thread j owns hidden unit j of the tile's sequences.
// gx [rows][2][4][256] fp32 = x W_ih^T + b_ih + b_hh (both directions); whh_t [2][256 k][4 * 256] fp32 (W_hh transposed);
// out [rows][2 * 256] fp32: h_t, forward then reverse
__global__ __launch_bounds__(256) void k_lstm(const float* __restrict__ gx, const float* __restrict__ whh_t,
                                              const int* __restrict__ off, const int* __restrict__ len, int nseq,
                                              float* __restrict__ out) {
  __shared__ float hs[kSeqTile][kHid];
  const int j = threadIdx.x, dir = blockIdx.y, s0 = blockIdx.x * kSeqTile;
  int L[kSeqTile], O[kSeqTile], maxlen = 0;
  float c[kSeqTile];
#pragma unroll
  for (int s = 0; s < kSeqTile; ++s) {
    const bool live = s0 + s < nseq;
    L[s] = live ? len[s0 + s] : 0;
    O[s] = live ? off[s0 + s] : 0;
    maxlen = max(maxlen, L[s]);
    c[s] = 0.f;
    hs[s][j] = 0.f;
  }
  __syncthreads();
  const float* W = whh_t + (size_t)dir * kHid * 4 * kHid + j;
  for (int step = 0; step < maxlen; ++step) {
    float acc[4][kSeqTile];
    int row[kSeqTile];
#pragma unroll
    for (int s = 0; s < kSeqTile; ++s) {
      const bool act = step < L[s];
      row[s] = act ? O[s] + (dir ? L[s] - 1 - step : step) : -1;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g][s] = act ? gx[((size_t)row[s] * 2 + dir) * 4 * kHid + g * kHid + j] : 0.f;
    }
    for (int k = 0; k < kHid; ++k) {
      const float w0 = W[(size_t)k * 4 * kHid], w1 = W[(size_t)k * 4 * kHid + kHid], w2 = W[(size_t)k * 4 * kHid + 2 * kHid],
                  w3 = W[(size_t)k * 4 * kHid + 3 * kHid];
#pragma unroll
      for (int s = 0; s < kSeqTile; ++s) {
        const float h = hs[s][k];
        acc[0][s] = fmaf(w0, h, acc[0][s]);
        acc[1][s] = fmaf(w1, h, acc[1][s]);
        acc[2][s] = fmaf(w2, h, acc[2][s]);
        acc[3][s] = fmaf(w3, h, acc[3][s]);
      }
    }
    float hn[kSeqTile];
#pragma unroll
    for (int s = 0; s < kSeqTile; ++s) {  // PyTorch gate order: input, forget, cell, output
      const float ig = sigmoidf_(acc[0][s]), fg = sigmoidf_(acc[1][s]), gg = tanhf(acc[2][s]), og = sigmoidf_(acc[3][s]);
      c[s] = fg * c[s] + ig * gg;
      hn[s] = og * tanhf(c[s]);
    }
    __syncthreads();  // every thread has read hs for this step
#pragma unroll
    for (int s = 0; s < kSeqTile; ++s) {
      if (row[s] < 0) continue;
      hs[s][j] = hn[s];
      out[(size_t)row[s] * 2 * kHid + dir * kHid + j] = hn[s];
    }
    __syncthreads();
  }
}

// one wave per row of logits [rows][C] fp32: p = softmax, p[ignored] = 0, p /= sum p -> argmax (first), max
__global__ __launch_bounds__(256) void k_ctc_probs(const float* __restrict__ logits, int rows, int C, const uint8_t* __restrict__ ignore,
                                                   int* __restrict__ idx, float* __restrict__ prob) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* l = logits + (size_t)r * C;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, l[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(l[c] - mx);
  se = wave_reduce_add(se);
  se = __shfl(se, 0, 64);
  float kept = 0.f, best = -1.f;
  int bi = 0;
  for (int c = lane; c < C; c += 64) {
    const float p = ignore[c] ? 0.f : expf(l[c] - mx) / se;
    kept += p;
    if (p > best) {
      best = p;
      bi = c;
    }
  }
  kept = wave_reduce_add(kept);
  kept = __shfl(kept, 0, 64);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // max, ties to the lower class
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) {
    idx[r] = bi;
    prob[r] = best / kept;
  }
}

int grid1(long long work) { return (int)((work + 255) / 256); }

int gemm_f32(const float* A, int M, int K, const float* W, int N, const float* bias, float* Cout, hipStream_t st, double* fl) {
  if (M == 0) return EIOKU_OK;
  hipLaunchKernelGGL(k_gemm_f32, dim3((unsigned)((N + 63) / 64), (unsigned)((M + 15) / 16)), dim3(256), 0, st, A, M, K, W, N, bias,
                     Cout);
  EIOKU_LAUNCH_CHECK();
  *fl += 2.0 * M * N * K;
  return EIOKU_OK;
}

}  // namespace

// ---- K15: CRAFT --------------------------------------------------------------------------------------------------
struct eioku_craft {
  ConvStack convs;
  DevBuf<__half> in8, p0, p1, cat1, cat2, cat3, cat4, col;
  DevBuf<float> y;
  DevBuf<uint8_t> src;  // staged host frames
  DevBuf<int> taps;
  std::vector<int> htaps;
  double flops_last = 0;
};

// ---- K16: CRNN ---------------------------------------------------------------------------------------------------
struct eioku_crnn {
  int num_class = 0;
  ConvStack convs;  // 7 VGG convs + "Prediction"
  // fp32, PyTorch layouts: per BiLSTM layer the input projection [2 * 1024][256] + (b_ih + b_hh) and the Linear [256][512]
  // + bias; Prediction [num_class][256] + bias
  DevBuf<float> wih[2], bih[2], wlin[2], blin[2], wpred, bpred;
  DevBuf<float> whh[2];  // [2][256][1024] transposed
  bool lstm_set[2] = {};
  DevBuf<__half> img, a0, a1;
  DevBuf<float> seq, gx, hid32, logits, prob;
  DevBuf<int> idx, offlen;
  DevBuf<uint8_t> ignore;
  std::vector<__half> himg;
  std::vector<int> hofflen;
  double flops_last = 0;
};

namespace {

int conv(const ConvWeights& cw, Slice in, int N, int H, int W, Slice out, float* out_f32, int act, hipStream_t st, double* fl) {
  *fl += cw.flops_per_pixel() * N * conv_out_dim(H, cw.ks, cw.stride) * conv_out_dim(W, cw.ks, cw.stride);
  return conv_forward(cw, in, N, H, W, out, out_f32, Slice{}, act, st);
}

int maxpool(Slice in, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw, Slice out,
            hipStream_t st, int* Ho_, int* Wo_) {
  const int Ho = (H + 2 * ph - kh) / sh + 1, Wo = (W + 2 * pw - kw) / sw + 1;
  const long long work = (long long)N * Ho * Wo * (C / 8);
  if (work > 0) {
    hipLaunchKernelGGL(k_maxpool, dim3(grid1(work)), dim3(256), 0, st, in.ptr + in.coff, in.cstride, N, H, W, C, kh, kw, sh, sw, ph,
                       pw, Ho, Wo, out.ptr + out.coff, out.cstride);
    EIOKU_LAUNCH_CHECK();
  }
  if (Ho_) *Ho_ = Ho;
  if (Wo_) *Wo_ = Wo;
  return EIOKU_OK;
}

int up2x(const __half* in, int N, int h, int w, int C, Slice out, hipStream_t st) {
  hipLaunchKernelGGL(k_up2x, dim3(grid1((long long)N * 4 * h * w * (C / 8))), dim3(256), 0, st, in, N, h, w, C, out.ptr + out.coff,
                     out.cstride);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

int im2col_dil(const __half* in, int N, int H, int W, int C, int d, __half* out, hipStream_t st) {
  hipLaunchKernelGGL(k_im2col_dil, dim3(grid1((long long)N * H * W * 9 * (C / 8))), dim3(256), 0, st, in, N, H, W, C, d, out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

int ctc_probs(const float* logits, int rows, int C, const uint8_t* ignore, int* idx, float* prob, hipStream_t st) {
  hipLaunchKernelGGL(k_ctc_probs, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, rows, C, ignore, idx, prob);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// a caller's DEVICE fp16 NHWC slice of the glue entry points: 16-byte vectors, 32-bit element offsets
int check_slice(const void* p, int cstride, int coff, int C, long long pixels, const char* what) {
  EIOKU_REQUIRE(p && ((uintptr_t)p & 15) == 0, "%s: NULL or not 16-byte aligned", what);
  EIOKU_REQUIRE(C > 0 && C % 8 == 0, "%s: %d channels (a multiple of 8)", what, C);
  EIOKU_REQUIRE(cstride % 8 == 0 && coff % 8 == 0 && coff >= 0 && coff + C <= cstride,
                "%s: channels %d..%d of a stride of %d (8-aligned, inside the stride)", what, coff, coff + C, cstride);
  EIOKU_REQUIRE(pixels * cstride <= (1LL << 31) - 1, "%s: %lld pixels x %d channels exceed 32-bit element offsets", what, pixels,
                cstride);
  return EIOKU_OK;
}

// OpenCV resize INTER_LINEAR taps of one axis (src -> dst): fx = (float)((d + 0.5) * src / dst - 0.5), sx = floor(fx),
// clamped at both ends with fx = 0; weights saturate_cast<short>((1 - fx) * 2048), saturate_cast<short>(fx * 2048)
void linear_taps(int src, int dst, int* out) {
  const double scale = (double)src / dst;
  for (int d = 0; d < dst; ++d) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    int sx = (int)std::floor(fx);
    fx -= sx;
    if (sx < 0) fx = 0.f, sx = 0;
    if (sx >= src - 1) fx = 0.f, sx = src - 1;
    out[3 * d] = sx;
    out[3 * d + 1] = (int)std::lrint((1.f - fx) * (1 << kTapBits));
    out[3 * d + 2] = (int)std::lrint(fx * (1 << kTapBits));
  }
}

// the CRAFT canvas of an h x w frame: the frame itself (copy) or INTER_LINEAR to th x tw, inside H x W (multiples of 32)
struct Canvas {
  bool copy;
  int th, tw, H, W;
};

int canvas_of(int h, int w, int canvas_size, Canvas* c) {
  EIOKU_REQUIRE(h > 0 && w > 0 && canvas_size >= 32, "bad argument");
  const int mx = std::max(h, w);
  c->copy = mx <= canvas_size;
  const double ratio = c->copy ? 1.0 : (double)canvas_size / mx;
  c->th = c->copy ? h : (int)(h * ratio);
  c->tw = c->copy ? w : (int)(w * ratio);
  EIOKU_REQUIRE(c->th > 0 && c->tw > 0, "frame %d x %d resizes to nothing", h, w);
  c->H = (c->th + 31) / 32 * 32;
  c->W = (c->tw + 31) / 32 * 32;
  return EIOKU_OK;
}

// the frames on the device (*d_src: HOST frames are staged in the handle) and, for a resize, its taps in r->taps
int craft_stage(eioku_craft* r, const uint8_t* bgr, int n, int h, int w, const Canvas& c, int mem, hipStream_t st,
                const uint8_t** d_src) {
  EIOKU_TRY(stage_host(r->src, bgr, (size_t)n * h * w * 3, mem, st, d_src));
  if (!c.copy) {
    std::vector<int>& taps = r->htaps;  // kept in the handle: the copy below is asynchronous
    taps.assign((size_t)3 * (c.tw + c.th), 0);
    linear_taps(w, c.tw, taps.data());
    linear_taps(h, c.th, taps.data() + 3 * c.tw);
    EIOKU_TRY(r->taps.grow(taps.size()));
    EIOKU_HIP_CHECK(hipMemcpyAsync(r->taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice, st));
  }
  return EIOKU_OK;
}

// the recogniser's buffers from the packed sequences on, for m sequences of `rows` steps in all; off / len (HOST, [m])
// and `ignore` (HOST, [num_class]) go to the device: r->offlen = [off | len | off[order[.]], the row offsets in the order
// of the conv passes (zeros without `order`)]
int tail_reserve(eioku_crnn* r, long long rows, int m, const int* off, const int* len, const int* order, const uint8_t* ignore,
                 hipStream_t st) {
  // the input projection holds rows x 2048 fp32 values: callers split larger batches (eioku_amd/ocr.py: 65,536 rows)
  EIOKU_REQUIRE(rows <= (1 << 18), "%lld sequence steps in one call (at most 262,144: split the crops)", rows);
  const int C = r->num_class;
  EIOKU_TRY(r->seq.grow((size_t)rows * kHid));
  EIOKU_TRY(r->gx.grow((size_t)rows * 8 * kHid));
  EIOKU_TRY(r->hid32.grow((size_t)rows * 2 * kHid));
  EIOKU_TRY(r->logits.grow((size_t)rows * C));
  EIOKU_TRY(r->prob.grow((size_t)rows));
  EIOKU_TRY(r->idx.grow((size_t)rows));
  EIOKU_TRY(r->offlen.grow((size_t)3 * m));
  EIOKU_TRY(r->ignore.grow((size_t)C));
  EIOKU_HIP_CHECK(hipMemcpyAsync(r->ignore, ignore, (size_t)C, hipMemcpyHostToDevice, st));
  std::vector<int>& ol = r->hofflen;  // kept in the handle: the copy below is asynchronous
  ol.assign(3 * (size_t)m, 0);
  for (int i = 0; i < m; ++i) ol[i] = off[i], ol[m + i] = len[i];
  if (order)
    for (int i = 0; i < m; ++i) ol[2 * m + i] = off[order[i]];
  EIOKU_HIP_CHECK(hipMemcpyAsync(r->offlen, ol.data(), ol.size() * 4, hipMemcpyHostToDevice, st));
  return EIOKU_OK;
}

// r->seq [rows][256] -> two BiLSTMs (input projection: one GEMM for both directions; recurrence; Linear(512, 256)),
// Prediction, k_ctc_probs -> HOST idx_out, prob_out [rows], logits_out [rows][num_class] (optional).  Synchronises.
int tail_run(eioku_crnn* r, long long rows, int m, int32_t* idx_out, float* prob_out, float* logits_out, hipStream_t st, double* fl) {
  const int C = r->num_class;
  int rc;
  for (int l = 0; l < 2; ++l) {
    if ((rc = gemm_f32(r->seq, (int)rows, kHid, r->wih[l], 8 * kHid, r->bih[l], r->gx, st, fl))) return rc;
    hipLaunchKernelGGL(k_lstm, dim3((unsigned)((m + kSeqTile - 1) / kSeqTile), 2), dim3(kHid), 0, st, r->gx.p, r->whh[l].p, r->offlen.p,
                       r->offlen + m, m, r->hid32.p);
    EIOKU_LAUNCH_CHECK();
    *fl += 2.0 * 2 * 4 * kHid * kHid * rows;
    if ((rc = gemm_f32(r->hid32, (int)rows, 2 * kHid, r->wlin[l], kHid, r->blin[l], r->seq, st, fl))) return rc;
  }
  if ((rc = gemm_f32(r->seq, (int)rows, kHid, r->wpred, C, r->bpred, r->logits, st, fl))) return rc;
  if ((rc = ctc_probs(r->logits, (int)rows, C, r->ignore, r->idx, r->prob, st))) return rc;
  EIOKU_HIP_CHECK(hipMemcpyAsync(idx_out, r->idx, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
  EIOKU_HIP_CHECK(hipMemcpyAsync(prob_out, r->prob, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
  if (logits_out) EIOKU_HIP_CHECK(hipMemcpyAsync(logits_out, r->logits, (size_t)rows * C * 4, hipMemcpyDeviceToHost, st));
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

// N staged frames -> out [N][H][W][8] fp16
int craft_prep(const eioku_craft* r, const uint8_t* d_src, int N, int h, int w, const Canvas& c, __half* out, hipStream_t st) {
  hipLaunchKernelGGL(k_craft_prep, dim3(grid1((long long)N * c.H * c.W)), dim3(256), 0, st, d_src, N, h, w, c.th, c.tw, c.H, c.W,
                     r->taps.p, c.copy ? 1 : 0, out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // namespace

extern "C" {

int eioku_craft_create(eioku_craft_t** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL argument");
  auto* r = new eioku_craft();
  // state dict prefixes of EasyOCR's craft.CRAFT (vgg16_bn basenet, U-Net, conv_cls); fc6's 3x3 / dilation 6 runs as
  // a 4608-channel 1x1 over an im2col (cin reported as 512, ksize 3)
  r->convs.add_all({{"basenet.slice1.0", 64, 3, 3},     {"basenet.slice1.3", 64, 64, 3},    {"basenet.slice1.7", 128, 64, 3},
                    {"basenet.slice1.10", 128, 128, 3}, {"basenet.slice2.14", 256, 128, 3}, {"basenet.slice2.17", 256, 256, 3},
                    {"basenet.slice3.20", 256, 256, 3}, {"basenet.slice3.24", 512, 256, 3}, {"basenet.slice3.27", 512, 512, 3},
                    {"basenet.slice4.30", 512, 512, 3}, {"basenet.slice4.34", 512, 512, 3}, {"basenet.slice4.37", 512, 512, 3},
                    {"basenet.slice5.1", 1024, 512, 3}, {"basenet.slice5.2", 1024, 1024, 1}, {"upconv1.conv.0", 512, 1536, 1},
                    {"upconv1.conv.3", 256, 512, 3},    {"upconv2.conv.0", 256, 768, 1},    {"upconv2.conv.3", 128, 256, 3},
                    {"upconv3.conv.0", 128, 384, 1},    {"upconv3.conv.3", 64, 128, 3},     {"upconv4.conv.0", 64, 192, 1},
                    {"upconv4.conv.3", 32, 64, 3},      {"conv_cls.0", 32, 32, 3},          {"conv_cls.2", 32, 32, 3},
                    {"conv_cls.4", 16, 32, 3},          {"conv_cls.6", 16, 16, 1},          {"conv_cls.8", 2, 16, 1}});
  *out = r;
  return EIOKU_OK;
}

void eioku_craft_destroy(eioku_craft_t* r) {
  if (!r) return;
  (void)hipDeviceSynchronize();
  delete r;
}

int eioku_craft_num_convs(const eioku_craft_t* r) { return r ? r->convs.size() : 0; }

int eioku_craft_conv_info(const eioku_craft_t* r, int idx, char* name, size_t cap, int* cout, int* cin, int* ksize) {
  EIOKU_REQUIRE(r, "bad convolution index %d", idx);
  return r->convs.info(idx, name, cap, cout, cin, ksize, nullptr);
}

// weight HOST fp32 [cout][cin][k][k] with the following BatchNorm folded in, bias HOST fp32 [cout]
int eioku_craft_set_conv(eioku_craft_t* r, int idx, const float* w, const float* b) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && idx >= 0 && idx < r->convs.size() && w && b, "bad argument");
  const ConvLayer& l = r->convs.layers[idx];
  ConvWeights* cw = &r->convs.w[idx];
  if (idx == 0) return r->convs.mark(idx, conv_weights_create_cin8(cw, l.cout, l.cin, 3, 1, w, b));  // the canvas has 8 channels
  if (l.name != "basenet.slice5.1") return r->convs.mark(idx, conv_weights_create(cw, l.cout, l.cin, l.k, 1, w, b));
  // fc6: [o][c][ky][kx] -> 1x1 over im2col channel (ky * 3 + kx) * 512 + c
  std::vector<float> wc((size_t)l.cout * 9 * l.cin);
  for (int o = 0; o < l.cout; ++o)
    for (int c = 0; c < l.cin; ++c)
      for (int t = 0; t < 9; ++t) wc[((size_t)o * 9 + t) * l.cin + c] = w[((size_t)o * l.cin + c) * 9 + t];
  return r->convs.mark(idx, conv_weights_create(cw, l.cout, 9 * l.cin, 1, 1, wc.data(), b));
}

// n BGR u8 frames h x w (host or device per mem) -> per frame the CRAFT score maps at half the canvas: text_out,
// link_out [n][H/2][W/2] fp32 and bin_out [n][H/2][W/2] u8 = (text > low_text) | (link > link_threshold), each DEVICE and
// optional.  Canvas: long side <= canvas_size: the frame itself, else OpenCV INTER_LINEAR to (int(h r), int(w r)) with
// r = canvas_size / max(h, w); then padded to multiples of 32 (H, W).  Synchronous.
int eioku_craft_forward(eioku_craft_t* r, const uint8_t* bgr, int n, int h, int w, int canvas_size, float low_text,
                        float link_threshold, float* text_out, float* link_out, uint8_t* bin_out, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && n >= 0, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  EIOKU_TRY(r->convs.all_set());
  Canvas cv;
  int rc = canvas_of(h, w, canvas_size, &cv);
  if (rc) return rc;
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr, "NULL frames");
  hipStream_t st = (hipStream_t)stream_;
  // H, W are multiples of 32: every interpolate in CRAFT is then an exact 2x (H / 16 -> H / 8 -> H / 4 -> H / 2)
  const int H = cv.H, W = cv.W;
  const long long fpx = (long long)H * W;
  // frames per pass: the widest tensor (64 channels at the full canvas) must stay within 32-bit element offsets
  const int chunk = (int)std::max(1LL, std::min(8LL, ((1LL << 31) - 1) / (fpx * 64)));
  const uint8_t* d_src = nullptr;
  if ((rc = craft_stage(r, bgr, n, h, w, cv, mem, st, &d_src))) return rc;
  const int cN = std::min(chunk, n);
  EIOKU_TRY(r->in8.grow((size_t)cN * fpx * 8));
  EIOKU_TRY(r->p0.grow((size_t)cN * fpx * 64));
  EIOKU_TRY(r->p1.grow((size_t)cN * fpx * 64));
  EIOKU_TRY(r->cat4.grow((size_t)cN * fpx / 4 * 192));
  EIOKU_TRY(r->cat3.grow((size_t)cN * fpx / 16 * 384));
  EIOKU_TRY(r->cat2.grow((size_t)cN * fpx / 64 * 768));
  EIOKU_TRY(r->cat1.grow((size_t)cN * fpx / 256 * 1536));
  EIOKU_TRY(r->col.grow((size_t)cN * fpx / 256 * 4608));
  EIOKU_TRY(r->y.grow((size_t)cN * fpx / 4 * 2));
  const auto& L = r->convs.w;
  double fl = 0;
  for (int f0 = 0; f0 < n; f0 += chunk) {
    const int N = std::min(chunk, n - f0);
    if ((rc = craft_prep(r, d_src + (size_t)f0 * h * w * 3, N, h, w, cv, r->in8, st))) return rc;
    int Hc = H, Wc = W;
    __half *P0 = r->p0, *P1 = r->p1;
    // slice1: conv1_1, conv1_2, pool, conv2_1, conv2_2 (+ slice2's in-place ReLU: the skip of upconv4)
    if ((rc = conv(L[0], Slice{r->in8, 8, 0}, N, Hc, Wc, Slice{P0, 64, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[1], Slice{P0, 64, 0}, N, Hc, Wc, Slice{P1, 64, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = maxpool(Slice{P1, 64, 0}, N, Hc, Wc, 64, 2, 2, 2, 2, 0, 0, Slice{P0, 64, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[2], Slice{P0, 64, 0}, N, Hc, Wc, Slice{P1, 128, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[3], Slice{P1, 128, 0}, N, Hc, Wc, Slice{r->cat4, 192, 64}, nullptr, kActReLU, st, &fl))) return rc;
    // slice2: pool, conv3_1, conv3_2 (+ slice3's in-place ReLU: the skip of upconv3)
    if ((rc = maxpool(Slice{r->cat4, 192, 64}, N, Hc, Wc, 128, 2, 2, 2, 2, 0, 0, Slice{P0, 128, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[4], Slice{P0, 128, 0}, N, Hc, Wc, Slice{P1, 256, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[5], Slice{P1, 256, 0}, N, Hc, Wc, Slice{r->cat3, 384, 128}, nullptr, kActReLU, st, &fl))) return rc;
    // slice3: conv3_3, pool, conv4_1, conv4_2 (+ slice4's in-place ReLU: the skip of upconv2)
    if ((rc = conv(L[6], Slice{r->cat3, 384, 128}, N, Hc, Wc, Slice{P1, 256, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = maxpool(Slice{P1, 256, 0}, N, Hc, Wc, 256, 2, 2, 2, 2, 0, 0, Slice{P0, 256, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[7], Slice{P0, 256, 0}, N, Hc, Wc, Slice{P1, 512, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[8], Slice{P1, 512, 0}, N, Hc, Wc, Slice{r->cat2, 768, 256}, nullptr, kActReLU, st, &fl))) return rc;
    // slice4: conv4_3, pool, conv5_1, conv5_2 (BN output: slice5 opens with a max pool, so the skip of upconv1 keeps
    // its negative values)
    if ((rc = conv(L[9], Slice{r->cat2, 768, 256}, N, Hc, Wc, Slice{P1, 512, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = maxpool(Slice{P1, 512, 0}, N, Hc, Wc, 512, 2, 2, 2, 2, 0, 0, Slice{P0, 512, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[10], Slice{P0, 512, 0}, N, Hc, Wc, Slice{P1, 512, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[11], Slice{P1, 512, 0}, N, Hc, Wc, Slice{r->cat1, 1536, 1024}, nullptr, kActNone, st, &fl))) return rc;
    // slice5: 3x3 / s1 / p1 max pool (no ReLU before it), fc6 (dilation 6), fc7 - no activation in between
    if ((rc = maxpool(Slice{r->cat1, 1536, 1024}, N, Hc, Wc, 512, 3, 3, 1, 1, 1, 1, Slice{P0, 512, 0}, st, nullptr, nullptr)))
      return rc;
    const long long px16 = (long long)N * Hc * Wc;
    if ((rc = im2col_dil(P0, N, Hc, Wc, 512, 6, r->col, st))) return rc;
    if ((rc = conv_forward(L[12], Slice{r->col, 4608, 0}, N, Hc, Wc, Slice{P1, 1024, 0}, nullptr, Slice{}, kActNone, st))) return rc;
    fl += 2.0 * 1024 * 512 * 9 * px16;
    if ((rc = conv(L[13], Slice{P1, 1024, 0}, N, Hc, Wc, Slice{r->cat1, 1536, 0}, nullptr, kActNone, st, &fl))) return rc;
    // U-Net: double_conv (1x1 + BN + ReLU, 3x3 + BN + ReLU), then 2x bilinear into the next concat
    if ((rc = conv(L[14], Slice{r->cat1, 1536, 0}, N, Hc, Wc, Slice{P0, 512, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[15], Slice{P0, 512, 0}, N, Hc, Wc, Slice{P1, 256, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = up2x(P1, N, Hc, Wc, 256, Slice{r->cat2, 768, 0}, st))) return rc;
    Hc *= 2, Wc *= 2;
    if ((rc = conv(L[16], Slice{r->cat2, 768, 0}, N, Hc, Wc, Slice{P0, 256, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[17], Slice{P0, 256, 0}, N, Hc, Wc, Slice{P1, 128, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = up2x(P1, N, Hc, Wc, 128, Slice{r->cat3, 384, 0}, st))) return rc;
    Hc *= 2, Wc *= 2;
    if ((rc = conv(L[18], Slice{r->cat3, 384, 0}, N, Hc, Wc, Slice{P0, 128, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[19], Slice{P0, 128, 0}, N, Hc, Wc, Slice{P1, 64, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = up2x(P1, N, Hc, Wc, 64, Slice{r->cat4, 192, 0}, st))) return rc;
    Hc *= 2, Wc *= 2;
    if ((rc = conv(L[20], Slice{r->cat4, 192, 0}, N, Hc, Wc, Slice{P0, 64, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[21], Slice{P0, 64, 0}, N, Hc, Wc, Slice{P1, 32, 0}, nullptr, kActReLU, st, &fl))) return rc;
    // conv_cls
    if ((rc = conv(L[22], Slice{P1, 32, 0}, N, Hc, Wc, Slice{P0, 32, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[23], Slice{P0, 32, 0}, N, Hc, Wc, Slice{P1, 32, 0}, nullptr, kActReLU, st, &fl))) return rc;
    // the 16-channel tensors sit in 32-channel strides: K4's 1x1 reads whole 32-channel chunks (the tail is zeroed in the
    // kernel, but its address must stay inside the tensor)
    if ((rc = conv(L[24], Slice{P1, 32, 0}, N, Hc, Wc, Slice{P0, 32, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[25], Slice{P0, 32, 0}, N, Hc, Wc, Slice{P1, 32, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[26], Slice{P1, 32, 0}, N, Hc, Wc, Slice{}, r->y, kActNone, st, &fl))) return rc;
    const long long hpx = (long long)Hc * Wc, off = (long long)f0 * hpx;
    hipLaunchKernelGGL(k_craft_maps, dim3(grid1(N * hpx)), dim3(256), 0, st, r->y.p, N * hpx, low_text, link_threshold,
                       text_out ? text_out + off : nullptr, link_out ? link_out + off : nullptr, bin_out ? bin_out + off : nullptr);
    EIOKU_LAUNCH_CHECK();
  }
  r->flops_last = fl;
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

int eioku_craft_last_flops(const eioku_craft_t* r, double* flops) {
  EIOKU_REQUIRE(r && flops, "NULL argument");
  *flops = r->flops_last;
  return EIOKU_OK;
}

// Stage: the canvas alone.  n BGR u8 frames (host or device per mem) -> out DEVICE fp16 [n][H][W][8], the network's
// input as eioku_craft_forward makes it (k_craft_prep with the same taps; channels 3..7 zero).  The handle lends its
// staging buffers and needs no weights.  Synchronous.
int eioku_craft_canvas(eioku_craft_t* r, const uint8_t* bgr, int n, int h, int w, int canvas_size, void* out, int mem,
                       void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && n >= 0, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  Canvas cv;
  int rc = canvas_of(h, w, canvas_size, &cv);
  if (rc) return rc;
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr, "NULL frames");
  if ((rc = check_slice(out, 8, 0, 8, (long long)n * cv.H * cv.W, "canvas"))) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const uint8_t* d_src = nullptr;
  if ((rc = craft_stage(r, bgr, n, h, w, cv, mem, st, &d_src))) return rc;
  if ((rc = craft_prep(r, d_src, n, h, w, cv, (__half*)out, st))) return rc;
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

// Stages: the glue kernels alone, over the caller's DEVICE fp16 NHWC tensors; asynchronous on the stream.
// in: channels in_coff .. + c of [n][h][w][in_cstride] -> out: channels out_coff .. + c of [n][ho][wo][out_cstride],
// ho = (h + 2 ph - kh) / sh + 1 (wo alike); padding never wins a maximum
int eioku_ocr_maxpool_f16(const void* in, int in_cstride, int in_coff, int n, int h, int w, int c, int kh, int kw, int sh, int sw,
                          int ph, int pw, void* out, int out_cstride, int out_coff, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(n > 0 && h > 0 && w > 0, "bad shape %d x %d x %d", n, h, w);
  EIOKU_REQUIRE(kh > 0 && kw > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0 && 2 * ph <= kh && 2 * pw <= kw,
                "bad window %d x %d / (%d, %d) / pad (%d, %d)", kh, kw, sh, sw, ph, pw);
  EIOKU_REQUIRE(h + 2 * ph >= kh && w + 2 * pw >= kw, "window %d x %d exceeds the padded %d x %d input", kh, kw, h, w);
  const int ho = (h + 2 * ph - kh) / sh + 1, wo = (w + 2 * pw - kw) / sw + 1;
  int rc;
  if ((rc = check_slice(in, in_cstride, in_coff, c, (long long)n * h * w, "max pool input"))) return rc;
  if ((rc = check_slice(out, out_cstride, out_coff, c, (long long)n * ho * wo, "max pool output"))) return rc;
  return maxpool(Slice{(__half*)in, in_cstride, in_coff}, n, h, w, c, kh, kw, sh, sw, ph, pw, Slice{(__half*)out, out_cstride, out_coff},
                 (hipStream_t)stream_, nullptr, nullptr);
}

// dense in [n][h][w][c] -> dense out [n][h][w][9][c]: the taps of a 3x3 / dilation d / pad d convolution, zero outside
int eioku_ocr_im2col_dil_f16(const void* in, int n, int h, int w, int c, int d, void* out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(n > 0 && h > 0 && w > 0 && d > 0 && d <= 1 << 16, "bad shape %d x %d x %d, dilation %d", n, h, w, d);
  int rc;
  if ((rc = check_slice(in, c, 0, c, (long long)n * h * w, "im2col input"))) return rc;
  if ((rc = check_slice(out, c, 0, c, (long long)n * h * w * 9, "im2col output"))) return rc;
  return im2col_dil((const __half*)in, n, h, w, c, d, (__half*)out, (hipStream_t)stream_);
}

// dense in [n][h][w][c] -> channels out_coff .. + c of out [n][2h][2w][out_cstride]: bilinear, align_corners=False
int eioku_ocr_up2x_f16(const void* in, int n, int h, int w, int c, void* out, int out_cstride, int out_coff, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(n > 0 && h > 0 && w > 0 && h <= 1 << 15 && w <= 1 << 15, "bad shape %d x %d x %d", n, h, w);
  int rc;
  if ((rc = check_slice(in, c, 0, c, (long long)n * h * w, "upsample input"))) return rc;
  if ((rc = check_slice(out, out_cstride, out_coff, c, (long long)n * 4 * h * w, "upsample output"))) return rc;
  return up2x((const __half*)in, n, h, w, c, Slice{(__half*)out, out_cstride, out_coff}, (hipStream_t)stream_);
}

// ---- K16 -----------------------------------------------------------------------------------------------------------

int eioku_crnn_create(int num_class, eioku_crnn_t** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out && num_class >= 2 && num_class <= 4096, "bad argument");
  auto* r = new eioku_crnn();
  r->num_class = num_class;
  // vgg_model.VGG_FeatureExtractor(1, 256) state dict prefixes (BatchNorm folded into ConvNet.11 / .14), then Prediction
  r->convs.add_all({{"FeatureExtraction.ConvNet.0", 32, 1, 3},     {"FeatureExtraction.ConvNet.3", 64, 32, 3},
                    {"FeatureExtraction.ConvNet.6", 128, 64, 3},   {"FeatureExtraction.ConvNet.8", 128, 128, 3},
                    {"FeatureExtraction.ConvNet.11", 256, 128, 3}, {"FeatureExtraction.ConvNet.14", 256, 256, 3},
                    {"FeatureExtraction.ConvNet.18", 256, 256, 2}, {"Prediction", num_class, kHid, 1}});
  *out = r;
  return EIOKU_OK;
}

void eioku_crnn_destroy(eioku_crnn_t* r) {
  if (!r) return;
  (void)hipDeviceSynchronize();
  delete r;
}

int eioku_crnn_num_convs(const eioku_crnn_t* r) { return r ? r->convs.size() : 0; }

int eioku_crnn_conv_info(const eioku_crnn_t* r, int idx, char* name, size_t cap, int* cout, int* cin, int* ksize) {
  EIOKU_REQUIRE(r, "bad convolution index %d", idx);
  return r->convs.info(idx, name, cap, cout, cin, ksize, nullptr);
}

// weight HOST fp32 [cout][cin][k][k] (BatchNorm folded in), bias HOST fp32 [cout]; "Prediction": [num_class][256]
int eioku_crnn_set_conv(eioku_crnn_t* r, int idx, const float* w, const float* b) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && idx >= 0 && idx < r->convs.size() && w && b, "bad argument");
  const ConvLayer& l = r->convs.layers[idx];
  ConvWeights* cw = &r->convs.w[idx];
  if (idx == 0) return r->convs.mark(idx, conv_weights_create_cin8(cw, l.cout, l.cin, 3, 1, w, b));  // the crop has 8 channels
  if (l.name == "Prediction") {  // fp32 GEMM operand
    int rc = r->wpred.upload(w, (size_t)l.cout * l.cin);
    if (!rc) rc = r->bpred.upload(b, (size_t)l.cout);
    return r->convs.mark(idx, rc);
  }
  if (l.k != 2) return r->convs.mark(idx, conv_weights_create(cw, l.cout, l.cin, l.k, 1, w, b));
  // 2x2 valid -> 3x3 / pad 1 with the weights in the bottom-right 2x2
  std::vector<float> w3((size_t)l.cout * l.cin * 9, 0.f);
  for (size_t i = 0; i < (size_t)l.cout * l.cin; ++i)
    for (int ky = 0; ky < 2; ++ky)
      for (int kx = 0; kx < 2; ++kx) w3[i * 9 + (ky + 1) * 3 + kx + 1] = w[i * 4 + ky * 2 + kx];
  return r->convs.mark(idx, conv_weights_create(cw, l.cout, l.cin, 3, 1, w3.data(), b));
}

// BiLSTM layer (0 or 1) of SequenceModeling: nn.LSTM(256, 256, bidirectional) + Linear(512, 256), HOST fp32, PyTorch
// layouts: w_ih [2][1024][256] (forward, reverse), w_hh [2][1024][256], b_ih [2][1024], b_hh [2][1024], w_lin [256][512],
// b_lin [256]
int eioku_crnn_set_lstm(eioku_crnn_t* r, int layer, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                        const float* w_lin, const float* b_lin) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && layer >= 0 && layer < 2 && w_ih && w_hh && b_ih && b_hh && w_lin && b_lin, "bad argument");
  constexpr int G = 4 * kHid;
  std::vector<float> b(2 * G);
  for (int i = 0; i < 2 * G; ++i) b[i] = b_ih[i] + b_hh[i];
  r->lstm_set[layer] = false;
  EIOKU_TRY(r->wih[layer].upload(w_ih, (size_t)2 * G * kHid));
  EIOKU_TRY(r->bih[layer].upload(b.data(), (size_t)2 * G));
  EIOKU_TRY(r->wlin[layer].upload(w_lin, (size_t)kHid * 2 * kHid));
  EIOKU_TRY(r->blin[layer].upload(b_lin, (size_t)kHid));
  std::vector<float> t((size_t)2 * kHid * G);
  for (int d = 0; d < 2; ++d)
    for (int g = 0; g < G; ++g)
      for (int k = 0; k < kHid; ++k) t[((size_t)d * kHid + k) * G + g] = w_hh[((size_t)d * G + g) * kHid + k];
  EIOKU_TRY(r->whh[layer].upload(t.data(), t.size()));
  r->lstm_set[layer] = true;
  return EIOKU_OK;
}

// m crops, each imgs HOST fp32 [64][widths[i]] already normalised and right-padded ((x / 255 - 0.5) / 0.5, packed one
// after another), widths[i] % 4 == 0 and >= 8.  ignore HOST u8 [num_class] (1: class zeroed before renormalising).
// Sequence i has T_i = widths[i] / 4 - 1 steps, rows packed in crop order: idx_out [sum T] int32 (argmax class),
// prob_out [sum T] fp32 (its probability), logits_out [sum T][num_class] fp32 (optional), all HOST.  Crops of equal width
// share the convolutions; every sequence keeps its own length through the BiLSTMs.  Synchronous.
int eioku_crnn_forward(eioku_crnn_t* r, const float* imgs, const int* widths, int m, const uint8_t* ignore, int32_t* idx_out,
                       float* prob_out, float* logits_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && m >= 0, "bad argument");
  for (int i = 0; i < r->convs.size(); ++i) EIOKU_REQUIRE(r->convs.set[i], "%s has no weights", r->convs.layers[i].name.c_str());
  EIOKU_REQUIRE(r->lstm_set[0] && r->lstm_set[1], "BiLSTM layers have no weights");
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(imgs && widths && ignore && idx_out && prob_out, "NULL buffer");
  hipStream_t st = (hipStream_t)stream_;
  std::vector<int> off(m), len(m);
  std::vector<size_t> ioff(m);
  long long rows = 0;
  size_t ipos = 0;
  int wmax = 0;
  for (int i = 0; i < m; ++i) {
    EIOKU_REQUIRE(widths[i] >= 8 && widths[i] % 4 == 0 && widths[i] <= 1 << 16, "crop %d: width %d (a multiple of 4, >= 8)", i,
                  widths[i]);
    off[i] = (int)rows;
    len[i] = widths[i] / 4 - 1;
    rows += len[i];
    ioff[i] = ipos;
    ipos += (size_t)64 * widths[i];
    wmax = std::max(wmax, widths[i]);
  }
  // crops grouped by width (ascending), each group one pass of the convolutions; at most kGroup crops per pass
  std::vector<int> order(m);
  for (int i = 0; i < m; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return widths[a] < widths[b]; });
  constexpr int kGroup = 64;
  int rc;
  if ((rc = tail_reserve(r, rows, m, off.data(), len.data(), order.data(), ignore, st))) return rc;
  const size_t gpx = (size_t)kGroup * 64 * wmax;
  EIOKU_TRY(r->img.grow(gpx * 8));
  EIOKU_TRY(r->a0.grow(gpx * 32));
  EIOKU_TRY(r->a1.grow(gpx * 32));
  const auto& L = r->convs.w;
  double fl = 0;
  for (int g0 = 0; g0 < m;) {
    const int wp = widths[order[g0]];
    int g1 = g0;
    while (g1 < m && g1 - g0 < kGroup && widths[order[g1]] == wp) ++g1;
    const int N = g1 - g0;
    EIOKU_HIP_CHECK(hipStreamSynchronize(st));  // the previous group's upload has left r->himg
    r->himg.assign((size_t)N * 64 * wp * 8, (__half)0.f);
    for (int s = 0; s < N; ++s) {
      const float* src = imgs + ioff[order[g0 + s]];
      __half* dst = r->himg.data() + (size_t)s * 64 * wp * 8;
      for (size_t p = 0; p < (size_t)64 * wp; ++p) dst[p * 8] = (__half)src[p];
    }
    EIOKU_HIP_CHECK(hipMemcpyAsync(r->img, r->himg.data(), r->himg.size() * 2, hipMemcpyHostToDevice, st));
    int Hc = 64, Wc = wp;
    __half *A = r->a0, *B = r->a1;
    if ((rc = conv(L[0], Slice{r->img, 8, 0}, N, Hc, Wc, Slice{A, 32, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = maxpool(Slice{A, 32, 0}, N, Hc, Wc, 32, 2, 2, 2, 2, 0, 0, Slice{B, 32, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[1], Slice{B, 32, 0}, N, Hc, Wc, Slice{A, 64, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = maxpool(Slice{A, 64, 0}, N, Hc, Wc, 64, 2, 2, 2, 2, 0, 0, Slice{B, 64, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[2], Slice{B, 64, 0}, N, Hc, Wc, Slice{A, 128, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[3], Slice{A, 128, 0}, N, Hc, Wc, Slice{B, 128, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = maxpool(Slice{B, 128, 0}, N, Hc, Wc, 128, 2, 1, 2, 1, 0, 0, Slice{A, 128, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[4], Slice{A, 128, 0}, N, Hc, Wc, Slice{B, 256, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = conv(L[5], Slice{B, 256, 0}, N, Hc, Wc, Slice{A, 256, 0}, nullptr, kActReLU, st, &fl))) return rc;
    if ((rc = maxpool(Slice{A, 256, 0}, N, Hc, Wc, 256, 2, 1, 2, 1, 0, 0, Slice{B, 256, 0}, st, &Hc, &Wc))) return rc;
    if ((rc = conv(L[6], Slice{B, 256, 0}, N, Hc, Wc, Slice{A, 256, 0}, nullptr, kActReLU, st, &fl))) return rc;
    fl += 2.0 * 256 * 256 * 4 * N * (Hc - 1) * (Wc - 1) - L[6].flops_per_pixel() * N * Hc * Wc;  // algorithmic: 2x2 valid
    hipLaunchKernelGGL(k_row_mean, dim3(grid1((long long)N * (Wc - 1) * kHid)), dim3(256), 0, st, A, N, Wc, kHid,
                       r->offlen + 2 * m + g0, r->seq.p);
    EIOKU_LAUNCH_CHECK();
    g0 = g1;
  }
  if ((rc = tail_run(r, rows, m, idx_out, prob_out, logits_out, st, &fl))) return rc;
  r->flops_last = fl;
  return EIOKU_OK;
}

// Stage: the recogniser from its packed sequences on (the first GEMM through k_ctc_probs, as eioku_crnn_forward runs
// them).  seq HOST fp32 [sum len][256]: m sequences of len[i] >= 1 steps, one after another; ignore, idx_out, prob_out,
// logits_out as eioku_crnn_forward.  Needs the BiLSTM and "Prediction" weights only.  Synchronous.
int eioku_crnn_tail(eioku_crnn_t* r, const float* seq, const int* len, int m, const uint8_t* ignore, int32_t* idx_out,
                    float* prob_out, float* logits_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && m >= 0, "bad argument");
  EIOKU_REQUIRE(r->convs.set.back(), "Prediction has no weights");
  EIOKU_REQUIRE(r->lstm_set[0] && r->lstm_set[1], "BiLSTM layers have no weights");
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(seq && len && ignore && idx_out && prob_out, "NULL buffer");
  hipStream_t st = (hipStream_t)stream_;
  std::vector<int> off(m);
  long long rows = 0;
  for (int i = 0; i < m; ++i) {
    EIOKU_REQUIRE(len[i] >= 1 && len[i] < 1 << 14, "sequence %d: %d steps (1 .. 16,383)", i, len[i]);
    off[i] = (int)rows;
    rows += len[i];
  }
  int rc;
  if ((rc = tail_reserve(r, rows, m, off.data(), len, nullptr, ignore, st))) return rc;
  EIOKU_HIP_CHECK(hipMemcpyAsync(r->seq, seq, (size_t)rows * kHid * 4, hipMemcpyHostToDevice, st));
  double fl = 0;
  if ((rc = tail_run(r, rows, m, idx_out, prob_out, logits_out, st, &fl))) return rc;
  r->flops_last = fl;
  return EIOKU_OK;
}

// Stage: k_ctc_probs alone.  logits DEVICE fp32 [rows][C], ignore DEVICE u8 [C] (not all set), 2 <= C <= 4096 -> idx_out
// [rows] int32, prob_out [rows] fp32, DEVICE; asynchronous on the stream.
int eioku_ctc_probs(const float* logits, int rows, int C, const uint8_t* ignore, int32_t* idx_out, float* prob_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(rows >= 0 && C >= 2 && C <= 4096, "bad shape %d x %d (2 <= classes <= 4096)", rows, C);
  if (rows == 0) return EIOKU_OK;
  EIOKU_REQUIRE(logits && ignore && idx_out && prob_out, "NULL buffer");
  EIOKU_REQUIRE((long long)rows * C <= (1LL << 31) - 1, "%d x %d logits exceed 32-bit element offsets", rows, C);
  return ctc_probs(logits, rows, C, ignore, idx_out, prob_out, (hipStream_t)stream_);
}

int eioku_crnn_last_flops(const eioku_crnn_t* r, double* flops) {
  EIOKU_REQUIRE(r && flops, "NULL argument");
  *flops = r->flops_last;
  return EIOKU_OK;
}

}  // extern "C"
