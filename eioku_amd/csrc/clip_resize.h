// Pillow's two-pass 8-bit resample of the centre-crop region, shared by K25 (actions.hip: bilinear tables, clips of T frames)
// and K26 (clip.hip: bicubic tables, single images).  The filter lives in the host's tables (22-bit fixed-point taps, which
// may be negative), so the kernels are the same for both; only the patch-row layout has arguments.  Everything here has
// internal linkage.
#pragma once

#include "common.h"
#include "gemm_f16.h"

namespace {

constexpr int kPrec = 22;  // Pillow Resample.c PRECISION_BITS for 8-bit pixels

// bounds [S][2] = {first input index, taps}; kk [S][ksize] int32 taps scaled by 2^22: the rows of Pillow's tables for the
// resized axis that the centre crop keeps.  horizontal: src [N][h][w][3] u8, rows y0 .. y0 + rows - 1 only -> tmp
// [N][rows][S][3] u8; one thread per (row, output column)
__global__ __launch_bounds__(256) void k_clip_resize_h(const uint8_t* __restrict__ src, int N, int h, int w, int y0, int rows, int S,
                                                       const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                       uint8_t* __restrict__ tmp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * rows * S) return;
  const int xx = (int)(i % S);
  const long long row = i / S;
  const int y = (int)(row % rows), n = (int)(row / rows);
  const int lo = bounds[2 * xx], cnt = bounds[2 * xx + 1];
  const uint8_t* p = src + (((size_t)n * h + y0 + y) * w + lo) * 3;
  int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const int k = kk[xx * ksize + t];
    s0 += p[3 * t] * k;
    s1 += p[3 * t + 1] * k;
    s2 += p[3 * t + 2] * k;
  }
  auto clip8 = [](int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
  uint8_t* o = tmp + (size_t)i * 3;
  o[0] = clip8(s0 >> kPrec);
  o[1] = clip8(s1 >> kPrec);
  o[2] = clip8(s2 >> kPrec);
}

struct Norm3 {
  float mean[3], std[3];  // R, G, B
};

// vertical + rescale + normalise: tmp [N][rows][S][3] u8 (B, G, R), N = clips * T frames -> patch rows of `ld` halfs,
// [clip][tok0 + patch][frame][c * p * p + ky * p + kx] fp16 (c = R, G, B; p = patch; tok0 rows at the head of every clip
// and the columns from 3 p p to ld are not written) and / or out_u8 [N][S][S][3] (R, G, B)
__global__ __launch_bounds__(256) void k_clip_resize_v(const uint8_t* __restrict__ tmp, int N, int T, int y0, int rows, int S,
                                                       const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                       Norm3 nrm, int patch_size, int tok0, int ld, h16* __restrict__ patches,
                                                       uint8_t* __restrict__ out_u8) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * S * S) return;
  const int x = (int)(i % S);
  const int yy = (int)((i / S) % S);
  const int n = (int)(i / ((long long)S * S));
  const int lo = bounds[2 * yy] - y0, cnt = bounds[2 * yy + 1];
  const uint8_t* p = tmp + (((size_t)n * rows + lo) * S + x) * 3;
  int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const int k = kk[yy * ksize + t];
    s0 += p[(size_t)t * S * 3] * k;
    s1 += p[(size_t)t * S * 3 + 1] * k;
    s2 += p[(size_t)t * S * 3 + 2] * k;
  }
  auto clip8 = [](int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); };
  const int rgb[3] = {clip8(s2 >> kPrec), clip8(s1 >> kPrec), clip8(s0 >> kPrec)};
  if (out_u8) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out_u8[(size_t)i * 3 + c] = (uint8_t)rgb[c];
  }
  if (patches) {
    const int side = S / patch_size, P = side * side, clip = n / T, t = n % T;
    const int patch = (yy / patch_size) * side + x / patch_size;
    h16* o = patches + (((size_t)clip * (tok0 + P) + tok0 + patch) * T + t) * ld + (yy % patch_size) * patch_size + x % patch_size;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * patch_size * patch_size] = (h16)(((float)rgb[c] * (1.0f / 255.0f) - nrm.mean[c]) / nrm.std[c]);
  }
}

int check_tables(const int32_t* bounds, int S, int k, int extent, const char* axis) {
  for (int i = 0; i < S; ++i) {
    const int lo = bounds[2 * i], cnt = bounds[2 * i + 1];
    EIOKU_REQUIRE(lo >= 0 && cnt >= 0 && cnt <= k && lo + cnt <= extent, "%s table row %d reads [%d, %d) of %d pixels with %d taps",
                  axis, i, lo, lo + cnt, extent, k);
  }
  return EIOKU_OK;
}

// The two passes over N frames of h x w (host or device per mem; src / tmp / tables are the caller's scratch): tables to
// the device, the source rows the vertical pass reads through the horizontal pass, then the vertical pass.
int clip_resize(const uint8_t* bgr, int N, int T, int h, int w, int S, const int32_t* xbounds, const int32_t* xk, int kx,
                const int32_t* ybounds, const int32_t* yk, int ky, const Norm3& nrm, int patch_size, int tok0, int ld, h16* patches,
                uint8_t* out_u8, int mem, eioku::DevBuf<int>& tables, eioku::DevBuf<uint8_t>& src, eioku::DevBuf<uint8_t>& tmp,
                hipStream_t stream) {
  using namespace eioku;
  EIOKU_TRY(check_tables(xbounds, S, kx, w, "x"));
  EIOKU_TRY(check_tables(ybounds, S, ky, h, "y"));
  int y0 = h, y1 = 0;  // the source rows the vertical pass reads
  for (int i = 0; i < S; ++i) {
    if (!ybounds[2 * i + 1]) continue;
    y0 = ybounds[2 * i] < y0 ? ybounds[2 * i] : y0;
    y1 = ybounds[2 * i] + ybounds[2 * i + 1] > y1 ? ybounds[2 * i] + ybounds[2 * i + 1] : y1;
  }
  EIOKU_REQUIRE(y1 > y0, "empty y table");
  const int rows = y1 - y0;
  EIOKU_TRY(grow_synced(tables, (size_t)S * (2 + kx + 2 + ky)));
  int* d_xb = tables;
  int* d_xk = d_xb + S * 2;
  int* d_yb = d_xk + (size_t)S * kx;
  int* d_yk = d_yb + S * 2;
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_xb, xbounds, (size_t)S * 2 * 4, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_xk, xk, (size_t)S * kx * 4, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_yb, ybounds, (size_t)S * 2 * 4, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_yk, yk, (size_t)S * ky * 4, hipMemcpyHostToDevice, stream));
  const uint8_t* d_src = bgr;
  if (mem == EIOKU_MEM_HOST) {
    const size_t bytes = (size_t)N * h * w * 3;
    EIOKU_TRY(grow_synced(src, bytes));
    EIOKU_HIP_CHECK(hipMemcpyAsync(src, bgr, bytes, hipMemcpyHostToDevice, stream));
    d_src = src;
  }
  EIOKU_TRY(grow_synced(tmp, (size_t)N * rows * S * 3));
  const long long w1 = (long long)N * rows * S, w2 = (long long)N * S * S;
  hipLaunchKernelGGL(k_clip_resize_h, dim3((unsigned)((w1 + 255) / 256)), dim3(256), 0, stream, d_src, N, h, w, y0, rows, S, d_xb, d_xk,
                     kx, tmp.p);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_clip_resize_v, dim3((unsigned)((w2 + 255) / 256)), dim3(256), 0, stream, tmp.p, N, T, y0, rows, S, d_yb, d_yk, ky,
                     nrm, patch_size, tok0, ld, patches, out_u8);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // namespace
