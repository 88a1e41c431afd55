// K18: scene thumbnails on gfx950 -- Pillow's bicubic resize and libjpeg's baseline encoder, byte for byte.
//
//   K18a  k_thumb_resize_h / k_thumb_resize_v   Pillow's two-pass 8-bit resample with host-built 22-bit tap tables
//         (eioku_amd/thumbs.py: bicubic_tables).  Horizontal first, 8-bit intermediate, then vertical; the horizontal
//         pass reads BGR and writes RGB.  One thread per output pixel.
//   K18b  k_jpeg_blocks   one thread per 8x8 block of a 4:2:0 scan: six blocks per 16x16 MCU (Y00 Y01 Y10 Y11 Cb Cr).
//         Colour conversion (16-bit fixed point), edge replication, h2v2 chroma averaging with the 1,2 bias, level
//         shift, the "islow" 13-bit integer DCT, rounded division by 8 q; 64 int16 per block in zigzag order.
//         Padding, as libjpeg does it: Y samples beyond the image replicate the last column / row.  Chroma columns
//         replicate the last pixel column; chroma ROWS beyond ceil(H / 2) copy the last downsampled row (pixel rows are
//         replicated only up to an even count before the averaging).  A luma block wholly beyond ceil(W / 8) block
//         columns or ceil(H / 8) block rows is a dummy: AC = 0, DC = the quantised DC of the block before it in the MCU.
//   K18c  k_jpeg_bitlen -> k_jpeg_scan -> k_jpeg_emit   Huffman coding with the Annex K tables.  (i) bit length of every
//         block's code (DC predictor: the previous block of the same component in scan order, 0 at the start of an
//         image); (ii) exclusive prefix sum per image, one workgroup per image, looped; (iii) every block writes its
//         bits MSB first at its offset into a zeroed buffer with atomicOr on byte-swapped 32-bit words, so the buffer
//         is the byte stream.  The host pads the last byte, stuffs FF -> FF 00 and writes the markers.
// All arithmetic is int32.  Buffers belong to the handle (no library scratch slot is used).
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int kPrec = 22;      // Pillow Resample.c PRECISION_BITS for 8-bit pixels
constexpr int kMaxSide = 1024; // thumbnail side
constexpr int kMaxN = 64;      // images per call
constexpr int kScanThreads = 256;

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- K18a ----------------------------------------------------------------------------------------------------------
// bounds [out][2] = {first input index, taps}; kk [out][ksize] int32 taps scaled by 2^22
// src [N][h][w][3] BGR -> tmp [N][h][tw][3] RGB
__global__ __launch_bounds__(256) void k_thumb_resize_h(const uint8_t* __restrict__ src, long long total, int w, int tw,
                                                        const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                        uint8_t* __restrict__ tmp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;  // total = N * h * tw
  const int xx = (int)(i % tw);
  const long long row = i / tw;
  const int lo = bounds[2 * xx], n = bounds[2 * xx + 1];
  const uint8_t* p = src + ((size_t)row * w + lo) * 3;
  const int* k = kk + (size_t)xx * ksize;
  int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < n; ++t) {
    const int c = k[t];
    s0 += p[3 * t] * c;
    s1 += p[3 * t + 1] * c;
    s2 += p[3 * t + 2] * c;
  }
  uint8_t* o = tmp + (size_t)i * 3;
  o[0] = (uint8_t)clip8(s2 >> kPrec);  // R
  o[1] = (uint8_t)clip8(s1 >> kPrec);
  o[2] = (uint8_t)clip8(s0 >> kPrec);  // B
}

// tmp [N][h][tw][3] -> out [N][th][tw][3]
__global__ __launch_bounds__(256) void k_thumb_resize_v(const uint8_t* __restrict__ tmp, long long total, int h, int th, int tw,
                                                        const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                        uint8_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;  // total = N * th * tw
  const int x = (int)(i % tw);
  const int yy = (int)((i / tw) % th);
  const long long n = i / ((long long)tw * th);
  const int lo = bounds[2 * yy], cnt = bounds[2 * yy + 1];
  const size_t pitch = (size_t)tw * 3;
  const uint8_t* p = tmp + (((size_t)n * h + lo) * tw + x) * 3;
  const int* k = kk + (size_t)yy * ksize;
  int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < cnt; ++t) {
    const int c = k[t];
    s0 += p[t * pitch] * c;
    s1 += p[t * pitch + 1] * c;
    s2 += p[t * pitch + 2] * c;
  }
  uint8_t* o = out + (size_t)i * 3;
  o[0] = (uint8_t)clip8(s0 >> kPrec);
  o[1] = (uint8_t)clip8(s1 >> kPrec);
  o[2] = (uint8_t)clip8(s2 >> kPrec);
}

// ---- K18b ----------------------------------------------------------------------------------------------------------
__device__ const uint8_t kZigzagOf[64] = {  // natural (row-major) index -> zigzag position
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c: one 8-point pass.  kFirst: the row pass (results scaled up by 2 bits), else the column pass.
template <bool kFirst>
__device__ __forceinline__ void dct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int sh = kFirst ? 13 - 2 : 13 + 2;
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kFirst) {
    d0 = (t10 + t11) * 4;
    d4 = (t10 - t11) * 4;
  } else {
    d0 = descale(t10 + t11, 2);
    d4 = descale(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  d2 = descale(z1 + t13 * 6270, sh);
  d6 = descale(z1 - t12 * 15137, sh);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = descale(u4 + z1 + z3, sh);
  d5 = descale(u5 + z2 + z4, sh);
  d3 = descale(u6 + z2 + z3, sh);
  d1 = descale(u7 + z1 + z4, sh);
}

// rgb [N][H][W][3]; qtab [2][64] divisors q (natural order); coef [N][nmcu][6][64] int16, zigzag
__global__ __launch_bounds__(64) void k_jpeg_blocks(const uint8_t* __restrict__ rgb, int N, int H, int W, int mx, int my,
                                                    const uint16_t* __restrict__ qtab, int16_t* __restrict__ coef) {
  const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
  const int nmcu = mx * my;
  if (gid >= (long long)N * nmcu * 6) return;
  const int slot = (int)(gid % 6);
  const int mcu = (int)((gid / 6) % nmcu);
  const int img = (int)(gid / ((long long)6 * nmcu));
  const int mcx = mcu % mx, mcy = mcu / mx;
  const uint8_t* im = rgb + (size_t)img * H * W * 3;
  int16_t* out = coef + (size_t)gid * 64;

  int d[64];
  bool dummy = false;
  if (slot < 4) {
    const int bw = (W + 7) >> 3, bh = (H + 7) >> 3;
    const bool col_in = 2 * mcx + 1 < bw, row_in = 2 * mcy + 1 < bh;  // the MCU's second block column / row exists
    int s = slot;  // the block whose DC this one carries: itself, or for a dummy the last real block before it
    if (s == 3 && !row_in) s = 2;
    else if (s == 3 && !col_in) { s = 2; dummy = true; }
    if (s == 2 && !row_in) { s = 1; dummy = true; }
    if (s == 1 && !col_in) { s = 0; dummy = true; }
    const int bx = 2 * mcx + (s & 1), by = 2 * mcy + (s >> 1);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = min(by * 8 + r, H - 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int x = min(bx * 8 + c, W - 1);
        const uint8_t* p = im + ((size_t)y * W + x) * 3;
        d[r * 8 + c] = ((19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16) - 128;
      }
    }
  } else {
    const int hc = (H + 1) >> 1;
    const bool cr = slot == 5;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int cy = min(mcy * 8 + r, hc - 1);  // rows past the last downsampled row copy it
      const int y0 = min(2 * cy, H - 1), y1 = min(2 * cy + 1, H - 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int cx = mcx * 8 + c;
        const int x0 = min(2 * cx, W - 1), x1 = min(2 * cx + 1, W - 1);
        int acc = 1 + (cx & 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint8_t* p = im + ((size_t)((q & 2) ? y1 : y0) * W + ((q & 1) ? x1 : x0)) * 3;
          const int R = p[0], G = p[1], B = p[2];
          acc += cr ? (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
                    : (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        }
        d[r * 8 + c] = (acc >> 2) - 128;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r)
    dct8<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    dct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
  const uint16_t* q = qtab + (slot < 4 ? 0 : 64);
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int qv = (int)q[i] * 8;
    const int v = d[i];
    const int mag = ((v < 0 ? -v : v) + (qv >> 1)) / qv;
    out[kZigzagOf[i]] = (int16_t)((dummy && i) ? 0 : (v < 0 ? -mag : mag));
  }
}

// ---- K18c ----------------------------------------------------------------------------------------------------------
// Huffman tables on the device: entry = code | length << 16.  [0..11] DC luma, [12..23] DC chroma, [24..279] AC luma,
// [280..535] AC chroma (indexed by the run / size symbol).
constexpr int kDcOff = 0, kAcOff = 24, kHuffEntries = 24 + 512;

__device__ __forceinline__ int nbits_of(int a) { return 32 - __clz(a); }  // a >= 0

// the DC predictor of block (mcu, slot): the previous block of the same component in scan order
__device__ __forceinline__ int dc_pred(const int16_t* __restrict__ img_coef, int mcu, int slot) {
  if (slot >= 1 && slot <= 3) return img_coef[((size_t)mcu * 6 + slot - 1) * 64];
  if (mcu == 0) return 0;
  return img_coef[((size_t)(mcu - 1) * 6 + (slot == 0 ? 3 : slot)) * 64];
}

struct BitCounter {
  unsigned n = 0;
  __device__ __forceinline__ void put(unsigned, int len) { n += (unsigned)len; }
};

// MSB-first writer at a bit offset; whole 32-bit words go out byte-swapped so that memory holds the byte stream
struct BitWriter {
  unsigned* buf;
  unsigned long long acc = 0;
  unsigned word;
  int fill;
  __device__ __forceinline__ BitWriter(unsigned* b, unsigned long long bitpos) : buf(b), word((unsigned)(bitpos >> 5)), fill((int)(bitpos & 31)) {}
  __device__ __forceinline__ void put(unsigned bits, int len) {
    acc = (acc << len) | bits;
    fill += len;
    if (fill >= 32) {
      fill -= 32;
      atomicOr(&buf[word++], __builtin_bswap32((unsigned)(acc >> fill)));
    }
  }
  __device__ __forceinline__ void flush() {
    if (fill > 0) atomicOr(&buf[word], __builtin_bswap32((unsigned)(acc << (32 - fill))));
  }
};

// jchuff.c encode_one_block on zigzag coefficients
template <typename Sink>
__device__ __forceinline__ void encode_block(const int16_t* __restrict__ blk, int pred, const unsigned* __restrict__ huff, int chroma,
                                             Sink& sink) {
  const unsigned* dc = huff + kDcOff + chroma * 12;
  const unsigned* ac = huff + kAcOff + chroma * 256;
  int v = (int)blk[0] - pred;
  int nb = nbits_of(v < 0 ? -v : v);
  unsigned e = dc[nb];
  sink.put(e & 0xFFFFu, (int)(e >> 16));
  if (nb) sink.put((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    v = blk[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      e = ac[0xF0];
      sink.put(e & 0xFFFFu, (int)(e >> 16));
      run -= 16;
    }
    nb = nbits_of(v < 0 ? -v : v);
    e = ac[(run << 4) + nb];
    sink.put(e & 0xFFFFu, (int)(e >> 16));
    sink.put((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
    run = 0;
  }
  if (run) {
    e = ac[0];
    sink.put(e & 0xFFFFu, (int)(e >> 16));
  }
}

// (i) len [N][nblk]
__global__ __launch_bounds__(256) void k_jpeg_bitlen(const int16_t* __restrict__ coef, int N, int nblk,
                                                     const unsigned* __restrict__ huff, unsigned* __restrict__ len) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)N * nblk) return;
  const int b = (int)(gid % nblk), img = (int)(gid / nblk);
  const int16_t* ic = coef + (size_t)img * nblk * 64;
  BitCounter cnt;
  encode_block(ic + (size_t)b * 64, dc_pred(ic, b / 6, b % 6), huff, b % 6 >= 4, cnt);
  len[gid] = cnt.n;
}

// (ii) one workgroup per image: off [N][nblk] = exclusive prefix sum of len, total [N]
__global__ __launch_bounds__(kScanThreads) void k_jpeg_scan(const unsigned* __restrict__ len, int nblk, unsigned* __restrict__ off,
                                                            unsigned* __restrict__ total) {
  __shared__ unsigned wave_sum[kScanThreads / 64];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned* l = len + (size_t)img * nblk;
  unsigned* o = off + (size_t)img * nblk;
  unsigned carry = 0;
  for (int base = 0; base < nblk; base += kScanThreads) {
    const int i = base + tid;
    const unsigned v = i < nblk ? l[i] : 0u;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned u = __shfl_up(inc, d, 64);
      if (lane >= d) inc += u;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      if (w < wave) before += wave_sum[w];
      all += wave_sum[w];
    }
    if (i < nblk) o[i] = before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) total[img] = carry;
}

// (iii) bits [sum of words]: image img starts at 32-bit word word_off[img]
__global__ __launch_bounds__(256) void k_jpeg_emit(const int16_t* __restrict__ coef, int N, int nblk, const unsigned* __restrict__ huff,
                                                   const unsigned* __restrict__ off, const unsigned* __restrict__ word_off,
                                                   unsigned* __restrict__ bits) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)N * nblk) return;
  const int b = (int)(gid % nblk), img = (int)(gid / nblk);
  const int16_t* ic = coef + (size_t)img * nblk * 64;
  BitWriter wr(bits + word_off[img], off[gid]);
  encode_block(ic + (size_t)b * 64, dc_pred(ic, b / 6, b % 6), huff, b % 6 >= 4, wr);
  wr.flush();
}

// ---- Annex K Huffman tables ----------------------------------------------------------------------------------------
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// JPEG C.2: symbol -> code | length << 16
void huff_fill(const uint8_t* bits, const uint8_t* vals, unsigned* table) {
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = code++ | (unsigned)len << 16;
    code <<= 1;
  }
}

enum { kEvResize0, kEvResize1, kEvJpeg0, kEvBlocks, kEvEntropy, kEvRead0, kEvRead1, kNumEvents };

}  // namespace

struct eioku_thumbs {
  eioku::DevBuf<unsigned> huff;
  eioku::DevBuf<int> tables;
  eioku::DevBuf<uint8_t> tmp;  // the resize's 8-bit intermediate
  eioku::DevBuf<uint16_t> qtab;
  eioku::DevBuf<int16_t> coef;
  eioku::DevBuf<unsigned> len;  // [n][nblk] bit lengths, then [n][nblk] offsets, [n] totals, [n] word offsets
  eioku::DevBuf<unsigned> bits;
  size_t bits_bytes = 0;  // of the last eioku_thumbs_jpeg call
  eioku::DevEvents ev;    // kNumEvents
  bool timed[3] = {false, false, false};  // resize, jpeg, read have run since create
};

extern "C" {

int eioku_thumbs_create(eioku_thumbs_t** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL out");
  *out = nullptr;
  eioku_thumbs* t = new eioku_thumbs();
  std::vector<unsigned> h(kHuffEntries, 0u);
  huff_fill(kDcLumaBits, kDcVals, h.data() + kDcOff);
  huff_fill(kDcChromaBits, kDcVals, h.data() + kDcOff + 12);
  huff_fill(kAcLumaBits, kAcLumaVals, h.data() + kAcOff);
  huff_fill(kAcChromaBits, kAcChromaVals, h.data() + kAcOff + 256);
  int rc = t->huff.upload(h.data(), kHuffEntries);
  if (!rc) rc = t->qtab.grow(128);
  if (!rc) rc = t->ev.ensure(kNumEvents);
  if (rc) {
    eioku_thumbs_destroy(t);
    return rc;
  }
  *out = t;
  return EIOKU_OK;
}

void eioku_thumbs_destroy(eioku_thumbs_t* t) {
  if (!t) return;
  delete t;
}

int eioku_thumbs_resize(eioku_thumbs_t* t, const uint8_t* bgr, int n, int h, int w, int th, int tw, const int32_t* xbounds,
                        const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, uint8_t* rgb_out,
                        void* stream_) {
  EIOKU_REQUIRE(t && n >= 0 && h > 0 && w > 0 && kx > 0 && ky > 0 && xbounds && xk && ybounds && yk, "bad argument");
  EIOKU_REQUIRE(n <= kMaxN, "n = %d frames per call, at most %d", n, kMaxN);
  EIOKU_REQUIRE(th >= 1 && tw >= 1 && th <= kMaxSide && tw <= kMaxSide, "thumbnail %d x %d outside [1, %d] per side", tw, th, kMaxSide);
  // the tables are read on the device without further checks: every tap must lie inside the source axis
  for (int i = 0; i < tw; ++i)
    EIOKU_REQUIRE(xbounds[2 * i] >= 0 && xbounds[2 * i + 1] >= 0 && xbounds[2 * i + 1] <= kx && xbounds[2 * i] + xbounds[2 * i + 1] <= w,
                  "xbounds[%d] leaves the source row", i);
  for (int i = 0; i < th; ++i)
    EIOKU_REQUIRE(ybounds[2 * i] >= 0 && ybounds[2 * i + 1] >= 0 && ybounds[2 * i + 1] <= ky && ybounds[2 * i] + ybounds[2 * i + 1] <= h,
                  "ybounds[%d] leaves the source column", i);
  EIOKU_REQUIRE_INIT();
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr && rgb_out, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  const size_t xb_n = (size_t)tw * 2, xk_n = (size_t)tw * kx, yb_n = (size_t)th * 2, yk_n = (size_t)th * ky;
  EIOKU_TRY(t->tables.grow(xb_n + xk_n + yb_n + yk_n));
  EIOKU_TRY(t->tmp.grow((size_t)n * h * tw * 3));
  int* d_xb = t->tables;
  int* d_xk = d_xb + xb_n;
  int* d_yb = d_xk + xk_n;
  int* d_yk = d_yb + yb_n;
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_xb, xbounds, xb_n * 4, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_xk, xk, xk_n * 4, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_yb, ybounds, yb_n * 4, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_yk, yk, yk_n * 4, hipMemcpyHostToDevice, stream));
  const long long w1 = (long long)n * h * tw, w2 = (long long)n * th * tw;
  EIOKU_TRY(t->ev.record(kEvResize0, stream));
  hipLaunchKernelGGL(k_thumb_resize_h, dim3((unsigned)((w1 + 255) / 256)), dim3(256), 0, stream, bgr, w1, w, tw, d_xb, d_xk, kx, t->tmp.p);
  hipLaunchKernelGGL(k_thumb_resize_v, dim3((unsigned)((w2 + 255) / 256)), dim3(256), 0, stream, t->tmp.p, w2, h, th, tw, d_yb, d_yk, ky,
                     rgb_out);
  EIOKU_LAUNCH_CHECK();
  EIOKU_TRY(t->ev.record(kEvResize1, stream));
  t->timed[0] = true;
  return EIOKU_OK;
}

int eioku_thumbs_jpeg(eioku_thumbs_t* t, const uint8_t* rgb, int n, int th, int tw, const uint16_t* qtab, int16_t* coef_out,
                      uint32_t* nbits_out, uint64_t* bytes_out, void* stream_) {
  EIOKU_REQUIRE(t && n >= 0 && qtab && nbits_out && bytes_out, "bad argument");
  EIOKU_REQUIRE(n <= kMaxN, "n = %d images per call, at most %d", n, kMaxN);
  EIOKU_REQUIRE(th >= 1 && tw >= 1 && th <= kMaxSide && tw <= kMaxSide, "thumbnail %d x %d outside [1, %d] per side", tw, th, kMaxSide);
  for (int i = 0; i < 128; ++i) EIOKU_REQUIRE(qtab[i] >= 1 && qtab[i] <= 255, "qtab[%d] = %d outside [1, 255]", i, (int)qtab[i]);
  EIOKU_REQUIRE_INIT();
  t->bits_bytes = 0;
  *bytes_out = 0;
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(rgb, "NULL image");
  hipStream_t stream = (hipStream_t)stream_;
  const int mx = (tw + 15) / 16, my = (th + 15) / 16, nblk = mx * my * 6;
  const size_t nb = (size_t)n * nblk;
  EIOKU_TRY(t->coef.grow(nb * 64));
  EIOKU_TRY(t->len.grow(2 * nb + 2 * (size_t)n));
  unsigned* d_len = t->len;
  unsigned* d_off = d_len + nb;
  unsigned* d_total = d_off + nb;
  unsigned* d_word = d_total + n;
  EIOKU_HIP_CHECK(hipMemcpyAsync(t->qtab, qtab, 128 * 2, hipMemcpyHostToDevice, stream));
  EIOKU_TRY(t->ev.record(kEvJpeg0, stream));
  hipLaunchKernelGGL(k_jpeg_blocks, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, stream, rgb, n, th, tw, mx, my, t->qtab.p, t->coef.p);
  EIOKU_LAUNCH_CHECK();
  EIOKU_TRY(t->ev.record(kEvBlocks, stream));
  hipLaunchKernelGGL(k_jpeg_bitlen, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, stream, t->coef.p, n, nblk, t->huff.p, d_len);
  hipLaunchKernelGGL(k_jpeg_scan, dim3((unsigned)n), dim3(kScanThreads), 0, stream, d_len, nblk, d_off, d_total);
  EIOKU_LAUNCH_CHECK();
  uint32_t totals[kMaxN];
  EIOKU_HIP_CHECK(hipMemcpyAsync(totals, d_total, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  // every image's stream starts on a 32-bit word; the sizes are known now, so the buffer holds exactly what was coded
  uint32_t word_off[kMaxN];
  size_t words = 0;
  for (int i = 0; i < n; ++i) {
    word_off[i] = (uint32_t)words;
    words += ((size_t)totals[i] + 31) / 32;
    nbits_out[i] = totals[i];
  }
  EIOKU_TRY(t->bits.grow(words));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_word, word_off, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemsetAsync(t->bits, 0, words * 4, stream));
  hipLaunchKernelGGL(k_jpeg_emit, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, stream, t->coef.p, n, nblk, t->huff.p, d_off, d_word,
                     t->bits.p);
  EIOKU_LAUNCH_CHECK();
  EIOKU_TRY(t->ev.record(kEvEntropy, stream));
  if (coef_out) EIOKU_HIP_CHECK(hipMemcpyAsync(coef_out, t->coef, nb * 64 * 2, hipMemcpyDeviceToHost, stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));  // word_off (stack) has been read; coef_out is filled
  t->bits_bytes = words * 4;
  *bytes_out = words * 4;
  t->timed[1] = true;
  return EIOKU_OK;
}

int eioku_thumbs_read(eioku_thumbs_t* t, uint8_t* out, size_t cap, void* stream_) {
  EIOKU_REQUIRE(t, "NULL handle");
  EIOKU_REQUIRE(cap >= t->bits_bytes, "buffer of %zu bytes for %zu bytes of bitstream", cap, t->bits_bytes);
  EIOKU_REQUIRE_INIT();
  if (t->bits_bytes == 0) return EIOKU_OK;
  EIOKU_REQUIRE(out, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  EIOKU_TRY(t->ev.record(kEvRead0, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(out, t->bits, t->bits_bytes, hipMemcpyDeviceToHost, stream));
  EIOKU_TRY(t->ev.record(kEvRead1, stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  t->timed[2] = true;
  return EIOKU_OK;
}

int eioku_thumbs_last_ms(eioku_thumbs_t* t, double* ms4) {
  EIOKU_REQUIRE(t && ms4, "bad argument");
  EIOKU_REQUIRE_INIT();
  const int pairs[4][3] = {{kEvResize0, kEvResize1, 0}, {kEvJpeg0, kEvBlocks, 1}, {kEvBlocks, kEvEntropy, 1}, {kEvRead0, kEvRead1, 2}};
  for (int i = 0; i < 4; ++i) {
    ms4[i] = 0.0;
    if (!t->timed[pairs[i][2]]) continue;
    EIOKU_TRY(t->ev.ms(pairs[i][0], pairs[i][1], &ms4[i]));
  }
  return EIOKU_OK;
}

}  // extern "C"
