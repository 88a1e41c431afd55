// K28: baseline JPEG decode on gfx950 -- Motion-JPEG frames from file bytes to BGR in HBM, bit for bit what libjpeg
// (libjpeg-turbo, and therefore Pillow) decodes by default.
//
//   K28a  entropy.  Every restart segment is cut into subsequences of S bits; one thread per subsequence
//         (jpeg_entropy.h holds the bit reader, the tables and the one-symbol step, shared with host programs).
//         k_sync_round  decodes, without storing coefficients, every subsequence whose entry state (p, b, z) changed,
//                       from its entry to the first symbol boundary at or past its end, and stores the exit state and
//                       the blocks closed.  Subsequence 0 of a segment starts in (0, 0, 0), subsequence i in round 1 in
//                       the guess (i S, 0, 0) and later in its left neighbour's exit state of the round before (two
//                       exit buffers alternate, so a round reads only what the round before wrote).  After round r the
//                       first r subsequences of every segment are exact, so at most max-subsequences-per-segment + 1
//                       rounds run; the host reads a per-round "somebody decoded" flag every kRoundGroup rounds.
//         k_sub_scan    exclusive scan of the blocks closed, per segment: every subsequence's first block ordinal; a
//                       segment that closes fewer blocks than it owns marks its frame's status.
//         k_write       decodes once more from the true states and stores DC differences and de-zigzagged AC
//                       coefficients, every store guarded by "block ordinal < blocks the segment owns".
//         k_dc_scan     per segment and component, DC differences -> DC values (predictor 0 at every restart).
//         One workgroup serves subsequences of one frame and stages that frame's four Huffman tables in LDS.
//   K28b  pixels.  k_idct: one thread per block, 64 samples in registers: dequantise, jidctint.c "islow" (CONST_BITS 13,
//         PASS1_BITS 2, descale 11 then 18), +128, clamp, into padded component planes.  k_colour: jdsample.c fancy
//         upsampling (h2v1 / h2v2; plain replication when the chroma plane is at most two samples wide, as libjpeg
//         chooses) fused with jdcolor.c YCbCr -> RGB, cropped to h x w, two pixels per thread.  k_luma copies Y.
// A call is processed in sub-batches of frames so that the coefficient buffer stays bounded; every frame is independent,
// so the split does not show in the result.  All buffers belong to the handle (no library scratch slot is used).
#include <algorithm>
#include <vector>

#include "common.h"
#include "jpeg_entropy.h"

namespace {

namespace je = jpeg_entropy;

constexpr int kMaxSide = 8192;
constexpr int kMaxFrames = 4096;               // per call
constexpr size_t kCoefBudget = 96u << 20;      // bytes of int16 coefficients per sub-batch
constexpr int kEntThreads = 128;               // subsequences per workgroup
constexpr int kScanThreads = 256;
constexpr int kRoundGroup = 4;                 // rounds between two reads of the flags
constexpr int kDefaultSubseqBits = 512;        // the fastest of 256 .. 2048 on 64 x 1080p (DESIGN.md "K28", profiles/mjpeg.json)
constexpr int kHuffBytes = 16 + 256;           // one table as the caller passes it: 16 counts, then the symbols

static_assert(sizeof(je::FrameTables) % 4 == 0, "FrameTables is copied to LDS word by word");

struct Seg {
  uint32_t frame;        // within the sub-batch
  uint32_t first_block;  // first_mcu * blocks per MCU
  uint32_t nblocks;      // blocks the segment owns
  uint32_t first_mcu, mcu_count;
  uint32_t word_off, nbits;
  uint32_t sub_first, nsub;
};

struct Geo {
  int h, w, ncomp, hs, vs;
  int mcux, mcuy, bpm;     // MCUs per row / column, blocks per MCU
  int yw, yh, cw, ch;      // padded plane sizes
  int blocks;              // per frame
};

__device__ __forceinline__ void stage_tables(je::FrameTables* dst, const je::FrameTables* src) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (int i = threadIdx.x; i < (int)(sizeof(je::FrameTables) / 4); i += blockDim.x) d[i] = s[i];
  __syncthreads();
}

// wg [workgroups] = {frame, first subsequence}; frame_sub_end [frames]
__global__ __launch_bounds__(kEntThreads) void k_sync_round(const uint32_t* __restrict__ words, const Seg* __restrict__ segs,
                                                            const uint32_t* __restrict__ sub_seg, const uint2* __restrict__ wg,
                                                            const uint32_t* __restrict__ frame_sub_end,
                                                            const je::FrameTables* __restrict__ tables, uint32_t S, int first_round,
                                                            const uint4* __restrict__ exit_old, uint4* __restrict__ exit_new,
                                                            uint4* __restrict__ prev, uint32_t* __restrict__ flag) {
  __shared__ je::FrameTables ft;
  const uint2 g = wg[blockIdx.x];
  stage_tables(&ft, tables + g.x);
  const uint32_t i = g.y + threadIdx.x;
  if (i >= frame_sub_end[g.x]) return;
  const Seg sg = segs[sub_seg[i]];
  const uint32_t k = i - sg.sub_first;
  je::State e = {0u, 0u, 0u};
  if (k > 0) {
    if (first_round) {
      e.p = k * S;
    } else {
      const uint4 x = exit_old[i - 1];
      e.p = x.x, e.b = x.y, e.z = x.z;
    }
  }
  if (!first_round) {
    const uint4 pv = prev[i];
    if (pv.x == e.p && pv.y == e.b && pv.z == e.z) {
      exit_new[i] = exit_old[i];
      return;
    }
  }
  prev[i] = make_uint4(e.p, e.b, e.z, 0u);
  je::NullSink sink;
  const uint32_t n = je::run(ft, words + sg.word_off, (sg.nbits + 31) >> 5, sg.nbits, (k + 1) * S, e, sink);
  exit_new[i] = make_uint4(e.p, e.b, e.z, n);
  *flag = 1u;
}

// one workgroup per segment: first [sub] = exclusive prefix sum of the blocks closed
__global__ __launch_bounds__(kScanThreads) void k_sub_scan(const Seg* __restrict__ segs, const uint4* __restrict__ exits,
                                                           uint32_t* __restrict__ first, int* __restrict__ status) {
  __shared__ unsigned wave_sum[kScanThreads / 64];
  const Seg sg = segs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned carry = 0;
  for (uint32_t base = 0; base < sg.nsub; base += kScanThreads) {
    const uint32_t i = base + tid;
    const unsigned v = i < sg.nsub ? exits[sg.sub_first + i].w : 0u;
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
    if (i < sg.nsub) first[sg.sub_first + i] = before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (tid == 0 && carry < sg.nblocks) atomicOr(&status[sg.frame], 1);
}

struct CoefSink {
  int16_t* base;  // the segment's first block
  uint32_t ord, owned;
  __device__ __forceinline__ void dc(int v) {
    if (ord < owned) base[(size_t)ord * 64] = (int16_t)v;
  }
  __device__ __forceinline__ void ac(int z, int v) {
    if (ord < owned) base[(size_t)ord * 64 + je::natural_of(z)] = (int16_t)v;
  }
  __device__ __forceinline__ void close() { ++ord; }
};

// coef [frames][blocks][64], zeroed
__global__ __launch_bounds__(kEntThreads) void k_write(const uint32_t* __restrict__ words, const Seg* __restrict__ segs,
                                                       const uint32_t* __restrict__ sub_seg, const uint2* __restrict__ wg,
                                                       const uint32_t* __restrict__ frame_sub_end,
                                                       const je::FrameTables* __restrict__ tables, uint32_t S,
                                                       const uint4* __restrict__ exits, const uint32_t* __restrict__ first,
                                                       int blocks_per_frame, int16_t* __restrict__ coef) {
  __shared__ je::FrameTables ft;
  const uint2 g = wg[blockIdx.x];
  stage_tables(&ft, tables + g.x);
  const uint32_t i = g.y + threadIdx.x;
  if (i >= frame_sub_end[g.x]) return;
  const Seg sg = segs[sub_seg[i]];
  const uint32_t k = i - sg.sub_first;
  je::State e = {0u, 0u, 0u};
  if (k > 0) {
    const uint4 x = exits[i - 1];
    e.p = x.x, e.b = x.y, e.z = x.z;
  }
  CoefSink sink = {coef + ((size_t)sg.frame * blocks_per_frame + sg.first_block) * 64, first[i], sg.nblocks};
  je::run(ft, words + sg.word_off, (sg.nbits + 31) >> 5, sg.nbits, (k + 1) * S, e, sink);
}

// one wave per (segment, component): inclusive sum of the DC differences over the component's blocks of the segment
__global__ __launch_bounds__(64) void k_dc_scan(const Seg* __restrict__ segs, Geo g, int16_t* __restrict__ coef) {
  const Seg sg = segs[blockIdx.x / g.ncomp];
  const int c = blockIdx.x % g.ncomp, lane = threadIdx.x;
  const int hv = c == 0 ? g.hs * g.vs : 1, off = c == 0 ? 0 : g.hs * g.vs + c - 1;
  const uint32_t nb = sg.mcu_count * (uint32_t)hv;
  int16_t* base = coef + ((size_t)sg.frame * g.blocks + sg.first_block) * 64;
  int carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
    const uint32_t j = b0 + lane;
    int16_t* p = base + ((size_t)(j / hv) * g.bpm + off + j % hv) * 64;
    int v = j < nb ? (int)*p : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    v += carry;
    if (j < nb) *p = (int16_t)v;
    carry = __shfl(v, 63, 64);
  }
}

// ---- K28b ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// jidctint.c: one 8-point pass in place; the results carry 13 more fraction bits than the inputs
__device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7, int shift) {
  int z2 = d2, z3 = d6;
  int z1 = (z2 + z3) * 4433;
  const int e2 = z1 + z3 * -15137, e3 = z1 + z2 * 6270;
  const int e0 = (d0 + d4) * 8192, e1 = (d0 - d4) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = d7, t1 = d5, t2 = d3, t3 = d1;
  z1 = t0 + t3;
  z2 = t1 + t2;
  z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446;
  t1 *= 16819;
  t2 *= 25172;
  t3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  d0 = descale(t10 + t3, shift);
  d7 = descale(t10 - t3, shift);
  d1 = descale(t11 + t2, shift);
  d6 = descale(t11 - t2, shift);
  d2 = descale(t12 + t1, shift);
  d5 = descale(t12 - t1, shift);
  d3 = descale(t13 + t0, shift);
  d4 = descale(t13 - t0, shift);
}

// coef [frames][blocks][64] natural order; qtab [frames][4][64] natural order; comp_q [frames][3];
// yplane [frames][yh][yw], cplane [frames][2][ch][cw]
__global__ __launch_bounds__(64) void k_idct(const int16_t* __restrict__ coef, long long total, Geo g,
                                             const uint16_t* __restrict__ qtab, const uint8_t* __restrict__ comp_q, int luma_only,
                                             uint8_t* __restrict__ yplane, uint8_t* __restrict__ cplane) {
  const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (gid >= total) return;
  const int f = (int)(gid / g.blocks), blk = (int)(gid % g.blocks);
  const int mcu = blk / g.bpm, bi = blk % g.bpm;
  const int mx = mcu % g.mcux, my = mcu / g.mcux;
  const int ny = g.hs * g.vs;
  int c, bx, by, stride;
  uint8_t* plane;
  if (bi < ny) {
    c = 0, bx = mx * g.hs + bi % g.hs, by = my * g.vs + bi / g.hs, stride = g.yw;
    plane = yplane + (size_t)f * g.yh * g.yw;
  } else {
    if (luma_only) return;
    c = bi - ny + 1, bx = mx, by = my, stride = g.cw;
    plane = cplane + ((size_t)f * 2 + (c - 1)) * g.ch * g.cw;
  }
  const uint16_t* q = qtab + ((size_t)f * 4 + (comp_q[f * 3 + c] & 3)) * 64;
  const int16_t* in = coef + (size_t)gid * 64;
  int d[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] = (int)in[i] * (int)q[i];
#pragma unroll
  for (int col = 0; col < 8; ++col)
    idct8(d[col], d[8 + col], d[16 + col], d[24 + col], d[32 + col], d[40 + col], d[48 + col], d[56 + col], 11);
  uint8_t* o = plane + (size_t)by * 8 * stride + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    idct8(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7], 18);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (uint32_t)clip8(d[r * 8 + x] + 128) << (8 * x);
      hi |= (uint32_t)clip8(d[r * 8 + 4 + x] + 128) << (8 * x);
    }
    *reinterpret_cast<uint2*>(o + (size_t)r * stride) = make_uint2(lo, hi);  // strides and bx * 8 are multiples of 8
  }
}

// jdcolor.c with SCALEBITS 16
__device__ __forceinline__ void store_pixel(uint8_t* o, int y, int cb, int cr, int rgb) {
  cb -= 128, cr -= 128;
  const int r = clip8(y + ((91881 * cr + 32768) >> 16));
  const int g = clip8(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  const int b = clip8(y + ((116130 * cb + 32768) >> 16));
  o[0] = (uint8_t)(rgb ? r : b);
  o[1] = (uint8_t)g;
  o[2] = (uint8_t)(rgb ? b : r);
}

// out [frames][h][w][3]; one thread per pair of pixels (2i, 2i + 1) of a row
__global__ __launch_bounds__(256) void k_colour(const uint8_t* __restrict__ yplane, const uint8_t* __restrict__ cplane, long long total,
                                                Geo g, int rgb, uint8_t* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int pw = (g.w + 1) >> 1;
  const int i = (int)(gid % pw), y = (int)((gid / pw) % g.h), f = (int)(gid / ((long long)pw * g.h));
  const uint8_t* yp = yplane + ((size_t)f * g.yh + y) * g.yw;
  const int x0 = 2 * i;
  const bool two = x0 + 1 < g.w;
  const int y0 = yp[x0], y1 = two ? yp[x0 + 1] : 0;
  uint8_t* o = out + (((size_t)f * g.h + y) * g.w + x0) * 3;
  if (g.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)y0;
    if (two) o[3] = o[4] = o[5] = (uint8_t)y1;
    return;
  }
  const uint8_t* cbp = cplane + (size_t)f * 2 * g.ch * g.cw;
  const uint8_t* crp = cbp + (size_t)g.ch * g.cw;
  int cb0, cb1, cr0, cr1;
  if (g.hs == 1) {
    const size_t at = (size_t)y * g.cw + x0;
    cb0 = cbp[at], cr0 = crp[at];
    cb1 = two ? cbp[at + 1] : 0, cr1 = two ? crp[at + 1] : 0;
  } else {
    const int dw = (g.w + 1) >> 1;  // the chroma plane's real width
    const int cy = g.vs == 2 ? y >> 1 : y;
    const size_t near = (size_t)cy * g.cw;
    if (dw <= 2) {  // libjpeg replicates: too narrow for the triangle filter
      cb0 = cb1 = cbp[near + i];
      cr0 = cr1 = crp[near + i];
    } else {
      const int il = max(i - 1, 0), ir = min(i + 1, dw - 1);
      if (g.vs == 1) {
        const int a = cbp[near + i], b = crp[near + i];
        cb0 = (3 * a + cbp[near + il] + 1) >> 2;
        cb1 = (3 * a + cbp[near + ir] + 2) >> 2;
        cr0 = (3 * b + crp[near + il] + 1) >> 2;
        cr1 = (3 * b + crp[near + ir] + 2) >> 2;
      } else {
        const int dh = (g.h + 1) >> 1;  // real downsampled rows: the rows above the first and below the last repeat them
        const size_t far = (size_t)((y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0)) * g.cw;
        const int a = 3 * cbp[near + i] + cbp[far + i], al = 3 * cbp[near + il] + cbp[far + il],
                  ar = 3 * cbp[near + ir] + cbp[far + ir];
        const int b = 3 * crp[near + i] + crp[far + i], bl = 3 * crp[near + il] + crp[far + il],
                  br = 3 * crp[near + ir] + crp[far + ir];
        cb0 = (3 * a + al + 8) >> 4;
        cb1 = (3 * a + ar + 7) >> 4;
        cr0 = (3 * b + bl + 8) >> 4;
        cr1 = (3 * b + br + 7) >> 4;
      }
    }
  }
  store_pixel(o, y0, cb0, cr0, rgb);
  if (two) store_pixel(o + 3, y1, cb1, cr1, rgb);
}

// out [frames][h][w]
__global__ __launch_bounds__(256) void k_luma(const uint8_t* __restrict__ yplane, long long total, Geo g, uint8_t* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int x = (int)(gid % g.w), y = (int)((gid / g.w) % g.h), f = (int)(gid / ((long long)g.w * g.h));
  out[gid] = yplane[((size_t)f * g.yh + y) * g.yw + x];
}

enum { kEvStart, kEvUploaded, kEvSynced, kEvWritten, kEvIdct, kEvColour, kNumEvents };

}  // namespace

struct eioku_mjpeg {
  eioku::DevBuf<uint32_t> words, sub_seg, frame_sub_end, first, flags;
  eioku::DevBuf<Seg> segs;
  eioku::DevBuf<uint2> wg;
  eioku::DevBuf<uint4> exits, prev;  // exits: two buffers of nsub
  eioku::DevBuf<je::FrameTables> tables;
  eioku::DevBuf<uint16_t> qtab;
  eioku::DevBuf<uint8_t> comp_q, yplane, cplane;
  eioku::DevBuf<int16_t> coef;
  eioku::DevBuf<int> status;
  eioku::DevEvents ev;  // kNumEvents
  int subseq_bits = kDefaultSubseqBits;
  int batch_frames = 0;  // 0: as many as the coefficient budget allows
  double ms[5] = {0, 0, 0, 0, 0};
  int rounds = 0;
};

namespace {

// everything a call needs, validated on the host before the device is touched
struct Call {
  Geo g;
  int n, nseg, fmt;
  const uint8_t* entropy;
  size_t entropy_bytes;
  const uint32_t* seg;  // [nseg][5]: frame, first MCU, MCU count, byte offset, bit length
  const uint16_t* qtab;
  const uint8_t* huff;
  const uint8_t* comp;  // [n][3][3]: quant table, DC table, AC table of each component
  std::vector<je::FrameTables> tables;
  std::vector<int> seg_begin;  // [n + 1]: the segments of frame f are [seg_begin[f], seg_begin[f + 1])
};

int validate(Call& c, int S) {
  Geo& g = c.g;
  EIOKU_REQUIRE(c.n >= 0 && c.n <= kMaxFrames, "n = %d frames per call, at most %d", c.n, kMaxFrames);
  EIOKU_REQUIRE(g.h >= 1 && g.w >= 1 && g.h <= kMaxSide && g.w <= kMaxSide, "frame %d x %d outside [1, %d] per side", g.w, g.h, kMaxSide);
  EIOKU_REQUIRE(g.ncomp == 1 || g.ncomp == 3, "%d components: 1 or 3", g.ncomp);
  EIOKU_REQUIRE((g.hs == 1 && g.vs == 1) || (g.ncomp == 3 && g.hs == 2 && (g.vs == 1 || g.vs == 2)),
                "luma sampling %d x %d: 1x1, 2x1 or 2x2 (1x1 for one component)", g.hs, g.vs);
  EIOKU_REQUIRE(c.fmt >= EIOKU_MJPEG_BGR && c.fmt <= EIOKU_MJPEG_LUMA, "output format %d", c.fmt);
  EIOKU_REQUIRE(S >= 32 && S <= 4096 && S % 32 == 0, "subsequence size %d", S);
  if (c.n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(c.entropy && c.seg && c.qtab && c.huff && c.comp, "NULL table");
  EIOKU_REQUIRE(c.nseg >= c.n, "%d segments for %d frames", c.nseg, c.n);
  EIOKU_REQUIRE(c.entropy_bytes % 4 == 0 && c.entropy_bytes < ((size_t)1 << 32), "entropy buffer of %zu bytes: a multiple of 4 below 4 GiB",
                c.entropy_bytes);
  g.mcux = (g.w + 8 * g.hs - 1) / (8 * g.hs);
  g.mcuy = (g.h + 8 * g.vs - 1) / (8 * g.vs);
  g.bpm = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
  g.yw = g.mcux * g.hs * 8, g.yh = g.mcuy * g.vs * 8;
  g.cw = g.mcux * 8, g.ch = g.mcuy * 8;
  g.blocks = g.mcux * g.mcuy * g.bpm;
  const uint32_t mcus = (uint32_t)(g.mcux * g.mcuy);
  c.seg_begin.assign(c.n + 1, 0);
  int f = 0;
  uint32_t next_mcu = 0;
  for (int s = 0; s < c.nseg; ++s) {
    const uint32_t* r = c.seg + (size_t)s * 5;
    if (r[0] != (uint32_t)f) {  // the next frame begins: the one before must be complete
      EIOKU_REQUIRE(r[0] == (uint32_t)f + 1 && (int)r[0] < c.n && next_mcu == mcus, "segment %d: frame %u after frame %d with %u of %u MCUs", s,
                    r[0], f, next_mcu, mcus);
      c.seg_begin[++f] = s;
      next_mcu = 0;
    }
    EIOKU_REQUIRE(r[1] == next_mcu && r[2] >= 1 && r[2] <= mcus - next_mcu, "segment %d: MCUs [%u, +%u) after %u of %u", s, r[1], r[2], next_mcu,
                  mcus);
    next_mcu += r[2];
    EIOKU_REQUIRE(r[3] % 4 == 0 && r[4] < (1u << 31) && (size_t)r[3] + ((size_t)r[4] + 7) / 8 <= c.entropy_bytes,
                  "segment %d: %u bits at byte %u of %zu", s, r[4], r[3], c.entropy_bytes);
  }
  EIOKU_REQUIRE(f == c.n - 1 && next_mcu == mcus, "the segment table ends in frame %d with %u of %u MCUs", f, next_mcu, mcus);
  c.seg_begin[c.n] = c.nseg;
  c.tables.resize(c.n);
  for (int i = 0; i < c.n; ++i) {
    je::FrameTables& t = c.tables[i];
    memset(&t, 0, sizeof(t));
    for (int k = 0; k < 4; ++k) {
      const uint8_t* p = c.huff + ((size_t)i * 4 + k) * kHuffBytes;
      EIOKU_REQUIRE(je::build_table(p, p + 16, k < 2 ? &t.dc[k] : &t.ac[k - 2]), "frame %d: Huffman table %d is not a prefix code", i, k);
    }
    t.blocks_per_mcu = (uint8_t)g.bpm;
    const uint8_t* cp = c.comp + (size_t)i * 9;
    for (int k = 0; k < 9; ++k) EIOKU_REQUIRE(cp[k] < (k % 3 == 0 ? 4 : 2), "frame %d: table selector %d of component %d", i, cp[k], k / 3);
    for (int b = 0; b < g.bpm; ++b) {
      const int comp = b < g.hs * g.vs ? 0 : b - g.hs * g.vs + 1;
      t.dc_of[b] = cp[comp * 3 + 1];
      t.ac_of[b] = cp[comp * 3 + 2];
    }
    for (int k = 0; k < 4 * 64; ++k) EIOKU_REQUIRE(c.qtab[(size_t)i * 256 + k] <= 255, "frame %d: 16-bit quantisation value", i);
  }
  return EIOKU_OK;
}

int add_ms(eioku_mjpeg* m, int stage, int a, int b) {
  double ms = 0.0;
  EIOKU_TRY(m->ev.ms(a, b, &ms));
  m->ms[stage] += ms;
  return EIOKU_OK;
}

// frames [f0, f1) of the call: entropy -> coefficients (-> pixels unless coef_out)
int run_batch(eioku_mjpeg* m, const Call& c, int f0, int f1, uint8_t* out, int16_t* coef_out, int* status, hipStream_t stream) {
  const Geo& g = c.g;
  const int nf = f1 - f0, s0 = c.seg_begin[f0], s1 = c.seg_begin[f1], nseg = s1 - s0;
  const uint32_t S = (uint32_t)m->subseq_bits;
  std::vector<Seg> segs(nseg);
  std::vector<uint32_t> frame_sub_end(nf);
  std::vector<uint2> wg;
  uint32_t nsub = 0, max_sub = 0;
  for (int s = 0; s < nseg; ++s) {
    const uint32_t* r = c.seg + (size_t)(s0 + s) * 5;
    Seg& sg = segs[s];
    sg.frame = r[0] - (uint32_t)f0;
    sg.first_mcu = r[1], sg.mcu_count = r[2];
    sg.first_block = r[1] * (uint32_t)g.bpm, sg.nblocks = r[2] * (uint32_t)g.bpm;
    sg.word_off = r[3] / 4, sg.nbits = r[4];
    sg.sub_first = nsub;
    sg.nsub = std::max(1u, (r[4] + S - 1) / S);
    nsub += sg.nsub;
    max_sub = std::max(max_sub, sg.nsub);
    frame_sub_end[sg.frame] = nsub;
  }
  std::vector<uint32_t> sub_seg(nsub);
  for (int s = 0; s < nseg; ++s) std::fill(sub_seg.begin() + segs[s].sub_first, sub_seg.begin() + segs[s].sub_first + segs[s].nsub, (uint32_t)s);
  for (int f = 0; f < nf; ++f)
    for (uint32_t b = f ? frame_sub_end[f - 1] : 0u; b < frame_sub_end[f]; b += kEntThreads) wg.push_back(make_uint2((uint32_t)f, b));

  const size_t ncoef = (size_t)nf * g.blocks * 64;
  EIOKU_TRY(eioku::grow_synced(m->segs, (size_t)nseg));
  EIOKU_TRY(eioku::grow_synced(m->sub_seg, (size_t)nsub));
  EIOKU_TRY(eioku::grow_synced(m->frame_sub_end, (size_t)nf));
  EIOKU_TRY(eioku::grow_synced(m->wg, wg.size()));
  EIOKU_TRY(eioku::grow_synced(m->exits, (size_t)nsub * 2));
  EIOKU_TRY(eioku::grow_synced(m->prev, (size_t)nsub));
  EIOKU_TRY(eioku::grow_synced(m->first, (size_t)nsub));
  EIOKU_TRY(eioku::grow_synced(m->flags, (size_t)kRoundGroup));
  EIOKU_TRY(eioku::grow_synced(m->tables, (size_t)nf));
  EIOKU_TRY(eioku::grow_synced(m->qtab, (size_t)nf * 256));
  EIOKU_TRY(eioku::grow_synced(m->comp_q, (size_t)nf * 3));
  EIOKU_TRY(eioku::grow_synced(m->coef, ncoef));
  EIOKU_TRY(eioku::grow_synced(m->status, (size_t)nf));
  if (!coef_out) {
    EIOKU_TRY(eioku::grow_synced(m->yplane, (size_t)nf * g.yh * g.yw));
    EIOKU_TRY(eioku::grow_synced(m->cplane, (size_t)nf * 2 * g.ch * g.cw));
  }
  const size_t nwords = c.entropy_bytes / 4;
  if (f0 == 0) EIOKU_TRY(eioku::grow_synced(m->words, nwords + 2));
  std::vector<uint8_t> comp_q((size_t)nf * 3);
  for (int f = 0; f < nf; ++f)
    for (int k = 0; k < 3; ++k) comp_q[f * 3 + k] = c.comp[(size_t)(f0 + f) * 9 + k * 3];

  EIOKU_TRY(m->ev.record(kEvStart, stream));
  if (f0 == 0) {  // the whole call's entropy bytes, once, and two zero words behind them
    EIOKU_HIP_CHECK(hipMemcpyAsync(m->words, c.entropy, nwords * 4, hipMemcpyHostToDevice, stream));
    EIOKU_HIP_CHECK(hipMemsetAsync(m->words.p + nwords, 0, 8, stream));
  }
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->segs, segs.data(), sizeof(Seg) * nseg, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->sub_seg, sub_seg.data(), 4 * (size_t)nsub, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->frame_sub_end, frame_sub_end.data(), 4 * (size_t)nf, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->wg, wg.data(), sizeof(uint2) * wg.size(), hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->tables, c.tables.data() + f0, sizeof(je::FrameTables) * nf, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->qtab, c.qtab + (size_t)f0 * 256, 512 * (size_t)nf, hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->comp_q, comp_q.data(), comp_q.size(), hipMemcpyHostToDevice, stream));
  EIOKU_HIP_CHECK(hipMemsetAsync(m->coef, 0, ncoef * 2, stream));
  EIOKU_HIP_CHECK(hipMemsetAsync(m->status, 0, 4 * (size_t)nf, stream));
  EIOKU_TRY(m->ev.record(kEvUploaded, stream));

  // synchronisation rounds: the fixed point is reached when a round decodes nothing
  uint4* ex[2] = {m->exits.p, m->exits.p + nsub};
  const unsigned nwg = (unsigned)wg.size();
  int launched = 0, cur = 0, rounds = 0;  // ex[cur] holds the exits of the last round
  bool done = false;
  while (!done) {
    // after round r the first r subsequences of every segment are exact: round max_sub + 1 decodes nothing
    EIOKU_REQUIRE(launched <= (int)max_sub + kRoundGroup, "the synchronisation did not end after %d rounds (%u subsequences)", launched, max_sub);
    EIOKU_HIP_CHECK(hipMemsetAsync(m->flags, 0, 4 * kRoundGroup, stream));
    for (int k = 0; k < kRoundGroup; ++k, ++launched) {
      hipLaunchKernelGGL(k_sync_round, dim3(nwg), dim3(kEntThreads), 0, stream, m->words.p, m->segs.p, m->sub_seg.p, m->wg.p,
                         m->frame_sub_end.p, m->tables.p, S, launched == 0 ? 1 : 0, ex[cur], ex[cur ^ 1], m->prev.p, m->flags.p + k);
      cur ^= 1;
    }
    EIOKU_LAUNCH_CHECK();
    uint32_t flags[kRoundGroup];
    EIOKU_HIP_CHECK(hipMemcpyAsync(flags, m->flags, 4 * kRoundGroup, hipMemcpyDeviceToHost, stream));
    EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
    for (int k = 0; k < kRoundGroup; ++k) {
      if (flags[k]) ++rounds;
      else done = true;
    }
  }
  m->rounds = std::max(m->rounds, rounds);
  EIOKU_TRY(m->ev.record(kEvSynced, stream));

  hipLaunchKernelGGL(k_sub_scan, dim3((unsigned)nseg), dim3(kScanThreads), 0, stream, m->segs.p, ex[cur], m->first.p, m->status.p);
  hipLaunchKernelGGL(k_write, dim3(nwg), dim3(kEntThreads), 0, stream, m->words.p, m->segs.p, m->sub_seg.p, m->wg.p, m->frame_sub_end.p,
                     m->tables.p, S, ex[cur], m->first.p, g.blocks, m->coef.p);
  hipLaunchKernelGGL(k_dc_scan, dim3((unsigned)(nseg * g.ncomp)), dim3(64), 0, stream, m->segs.p, g, m->coef.p);
  EIOKU_LAUNCH_CHECK();
  EIOKU_TRY(m->ev.record(kEvWritten, stream));

  if (coef_out) {
    EIOKU_HIP_CHECK(hipMemcpyAsync(coef_out + (size_t)f0 * g.blocks * 64, m->coef, ncoef * 2, hipMemcpyDeviceToHost, stream));
  } else {
    const bool luma = c.fmt == EIOKU_MJPEG_LUMA;
    const long long nblk = (long long)nf * g.blocks;
    hipLaunchKernelGGL(k_idct, dim3((unsigned)((nblk + 63) / 64)), dim3(64), 0, stream, m->coef.p, nblk, g, m->qtab.p, m->comp_q.p, luma ? 1 : 0,
                       m->yplane.p, m->cplane.p);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY(m->ev.record(kEvIdct, stream));
    if (luma) {
      const long long px = (long long)nf * g.h * g.w;
      hipLaunchKernelGGL(k_luma, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, stream, m->yplane.p, px, g, out + (size_t)f0 * g.h * g.w);
    } else {
      const long long pairs = (long long)nf * g.h * ((g.w + 1) / 2);
      hipLaunchKernelGGL(k_colour, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, stream, m->yplane.p, m->cplane.p, pairs, g,
                         c.fmt == EIOKU_MJPEG_RGB ? 1 : 0, out + (size_t)f0 * g.h * g.w * 3);
    }
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY(m->ev.record(kEvColour, stream));
  }
  EIOKU_HIP_CHECK(hipMemcpyAsync(status + f0, m->status, 4 * (size_t)nf, hipMemcpyDeviceToHost, stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));  // the host vectors above have been read; status and coef_out are filled
  EIOKU_TRY(add_ms(m, 0, kEvStart, kEvUploaded));
  EIOKU_TRY(add_ms(m, 1, kEvUploaded, kEvSynced));
  EIOKU_TRY(add_ms(m, 2, kEvSynced, kEvWritten));
  if (!coef_out) {
    EIOKU_TRY(add_ms(m, 3, kEvWritten, kEvIdct));
    EIOKU_TRY(add_ms(m, 4, kEvIdct, kEvColour));
  }
  return EIOKU_OK;
}

int run_call(eioku_mjpeg* m, Call& c, uint8_t* out, int16_t* coef_out, int32_t* status, void* stream_) {
  EIOKU_REQUIRE(m, "NULL handle");
  EIOKU_TRY(validate(c, m->subseq_bits));
  EIOKU_REQUIRE_INIT();
  for (double& v : m->ms) v = 0.0;
  m->rounds = 0;
  if (c.n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(status && (out || coef_out), "NULL output");
  hipStream_t stream = (hipStream_t)stream_;
  const size_t per_frame = (size_t)c.g.blocks * 128;
  int step = (int)std::max<size_t>(1, kCoefBudget / per_frame);
  if (m->batch_frames > 0) step = std::min(step, m->batch_frames);
  for (int f0 = 0; f0 < c.n; f0 += step) EIOKU_TRY(run_batch(m, c, f0, std::min(c.n, f0 + step), out, coef_out, status, stream));
  return EIOKU_OK;
}

}  // namespace

extern "C" {

int eioku_mjpeg_create(eioku_mjpeg_t** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL out");
  *out = nullptr;
  eioku_mjpeg* m = new eioku_mjpeg();
  if (const int rc = m->ev.ensure(kNumEvents)) {
    eioku_mjpeg_destroy(m);
    return rc;
  }
  *out = m;
  return EIOKU_OK;
}

void eioku_mjpeg_destroy(eioku_mjpeg_t* m) {
  if (!m) return;
  delete m;
}

int eioku_mjpeg_set_subseq_bits(eioku_mjpeg_t* m, int bits) {
  EIOKU_REQUIRE(m, "NULL handle");
  EIOKU_REQUIRE(bits >= 32 && bits <= 4096 && bits % 32 == 0, "subsequence size %d: a multiple of 32 in [32, 4096]", bits);
  m->subseq_bits = bits;
  return EIOKU_OK;
}

int eioku_mjpeg_set_batch_frames(eioku_mjpeg_t* m, int frames) {
  EIOKU_REQUIRE(m, "NULL handle");
  EIOKU_REQUIRE(frames >= 0, "%d frames per sub-batch", frames);
  m->batch_frames = frames;
  return EIOKU_OK;
}

int eioku_mjpeg_decode(eioku_mjpeg_t* m, const uint8_t* entropy, size_t entropy_bytes, const uint32_t* seg, int nseg, const uint16_t* qtab,
                       const uint8_t* huff, const uint8_t* comp, int n, int h, int w, int ncomp, int hs, int vs, int fmt, uint8_t* out,
                       int32_t* status, void* stream) {
  Call c = {};
  c.g.h = h, c.g.w = w, c.g.ncomp = ncomp, c.g.hs = hs, c.g.vs = vs;
  c.n = n, c.nseg = nseg, c.fmt = fmt;
  c.entropy = entropy, c.entropy_bytes = entropy_bytes, c.seg = seg, c.qtab = qtab, c.huff = huff, c.comp = comp;
  EIOKU_REQUIRE(n <= 0 || out, "NULL output");
  return run_call(m, c, out, nullptr, status, stream);
}

int eioku_mjpeg_coefficients(eioku_mjpeg_t* m, const uint8_t* entropy, size_t entropy_bytes, const uint32_t* seg, int nseg,
                             const uint16_t* qtab, const uint8_t* huff, const uint8_t* comp, int n, int h, int w, int ncomp, int hs, int vs,
                             int16_t* coef, int32_t* status, void* stream) {
  Call c = {};
  c.g.h = h, c.g.w = w, c.g.ncomp = ncomp, c.g.hs = hs, c.g.vs = vs;
  c.n = n, c.nseg = nseg, c.fmt = EIOKU_MJPEG_LUMA;
  c.entropy = entropy, c.entropy_bytes = entropy_bytes, c.seg = seg, c.qtab = qtab, c.huff = huff, c.comp = comp;
  EIOKU_REQUIRE(n <= 0 || coef, "NULL output");
  return run_call(m, c, nullptr, coef, status, stream);
}

int eioku_mjpeg_last(eioku_mjpeg_t* m, double* ms5, int* rounds) {
  EIOKU_REQUIRE(m && ms5 && rounds, "bad argument");
  for (int i = 0; i < 5; ++i) ms5[i] = m->ms[i];
  *rounds = m->rounds;
  return EIOKU_OK;
}

}  // extern "C"
