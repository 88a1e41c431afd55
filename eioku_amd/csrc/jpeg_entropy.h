// Baseline JPEG entropy decoding, shared by the device kernels of mjpeg.hip (K28) and by host programs: the bit reader,
// the Huffman table builder and the one-symbol step.  Plain C++ with no dependency but <stdint.h>; every function is
// __host__ __device__ under hipcc and an ordinary inline function under any other compiler, so the host test program
// (tests/mjpeg_entropy_host.cpp) runs the very code the kernels run.
//
// A scan segment is the entropy-coded data between two restart markers, unstuffed (FF 00 -> FF), as big-endian bits in
// 32-bit words.  A decoder's state is (p, b, z): bit position, block-in-MCU index (it selects the component's DC / AC
// tables) and zigzag index.  z == 0 expects a DC symbol, anything else an AC symbol.  Every memory access is bounded by
// the word count the caller states, and every step consumes at least one bit, whatever the bits are.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

namespace jpeg_entropy {

constexpr int kLookBits = 9;
constexpr int kMaxBlocksPerMcu = 6;  // 2x2 luma + Cb + Cr

// One Huffman table: a 9-bit prefix look-up, and the canonical maxcode / valptr form (JPEG F.2.2.3) for longer codes.
struct HuffTable {
  uint16_t look[1 << kLookBits];  // length << 8 | symbol for codes of up to 9 bits; 0: longer, or no such code
  int32_t maxcode[18];            // [l], l = 1..16: the largest code of length l, -1 if there is none; [17] ends every search
  int32_t valoff[17];             // [l]: index into vals of the first code of length l, minus that code
  uint8_t vals[256];
};

// The tables of one frame and how its blocks use them.
struct FrameTables {
  HuffTable dc[2], ac[2];
  uint8_t blocks_per_mcu;
  uint8_t dc_of[kMaxBlocksPerMcu];  // block-in-MCU index -> DC table
  uint8_t ac_of[kMaxBlocksPerMcu];
  uint8_t pad;
};

struct State {
  uint32_t p;  // bit position in the segment
  uint32_t b;  // block-in-MCU index
  uint32_t z;  // zigzag index, 0..63
};

// zigzag position -> natural (row-major) index
JPEG_HD int natural_of(int z) {
  // 64 six-bit entries would need a table in constant memory on one side and static storage on the other; the closed
  // form below is not worth it either, so the table lives in the function (the compilers place it in constant data).
  const uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[z & 63];
}

// DHT payload (16 counts, then the symbols in code order) -> table.  False, with the table unusable, when the counts
// describe no prefix code (more than 256 symbols, or more codes of a length than that length has left).
JPEG_HD bool build_table(const uint8_t* counts, const uint8_t* symbols, HuffTable* t) {
  for (int i = 0; i < (1 << kLookBits); ++i) t->look[i] = 0;
  for (int i = 0; i < 256; ++i) t->vals[i] = 0;
  int total = 0;
  for (int l = 1; l <= 16; ++l) total += counts[l - 1];
  if (total > 256) return false;
  for (int i = 0; i < total; ++i) t->vals[i] = symbols[i];
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = counts[l - 1];
    if (code + n > (1 << l)) return false;
    t->valoff[l] = k - code;
    if (l <= kLookBits)
      for (int i = 0; i < n; ++i) {
        const int first = (code + i) << (kLookBits - l);
        for (int j = 0; j < (1 << (kLookBits - l)); ++j) t->look[first + j] = (uint16_t)(l << 8 | t->vals[k + i]);
      }
    k += n;
    code += n;
    t->maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  t->maxcode[0] = -1;
  t->valoff[0] = 0;
  t->maxcode[17] = 0x7FFFFFFF;
  return true;
}

// 32 bits from bit position p of a segment of `nwords` big-endian words; bits past the last word read as zero
JPEG_HD uint32_t peek32(const uint32_t* words, uint32_t nwords, uint32_t p) {
  const uint32_t w = p >> 5, s = p & 31;
  const uint32_t hi = w < nwords ? __builtin_bswap32(words[w]) : 0u;
  const uint32_t lo = w + 1 < nwords ? __builtin_bswap32(words[w + 1]) : 0u;
  return s ? (hi << s) | (lo >> (32 - s)) : hi;
}

// top 16 bits of `bits` -> symbol and code length; length 0: the prefix matches no code
JPEG_HD int decode_symbol(const HuffTable& t, uint32_t bits, int* length) {
  const uint32_t e = t.look[bits >> (32 - kLookBits)];
  if (e) {
    *length = (int)(e >> 8);
    return (int)(e & 255u);
  }
  int l = kLookBits + 1;
  while ((int32_t)(bits >> (32 - l)) > t.maxcode[l]) ++l;  // maxcode[17] stops it
  if (l > 16) {
    *length = 0;
    return 0;
  }
  *length = l;
  return t.vals[((int32_t)(bits >> (32 - l)) + t.valoff[l]) & 255];
}

JPEG_HD int extend(uint32_t v, int s) { return s == 0 ? 0 : ((int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v); }

// A sink that stores nothing: the synchronisation rounds only follow the state.
struct NullSink {
  JPEG_HD void dc(int) {}
  JPEG_HD void ac(int, int) {}
  JPEG_HD void close() {}
};

// One symbol.  `s` moves to the next symbol boundary (p never beyond `nbits`); the sink hears of a DC difference, of an AC
// coefficient with its zigzag index, and of a block being closed.
//   DC symbol n (its low four bits): n value bits follow; z = 1.
//   AC symbol (r, n): n = 0, r = 15 skips 16 coefficients; n = 0 otherwise ends the block; else r zeros, then a coefficient
//   of n bits.  z >= 64 closes the block and moves b on, modulo the blocks per MCU.
//   A prefix that matches no code consumes one bit and changes nothing else.
template <typename Sink>
JPEG_HD void step(const FrameTables& ft, const uint32_t* words, uint32_t nwords, uint32_t nbits, State& s, Sink& sink) {
  const uint32_t bits = peek32(words, nwords, s.p);
  const bool is_dc = s.z == 0;
  const HuffTable& t = is_dc ? ft.dc[ft.dc_of[s.b] & 1] : ft.ac[ft.ac_of[s.b] & 1];
  int len;
  const int sym = decode_symbol(t, bits, &len);
  uint32_t used = 1;
  if (len) {
    const int n = sym & 15, r = is_dc ? 0 : sym >> 4;
    const uint32_t v = n ? (bits << len) >> (32 - n) : 0u;  // len <= 16 and n <= 15: within the 32 bits
    used = (uint32_t)(len + n);
    bool closed = false;
    if (is_dc) {
      sink.dc(extend(v, n));
      s.z = 1;
    } else if (n == 0) {
      if (r == 15) s.z += 16;
      else closed = true;
    } else {
      s.z += (uint32_t)r;
      if (s.z < 64) sink.ac((int)s.z, extend(v, n));
      s.z += 1;
    }
    if (closed || s.z >= 64) {
      sink.close();
      s.z = 0;
      s.b = s.b + 1 >= ft.blocks_per_mcu ? 0 : s.b + 1;
    }
  }
  s.p = nbits - s.p <= used ? nbits : s.p + used;
}

// From state `s` to the first symbol boundary at or past `stop` (at most nbits).  Returns the number of blocks closed.
template <typename Sink>
JPEG_HD uint32_t run(const FrameTables& ft, const uint32_t* words, uint32_t nwords, uint32_t nbits, uint32_t stop, State& s,
                     Sink& sink) {
  struct Counting {
    Sink& inner;
    uint32_t n;
    JPEG_HD void dc(int v) { inner.dc(v); }
    JPEG_HD void ac(int z, int v) { inner.ac(z, v); }
    JPEG_HD void close() {
      inner.close();
      ++n;
    }
  } c{sink, 0};
  if (stop > nbits) stop = nbits;
  while (s.p < stop) step(ft, words, nwords, nbits, s, c);
  return c.n;
}

}  // namespace jpeg_entropy
