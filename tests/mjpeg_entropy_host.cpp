// Host program for tests/test_mjpeg_host.py: runs the entropy stage of K28 -- the very code of csrc/jpeg_entropy.h that the
// kernels run -- on the CPU, in the order the kernels run it (synchronisation rounds, scan, guarded write pass, DC scan),
// so that it can be built with -fsanitize=address,undefined.
//
//   mjpeg_entropy_host <fixtures.bin>
//
// The file holds well-formed frames with the coefficients expected of them.  Each is decoded at S = 32 and S = 1024 and
// compared; then its entropy data is truncated, and replaced by garbage, and decoded again: those runs must end, and
// where the damage leaves a segment too few bits for its blocks the status must say so.  Exit code 0: all of that held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy.h"

namespace je = jpeg_entropy;

struct Fixture {
  int h, w, ncomp, hs, vs, nseg, entropy_bytes, blocks;
  std::vector<uint32_t> seg;  // [nseg][5]: frame, first MCU, MCU count, byte offset, bit length
  std::vector<uint8_t> huff, comp, entropy;
  std::vector<int16_t> coef;
};

template <typename T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct CoefSink {
  int16_t* base;
  uint32_t ord, owned;
  void dc(int v) {
    if (ord < owned) base[(size_t)ord * 64] = (int16_t)v;
  }
  void ac(int z, int v) {
    if (ord < owned) base[(size_t)ord * 64 + je::natural_of(z)] = (int16_t)v;
  }
  void close() { ++ord; }
};

// -> status; rounds: synchronisation rounds in which a subsequence was decoded (the largest over the segments)
static int decode(const Fixture& fx, const std::vector<uint8_t>& entropy, const std::vector<uint32_t>& seg, uint32_t S,
                  std::vector<int16_t>& coef, int* rounds) {
  je::FrameTables ft;
  memset(&ft, 0, sizeof(ft));
  for (int k = 0; k < 4; ++k) {
    const uint8_t* p = fx.huff.data() + (size_t)k * 272;
    if (!je::build_table(p, p + 16, k < 2 ? &ft.dc[k] : &ft.ac[k - 2])) return -1;
  }
  const int ny = fx.hs * fx.vs, bpm = fx.ncomp == 1 ? 1 : ny + 2;
  ft.blocks_per_mcu = (uint8_t)bpm;
  for (int b = 0; b < bpm; ++b) {
    const int c = b < ny ? 0 : b - ny + 1;
    ft.dc_of[b] = fx.comp[c * 3 + 1];
    ft.ac_of[b] = fx.comp[c * 3 + 2];
  }
  std::vector<uint32_t> words(entropy.size() / 4);
  if (!words.empty()) memcpy(words.data(), entropy.data(), words.size() * 4);
  coef.assign((size_t)fx.blocks * 64, 0);
  int status = 0;
  *rounds = 0;
  for (int s = 0; s < fx.nseg; ++s) {
    const uint32_t* r = seg.data() + (size_t)s * 5;
    const uint32_t nbits = r[4], nwords = (nbits + 31) / 32;
    const uint32_t* w = words.data() + r[3] / 4;
    const uint32_t nsub = nbits ? (nbits + S - 1) / S : 1;
    struct Exit {
      je::State s;
      uint32_t closed;
    };
    std::vector<je::State> entry(nsub), last(nsub);
    std::vector<Exit> exits(nsub);
    for (uint32_t i = 0; i < nsub; ++i) entry[i] = {i * S, 0u, 0u};
    int n_rounds = 0;
    for (bool first = true;; first = false) {
      bool decoded = false;
      for (uint32_t i = 0; i < nsub; ++i) {
        const je::State e = entry[i];
        if (!first && last[i].p == e.p && last[i].b == e.b && last[i].z == e.z) continue;
        last[i] = e;
        je::State st = e;
        je::NullSink sink;
        exits[i].closed = je::run(ft, w, nwords, nbits, (i + 1) * S, st, sink);
        exits[i].s = st;
        decoded = true;
      }
      if (!decoded) break;
      ++n_rounds;
      if (n_rounds > (int)nsub + 1) return -2;  // the iteration must end after at most nsub + 1 rounds
      for (uint32_t i = 1; i < nsub; ++i) entry[i] = exits[i - 1].s;
    }
    if (n_rounds > *rounds) *rounds = n_rounds;
    const uint32_t owned = r[2] * (uint32_t)bpm;
    uint32_t ord = 0;
    for (uint32_t i = 0; i < nsub; ++i) {  // exclusive scan and write pass
      je::State st = entry[i];
      CoefSink sink = {coef.data() + (size_t)r[1] * bpm * 64, ord, owned};
      je::run(ft, w, nwords, nbits, (i + 1) * S, st, sink);
      ord += exits[i].closed;
    }
    if (ord < owned) status = 1;
    for (int c = 0; c < fx.ncomp; ++c) {  // DC differences -> DC values, predictor 0 at the restart
      const int hv = c == 0 ? ny : 1, off = c == 0 ? 0 : ny + c - 1;
      uint32_t pred = 0;
      for (uint32_t j = 0; j < r[2] * (uint32_t)hv; ++j) {
        int16_t* p = coef.data() + ((size_t)(r[1] + j / hv) * bpm + off + j % hv) * 64;
        pred += (uint32_t)(int)*p;
        *p = (int16_t)(uint16_t)pred;
      }
    }
  }
  return status;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int nfix = 0;
  if (fread(&nfix, 4, 1, f) != 1 || nfix < 1 || nfix > 64) return 2;
  int failures = 0;
  for (int k = 0; k < nfix; ++k) {
    Fixture fx;
    int head[8];
    if (fread(head, 4, 8, f) != 8) return 2;
    fx.h = head[0], fx.w = head[1], fx.ncomp = head[2], fx.hs = head[3], fx.vs = head[4], fx.nseg = head[5], fx.entropy_bytes = head[6],
    fx.blocks = head[7];
    if (fx.nseg < 1 || fx.nseg > 1 << 20 || fx.entropy_bytes < 0 || fx.entropy_bytes % 4 || fx.blocks < 1 || fx.blocks > 1 << 22) return 2;
    if (!read_vec(f, fx.seg, (size_t)fx.nseg * 5) || !read_vec(f, fx.huff, 4 * 272) || !read_vec(f, fx.comp, 12) ||
        !read_vec(f, fx.entropy, (size_t)fx.entropy_bytes) || !read_vec(f, fx.coef, (size_t)fx.blocks * 64))
      return 2;
    std::vector<int16_t> coef;
    int rounds32 = 0, rounds = 0;
    for (uint32_t S : {32u, 1024u}) {
      const int st = decode(fx, fx.entropy, fx.seg, S, coef, S == 32 ? &rounds32 : &rounds);
      const bool same = coef == fx.coef;
      printf("fixture %d S %u: status %d, coefficients %s\n", k, S, st, same ? "equal" : "DIFFER");
      if (st != 0 || !same) ++failures;
    }
    printf("fixture %d rounds32 %d\n", k, rounds32);

    // truncated: a quarter of every segment's bits cannot close its blocks
    std::vector<uint32_t> seg = fx.seg;
    for (int s = 0; s < fx.nseg; ++s) seg[(size_t)s * 5 + 4] /= 4;
    int st = decode(fx, fx.entropy, seg, 32, coef, &rounds);
    printf("fixture %d truncated: status %d\n", k, st);
    if (st != 1) ++failures;
    // garbage, short: a block takes at least two bits (one code for DC, one for the end of the block)
    std::vector<uint8_t> junk(fx.entropy.size());
    uint32_t x = 12345u + (uint32_t)k;
    for (uint8_t& b : junk) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
    seg = fx.seg;
    for (int s = 0; s < fx.nseg; ++s) {
      uint32_t* r = seg.data() + (size_t)s * 5;
      const uint32_t owned = r[2] * (uint32_t)(fx.ncomp == 1 ? 1 : fx.hs * fx.vs + 2);
      if (r[4] > owned) r[4] = owned;
    }
    st = decode(fx, junk, seg, 32, coef, &rounds);
    printf("fixture %d short garbage: status %d\n", k, st);
    if (st != 1) ++failures;
    // garbage at full length, all ones, all zeros: must end without touching anything it does not own
    for (int kind = 0; kind < 3; ++kind) {
      if (kind == 1) std::fill(junk.begin(), junk.end(), (uint8_t)0xFF);
      if (kind == 2) std::fill(junk.begin(), junk.end(), (uint8_t)0);
      for (uint32_t S : {32u, 256u}) {
        st = decode(fx, junk, fx.seg, S, coef, &rounds);
        printf("fixture %d garbage %d S %u: status %d rounds %d\n", k, kind, S, st, rounds);
        if (st < 0) ++failures;
      }
    }
  }
  fclose(f);
  printf("%s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
