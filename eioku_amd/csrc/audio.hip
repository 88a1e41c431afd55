// K23: audio front end for gfx950 -- interleaved PCM of any rate, width and channel count -> 16 kHz mono fp32, the input of
// the VAD (K22) and of Whisper's log-mel stage.
//
// The resampler is the polyphase form of scipy.signal.resample_poly(x, up, down) with up / down = 16000 / rate in lowest
// terms: for output n, t = n * down + half, p = t mod up, i0 = t div up, y[n] = sum_q B[p][q] * x[i0 - q] over q = 0..T-1 with
// x = 0 outside the file, accumulated in fp32 from 0 in ascending q with a separate multiply and add (no FMA), so that a
// numpy fp32 loop gives the same bits.  The taps are designed on the host; this file only applies them.
//
//   k_audio_resample   one workgroup per tile of `tile` outputs (persistent: a workgroup stages the bank once and walks
//                      tiles with the grid's stride).  Per tile it decodes and downmixes the tile's input span,
//                      (tile - 1) * down / up + T frames, into LDS once; then thread i runs the q loop of output i out of LDS.
//                      Bank layout in LDS: W[q][j] with j the place of phase p in the order in which consecutive outputs
//                      visit the phases, p = (j * (down mod up)) mod up.  Output n reads W[q][(j0 + n) mod up]: a wave's 64
//                      lanes read consecutive dwords (one wrap at most when up >= 32, the same few addresses when up is
//                      small), where the definition's B[p][q] would put them T dwords apart on one bank whenever T is a
//                      multiple of 32.
//   k_audio_decode     rate == 16000: decode and downmix only.
//
// Decode: u8 (v - 128) / 128, s16 v / 2^15, s24 (little-endian, sign-extended) v / 2^23, s32 float(v) * 2^-31, f32 as is; the
// channels are summed in order in fp32 and divided (IEEE) by their count.  A lane loads the aligned dwords that hold its
// frame's samples: consecutive lanes take consecutive frames, so a wave's loads cover one contiguous run of bytes.
//
// Long files run in slabs of slab_out outputs.  Absolute positions are 64-bit and stay on the host (audio_plan); the kernel
// sees slab-relative indices below 2^31, the slab's first phase and the count of zero frames in front of the slab's input.
#include "common.h"

#include <vector>

using namespace eioku;

namespace {

constexpr int kThreads = 256;
constexpr int kLdsFloats = 16384;       // 64 KiB static LDS: bank, then the tile's input span
constexpr int kMaxTaps = 14336;
constexpr int kMaxChannels = 8;

struct Plan {            // one slab, in 64-bit on the host
  long long out_start, n_out, first_frame, frames, lead, trail, phase;
};

// up, down coprime.  0 when slab is past the end.
bool audio_plan(int up, int down, int T, long long slab_out, long long n_frames, long long slab, Plan* pl) {
  const long long half = up == 1 && down == 1 ? 0 : 10LL * (up > down ? up : down);   // the passthrough has no filter delay
  const long long total = (n_frames * up + down - 1) / down;
  long long eff = (2147483647LL - up - (long long)T * up) / down;   // phase + n * down, and the T frames behind it, stay below 2^31
  if (slab_out < eff) eff = slab_out;
  const long long n0 = slab * eff;
  if (n0 >= total) return false;
  const long long cnt = total - n0 < eff ? total - n0 : eff;
  const long long t0 = n0 * down + half, t1 = (n0 + cnt - 1) * down + half;
  const long long lo = t0 / up - (T - 1), hi = t1 / up + 1;   // input frames [lo, hi), before clipping to the file
  long long first = lo < 0 ? 0 : lo;
  if (first > n_frames) first = n_frames;
  const long long end = hi < n_frames ? hi : n_frames;
  pl->out_start = n0;
  pl->n_out = cnt;
  pl->first_frame = first;
  pl->frames = end > first ? end - first : 0;
  pl->lead = first - lo;
  pl->trail = (hi - lo) - pl->lead - pl->frames;
  pl->phase = t0 % up;
  return true;
}

struct Src {
  const uint32_t* raw;   // the slab's frames, 4-byte aligned, with 8 readable bytes behind the last frame
  unsigned lead, cnt;    // frame r of the slab is raw's frame r - lead for r in [lead, lead + cnt), zero elsewhere
  int fmt, ch;
};

// Sample width in bytes.
__host__ __device__ inline int fmt_bytes(int fmt) { return fmt == EIOKU_PCM_U8 ? 1 : fmt == EIOKU_PCM_S16 ? 2 : fmt == EIOKU_PCM_S24 ? 3 : 4; }

__device__ __forceinline__ float decode_frame(const Src& s, unsigned r) {
  if (r < s.lead || r - s.lead >= s.cnt) return 0.f;
  const int bps = fmt_bytes(s.fmt);
  unsigned o = (r - s.lead) * (unsigned)(bps * s.ch);     // below 2^31: checked on the host
  float sum = 0.f;
  for (int c = 0; c < s.ch; ++c, o += bps) {
    const uint32_t lo = s.raw[o >> 2];
    float v;
    if (s.fmt == EIOKU_PCM_S24) {   // three bytes at any of the four offsets: two dwords, shifted as one
      const uint32_t hi = s.raw[(o >> 2) + 1];
      const uint32_t w = (uint32_t)((((uint64_t)hi << 32) | lo) >> ((o & 3) * 8));
      v = (float)((int32_t)(w << 8) >> 8) * (1.f / 8388608.f);
    } else if (s.fmt == EIOKU_PCM_S16) {
      v = (float)(int16_t)(lo >> ((o & 2) * 8)) * (1.f / 32768.f);
    } else if (s.fmt == EIOKU_PCM_U8) {
      v = (float)((int)((lo >> ((o & 3) * 8)) & 0xff) - 128) * (1.f / 128.f);
    } else if (s.fmt == EIOKU_PCM_S32) {
      v = (float)(int32_t)lo * (1.f / 2147483648.f);
    } else {
      v = __uint_as_float(lo);
    }
    sum = c ? __fadd_rn(sum, v) : v;
  }
  return __fdiv_rn(sum, (float)s.ch);
}

__global__ __launch_bounds__(kThreads) void k_audio_decode(Src s, unsigned n, float* __restrict__ out) {
  const unsigned i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = decode_frame(s, i);
}

// W [T][up] (permuted bank); p0 the slab's first phase, j0 its place in the permuted order; up * T + the span of a tile
// (at most (up - 1 + (tile - 1) * down) / up + T frames) fit kLdsFloats: checked at create.
__global__ __launch_bounds__(kThreads) void k_audio_resample(Src s, const float* __restrict__ W, int up, int down, int T, int tile,
                                                             unsigned p0, unsigned j0, unsigned n_out, float* __restrict__ out) {
  __shared__ float lds[kLdsFloats];
  const int tid = threadIdx.x;
  float* wb = lds;
  float* xs = lds + up * T;
  for (int i = tid; i < up * T; i += kThreads) wb[i] = W[i];
  const unsigned n_tiles = (n_out + tile - 1) / tile;
  for (unsigned ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    __syncthreads();   // the previous tile's reads of xs are over (and, the first time, nothing else)
    const unsigned n_first = ti * (unsigned)tile;
    const unsigned n_last = (n_first + tile < n_out ? n_first + tile : n_out) - 1;
    const unsigned r_first = (p0 + n_first * (unsigned)down) / (unsigned)up;   // the oldest frame of the tile's first output
    const unsigned span = (p0 + n_last * (unsigned)down) / (unsigned)up + T - r_first;
    for (unsigned i = tid; i < span; i += kThreads) xs[i] = decode_frame(s, r_first + i);
    __syncthreads();
    const unsigned n = n_first + tid;
    if (tid < tile && n <= n_last) {
      const unsigned i0 = (p0 + n * (unsigned)down) / (unsigned)up;
      const float* xp = xs + (i0 - r_first) + (T - 1);     // x[i0 - q] = xp[-q]
      const float* wp = wb + (j0 + n) % (unsigned)up;
      float acc = 0.f;
      for (int q = 0; q < T; ++q) acc = __fadd_rn(acc, __fmul_rn(wp[q * up], xp[-q]));
      out[n] = acc;
    }
  }
}

}  // namespace

struct eioku_audio {
  int up = 1, down = 1, T = 0, tile = 0;
  unsigned dinv = 0;          // (down mod up)^-1 mod up: phase p sits at j = p * dinv mod up
  long long slab = 0;         // outputs per slab, after the 31-bit clamp
  hipStream_t st = nullptr;
  DevBuf<float> bank;         // W [T][up]
  DevBuf<float> out;          // slab
  DevBuf<uint32_t> raw;       // the slab's input frames
  DevEvents ev;               // 2 per slab of the last call
  double ms = 0;
};

extern "C" {

int eioku_audio_plan(int up, int down, int taps_per_phase, long long slab_out, long long n_frames, long long slab,
                     long long* plan7) {
  EIOKU_REQUIRE(up >= 1 && down >= 1 && taps_per_phase >= 1 && slab_out >= 1 && n_frames >= 0 && slab >= 0 && plan7, "bad argument");
  EIOKU_REQUIRE(n_frames <= (1LL << 40), "%lld frames: more than 2^40", n_frames);
  Plan pl{};
  if (!audio_plan(up, down, taps_per_phase, slab_out, n_frames, slab, &pl)) return 1;
  const long long v[7] = {pl.out_start, pl.n_out, pl.first_frame, pl.frames, pl.lead, pl.trail, pl.phase};
  memcpy(plan7, v, sizeof v);
  return EIOKU_OK;
}

void eioku_audio_destroy(eioku_audio* a) {
  if (!a) return;
  if (a->st) (void)hipStreamSynchronize(a->st);
  if (a->st) (void)hipStreamDestroy(a->st);
  delete a;  // every buffer and event frees itself
}

int eioku_audio_create(int up, int down, int taps_per_phase, const float* bank, long long slab_out, eioku_audio** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL argument");
  EIOKU_REQUIRE(up >= 1 && down >= 1, "up %d / down %d must be positive", up, down);
  EIOKU_REQUIRE(slab_out >= 1 && slab_out <= (1LL << 26), "slab_out %lld outside 1..2^26", slab_out);
  const int T = taps_per_phase;
  const bool pass = up == 1 && down == 1;
  int tile = 0;
  unsigned dinv = 0;
  if (pass) {
    EIOKU_REQUIRE(T == 0 && !bank, "up == down == 1 is a passthrough: it takes no bank");
  } else {
    int a = up, b = down;
    while (b) { const int t = a % b; a = b; b = t; }
    EIOKU_REQUIRE(a == 1, "up %d and down %d are not in lowest terms", up, down);
    const long long L = 20LL * (up > down ? up : down) + 1;
    EIOKU_REQUIRE(L <= kMaxTaps, "up %d / down %d: the filter has %lld taps, more than %d", up, down, L, kMaxTaps);
    EIOKU_REQUIRE(bank && T == (int)((L + up - 1) / up), "up %d / down %d takes %lld taps per phase, got %d", up, down, (L + up - 1) / up, T);
    for (tile = kThreads; tile >= 32; tile /= 2)
      if ((long long)up * T + ((long long)(up - 1) + (long long)(tile - 1) * down) / up + T <= kLdsFloats) break;
    EIOKU_REQUIRE(tile >= 32, "up %d / down %d: the bank of %d taps and the input span of a tile do not fit %d KiB of LDS", up, down,
                  up * T, kLdsFloats / 256);
    const unsigned d = (unsigned)(down % up);
    for (unsigned j = 0; j < (unsigned)up; ++j)
      if ((j * d) % (unsigned)up == 1u % (unsigned)up) { dinv = j; break; }
  }
  auto* h = new eioku_audio();
  h->up = up, h->down = down, h->T = T, h->tile = tile, h->dinv = dinv;
  const long long eff = (2147483647LL - up - (long long)(T ? T : 1) * up) / down;   // as audio_plan clamps it
  h->slab = slab_out < eff ? slab_out : eff;
  auto fail = [&](int rc, const char* what) {
    set_error("eioku_audio_create: %s failed", what);
    eioku_audio_destroy(h);
    return rc;
  };
  if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) {
    h->st = nullptr;
    return fail(EIOKU_EHIP, "hipStreamCreate");
  }
  if (h->out.grow((size_t)h->slab)) return fail(EIOKU_ENOMEM, "hipMalloc");
  if (!pass) {
    std::vector<float> w((size_t)up * T);    // W[q][j] = B[(j * d) mod up][q]
    const unsigned d = (unsigned)(down % up);
    for (int q = 0; q < T; ++q)
      for (unsigned j = 0; j < (unsigned)up; ++j) w[(size_t)q * up + j] = bank[(size_t)((j * d) % (unsigned)up) * T + q];
    if (const int rc = h->bank.upload(w.data(), w.size())) return fail(rc, rc == EIOKU_ENOMEM ? "hipMalloc" : "hipMemcpy");
  }
  *out = h;
  return EIOKU_OK;
}

int eioku_audio_tile(const eioku_audio* a, int* tile) {
  EIOKU_REQUIRE(a && tile, "NULL argument");
  *tile = a->T ? a->tile : kThreads;
  return EIOKU_OK;
}

int eioku_audio_resample(eioku_audio* a, const void* pcm, int format, int channels, long long n_frames, float* samples_out,
                         long long n_out_cap, long long* n_out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(a && n_frames >= 0 && (pcm || n_frames == 0) && n_out, "bad argument");
  EIOKU_REQUIRE(format >= EIOKU_PCM_U8 && format <= EIOKU_PCM_F32, "unknown PCM format %d", format);
  EIOKU_REQUIRE(channels >= 1 && channels <= kMaxChannels, "%d channels: outside 1..%d", channels, kMaxChannels);
  EIOKU_REQUIRE(n_frames <= (1LL << 40), "%lld frames: more than 2^40", n_frames);
  const long long total = (n_frames * a->up + a->down - 1) / a->down;
  *n_out = total;
  EIOKU_REQUIRE(total == 0 || (samples_out && n_out_cap >= total), "samples_out holds %lld values, %lld frames give %lld", n_out_cap,
                n_frames, total);
  a->ms = 0;
  if (!total) return EIOKU_OK;
  const int T = a->T ? a->T : 1;
  const size_t fb = (size_t)fmt_bytes(format) * channels;
  // frames of a full slab, at most: the byte offset of every frame stays below 2^31 (slab <= 2^26, fb <= 32 leaves room
  // only for ratios up to 1; larger ones shrink the slab of this call)
  long long slab = a->slab;
  const long long max_frames = (2147483647LL - 64) / (long long)fb;
  if ((slab * a->down + a->up) / a->up + T + 1 > max_frames) slab = (max_frames - T - 2) * a->up / a->down;
  EIOKU_REQUIRE(slab >= 1, "a slab of one output does not fit 2^31 bytes");
  const long long n_slabs = (total + slab - 1) / slab;
  const size_t need = (size_t)((slab * a->down + a->up) / a->up + T + 1) * fb + 16;
  if (need > a->raw.cap * 4) {
    EIOKU_HIP_CHECK(hipStreamSynchronize(a->st));
    EIOKU_TRY(a->raw.grow((need + 3) / 4));
  }
  EIOKU_TRY(a->ev.ensure((size_t)(2 * n_slabs)));
  hipStream_t st = a->st;
  static const int cus = num_cus();
  for (long long k = 0; k < n_slabs; ++k) {
    Plan pl{};
    EIOKU_REQUIRE(audio_plan(a->up, a->down, T, slab, n_frames, k, &pl), "slab %lld is past the end", k);
    const size_t bytes = (size_t)pl.frames * fb;
    EIOKU_REQUIRE(pl.n_out <= a->slab && bytes + 16 <= a->raw.cap * 4 && pl.lead + pl.frames < (1LL << 31), "slab %lld does not fit its buffers", k);
    if (bytes)
      EIOKU_HIP_CHECK(hipMemcpyAsync(a->raw.p, (const char*)pcm + (size_t)pl.first_frame * fb, bytes, hipMemcpyHostToDevice, st));
    const Src src{a->raw, (unsigned)pl.lead, (unsigned)pl.frames, format, channels};
    EIOKU_TRY(a->ev.record(2 * k, st));
    if (a->T) {
      const unsigned tiles = (unsigned)((pl.n_out + a->tile - 1) / a->tile);
      const unsigned grid = tiles < 2u * cus ? tiles : 2u * cus;     // two 64 KiB workgroups per CU
      hipLaunchKernelGGL(k_audio_resample, dim3(grid), dim3(kThreads), 0, st, src, a->bank.p, a->up, a->down, a->T, a->tile,
                         (unsigned)pl.phase, (unsigned)((unsigned long long)pl.phase * a->dinv % a->up), (unsigned)pl.n_out, a->out.p);
    } else {
      hipLaunchKernelGGL(k_audio_decode, dim3((unsigned)((pl.n_out + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, src,
                         (unsigned)pl.n_out, a->out.p);
    }
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY(a->ev.record(2 * k + 1, st));
    // the next slab reuses raw and out: stream order keeps its copy behind this slab's kernel and read-back
    EIOKU_HIP_CHECK(hipMemcpyAsync(samples_out + pl.out_start, a->out, (size_t)pl.n_out * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  for (long long k = 0; k < n_slabs; ++k) {
    double t = 0;
    EIOKU_TRY(a->ev.ms(2 * k, 2 * k + 1, &t));
    a->ms += t;
  }
  return EIOKU_OK;
}

int eioku_audio_last_ms(const eioku_audio* a, double* kernel_ms) {
  EIOKU_REQUIRE(a && kernel_ms, "NULL argument");
  *kernel_ms = a->ms;
  return EIOKU_OK;
}

}  // extern "C"
