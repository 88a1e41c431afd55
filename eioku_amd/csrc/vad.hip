// K22: voice activity (Silero VAD v5/v6, 16 kHz branch) for gfx950 -- the speech gate in front of the Whisper decode.
//
// The network runs one chunk of 512 new samples at a time, prefixed with the last 64 samples of the previous chunk (zeros
// before the first): reflect-pad 64 on the right -> STFT as a strided convolution with the checkpoint's basis (258 x 256,
// stride 128, 4 frames) -> magnitude [129][4] -> four Conv1d(k=3, pad 1)+ReLU (129->128 s1, 128->64 s2, 64->64 s2,
// 64->128 s1; lengths 4, 4, 2, 1, 1) -> LSTMCell(128, 128) carried from chunk to chunk -> sigmoid(w_out . relu(h) + b_out).
// fp32 throughout: the probabilities are compared against thresholds and the published model runs in fp32.
//
//   k_vad_encode   everything without a dependence between chunks, up to gx = W_ih e + b_ih + b_hh.  One workgroup per tile
//                  of kTile chunks, activations in LDS, every weight read once per tile and applied to the tile's chunks
//                  from a register (weights are stored transposed, [k][row], so a wave's load is one contiguous line).
//                  Each chunk's dot products are summed in a fixed order that does not depend on the chunk's place in the
//                  tile or the slab.
//   k_vad_lstm     the recurrence: one workgroup of 512 threads for the whole file, thread r keeps row r of W_hh (128 fp32)
//                  in registers for every step, h lives in LDS, c in the 128 threads that own a hidden unit; the output
//                  dot product of step t is reduced by an otherwise idle wave while step t + 1 runs its matrix product.
//
// Long files run in slabs of slab_chunks chunks: the audio of a slab is staged behind the 64 context samples the previous
// slab left, (h, c) stay in a device buffer between the slabs' launches.  The handle owns its stream and every buffer.
#include "common.h"

#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kChunk = 512;    // new samples per chunk
constexpr int kCtx = 64;       // samples carried from the previous chunk
constexpr int kIn = kChunk + kCtx;
constexpr int kPadded = kIn + 64;   // after the right reflect pad
constexpr int kWin = 256, kHopV = 128, kFrames = 4, kBins = 129;
constexpr int kHid = 128, kGates = 4 * kHid;
constexpr int kTile = 4;       // chunks per k_vad_encode workgroup

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

struct EncW {
  const float *basis_t;                 // [256 k][258 rows]
  const float *w0, *b0, *w1, *b1, *w2, *b2, *w3, *b3;   // conv weights [cin * 3][cout]
  const float *wih_t, *bih, *bhh;       // [128 k][512 rows]
};

// grid ceil(n / kTile), 256 threads.  audio: kCtx context samples, then n * 512 samples; chunk i reads audio[512 i .. + 575].
// gx [n][512] fp32.
__global__ __launch_bounds__(256) void k_vad_encode(const float* __restrict__ audio, int n, EncW W, float* __restrict__ gx) {
  __shared__ float4 xp4[kTile][kPadded / 4];
  __shared__ float4 mag4[kTile][kBins];      // [chunk][bin] -> 4 frames
  __shared__ float4 a1[kTile][128];          // [chunk][channel] -> 4 steps
  __shared__ float2 a2[kTile][64];
  __shared__ float a3[kTile][64];
  __shared__ float a4[kTile][kHid];
  __shared__ float part[kTile * kFrames * 2][8];
  const int tid = threadIdx.x, c0 = blockIdx.x * kTile;

  float* xp = reinterpret_cast<float*>(xp4);
  for (int i = tid; i < kTile * kPadded; i += 256) {
    const int c = i / kPadded, j = i - c * kPadded;
    const int src = j < kIn ? j : 2 * kIn - 2 - j;    // xp[576 + q] = x[574 - q]
    xp[i] = c0 + c < n ? audio[(size_t)(c0 + c) * kChunk + src] : 0.f;
  }
  __syncthreads();

  {  // STFT bins 0..127: thread (bin, chunk pair), real and imaginary rows of its bin for 2 chunks x 4 frames
    const int b = tid & 127, ch = tid >> 7;
    float re[2][kFrames] = {}, im[2][kFrames] = {};
    for (int k = 0; k < kWin; k += 4) {
      float wr[4], wi[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        wr[q] = W.basis_t[(k + q) * 2 * kBins + b];
        wi[q] = W.basis_t[(k + q) * 2 * kBins + kBins + b];
      }
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int f = 0; f < kFrames; ++f) {
          const float4 x = xp4[2 * ch + cc][(kHopV * f + k) >> 2];
          re[cc][f] = fmaf(wr[0], x.x, re[cc][f]);
          im[cc][f] = fmaf(wi[0], x.x, im[cc][f]);
          re[cc][f] = fmaf(wr[1], x.y, re[cc][f]);
          im[cc][f] = fmaf(wi[1], x.y, im[cc][f]);
          re[cc][f] = fmaf(wr[2], x.z, re[cc][f]);
          im[cc][f] = fmaf(wi[2], x.z, im[cc][f]);
          re[cc][f] = fmaf(wr[3], x.w, re[cc][f]);
          im[cc][f] = fmaf(wi[3], x.w, im[cc][f]);
        }
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      float m[kFrames];
#pragma unroll
      for (int f = 0; f < kFrames; ++f) m[f] = sqrtf(fmaf(re[cc][f], re[cc][f], im[cc][f] * im[cc][f]));
      mag4[2 * ch + cc][b] = make_float4(m[0], m[1], m[2], m[3]);
    }
  }
  {  // bin 128 (rows 128 and 257): thread (chunk, frame, re/im, k slice of 32), partial sums joined in slice order below
    const int ks = tid & 7, item = tid >> 3, p = item & 1, f = (item >> 1) & 3, c = item >> 3;
    const int row = p ? 2 * kBins - 1 : kBins - 1;
    float s = 0.f;
    for (int k = ks * 32; k < ks * 32 + 32; ++k) s = fmaf(W.basis_t[k * 2 * kBins + row], xp[c * kPadded + kHopV * f + k], s);
    part[item][ks] = s;
  }
  __syncthreads();
  if (tid < kTile * kFrames) {
    const int c = tid >> 2, f = tid & 3;
    float s[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float* q = part[(c * kFrames + f) * 2 + p];
      s[p] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    reinterpret_cast<float*>(&mag4[c][kBins - 1])[f] = sqrtf(fmaf(s[0], s[0], s[1] * s[1]));
  }
  __syncthreads();

  {  // encoder.0: 129 -> 128, stride 1, 4 -> 4 steps; thread (channel, chunk pair)
    const int o = tid & 127, ch = tid >> 7;
    const float bias = W.b0[o];
    float acc[2][4];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[cc][t] = bias;
    for (int ci = 0; ci < kBins; ++ci) {
      const float w0 = W.w0[(ci * 3 + 0) * 128 + o], w1 = W.w0[(ci * 3 + 1) * 128 + o], w2 = W.w0[(ci * 3 + 2) * 128 + o];
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const float4 m = mag4[2 * ch + cc][ci];
        acc[cc][0] = fmaf(w2, m.y, fmaf(w1, m.x, acc[cc][0]));
        acc[cc][1] = fmaf(w2, m.z, fmaf(w1, m.y, fmaf(w0, m.x, acc[cc][1])));
        acc[cc][2] = fmaf(w2, m.w, fmaf(w1, m.z, fmaf(w0, m.y, acc[cc][2])));
        acc[cc][3] = fmaf(w1, m.w, fmaf(w0, m.z, acc[cc][3]));
      }
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
      a1[2 * ch + cc][o] = make_float4(fmaxf(acc[cc][0], 0.f), fmaxf(acc[cc][1], 0.f), fmaxf(acc[cc][2], 0.f), fmaxf(acc[cc][3], 0.f));
  }
  __syncthreads();
  {  // encoder.1: 128 -> 64, stride 2, 4 -> 2 steps (inputs -1..1 and 1..3); thread (channel, chunk)
    const int o = tid & 63, c = tid >> 6;
    float t0 = W.b1[o], t1 = t0;
    for (int ci = 0; ci < 128; ++ci) {
      const float w0 = W.w1[(ci * 3 + 0) * 64 + o], w1 = W.w1[(ci * 3 + 1) * 64 + o], w2 = W.w1[(ci * 3 + 2) * 64 + o];
      const float4 m = a1[c][ci];
      t0 = fmaf(w2, m.y, fmaf(w1, m.x, t0));
      t1 = fmaf(w2, m.w, fmaf(w1, m.z, fmaf(w0, m.y, t1)));
    }
    a2[c][o] = make_float2(fmaxf(t0, 0.f), fmaxf(t1, 0.f));
  }
  __syncthreads();
  {  // encoder.2: 64 -> 64, stride 2, 2 -> 1 step (inputs -1..1)
    const int o = tid & 63, c = tid >> 6;
    float t0 = W.b2[o];
    for (int ci = 0; ci < 64; ++ci) {
      const float w1 = W.w2[(ci * 3 + 1) * 64 + o], w2 = W.w2[(ci * 3 + 2) * 64 + o];
      const float2 m = a2[c][ci];
      t0 = fmaf(w2, m.y, fmaf(w1, m.x, t0));
    }
    a3[c][o] = fmaxf(t0, 0.f);
  }
  __syncthreads();
  {  // encoder.3: 64 -> 128, 1 -> 1 step: only the centre tap meets a sample
    const int o = tid & 127, ch = tid >> 7;
    float t0 = W.b3[o], t1 = t0;
    for (int ci = 0; ci < 64; ++ci) {
      const float w1 = W.w3[(ci * 3 + 1) * 128 + o];
      t0 = fmaf(w1, a3[2 * ch][ci], t0);
      t1 = fmaf(w1, a3[2 * ch + 1][ci], t1);
    }
    a4[2 * ch][o] = fmaxf(t0, 0.f);
    a4[2 * ch + 1][o] = fmaxf(t1, 0.f);
  }
  __syncthreads();
  {  // LSTM input projection: thread owns gate rows tid and tid + 256 of the tile's chunks
    float acc[2][kTile] = {};
    for (int k = 0; k < kHid; ++k) {
      const float wa = W.wih_t[k * kGates + tid], wb = W.wih_t[k * kGates + 256 + tid];
#pragma unroll
      for (int c = 0; c < kTile; ++c) {
        const float e = a4[c][k];
        acc[0][c] = fmaf(wa, e, acc[0][c]);
        acc[1][c] = fmaf(wb, e, acc[1][c]);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = tid + 256 * h;
      const float bi = W.bih[row], bh = W.bhh[row];
#pragma unroll
      for (int c = 0; c < kTile; ++c)
        if (c0 + c < n) gx[(size_t)(c0 + c) * kGates + row] = (acc[h][c] + bi) + bh;
    }
  }
}

// One workgroup, 512 threads, n >= 1 steps.  gx [n][512]; whh_t [128 k][512 rows]; state [256]: h then c, read at the start
// and written at the end (the carry between slabs); probs [n].
__global__ __launch_bounds__(512) void k_vad_lstm(const float* __restrict__ gx, int n, const float* __restrict__ whh_t,
                                                  const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                  float* __restrict__ state, float* __restrict__ probs) {
  __shared__ float4 hs4[kHid / 4];
  __shared__ float gates[kGates];
  __shared__ float hw[kHid];
  float* hs = reinterpret_cast<float*>(hs4);
  const int r = threadIdx.x, lane = r & 63, wave = r >> 6;
  float w[kHid];
#pragma unroll
  for (int k = 0; k < kHid; ++k) w[k] = whh_t[k * kGates + r];
  float c = 0.f, wo = 0.f;
  if (r < kHid) {
    hs[r] = state[r];
    c = state[kHid + r];
    wo = w_out[r];
  }
  const float bo = b_out[0];
  __syncthreads();
  float g_next = gx[r];
  for (int t = 0; t < n; ++t) {
    const float g = g_next;
    if (t + 1 < n) g_next = gx[(size_t)(t + 1) * kGates + r];
    float s0 = g, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int q = 0; q < kHid / 4; ++q) {
      const float4 h = hs4[q];
      s0 = fmaf(w[4 * q], h.x, s0);
      s1 = fmaf(w[4 * q + 1], h.y, s1);
      s2 = fmaf(w[4 * q + 2], h.z, s2);
      s3 = fmaf(w[4 * q + 3], h.w, s3);
    }
    gates[r] = (s0 + s1) + (s2 + s3);
    if (wave == 2 && t > 0) {  // the previous step's output, off the critical path of the unit owners (waves 0 and 1)
      const float v = wave_reduce_add(hw[lane] + hw[lane + 64]);
      if (lane == 0) probs[t - 1] = sigmoidf_(v + bo);
    }
    __syncthreads();
    if (r < kHid) {  // PyTorch gate order: input, forget, cell, output
      const float ig = sigmoidf_(gates[r]), fg = sigmoidf_(gates[kHid + r]), gg = tanhf(gates[2 * kHid + r]),
                  og = sigmoidf_(gates[3 * kHid + r]);
      c = fg * c + ig * gg;
      const float h = og * tanhf(c);
      hs[r] = h;
      hw[r] = fmaxf(h, 0.f) * wo;
    }
    __syncthreads();
  }
  if (wave == 2) {
    const float v = wave_reduce_add(hw[lane] + hw[lane + 64]);
    if (lane == 0) probs[n - 1] = sigmoidf_(v + bo);
  }
  if (r < kHid) {
    state[r] = hs[r];
    state[kHid + r] = c;
  }
}

struct VTensor {
  const char* name;
  int rows, cols;
  DevBuf<float> dev;
  bool set = false;
};

enum { V_BASIS, V_W0, V_B0, V_W1, V_B1, V_W2, V_B2, V_W3, V_B3, V_WIH, V_WHH, V_BIH, V_BHH, V_WOUT, V_BOUT, V_NUM };

}  // namespace

struct eioku_vad {
  int slab = 0;
  hipStream_t st = nullptr;
  VTensor t[V_NUM] = {{"stft.forward_basis_buffer", 2 * kBins, kWin},
                      {"encoder.0.weight", 128, kBins * 3}, {"encoder.0.bias", 128, 1},
                      {"encoder.1.weight", 64, 128 * 3},    {"encoder.1.bias", 64, 1},
                      {"encoder.2.weight", 64, 64 * 3},     {"encoder.2.bias", 64, 1},
                      {"encoder.3.weight", 128, 64 * 3},    {"encoder.3.bias", 128, 1},
                      {"decoder.rnn.weight_ih", kGates, kHid}, {"decoder.rnn.weight_hh", kGates, kHid},
                      {"decoder.rnn.bias_ih", kGates, 1},   {"decoder.rnn.bias_hh", kGates, 1},
                      {"decoder.out.weight", 1, kHid},      {"decoder.out.bias", 1, 1}};
  DevBuf<float> audio;      // kCtx + slab * 512
  DevBuf<float> gx;         // slab * 512
  DevBuf<float> probs;      // slab
  DevBuf<float> state;      // h [128], c [128]
  DevEvents ev;             // 3 per slab of the last call
  double encode_ms = 0, lstm_ms = 0;
};

extern "C" {

void eioku_vad_destroy(eioku_vad* v) {
  if (!v) return;
  if (v->st) (void)hipStreamSynchronize(v->st);
  if (v->st) (void)hipStreamDestroy(v->st);
  delete v;  // every buffer and event frees itself
}

int eioku_vad_create(int slab_chunks, eioku_vad** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL argument");
  EIOKU_REQUIRE(slab_chunks >= 1 && slab_chunks <= (1 << 20), "slab_chunks %d outside 1..2^20", slab_chunks);
  auto* v = new eioku_vad();
  v->slab = slab_chunks;
  auto fail = [&](int rc, const char* what) {
    set_error("eioku_vad_create: %s failed", what);
    eioku_vad_destroy(v);
    return rc;
  };
  if (hipStreamCreateWithFlags(&v->st, hipStreamNonBlocking) != hipSuccess) {
    v->st = nullptr;
    return fail(EIOKU_EHIP, "hipStreamCreate");
  }
  int rc = EIOKU_OK;
  for (auto& t : v->t)
    if (!rc) rc = t.dev.grow((size_t)t.rows * t.cols);
  const size_t s = (size_t)slab_chunks;
  if (rc || v->audio.grow(kCtx + s * kChunk) || v->gx.grow(s * kGates) || v->probs.grow(s) || v->state.grow(2 * kHid))
    return fail(EIOKU_ENOMEM, "hipMalloc");
  *out = v;
  return EIOKU_OK;
}

int eioku_vad_num_tensors(const eioku_vad* v) { return v ? V_NUM : 0; }

int eioku_vad_tensor_info(const eioku_vad* v, int idx, char* name, size_t cap, int* rows, int* cols) {
  EIOKU_REQUIRE(v && idx >= 0 && idx < V_NUM, "bad tensor index %d", idx);
  if (name && cap) snprintf(name, cap, "%s", v->t[idx].name);
  if (rows) *rows = v->t[idx].rows;
  if (cols) *cols = v->t[idx].cols;
  return EIOKU_OK;
}

// Matrices are kept transposed ([col][row]) so that a wave's load of one k is contiguous over its rows.
int eioku_vad_set_tensor(eioku_vad* v, int idx, const float* host, size_t numel) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(v && idx >= 0 && idx < V_NUM && host, "bad argument");
  VTensor& t = v->t[idx];
  const size_t want = (size_t)t.rows * t.cols;
  EIOKU_REQUIRE(numel == want, "%s: expected %zu elements, got %zu", t.name, want, numel);
  std::vector<float> tr;
  const float* src = host;
  if (t.rows > 1 && t.cols > 1) {
    tr.resize(want);
    for (int r = 0; r < t.rows; ++r)
      for (int c = 0; c < t.cols; ++c) tr[(size_t)c * t.rows + r] = host[(size_t)r * t.cols + c];
    src = tr.data();
  }
  EIOKU_HIP_CHECK(hipStreamSynchronize(v->st));
  EIOKU_HIP_CHECK(hipMemcpy(t.dev.p, src, want * sizeof(float), hipMemcpyHostToDevice));
  t.set = true;
  return EIOKU_OK;
}

int eioku_vad_probs(eioku_vad* v, const float* samples, long long n_samples, float* probs_out, long long n_probs_cap,
                    long long* n_probs) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(v && n_samples >= 0 && (samples || n_samples == 0) && n_probs, "bad argument");
  for (const auto& t : v->t) EIOKU_REQUIRE(t.set, "tensor %s has not been set", t.name);
  // faster-whisper pads by 512 - n % 512: a whole zero chunk when n is a multiple of 512
  const long long n = n_samples / kChunk + 1;
  *n_probs = n;
  EIOKU_REQUIRE(probs_out && n_probs_cap >= n, "probs_out holds %lld values, %lld samples give %lld", n_probs_cap, n_samples, n);
  const long long n_slabs = (n + v->slab - 1) / v->slab;
  EIOKU_TRY(v->ev.ensure((size_t)(3 * n_slabs)));
  const EncW W{v->t[V_BASIS].dev, v->t[V_W0].dev, v->t[V_B0].dev, v->t[V_W1].dev, v->t[V_B1].dev, v->t[V_W2].dev, v->t[V_B2].dev,
               v->t[V_W3].dev,    v->t[V_B3].dev, v->t[V_WIH].dev, v->t[V_BIH].dev, v->t[V_BHH].dev};
  hipStream_t st = v->st;
  v->encode_ms = v->lstm_ms = 0;
  EIOKU_HIP_CHECK(hipMemsetAsync(v->state, 0, 2 * kHid * sizeof(float), st));
  EIOKU_HIP_CHECK(hipMemsetAsync(v->audio, 0, kCtx * sizeof(float), st));
  for (long long s = 0; s < n_slabs; ++s) {
    const long long first = s * v->slab;
    const int m = (int)(n - first < v->slab ? n - first : v->slab);
    const long long a0 = first * kChunk;   // first sample of the slab
    long long have = n_samples - a0;
    if (have > (long long)m * kChunk) have = (long long)m * kChunk;
    if (have < 0) have = 0;
    if (s > 0)  // the previous slab was full: its last 64 samples become this slab's context (disjoint ranges)
      EIOKU_HIP_CHECK(hipMemcpyAsync(v->audio, v->audio + (size_t)v->slab * kChunk, kCtx * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (have) EIOKU_HIP_CHECK(hipMemcpyAsync(v->audio + kCtx, samples + a0, (size_t)have * sizeof(float), hipMemcpyHostToDevice, st));
    if (have < (long long)m * kChunk)
      EIOKU_HIP_CHECK(hipMemsetAsync(v->audio + kCtx + have, 0, (size_t)((long long)m * kChunk - have) * sizeof(float), st));
    EIOKU_TRY(v->ev.record(3 * s, st));
    hipLaunchKernelGGL(k_vad_encode, dim3((unsigned)((m + kTile - 1) / kTile)), dim3(256), 0, st, v->audio.p, m, W, v->gx.p);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY(v->ev.record(3 * s + 1, st));
    hipLaunchKernelGGL(k_vad_lstm, dim3(1), dim3(kGates), 0, st, v->gx.p, m, v->t[V_WHH].dev.p, v->t[V_WOUT].dev.p, v->t[V_BOUT].dev.p,
                       v->state.p, v->probs.p);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY(v->ev.record(3 * s + 2, st));
    // the next slab reuses audio, gx and probs: stream order keeps its copies behind this slab's kernels and read-back
    EIOKU_HIP_CHECK(hipMemcpyAsync(probs_out + first, v->probs, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  for (long long s = 0; s < n_slabs; ++s) {
    double a = 0, b = 0;
    EIOKU_TRY(v->ev.ms(3 * s, 3 * s + 1, &a));
    EIOKU_TRY(v->ev.ms(3 * s + 1, 3 * s + 2, &b));
    v->encode_ms += a;
    v->lstm_ms += b;
  }
  return EIOKU_OK;
}

int eioku_vad_last_ms(const eioku_vad* v, double* encode_ms, double* lstm_ms) {
  EIOKU_REQUIRE(v, "NULL handle");
  if (encode_ms) *encode_ms = v->encode_ms;
  if (lstm_ms) *lstm_ms = v->lstm_ms;
  return EIOKU_OK;
}

}  // extern "C"
