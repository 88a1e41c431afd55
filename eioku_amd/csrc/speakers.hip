// K24: speaker labels - WeSpeaker ResNet speaker embeddings per window of a transcript segment, clustered per video.
//
// Fills the "speaker" key of transcribe_video's segments (eioku_amd/speakers.py).  [PUBLIC-LIB]: the front end, the
// network and the pooling are restated from the public WeSpeaker / Kaldi sources; no checkpoint is a dependency.
//   k_spk_fbank      K24a: one workgroup per (window, frame): 400 samples x 32768, frame mean removed, pre-emphasis 0.97,
//                    Povey window, 512-point DFT from a cosine table in LDS, power spectrum, 80 Kaldi mel triangles over
//                    bins 0..255, log(max(e, FLT_EPSILON)) - all in fp64 (the DFT as K19), one value per (bin, frame)
//   k_spk_cmn        per (window, bin): mean over the valid frames in frame order (as offsets from frame 0, so that a
//                    constant row gives exactly 0), one rounding to fp32, then to fp16 -> NHWC8 [B][80][win][8], channel 0;
//                    frames at or past `valid` are 0
//   the BasicBlocks  K24b: K4's 3x3 kernels (conv.hip) with every BatchNorm folded into its conv; the 1x1 / s2 shortcut as
//                    the centre tap of a 3x3 / s2 (as resnet.hip); kActReLU / kActResReLU epilogues
//   k_spk_pool       K24c: per (channel, frequency) row the mean and sqrt(unbiased variance + 1e-7) over the window's
//                    ceil(valid / 8) valid columns, in column order, fp32 -> [B][5120] (mean | std, each f * 256 + c)
//   k_spk_head       seg_1 (5120 -> 256, fp32): a workgroup per output keeps its weight row in registers and walks the
//                    windows; each window is reduced on its own in a fixed order (bits independent of the batch)
//   k_spk_segments   K24d: mean of a segment's window vectors in window order, L2 normalised
//   k_spk_centroids / k_spk_assign   centroid of each DBSCAN label (members summed in row order, normalised); every noise
//                    row takes the nearest centroid's label if 1 - cos <= assign_max (ties: the smaller label)
// Numerics of the network: fp16 storage, fp32 accumulation (the detector's arithmetic, as K11 / K13).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "convnet.h"

using namespace eioku;

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int kFrame = 400, kShift = 160, kFft = 512, kBins = 256, kMel = 80;
constexpr int kEmb = 256, kChan = 256, kFreq = kMel / 8, kStat = 2 * kChan * kFreq;  // 5120
constexpr int kPass = 64;  // windows per network pass (activations: 4 x 1 MB per window at win = 200)

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  v = wave_reduce_add(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

__device__ __forceinline__ float block_sum_256f(float v, float* red) {
  v = wave_reduce_add(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

// ---- K24a ------------------------------------------------------------------------------------------------------------
// plan [m][2] = (first sample, valid frames); grid (win, m); logmel [m][80][win] fp64 (frames < valid written)
__global__ __launch_bounds__(256) void k_spk_fbank(const float* __restrict__ audio, const int* __restrict__ plan, int win,
                                                   const double* __restrict__ window, const double* __restrict__ costab,
                                                   const double* __restrict__ mel, const int* __restrict__ mel_range,
                                                   double* __restrict__ logmel) {
  __shared__ double xs[kFrame];
  __shared__ double ys[kFrame];
  __shared__ double ct[kFft];
  __shared__ double pw[kBins];
  __shared__ double red[4];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (t >= plan[2 * b + 1]) return;
  const float* x = audio + (size_t)plan[2 * b] + (size_t)kShift * t;
  double part = 0.0;
  for (int i = tid; i < kFrame; i += 256) {
    const double v = (double)x[i] * 32768.0;
    xs[i] = v;
    part += v;
  }
  for (int i = tid; i < kFft; i += 256) ct[i] = costab[i];
  __syncthreads();
  const double mean = block_sum_256(part, red) / (double)kFrame;
  for (int i = tid; i < kFrame; i += 256) {
    const double cur = xs[i] - mean, prev = xs[i ? i - 1 : 0] - mean;
    ys[i] = (cur - 0.97 * prev) * window[i];
  }
  __syncthreads();
  {
    double re = 0.0, im = 0.0;
    unsigned idx = 0;
    for (int n = 0; n < kFrame; ++n) {
      const double y = ys[n];
      re += y * ct[idx & (kFft - 1)];
      im += y * ct[(idx + 3 * kFft / 4) & (kFft - 1)];  // sin(a) = cos(a - pi / 2)
      idx += (unsigned)tid;
    }
    pw[tid] = re * re + im * im;
  }
  __syncthreads();
  if (tid < kMel) {
    const int lo = mel_range[2 * tid], hi = mel_range[2 * tid + 1];
    double e = 0.0;
    for (int i = lo; i < hi; ++i) e += mel[tid * kBins + i] * pw[i];
    logmel[((size_t)b * kMel + tid) * win + t] = log(fmax(e, (double)1.1920929e-07f));
  }
}

// one thread per (window, bin): CMN over the valid frames -> f32 [m][80][win] (optional) and fp16 [m][80][win][8]
__global__ __launch_bounds__(256) void k_spk_cmn(const double* __restrict__ logmel, const int* __restrict__ plan, int m, int win,
                                                 float* __restrict__ f32, __half* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m * kMel) return;
  const int valid = plan[2 * (i / kMel) + 1];
  const double* r = logmel + (size_t)i * win;
  const double x0 = r[0];
  double s = 0.0;
  for (int t = 0; t < valid; ++t) s += r[t] - x0;
  const double mean = x0 + s / (double)valid;
  for (int t = 0; t < win; ++t) {
    const float v = t < valid ? (float)(r[t] - mean) : 0.f;
    if (f32) f32[(size_t)i * win + t] = v;
    half8 h = {};
    h[0] = (_Float16)v;
    *reinterpret_cast<uint4*>(out + ((size_t)i * win + t) * 8) = __builtin_bit_cast(uint4, h);
  }
}

// ---- K24c ------------------------------------------------------------------------------------------------------------
// x [m][10][Wf][256] fp16; grid (10, m), thread = channel; stats [m][5120]
__global__ __launch_bounds__(256) void k_spk_pool(const __half* __restrict__ x, const int* __restrict__ valid, int Wf,
                                                  float* __restrict__ stats) {
  const int f = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
  const int T = (valid[b] + 7) / 8;
  const __half* p = x + (((size_t)b * kFreq + f) * Wf) * kChan + c;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += __half2float(p[(size_t)t * kChan]);
  const float mean = s / (float)T;
  float q = 0.f;
  for (int t = 0; t < T; ++t) {
    const float d = __half2float(p[(size_t)t * kChan]) - mean;
    q += d * d;
  }
  float* o = stats + (size_t)b * kStat + f * kChan + c;
  o[0] = mean;
  o[kStat / 2] = sqrtf(q / (float)(T - 1) + 1e-7f);
}

// grid 256 (outputs), 256 threads: thread holds columns tid + 256 j of its output's weight row
__global__ __launch_bounds__(256) void k_spk_head(const float* __restrict__ stats, int m, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ float red[4];
  const int o = blockIdx.x, tid = threadIdx.x;
  float wr[kStat / 256];
#pragma unroll
  for (int j = 0; j < kStat / 256; ++j) wr[j] = w[(size_t)o * kStat + tid + 256 * j];
  const float bo = bias[o];
  for (int b = 0; b < m; ++b) {
    const float* s = stats + (size_t)b * kStat + tid;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < kStat / 256; ++j) a += wr[j] * s[256 * j];
    a = block_sum_256f(a, red);
    if (tid == 0) out[(size_t)b * kEmb + o] = a + bo;
  }
}

// ---- K24d ------------------------------------------------------------------------------------------------------------
// seg_first [n_seg + 1]: segment i owns window rows seg_first[i] .. seg_first[i + 1] - 1 (at least one)
__global__ __launch_bounds__(256) void k_spk_segments(const float* __restrict__ wv, const int* __restrict__ seg_first,
                                                      float* __restrict__ out) {
  __shared__ float red[4];
  const int i = blockIdx.x, d = threadIdx.x;
  const int lo = seg_first[i], hi = seg_first[i + 1];
  float s = 0.f;
  for (int r = lo; r < hi; ++r) s += wv[(size_t)r * kEmb + d];
  const float v = s / (float)(hi - lo);
  const float nrm = fmaxf(sqrtf(block_sum_256f(v * v, red)), 1e-12f);
  out[(size_t)i * kEmb + d] = v / nrm;
}

// a workgroup per label: the normalised sum of its rows in row order
__global__ __launch_bounds__(256) void k_spk_centroids(const float* __restrict__ e, int n, const int* __restrict__ labels,
                                                       float* __restrict__ cent) {
  __shared__ float red[4];
  const int k = blockIdx.x, d = threadIdx.x;
  float s = 0.f;
  for (int i = 0; i < n; ++i)
    if (labels[i] == k) s += e[(size_t)i * kEmb + d];
  const float nrm = fmaxf(sqrtf(block_sum_256f(s * s, red)), 1e-12f);
  cent[(size_t)k * kEmb + d] = s / nrm;
}

// a wave per row: lane l holds dimensions 4 l .. 4 l + 3
__global__ __launch_bounds__(256) void k_spk_assign(const float* __restrict__ e, int n, const int* __restrict__ labels,
                                                    const float* __restrict__ cent, int k, float assign_max,
                                                    int* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  int lab = labels[row];
  if (lab < 0) {
    const float4 v = *reinterpret_cast<const float4*>(e + (size_t)row * kEmb + 4 * lane);
    float best = INFINITY;
    for (int j = 0; j < k; ++j) {
      const float4 c = *reinterpret_cast<const float4*>(cent + (size_t)j * kEmb + 4 * lane);
      float dot = (v.x * c.x + v.y * c.y) + (v.z * c.z + v.w * c.w);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
      const float dist = 1.0f - dot;
      if (dist < best) {
        best = dist;
        lab = j;
      }
    }
    if (!(best <= assign_max)) lab = -1;
  }
  if (lane == 0) out[row] = lab;
}

struct Block {
  int conv1, conv2, down;  // layer indices (down = -1: identity shortcut)
  int cin, cout, stride;
};

}  // namespace

struct eioku_spk {
  int depths[4] = {};
  int win = 0;
  ConvStack convs;
  std::vector<Block> blocks;
  DevBuf<float> seg_w;         // [256][5120] fp32, device column order
  DevBuf<float> seg_b;
  bool seg_set = false;
  DevBuf<double> tables;       // window [400] | cosine [512] | mel [80][256]
  DevBuf<int> mel_range;       // [80][2]
  DevBuf<float> audio;         // the video's 16 kHz samples
  long long n_audio = 0;
  // pass buffers, grown to the most windows seen in one pass
  DevBuf<double> logmel;       // [m][80][win]
  DevBuf<__half> in16;         // [m][80][win][8]
  DevBuf<__half> buf[4];       // [m][80][win][32] each
  DevBuf<float> stats;         // [m][5120]
  DevBuf<int> plan;            // [cap][2] | valid [cap], cap = plan.cap / 3 windows
  int* valid() const { return plan.p + plan.cap / 3 * 2; }
  DevEvents ev;                // 4: around features, network, pooling + head of one pass
  double ms[3] = {};           // features, network, pooling + head of the last embed
};

namespace {

int ensure_cap(eioku_spk* s, int m) {
  const size_t px = (size_t)m * kMel * s->win;
  EIOKU_TRY(s->logmel.grow(px));
  EIOKU_TRY(s->in16.grow(px * 8));
  for (auto& b : s->buf) EIOKU_TRY(b.grow(px * 32));
  EIOKU_TRY(s->stats.grow((size_t)m * kStat));
  return s->plan.grow((size_t)m * 3);
}

// plan rows (first sample, valid) against the window length and the uploaded audio
int check_plan(const eioku_spk* s, const int* plan, int m) {
  for (int i = 0; i < m; ++i) {
    const long long first = plan[2 * i], valid = plan[2 * i + 1];
    EIOKU_REQUIRE(valid >= 1 && valid <= s->win, "window %d: %lld valid frames outside [1, %d]", i, valid, s->win);
    EIOKU_REQUIRE(first >= 0 && first + kFrame + (long long)kShift * (valid - 1) <= s->n_audio,
                  "window %d: samples [%lld, %lld) outside the audio (%lld samples)", i, first,
                  first + kFrame + (long long)kShift * (valid - 1), s->n_audio);
  }
  return EIOKU_OK;
}

// features of mc windows (device plan rows d_plan) -> s->in16 (and f32 when given)
int run_features(eioku_spk* s, const int* d_plan, int mc, float* f32, __half* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_spk_fbank, dim3((unsigned)s->win, (unsigned)mc), dim3(256), 0, stream, s->audio.p, d_plan, s->win, s->tables.p,
                     s->tables + kFrame, s->tables + kFrame + kFft, s->mel_range.p, s->logmel.p);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_spk_cmn, dim3((unsigned)((mc * kMel + 255) / 256)), dim3(256), 0, stream, s->logmel.p, d_plan, mc, s->win, f32,
                     out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// the network on s->in16 ([m][80][win][8]); upto_block >= 0: stop after that block and copy its output to act_out;
// otherwise buf[*x_out] holds the last map [m][10][win / 8][256]
int run_network(eioku_spk* s, int m, int upto_block, void* act_out, int* x_out, hipStream_t stream) {
  EIOKU_TRY(s->convs.all_set());
  const auto& cw = s->convs.w;
  int H = kMel, W = s->win;
  EIOKU_TRY(conv_forward(cw[0], Slice{s->in16, 8, 0}, m, H, W, Slice{s->buf[0], 32, 0}, nullptr, Slice{}, kActReLU, stream));
  int x = 0;
  for (size_t bi = 0; bi < s->blocks.size(); ++bi) {
    const Block& b = s->blocks[bi];
    EIOKU_TRY(basic_block(cw[b.conv1], cw[b.conv2], b.down >= 0 ? &cw[b.down] : nullptr, s->buf, &x, m, &H, &W, stream));
    if ((int)bi == upto_block) {
      EIOKU_HIP_CHECK(hipMemcpyAsync(act_out, s->buf[x], (size_t)m * H * W * b.cout * 2, hipMemcpyDeviceToDevice, stream));
      return EIOKU_OK;
    }
  }
  *x_out = x;
  return EIOKU_OK;
}

int run_pool_head(eioku_spk* s, int m, int x, const int* d_valid, float* emb_out, hipStream_t stream) {
  EIOKU_REQUIRE(s->seg_set, "seg_1 has no weights");
  hipLaunchKernelGGL(k_spk_pool, dim3(kFreq, (unsigned)m), dim3(256), 0, stream, s->buf[x].p, d_valid, s->win / 8, s->stats.p);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_spk_head, dim3(kEmb), dim3(256), 0, stream, s->stats.p, m, s->seg_w.p, s->seg_b.p, emb_out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // namespace

extern "C" {

// depths: BasicBlocks per stage (r18 [2,2,2,2], r34 [3,4,6,3]); win_frames: frames per window (a multiple of 8, >= 16);
// window HOST fp64 [400] (Povey), mel HOST fp64 [80][256] (Kaldi triangles over FFT bins 0..255)
int eioku_spk_create(const int* depths, int win_frames, const double* window, const double* mel, eioku_spk_t** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out && depths && window && mel, "NULL argument");
  EIOKU_REQUIRE(win_frames >= 16 && win_frames % 8 == 0 && win_frames <= 4096, "win_frames = %d must be a multiple of 8 in [16, 4096]",
                win_frames);
  for (int st = 0; st < 4; ++st) EIOKU_REQUIRE(depths[st] >= 1 && depths[st] <= 64, "stage %d depth %d outside [1, 64]", st + 1, depths[st]);
  auto* s = new eioku_spk();
  s->win = win_frames;
  ConvStack& cs = s->convs;
  cs.add({"conv1", 32, 1, 3, 1});
  const int widths[4] = {32, 64, 128, 256};
  int inplanes = 32;
  for (int st = 0; st < 4; ++st) {
    s->depths[st] = depths[st];
    const int planes = widths[st];
    for (int b = 0; b < depths[st]; ++b) {
      const std::string p = "layer" + std::to_string(st + 1) + "." + std::to_string(b);
      const int cin = b == 0 ? inplanes : planes, stride = b == 0 && st > 0 ? 2 : 1;
      Block blk{cs.size(), cs.size() + 1, -1, cin, planes, stride};
      cs.add({p + ".conv1", planes, cin, 3, stride});
      cs.add({p + ".conv2", planes, planes, 3, 1});
      if (stride != 1 || cin != planes) blk.down = cs.add({p + ".shortcut.0", planes, cin, 1, stride});
      s->blocks.push_back(blk);
    }
    inplanes = planes;
  }
  std::vector<double> tab((size_t)kFrame + kFft + (size_t)kMel * kBins);
  std::copy(window, window + kFrame, tab.begin());
  for (int i = 0; i < kFft; ++i) tab[kFrame + i] = std::cos(2.0 * M_PI * (double)i / (double)kFft);
  std::copy(mel, mel + (size_t)kMel * kBins, tab.begin() + kFrame + kFft);
  std::vector<int> range(2 * kMel);
  for (int j = 0; j < kMel; ++j) {
    int lo = kBins, hi = 0;
    for (int i = 0; i < kBins; ++i)
      if (mel[(size_t)j * kBins + i] != 0.0) {
        lo = std::min(lo, i);
        hi = i + 1;
      }
    range[2 * j] = std::min(lo, hi);
    range[2 * j + 1] = hi;
  }
  int rc = s->tables.upload(tab.data(), tab.size());
  if (!rc) rc = s->mel_range.upload(range.data(), range.size());
  if (!rc) rc = s->ev.ensure(4);
  if (rc) {
    eioku_spk_destroy(s);
    return rc;
  }
  *out = s;
  return EIOKU_OK;
}

void eioku_spk_destroy(eioku_spk_t* s) {
  if (!s) return;
  (void)hipDeviceSynchronize();
  delete s;
}

int eioku_spk_num_convs(const eioku_spk_t* s) { return s ? s->convs.size() : 0; }

int eioku_spk_conv_info(const eioku_spk_t* s, int idx, char* name, size_t cap, int* cout, int* cin, int* ksize, int* stride) {
  EIOKU_REQUIRE(s, "bad convolution index %d", idx);
  return s->convs.info(idx, name, cap, cout, cin, ksize, stride);
}

// weight HOST fp32 [cout][cin][k][k] with the following BatchNorm folded in, bias HOST fp32 [cout]
int eioku_spk_set_conv(eioku_spk_t* s, int idx, const float* w, const float* b) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(s && idx >= 0 && idx < s->convs.size() && w && b, "bad argument");
  const ConvLayer& l = s->convs.layers[idx];
  ConvWeights* cw = &s->convs.w[idx];
  // the stem reads the features' 8 channels; a 1x1 shortcut runs as a 3x3 of its stride with the weights on the centre tap
  return s->convs.mark(idx, idx == 0   ? conv_weights_create_cin8(cw, l.cout, l.cin, l.k, l.stride, w, b)
                            : l.k == 1 ? conv_weights_create_centre(cw, l.cout, l.cin, l.stride, w, b)
                                       : conv_weights_create(cw, l.cout, l.cin, l.k, l.stride, w, b));
}

// seg_1: weight HOST fp32 [256][5120], columns in the device's order (mean | std, each f * 256 + c), bias HOST fp32 [256]
int eioku_spk_set_head(eioku_spk_t* s, const float* w, const float* b) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(s && w && b, "bad argument");
  EIOKU_TRY(s->seg_w.upload(w, (size_t)kEmb * kStat));
  EIOKU_TRY(s->seg_b.upload(b, kEmb));
  s->seg_set = true;
  return EIOKU_OK;
}

// the video's 16 kHz mono samples (host or device per mem), kept on the device until the next call.  Synchronous.
int eioku_spk_set_audio(eioku_spk_t* s, const float* samples, long long n, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(s && n >= 0 && n < (1ll << 31) - kFrame, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  EIOKU_REQUIRE(n == 0 || samples, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  s->n_audio = 0;
  EIOKU_TRY(s->audio.grow((size_t)n));
  if (n)
    EIOKU_HIP_CHECK(hipMemcpyAsync(s->audio, samples, (size_t)n * 4, mem == EIOKU_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                                   stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  s->n_audio = n;
  return EIOKU_OK;
}

// K24a alone (parity helper): plan HOST int32 [m][2] = (first sample, valid frames), m <= 64 -> out_f16 [m][80][win][8]
// fp16 and (optional) out_f32 [m][80][win] fp32 before the rounding, both device.  Synchronous.
int eioku_spk_features(eioku_spk_t* s, const int* plan, int m, void* out_f16, float* out_f32, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(s && m >= 0 && m <= kPass, "at most %d windows per call", kPass);
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(plan && out_f16, "NULL buffer");
  int rc = check_plan(s, plan, m);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  rc = ensure_cap(s, m);
  if (rc) return rc;
  EIOKU_HIP_CHECK(hipMemcpyAsync(s->plan, plan, (size_t)m * 8, hipMemcpyHostToDevice, stream));
  rc = run_features(s, s->plan, m, out_f32, (__half*)out_f16, stream);
  if (rc) return rc;
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// The raw network on features in_f16 [m][80][win][8] (device), valid HOST int32 [m] (frames, in [1, win]), m <= 64.
// upto_block >= 0: that block's NHWC fp16 output -> act_out (device).  Otherwise stats_out [m][5120] (optional) and
// emb_out [m][256] fp32 (device): the unnormalised window vectors.  Synchronous.
int eioku_spk_forward(eioku_spk_t* s, const void* in_f16, const int* valid, int m, int upto_block, void* act_out, float* stats_out,
                      float* emb_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(s && m >= 0 && upto_block < (int)s->blocks.size(), "bad argument");
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(m <= kPass, "at most %d windows per forward", kPass);
  EIOKU_REQUIRE(in_f16 && (upto_block >= 0 ? act_out != nullptr : (emb_out != nullptr && valid != nullptr)), "NULL buffer");
  if (upto_block < 0)
    for (int i = 0; i < m; ++i)
      EIOKU_REQUIRE(valid[i] >= 9 && valid[i] <= s->win, "window %d: %d valid frames outside [9, %d]", i, valid[i], s->win);
  hipStream_t stream = (hipStream_t)stream_;
  int rc = ensure_cap(s, m);
  if (rc) return rc;
  EIOKU_HIP_CHECK(hipMemcpyAsync(s->in16, in_f16, (size_t)m * kMel * s->win * 8 * 2, hipMemcpyDeviceToDevice, stream));
  int x = 0;
  rc = run_network(s, m, upto_block, act_out, &x, stream);
  if (rc) return rc;
  if (upto_block < 0) {
    int* d_valid = s->valid();
    EIOKU_HIP_CHECK(hipMemcpyAsync(d_valid, valid, (size_t)m * 4, hipMemcpyHostToDevice, stream));
    rc = run_pool_head(s, m, x, d_valid, emb_out, stream);
    if (rc) return rc;
    if (stats_out) EIOKU_HIP_CHECK(hipMemcpyAsync(stats_out, s->stats, (size_t)m * kStat * 4, hipMemcpyDeviceToDevice, stream));
  }
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// Features + network + pooling + seg_1 for m windows of the uploaded audio (plan HOST int32 [m][2], valid >= 9), in passes
// of 64 -> emb_out [m][256] fp32 (device).  Synchronous.
int eioku_spk_embed(eioku_spk_t* s, const int* plan, int m, float* emb_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(s && m >= 0, "bad argument");
  s->ms[0] = s->ms[1] = s->ms[2] = 0;
  if (m == 0) return EIOKU_OK;
  EIOKU_REQUIRE(plan && emb_out, "NULL buffer");
  int rc = check_plan(s, plan, m);
  if (rc) return rc;
  for (int i = 0; i < m; ++i) EIOKU_REQUIRE(plan[2 * i + 1] >= 9, "window %d: %d valid frames, fewer than 9", i, plan[2 * i + 1]);
  hipStream_t stream = (hipStream_t)stream_;
  rc = ensure_cap(s, std::min(m, kPass));
  if (rc) return rc;
  std::vector<int> pv((size_t)3 * kPass);
  for (int c0 = 0; c0 < m; c0 += kPass) {
    const int mc = std::min(kPass, m - c0);
    std::copy(plan + 2 * (size_t)c0, plan + 2 * (size_t)(c0 + mc), pv.begin());
    for (int i = 0; i < mc; ++i) pv[2 * (size_t)kPass + i] = plan[2 * (size_t)(c0 + i) + 1];
    EIOKU_HIP_CHECK(hipMemcpyAsync(s->plan, pv.data(), (size_t)mc * 8, hipMemcpyHostToDevice, stream));
    EIOKU_HIP_CHECK(hipMemcpyAsync(s->valid(), pv.data() + 2 * (size_t)kPass, (size_t)mc * 4, hipMemcpyHostToDevice,
                                   stream));
    EIOKU_TRY(s->ev.record(0, stream));
    rc = run_features(s, s->plan, mc, nullptr, s->in16, stream);
    if (rc) return rc;
    EIOKU_TRY(s->ev.record(1, stream));
    int x = 0;
    rc = run_network(s, mc, -1, nullptr, &x, stream);
    if (rc) return rc;
    EIOKU_TRY(s->ev.record(2, stream));
    rc = run_pool_head(s, mc, x, s->valid(), emb_out + (size_t)c0 * kEmb, stream);
    if (rc) return rc;
    EIOKU_TRY(s->ev.record(3, stream));
    EIOKU_HIP_CHECK(hipStreamSynchronize(stream));  // pv and the plan buffer are reused by the next pass
    for (int k = 0; k < 3; ++k) {
      double t = 0.0;
      EIOKU_TRY(s->ev.ms(k, k + 1, &t));
      s->ms[k] += t;
    }
  }
  return EIOKU_OK;
}

// device milliseconds of the last eioku_spk_embed: features, network, pooling + seg_1
int eioku_spk_last_ms(const eioku_spk_t* s, double* features_ms, double* network_ms, double* head_ms) {
  EIOKU_REQUIRE(s && features_ms && network_ms && head_ms, "NULL argument");
  *features_ms = s->ms[0];
  *network_ms = s->ms[1];
  *head_ms = s->ms[2];
  return EIOKU_OK;
}

// window vectors win_emb [rows][256] fp32 (device), seg_first HOST int32 [n_seg + 1] (ascending, every segment at least one
// row) -> out [n_seg][256] fp32 unit vectors (device).  Synchronous.
int eioku_spk_segments(const float* win_emb, const int* seg_first, int n_seg, float* out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(n_seg >= 0, "bad argument");
  if (n_seg == 0) return EIOKU_OK;
  EIOKU_REQUIRE(win_emb && seg_first && out, "NULL buffer");
  EIOKU_REQUIRE(seg_first[0] == 0, "seg_first must start at 0");
  for (int i = 0; i < n_seg; ++i) EIOKU_REQUIRE(seg_first[i + 1] > seg_first[i], "segment %d has no window", i);
  hipStream_t stream = (hipStream_t)stream_;
  int* d = (int*)scratch(kSlotWork0, (size_t)(n_seg + 1) * 4);
  if (!d) return EIOKU_EHIP;
  EIOKU_HIP_CHECK(hipMemcpyAsync(d, seg_first, (size_t)(n_seg + 1) * 4, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_spk_segments, dim3((unsigned)n_seg), dim3(256), 0, stream, win_emb, d, out);
  EIOKU_LAUNCH_CHECK();
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// emb [n][256] fp32 unit rows and DBSCAN labels [n] int32 (both device; labels -1 or 0 .. k - 1) -> labels_out [n] int32
// (device; may alias labels): noise rows take the label of the nearest centroid when 1 - cos <= assign_max, ties to the
// smaller label.  centroids_out (optional, device) [k][256]; *n_labels = k.  Synchronous.
int eioku_spk_assign(const float* emb, int n, const int32_t* labels, float assign_max, int32_t* labels_out, float* centroids_out,
                     int* n_labels, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(n >= 0 && n <= 65536, "n = %d outside [0, 65536]", n);
  EIOKU_REQUIRE(assign_max >= 0.f && assign_max <= 2.f, "assign_max = %g outside [0, 2]", (double)assign_max);
  if (n_labels) *n_labels = 0;
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(emb && labels && labels_out, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<int32_t> h((size_t)n);
  EIOKU_HIP_CHECK(hipMemcpyAsync(h.data(), labels, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  int k = 0;
  for (int i = 0; i < n; ++i) {
    EIOKU_REQUIRE(h[i] >= -1 && h[i] < n, "label %d of row %d outside [-1, %d)", h[i], i, n);
    k = std::max(k, h[i] + 1);
  }
  if (n_labels) *n_labels = k;
  float* cent = nullptr;
  if (k) {
    cent = (float*)scratch(kSlotWork1, (size_t)k * kEmb * 4);
    if (!cent) return EIOKU_EHIP;
    hipLaunchKernelGGL(k_spk_centroids, dim3((unsigned)k), dim3(256), 0, stream, emb, n, labels, cent);
    EIOKU_LAUNCH_CHECK();
    if (centroids_out) EIOKU_HIP_CHECK(hipMemcpyAsync(centroids_out, cent, (size_t)k * kEmb * 4, hipMemcpyDeviceToDevice, stream));
  }
  hipLaunchKernelGGL(k_spk_assign, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, emb, n, labels, cent, k, assign_max, labels_out);
  EIOKU_LAUNCH_CHECK();
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

}  // extern "C"
