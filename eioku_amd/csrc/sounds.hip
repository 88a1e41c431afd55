// K29: sound tagging on gfx950 - the Audio Spectrogram Transformer (AST) on AudioSet labels (DESIGN.md "K29 sound events").
//   k_ast_fbank         K29a: one workgroup per (window, frame row): 400 samples of the [-1, 1] waveform (no 2^15 scale), frame
//                       mean removed, pre-emphasis 0.97, the symmetric Hann window, a 512-point DFT (257 bins) by cosine table,
//                       |.|^2, the 257 x bins Kaldi-scale mel matrix, log(max(., 2^-23)), (x - mean) / (2 std), all in fp64, one
//                       rounding to fp32; rows at or past the window's valid frames hold the normalised zero
//   k_ast_patches       K29b: the fp32 spectrogram [window][time][mel] cut into overlapping 16 x 16 patches, frequency-major
//                       (patch fi t + ti), as fp16 rows of 256 with element 16 df + dt = spec[ts ti + dt][fs fi + df]
//   k_gemm<., EPI_POS>  (gemm_f16.h) patch projection + bias + position rows 2 .. P + 1 into the fp32 residual stream, one
//                       launch per window (a window's patch rows start two rows into its tokens)
//   k_ast_tokens        the CLS and distillation rows: token + position 0 / 1
//   k_ln<h16>           (layernorm.h) LayerNorm, fp32 row -> fp16
//   k_attn_tiles<DenseSeq, false>  (attn_f16.h) attention over the n = P + 2 tokens of a window; a layer is attn_sublayer and
//                       mlp_sublayer of encoder.h
//   k_ast_head          K29c: one workgroup per window: the encoder's final LayerNorm on rows 0 and 1 only, their mean, the
//                       classifier's LayerNorm, dense -> logits fp32; sigmoid; top-k by logit (block_argmax_256,
//                       layernorm.h), ties to the smaller index
// Residual stream x, fp32, in the model's token order: row b n + tok, tok = cls, distillation, then the P patches.
// Precision points (tests/sounds_oracle.py, fp16=True, rounds at the same places): linear / conv weights fp16; biases,
// LayerNorm parameters, the tokens and the position table fp32; the residual stream fp32; the patch rows, LayerNorm outputs
// that feed a GEMM (the classifier's included), q / k / v, attention outputs and GELU outputs are rounded to fp16; the
// attention kernel rounds its softmax numerators exp(s - max) to fp16 for the PV MFMA.
#include "common.h"
#include "encoder.h"

#include <cmath>
#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kFrame = 400, kShift = 160, kFft = 512, kBins = kFft / 2 + 1;
constexpr int kPatch = 16, kPatchK = kPatch * kPatch;
constexpr int kMaxMel = 128, kMaxTokens = 4094, kMaxHidden = 2048, kMaxLabels = 8192;
constexpr int kPass = 64;  // windows per call (at the published dimensions: 0.6 GB of activations per 32 windows)
constexpr double kMelFloor = 1.192092955078125e-07;

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  v = wave_reduce_add(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

// ---- K29a -------------------------------------------------------------------------------------------------------------------
// plan [m][2] = (first sample, valid frames); grid (T, m); spec [m][T][bins] fp32.  mel [257][bins], window [400], costab
// [512] = cos(2 pi i / 512).  A frame row t < valid reads samples first + 160 t .. + 399 only.
__global__ __launch_bounds__(256) void k_ast_fbank(const float* __restrict__ audio, const int* __restrict__ plan, int T, int bins,
                                                   const double* __restrict__ window, const double* __restrict__ costab,
                                                   const double* __restrict__ mel, double mean, double std, float pad,
                                                   float* __restrict__ spec) {
  __shared__ double xs[kFrame];
  __shared__ double ys[kFrame];
  __shared__ double ct[kFft];
  __shared__ double pw[kBins];
  __shared__ double red[4];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float* out = spec + ((size_t)b * T + t) * bins;
  if (t >= plan[2 * b + 1]) {  // the extractor pads with zeros before it normalises
    if (tid < bins) out[tid] = pad;
    return;
  }
  const float* x = audio + (size_t)plan[2 * b] + (size_t)kShift * t;
  double part = 0.0;
  for (int i = tid; i < kFrame; i += 256) {
    const double v = (double)x[i];
    xs[i] = v;
    part += v;
  }
  for (int i = tid; i < kFft; i += 256) ct[i] = costab[i];
  __syncthreads();
  const double fmean = block_sum_256(part, red) / (double)kFrame;
  double alt = 0.0;  // this thread's share of bin 256: sum of y[i] (-1)^i
  for (int i = tid; i < kFrame; i += 256) {
    const double cur = xs[i] - fmean;
    const double e = i ? cur - 0.97 * (xs[i - 1] - fmean) : cur * (1.0 - 0.97);
    const double y = e * window[i];
    ys[i] = y;
    alt += (i & 1) ? -y : y;
  }
  __syncthreads();
  const double nyq = block_sum_256(alt, red);
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
    if (tid == 0) pw[kBins - 1] = nyq * nyq;
  }
  __syncthreads();
  if (tid < bins) {
    double e = 0.0;
    for (int i = 0; i < kBins; ++i) e += mel[(size_t)i * bins + tid] * pw[i];
    out[tid] = (float)((log(fmax(e, kMelFloor)) - mean) / (2.0 * std));
  }
}

// ---- K29b -------------------------------------------------------------------------------------------------------------------
// spec [m][T][bins] fp32 -> rows [m][F Tt][256] fp16, one thread per element
__global__ __launch_bounds__(256) void k_ast_patches(const float* __restrict__ spec, int m, int T, int bins, int fs, int ts, int Tt,
                                                     int P, h16* __restrict__ rows) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)m * P * kPatchK) return;
  const int e = (int)(i % kPatchK), df = e / kPatch, dt = e % kPatch;
  const size_t row = i / kPatchK;
  const int p = (int)(row % P), b = (int)(row / P);
  const int fi = p / Tt, ti = p % Tt;
  rows[i] = (h16)spec[((size_t)b * T + (size_t)ts * ti + dt) * bins + fs * fi + df];
}

// ---- tokens -----------------------------------------------------------------------------------------------------------------
// x[b n + 0] = cls + pos[0], x[b n + 1] = distillation + pos[1]
__global__ __launch_bounds__(256) void k_ast_tokens(const float* __restrict__ cls, const float* __restrict__ dist,
                                                    const float* __restrict__ pos, int B, int n, int d, float* __restrict__ x) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * 2 * d) return;
  const int c = (int)(i % d), tok = (int)((i / d) & 1), b = (int)(i / ((size_t)2 * d));
  x[((size_t)b * n + tok) * d + c] = (tok ? dist[c] : cls[c]) + pos[(size_t)tok * d + c];
}

// ---- K29c -------------------------------------------------------------------------------------------------------------------
// grid (windows), 4 waves.  x != NULL: rows b n and b n + 1 of the stream -> LayerNorm (final_g / final_b) each, their mean, the
// classifier's LayerNorm rounded to fp16, logits[b][j] = w[j] . h + bias[j] with fp16 weights and fp32 sums.  x == NULL: the
// logits are read.  top_k > 0: score = sigmoid(logit) (taken in fp64, rounded to fp32 once) of the top_k largest logits in
// descending order, the smaller label on a tie.  Dynamic LDS: (2 d + labels) floats.
__global__ __launch_bounds__(256) void k_ast_head(const float* __restrict__ x, int n, int d, int labels, float eps,
                                                  const float* __restrict__ final_g, const float* __restrict__ final_b,
                                                  const float* __restrict__ cls_g, const float* __restrict__ cls_b,
                                                  const h16* __restrict__ w, const float* __restrict__ bias, float* __restrict__ logits,
                                                  int top_k, float* __restrict__ score_out, int* __restrict__ id_out) {
  extern __shared__ float s_mem[];
  __shared__ float s_f[4];
  __shared__ int s_i[4];
  float* s_row = s_mem;          // [2][d]: the two normalised rows, then [0][.] the pooled row and [1][.] the head's input
  float* s_l = s_mem + 2 * d;    // [labels]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* lg = logits + (size_t)b * labels;
  if (x) {
    if (wave < 2) {
      const float* xr = x + ((size_t)b * n + wave) * d;
      const RowStats st = row_stats(lane, d, eps, [&](int i) { return xr[i]; });
      for (int i = lane; i < d; i += 64) s_row[wave * d + i] = (xr[i] - st.mean) * st.inv * final_g[i] + final_b[i];
    }
    __syncthreads();
    for (int i = tid; i < d; i += 256) s_row[i] = (s_row[i] + s_row[d + i]) / 2.f;
    __syncthreads();
    {
      const RowStats st = row_stats(lane, d, eps, [&](int i) { return s_row[i]; });  // every wave: the same values
      for (int i = tid; i < d; i += 256) s_row[d + i] = (float)(h16)((s_row[i] - st.mean) * st.inv * cls_g[i] + cls_b[i]);
    }
    __syncthreads();
    for (int j = wave; j < labels; j += 4) {
      const h16* wr = w + (size_t)j * d;
      float s = 0.f;
      for (int i = lane; i < d; i += 64) s += (float)wr[i] * s_row[d + i];
      s = wave_sum(s) + bias[j];
      if (lane == 0) lg[j] = s, s_l[j] = s;
    }
  } else {
    for (int j = tid; j < labels; j += 256) s_l[j] = lg[j];
  }
  __syncthreads();
  for (int k = 0; k < top_k; ++k) {
    Best best = block_argmax_256(s_l, labels, -INFINITY, s_f, s_i);  // taken entries are set to NaN, which compares false
    if (best.i >= labels) best.i = 0;  // only NaN logits are left
    if (tid == 0) {
      score_out[(size_t)b * top_k + k] = (float)(1.0 / (1.0 + exp(-(double)best.v)));
      id_out[(size_t)b * top_k + k] = best.i;
      s_l[best.i] = NAN;
    }
    __syncthreads();
  }
}

}  // namespace

struct eioku_ast : TensorTable {
  int bins = 0, T = 0, fs = 0, ts = 0, Ft = 0, Tt = 0, P = 0, n = 0;
  int d = 0, layers = 0, heads = 0, ffn = 0, labels = 0;
  float eps = 1e-12f, pad = 0.f;
  double mean = 0, std = 1;
  std::vector<EncLayer> L;
  int cls_token = 0, dist_token = 0, pos = 0;
  Lin proj{}, dense{};
  LNorm final_ln{}, cls_ln{};
  DevBuf<double> tables;  // window [400] | cosine [512] | mel [257][bins]
  DevBuf<float> audio;    // the file's 16 kHz samples
  long long n_audio = 0;
  // one call's buffers, grown to the most windows seen
  DevBuf<int> plan;
  DevBuf<float> spec;
  DevBuf<h16> patches;
  EncWork work;
  DevBuf<float> logits, scores;
  DevBuf<int> ids;
  StageClock<3> clock;  // features / encoder / head
  double flops = 0;
};

namespace {

typedef eioku_ast Model;

int ensure_batch(Model* m, int B) {
  EIOKU_TRY(m->work.grow((size_t)B * m->n, m->d, m->ffn));
  EIOKU_TRY(grow_synced(m->logits, (size_t)B * m->labels));
  EIOKU_TRY(grow_synced(m->scores, (size_t)B * m->labels));
  return grow_synced(m->ids, (size_t)B * m->labels);
}

int ensure_features(Model* m, int B) {
  EIOKU_TRY(grow_synced(m->plan, (size_t)B * 2));
  EIOKU_TRY(grow_synced(m->spec, (size_t)B * m->T * m->bins));
  return grow_synced(m->patches, (size_t)B * m->P * kPatchK);
}

// plan rows (first sample, valid frames) against the window length and the uploaded audio
int check_plan(const Model* m, const int* plan, int B) {
  for (int i = 0; i < B; ++i) {
    const long long first = plan[2 * i], valid = plan[2 * i + 1];
    EIOKU_REQUIRE(valid >= 1 && valid <= m->T, "window %d: %lld valid frames outside [1, %d]", i, valid, m->T);
    EIOKU_REQUIRE(first >= 0 && first + kFrame + (long long)kShift * (valid - 1) <= m->n_audio,
                  "window %d: samples [%lld, %lld) outside the audio (%lld samples)", i, first,
                  first + kFrame + (long long)kShift * (valid - 1), m->n_audio);
  }
  return EIOKU_OK;
}

// plan (HOST) -> m->spec and m->patches of B windows
int run_features(Model* m, const int* plan, int B, hipStream_t st) {
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->plan, plan, (size_t)B * 8, hipMemcpyHostToDevice, st));
  const double* tab = m->tables;
  hipLaunchKernelGGL(k_ast_fbank, dim3((unsigned)m->T, (unsigned)B), dim3(256), 0, st, m->audio.p, m->plan.p, m->T, m->bins, tab,
                     tab + kFrame, tab + kFrame + kFft, m->mean, m->std, m->pad, m->spec.p);
  EIOKU_LAUNCH_CHECK();
  const size_t e = (size_t)B * m->P * kPatchK;
  hipLaunchKernelGGL(k_ast_patches, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st, m->spec.p, B, m->T, m->bins, m->fs, m->ts, m->Tt,
                     m->P, m->patches.p);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// patches [B P][256] fp16 (device) -> the residual stream after every layer in m->work.x
int run_encoder(Model* m, const h16* patches, int B, hipStream_t st) {
  const Enc enc{m, st, m->d, m->eps, &m->flops};
  const int d = m->d, n = m->n, P = m->P;
  float* x = m->work.x;
  for (int b = 0; b < B; ++b)
    EIOKU_TRY((enc.gemm<4, EPI_POS>(patches + (size_t)b * P * kPatchK, kPatchK, m->proj, P, d, kPatchK, x + ((size_t)b * n + 2) * d, d,
                                    m->F(m->pos) + (size_t)2 * d, P)));
  hipLaunchKernelGGL(k_ast_tokens, dim3((unsigned)(((size_t)B * 2 * d + 255) / 256)), dim3(256), 0, st, m->F(m->cls_token),
                     m->F(m->dist_token), m->F(m->pos), B, n, d, x);
  EIOKU_LAUNCH_CHECK();
  for (const EncLayer& L : m->L) {
    EIOKU_TRY(attn_sublayer<false>(enc, m->work, L, B, n, m->heads));
    EIOKU_TRY(mlp_sublayer(enc, m->work, B * n, L.ln2, L.fc1, L.fc2, m->ffn, false));
  }
  return EIOKU_OK;
}

// x == NULL: selection on `logits` alone
int launch_head(Model* m, const float* x, float* logits, int B, int top_k, float* scores, int* ids, hipStream_t st) {
  const size_t lds = ((size_t)2 * m->d + m->labels) * sizeof(float);
  hipLaunchKernelGGL(k_ast_head, dim3(B), dim3(256), lds, st, x, m->n, m->d, m->labels, m->eps, m->F(m->final_ln.g), m->F(m->final_ln.b),
                     m->F(m->cls_ln.g), m->F(m->cls_ln.b), m->H(m->dense.w), m->F(m->dense.b), logits, top_k, scores, ids);
  EIOKU_LAUNCH_CHECK();
  if (x) m->flops += 2.0 * B * m->labels * m->d;
  return EIOKU_OK;
}

}  // namespace

extern "C" {

int eioku_ast_create(int num_mel_bins, int max_length, int fstride, int tstride, int hidden, int layers, int heads, int ffn, int labels,
                     float ln_eps, const double* window, const double* mel, double mean, double std, eioku_ast** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out && window && mel, "NULL argument");
  EIOKU_REQUIRE(hidden > 0 && heads > 0 && heads * 64 == hidden, "head_dim must be 64 (hidden %d / heads %d)", hidden, heads);
  EIOKU_REQUIRE(hidden <= kMaxHidden, "hidden_size must be at most %d (got %d)", kMaxHidden, hidden);
  EIOKU_REQUIRE(num_mel_bins >= kPatch && num_mel_bins <= kMaxMel, "num_mel_bins must be in [%d, %d] (got %d)", kPatch, kMaxMel,
                num_mel_bins);
  EIOKU_REQUIRE(fstride >= 1 && fstride <= kPatch, "frequency_stride must be in [1, %d] (got %d)", kPatch, fstride);
  EIOKU_REQUIRE(tstride >= 1 && tstride <= kPatch, "time_stride must be in [1, %d] (got %d)", kPatch, tstride);
  EIOKU_REQUIRE(max_length >= kPatch, "max_length must be at least %d (got %d)", kPatch, max_length);
  const long long F = (num_mel_bins - kPatch) / fstride + 1, Tt = ((long long)max_length - kPatch) / tstride + 1;
  EIOKU_REQUIRE(F * Tt + 2 <= kMaxTokens, "at most %d tokens (max_length %d and the strides give %lld)", kMaxTokens, max_length,
                F * Tt + 2);
  EIOKU_REQUIRE(labels >= 1, "num_labels must be at least 1 (got %d)", labels);
  EIOKU_REQUIRE(labels <= kMaxLabels, "num_labels must be at most %d (got %d)", kMaxLabels, labels);
  EIOKU_REQUIRE(layers >= 0 && ffn > 0 && ffn % 32 == 0 && ln_eps > 0.f && std > 0.0,
                "bad config (layers %d, ffn %d a multiple of 32, ln_eps %g, std %g)", layers, ffn, (double)ln_eps, std);
  auto* m = new eioku_ast();
  m->bins = num_mel_bins, m->T = max_length, m->fs = fstride, m->ts = tstride, m->Ft = (int)F, m->Tt = (int)Tt;
  m->P = (int)(F * Tt), m->n = m->P + 2;
  m->d = hidden, m->layers = layers, m->heads = heads, m->ffn = ffn, m->labels = labels, m->eps = ln_eps;
  m->mean = mean, m->std = std, m->pad = (float)((0.0 - mean) / (2.0 * std));
  const int d = hidden;
  const std::string a = "audio_spectrogram_transformer.", e = a + "embeddings.";
  m->cls_token = m->add(e + "cls_token", 1, d, T_F32);
  m->dist_token = m->add(e + "distillation_token", 1, d, T_F32);
  m->pos = m->add(e + "position_embeddings", m->n, d, T_F32);
  m->proj = m->lin(e + "patch_embeddings.projection", d, kPatchK);
  for (int l = 0; l < layers; ++l) {
    const std::string p = a + "layers." + std::to_string(l) + ".";
    EncLayer L;
    L.qkv.w = m->packed(p + "attention.qkv.weight", 3 * d, d, T_F16);
    L.qkv.b = m->packed(p + "attention.qkv.bias", 3 * d, 1, T_F32);
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
      m->part(p + "attention." + names[j] + ".weight", d, d, L.qkv.w, j * d);
      m->part(p + "attention." + names[j] + ".bias", d, 1, L.qkv.b, j * d);
    }
    L.out = m->lin(p + "attention.o_proj", d, d);
    L.ln1 = m->lnorm(p + "layernorm_before", d);
    L.ln2 = m->lnorm(p + "layernorm_after", d);
    L.fc1 = m->lin(p + "mlp.fc1", ffn, d);
    L.fc2 = m->lin(p + "mlp.fc2", d, ffn);
    m->L.push_back(L);
  }
  m->final_ln = m->lnorm(a + "layernorm", d);
  m->cls_ln = m->lnorm("classifier.layernorm", d);
  m->dense = m->lin("classifier.dense", labels, d);
  auto fail = [&](int rc) {
    eioku_ast_destroy(m);
    return rc;
  };
  if (const int rc = m->finish()) return fail(rc);
  std::vector<double> tab((size_t)kFrame + kFft + (size_t)kBins * num_mel_bins);
  std::copy(window, window + kFrame, tab.begin());
  for (int i = 0; i < kFft; ++i) tab[kFrame + i] = std::cos(2.0 * M_PI * (double)i / (double)kFft);
  std::copy(mel, mel + (size_t)kBins * num_mel_bins, tab.begin() + kFrame + kFft);
  if (const int rc = m->tables.upload(tab.data(), tab.size())) return fail(rc);
  if (const int rc = m->clock.create()) return fail(rc);
  *out = m;
  return EIOKU_OK;
}

void eioku_ast_destroy(eioku_ast* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  delete m;  // every buffer and event frees itself
}

int eioku_ast_num_tensors(const eioku_ast* m) { return TensorTable::count(m); }

int eioku_ast_tensor_info(const eioku_ast* m, int idx, char* name, size_t cap, int* rows, int* cols) {
  return TensorTable::info(m, idx, name, cap, rows, cols);
}

int eioku_ast_set_tensor(eioku_ast* m, int idx, const float* host, size_t numel) { return TensorTable::set(m, idx, host, numel); }

// the file's 16 kHz mono samples in [-1, 1] (host or device per mem), kept on the device until the next call.  Synchronous.
int eioku_ast_set_audio(eioku_ast* m, const float* samples, long long n, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n >= 0 && n < (1ll << 31) - kFrame, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  EIOKU_REQUIRE(n == 0 || samples, "NULL buffer");
  hipStream_t st = (hipStream_t)stream_;
  m->n_audio = 0;
  EIOKU_TRY(grow_synced(m->audio, (size_t)n));
  if (n)
    EIOKU_HIP_CHECK(hipMemcpyAsync(m->audio, samples, (size_t)n * 4, mem == EIOKU_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  m->n_audio = n;
  return EIOKU_OK;
}

// K29a and K29b alone (parity entry): plan HOST int32 [n_windows][2] = (first sample, valid frames) -> spec_out [n_windows]
// [max_length][num_mel_bins] fp32 and / or patches_out [n_windows][P][256] fp16 (device, each optional).  Synchronous.
int eioku_ast_features(eioku_ast* m, const int32_t* plan, int n_windows, float* spec_out, void* patches_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n_windows >= 0, "bad argument");
  EIOKU_REQUIRE(n_windows <= kPass, "at most %d windows per call (got %d)", kPass, n_windows);
  if (n_windows == 0) return EIOKU_OK;
  EIOKU_REQUIRE(plan, "NULL buffer");
  EIOKU_TRY(check_plan(m, plan, n_windows));
  hipStream_t st = (hipStream_t)stream_;
  EIOKU_TRY(ensure_features(m, n_windows));
  m->flops = 0;
  m->clock.begin(0b001);
  EIOKU_TRY(m->clock.mark(0, st));
  EIOKU_TRY(run_features(m, plan, n_windows, st));
  EIOKU_TRY(m->clock.mark(1, st));
  if (spec_out)
    EIOKU_HIP_CHECK(hipMemcpyAsync(spec_out, m->spec, (size_t)n_windows * m->T * m->bins * 4, hipMemcpyDeviceToDevice, st));
  if (patches_out)
    EIOKU_HIP_CHECK(hipMemcpyAsync(patches_out, m->patches, (size_t)n_windows * m->P * kPatchK * 2, hipMemcpyDeviceToDevice, st));
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

// The raw network: patches [n_windows][P][256] fp16 (device) -> logits_out [n_windows][labels] fp32 (device), and optionally
// hidden_out [n_windows][P + 2][hidden] fp32 (device): the residual stream before the final LayerNorm.  Asynchronous.
int eioku_ast_forward(eioku_ast* m, const void* patches, int n_windows, float* logits_out, float* hidden_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n_windows >= 0, "bad argument");
  EIOKU_REQUIRE(n_windows <= kPass, "at most %d windows per call (got %d)", kPass, n_windows);
  if (n_windows == 0) return EIOKU_OK;
  EIOKU_REQUIRE(patches && logits_out, "NULL buffer");
  EIOKU_TRY(m->check());
  hipStream_t st = (hipStream_t)stream_;
  EIOKU_TRY(ensure_batch(m, n_windows));
  m->flops = 0;
  m->clock.begin(0b110);
  EIOKU_TRY(m->clock.mark(1, st));
  EIOKU_TRY(run_encoder(m, (const h16*)patches, n_windows, st));
  EIOKU_TRY(m->clock.mark(2, st));
  EIOKU_TRY(launch_head(m, m->work.x, m->logits, n_windows, 0, nullptr, nullptr, st));
  EIOKU_TRY(m->clock.mark(3, st));
  EIOKU_HIP_CHECK(hipMemcpyAsync(logits_out, m->logits, (size_t)n_windows * m->labels * 4, hipMemcpyDeviceToDevice, st));
  if (hidden_out)
    EIOKU_HIP_CHECK(hipMemcpyAsync(hidden_out, m->work.x, (size_t)n_windows * m->n * m->d * 4, hipMemcpyDeviceToDevice, st));
  return EIOKU_OK;
}

// sigmoid and top_k of logits [n][labels] fp32 (device) -> score_out [n][top_k] fp32, id_out [n][top_k] int32 (device): the
// head's selection on its own (parity helper).  Asynchronous.
int eioku_ast_topk(eioku_ast* m, const float* logits, int n, int top_k, float* score_out, int32_t* id_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n >= 0 && top_k >= 1 && top_k <= m->labels, "bad argument (top_k %d of %d labels)", top_k, m ? m->labels : 0);
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(logits && score_out && id_out, "NULL buffer");
  return launch_head(m, nullptr, const_cast<float*>(logits), n, top_k, score_out, id_out, (hipStream_t)stream_);
}

// detect_sounds' per-window arithmetic on n_windows windows of the uploaded audio: fbank -> patch rows -> network -> sigmoid
// -> top_k by (logit desc, label asc) -> score_out [n_windows][top_k] fp32, id_out [n_windows][top_k] int32 (HOST when mem ==
// EIOKU_MEM_HOST, else device); logits_out and hidden_out optional ([n_windows][labels], [n_windows][P + 2][hidden], same
// side).  Host outputs synchronise the stream.
int eioku_ast_classify(eioku_ast* m, const int32_t* plan, int n_windows, int top_k, float* score_out, int32_t* id_out,
                       float* logits_out, float* hidden_out, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n_windows >= 0, "bad argument");
  EIOKU_REQUIRE(top_k >= 1 && top_k <= m->labels, "bad argument (top_k %d of %d labels)", top_k, m->labels);
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  EIOKU_REQUIRE(n_windows <= kPass, "at most %d windows per call (got %d)", kPass, n_windows);
  if (n_windows == 0) return EIOKU_OK;
  EIOKU_REQUIRE(plan && score_out && id_out, "NULL buffer");
  EIOKU_TRY(m->check());
  EIOKU_TRY(check_plan(m, plan, n_windows));
  hipStream_t st = (hipStream_t)stream_;
  EIOKU_TRY(ensure_features(m, n_windows));
  EIOKU_TRY(ensure_batch(m, n_windows));
  m->flops = 0;
  m->clock.begin(0b111);
  EIOKU_TRY(m->clock.mark(0, st));
  EIOKU_TRY(run_features(m, plan, n_windows, st));
  EIOKU_TRY(m->clock.mark(1, st));
  EIOKU_TRY(run_encoder(m, m->patches.p, n_windows, st));
  EIOKU_TRY(m->clock.mark(2, st));
  EIOKU_TRY(launch_head(m, m->work.x, m->logits, n_windows, top_k, m->scores, m->ids, st));
  EIOKU_TRY(m->clock.mark(3, st));
  const hipMemcpyKind kind = mem == EIOKU_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  EIOKU_HIP_CHECK(hipMemcpyAsync(score_out, m->scores, (size_t)n_windows * top_k * 4, kind, st));
  EIOKU_HIP_CHECK(hipMemcpyAsync(id_out, m->ids, (size_t)n_windows * top_k * 4, kind, st));
  if (logits_out) EIOKU_HIP_CHECK(hipMemcpyAsync(logits_out, m->logits, (size_t)n_windows * m->labels * 4, kind, st));
  if (hidden_out) EIOKU_HIP_CHECK(hipMemcpyAsync(hidden_out, m->work.x, (size_t)n_windows * m->n * m->d * 4, kind, st));
  if (mem == EIOKU_MEM_HOST) EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

int eioku_ast_last_flops(const eioku_ast* m, double* flops) {
  EIOKU_REQUIRE(m && flops, "NULL argument");
  *flops = m->flops;
  return EIOKU_OK;
}

// device milliseconds of the last features / forward / classify call per stage (0 for a stage that call did not run); waits
int eioku_ast_last_ms(const eioku_ast* m, double* features_ms, double* encoder_ms, double* head_ms) {
  EIOKU_REQUIRE(m && features_ms && encoder_ms && head_ms, "NULL argument");
  double* const out[3] = {features_ms, encoder_ms, head_ms};
  return m->clock.last_ms(out);
}

}  // extern "C"
