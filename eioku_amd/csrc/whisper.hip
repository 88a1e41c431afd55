// K19 / K20 / K21: Whisper transcription on gfx950 (DESIGN.md "K19 / K20").
//   K19  k_mel_frames / k_mel_max / k_mel_finish   log-mel spectrogram, DFT and mel product in fp64
//   K20  k_gemm         (gemm_f16.h, shared with actions.hip) C = A . W^T on v_mfma_f32_16x16x32_f16: 16 weight rows per wave against MT tiles of 16 activation
//                       rows.  MT = 4 for the encoder (M = B * ctx), MT = 1 for the decoder step (M = B <= 16: every
//                       weight element is read once and used once per lane: a weight-streaming GEMM)
//        k_attn         softmax(q k^T / 8) v for head dimension 64 and any number of keys (encoder self-attention over ctx
//                       keys, decoder self-attention against the KV cache, cross-attention), scores in LDS, fp32
//        k_logits       logits against the tied embedding, the logit rules, and per-workgroup partials (max / argmax over
//                       text and timestamp ids, log-sum-exp over all and over timestamp ids); the vocab-wide logits are
//                       written only for the debug entry points
//        k_select       combines the partials, applies the timestamp-mass rule, picks the token, updates the lane state
//   K20b k_logits<., true> / k_beam_select   beam search: per-block top W + 1 text and timestamp ids next to the partials,
//                       then per window the per-beam merge, the cross-beam walk, and the permuted lane state, ancestry
//                       table, token history and finished records (DESIGN.md "K20b beam search")
//   K20c k_logits<., false, true> / k_sample_select   sampling at a temperature: Gumbel-max scores with counter-based noise
//                       computed next to the mask, per-block best score per class in the partials
//        k_embed_seq / k_attn<2, false, true> / k_kv_to_cache / k_gather_rows   the one-pass prompt prefill: all prompt
//                       positions through the M-tiled GEMMs and causal attention, keys / values into the cache layout
//                       (DESIGN.md "K20c sampling and prompt prefill")
//   K21  k_attn_weights / k_align_stats / k_align_cost / k_dtw / k_align_logits / k_align_prob   word alignment: the
//                       cross-attention probabilities of the alignment heads from one teacher-forced prefill pass, their
//                       z-scores, median filter and head mean as a cost, dynamic time warping on an anti-diagonal wavefront
//                       with a 2-bit trace, and the forced-token probabilities (DESIGN.md "K21 word alignment")
// Precision points (tests/whisper_oracle.py, fp16=True, rounds at the same places): weights of every linear / conv layer
// and the token embedding are fp16; biases, LayerNorm parameters and both position tables fp32; the residual stream is
// fp32; LayerNorm outputs, q / k / v, attention outputs, GELU outputs and the mel input are rounded to fp16.
#include "common.h"
#include "gemm_f16.h"
#include "layernorm.h"
#include "tensors.h"

#include <hip/hip_fp16.h>

#include <cmath>
#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kNfft = 400, kHop = 160, kBins = 201, kPad = 200;
constexpr float kNegInf = -INFINITY;

// ---- K19 ---------------------------------------------------------------------------------------------------------------
// grid (T, B), 256 threads.  Frame t of window b: the window's chunk is samples[off .. off + T * hop) (zeros past the end
// of the audio), reflect-padded by 200; x[n] = chunk[t * hop + n - 200] * hann[n].  Threads k < 201 compute the DFT bin k
// with the twiddles tw[(k n) mod 400]; threads m < n_mels the mel row m.  out: log10(max(mel, 1e-10)) [B][n_mels][T] fp64.
__global__ __launch_bounds__(256) void k_mel_frames(const float* __restrict__ samples, long long n_samples,
                                                    const long long* __restrict__ offsets, int T, int n_mels,
                                                    const double* __restrict__ hann, const double* __restrict__ tw_cos,
                                                    const double* __restrict__ tw_sin, const double* __restrict__ filt,
                                                    double* __restrict__ out) {
  __shared__ double x[kNfft];
  __shared__ double pw[kBins];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long long off = offsets[b];
  const long long N = (long long)T * kHop;
  for (int n = tid; n < kNfft; n += 256) {
    long long i = (long long)t * kHop + n - kPad;
    if (i < 0) i = -i;
    if (i >= N) i = 2 * (N - 1) - i;
    const long long g = off + i;
    const double s = (g >= 0 && g < n_samples) ? (double)samples[g] : 0.0;
    x[n] = s * hann[n];
  }
  __syncthreads();
  if (tid < kBins) {
    double re = 0.0, im = 0.0;
    int idx = 0;
    for (int n = 0; n < kNfft; ++n) {
      re += x[n] * tw_cos[idx];
      im -= x[n] * tw_sin[idx];
      idx += tid;
      if (idx >= kNfft) idx -= kNfft;
    }
    pw[tid] = re * re + im * im;
  }
  __syncthreads();
  for (int m = tid; m < n_mels; m += 256) {
    double a = 0.0;
    const double* f = filt + (size_t)m * kBins;
    for (int k = 0; k < kBins; ++k) a += f[k] * pw[k];
    out[((size_t)b * n_mels + m) * T + t] = log10(fmax(a, 1e-10));
  }
}

__global__ __launch_bounds__(256) void k_mel_max(const double* __restrict__ v, long long per_window, double* __restrict__ mx) {
  __shared__ double red[256];
  const double* p = v + (size_t)blockIdx.x * per_window;
  double m = -INFINITY;
  for (long long i = threadIdx.x; i < per_window; i += 256) m = fmax(m, p[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) mx[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_mel_finish(const double* __restrict__ v, long long per_window, const double* __restrict__ mx,
                                                    long long total, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double floor_ = mx[i / per_window] - 8.0;
  out[i] = (float)((fmax(v[i], floor_) + 4.0) / 4.0);
}

// ---- im2col for the two k3 p1 convolutions ------------------------------------------------------------------------------
// mel [B][C][Tin] fp32 -> col [B * Tin][ldk] fp16, col[(b, t)][tap * C + c] = mel[b][c][t + tap - 1]
__global__ __launch_bounds__(256) void k_im2col_mel(const float* __restrict__ mel, int B, int C, int Tin, int ldk, h16* __restrict__ col) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * Tin * ldk) return;
  const int k = (int)(i % ldk);
  const size_t row = i / ldk;
  const int t = (int)(row % Tin), b = (int)(row / Tin);
  float v = 0.f;
  if (k < 3 * C) {
    const int tap = k / C, c = k % C, ts = t + tap - 1;
    if (ts >= 0 && ts < Tin) v = mel[((size_t)b * C + c) * Tin + ts];
  }
  col[i] = (h16)v;
}

// h [B][Tin][C] fp16 -> col [B * Tout][3 C], col[(b, t)][tap * C + c] = h[b][2 t + tap - 1][c]  (stride 2, Tout = Tin / 2)
__global__ __launch_bounds__(256) void k_im2col_s2(const h16* __restrict__ h, int B, int C, int Tin, h16* __restrict__ col) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int Tout = Tin / 2, K = 3 * C;
  if (i >= (size_t)B * Tout * K) return;
  const int k = (int)(i % K);
  const size_t row = i / K;
  const int t = (int)(row % Tout), b = (int)(row / Tout);
  const int tap = k / C, c = k % C, ts = 2 * t + tap - 1;
  col[i] = (ts >= 0 && ts < Tin) ? h[((size_t)b * Tin + ts) * C + c] : (h16)0.f;
}

// decoder input: x[b] = embed[token][:] + pos[s][:].  token = toks ? toks[b * tstride] : uniform
__global__ __launch_bounds__(256) void k_embed(const int* __restrict__ toks, int tstride, int uniform, int vocab, int d, int s,
                                               const h16* __restrict__ emb, const float* __restrict__ pos, float* __restrict__ x) {
  const int b = blockIdx.x;
  int tok = toks ? toks[(size_t)b * tstride] : uniform;
  tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
  for (int i = threadIdx.x; i < d; i += 256) x[(size_t)b * d + i] = (float)emb[(size_t)tok * d + i] + pos[(size_t)s * d + i];
}

// ---- attention ----------------------------------------------------------------------------------------------------------
// grid (ceil(n_q / (4 QPW)), heads, B), 4 waves, each wave QPW query rows against all n_keys keys of its head.  Pass 1: lane
// j takes keys j, j + 64, ...: score = (q . k) / 8 into LDS, running max.  Pass 2: exp and sum.  Pass 3: lane = output
// dimension, o = sum_j p_j v[j][lane] (a 128-byte row per key).  Dynamic LDS: 4 QPW (n_keys + 64) floats.
// Query batch b reads the keys of batch b / kv_div (beam search: the W lanes of a window share its cross-attention K / V).
// ANC: key j of batch b is row j of batch anc[b * anc_ld + j] (beam search: the lane whose step j is in b's history).
// kvmap (may be NULL): query batch b reads the keys of batch kvmap[b] instead (prompted decode: the row -> window map).
// CAUSAL (prompt prefill, n_keys == n_q): query qi sees keys 0 .. qi; a wave's loops end at its last query's key, and a
// wave with no query runs none.
template <int QPW, bool ANC = false, bool CAUSAL = false>
__global__ __launch_bounds__(256) void k_attn(const h16* __restrict__ Q, long long q_bs, int q_rs, const h16* __restrict__ Kc,
                                              const h16* __restrict__ Vc, long long kv_bs, int kv_rs, int n_q, int n_keys,
                                              h16* __restrict__ O, long long o_bs, int o_rs, int kv_div,
                                              const uint8_t* __restrict__ anc, int anc_ld,
                                              const int* __restrict__ kvmap) {
  extern __shared__ float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, head = blockIdx.y, b = blockIdx.z;
  const int q0 = (blockIdx.x * 4 + wave) * QPW;
  float* sc = smem + (size_t)wave * QPW * n_keys;
  float* qs = smem + (size_t)4 * QPW * n_keys + wave * QPW * 64;
#pragma unroll
  for (int i = 0; i < QPW; ++i) {
    const int qi = q0 + i;
    qs[i * 64 + lane] = qi < n_q ? (float)Q[(size_t)b * q_bs + (size_t)qi * q_rs + head * 64 + lane] : 0.f;
  }
  __syncthreads();
  const size_t kvb = ANC ? 0 : (size_t)(kvmap ? kvmap[b] : b / kv_div);
  const int nk = !CAUSAL ? n_keys : (q0 >= n_q ? 0 : (q0 + QPW < n_keys ? q0 + QPW : n_keys));
  const h16* kb = Kc + kvb * kv_bs + head * 64;
  const h16* vb = Vc + kvb * kv_bs + head * 64;
  const uint8_t* an = ANC ? anc + (size_t)b * anc_ld : nullptr;
  float mx[QPW], sum[QPW], o[QPW];
#pragma unroll
  for (int i = 0; i < QPW; ++i) mx[i] = kNegInf, sum[i] = 0.f, o[i] = 0.f;
  for (int j = lane; j < nk; j += 64) {
    const uint4* kr = reinterpret_cast<const uint4*>(kb + (ANC ? (size_t)an[j] * kv_bs : 0) + (size_t)j * kv_rs);
    float s[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) s[i] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const half8 kk = __builtin_bit_cast(half8, kr[c]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float kf = (float)kk[e];
#pragma unroll
        for (int i = 0; i < QPW; ++i) s[i] += qs[i * 64 + c * 8 + e] * kf;
      }
    }
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
      s[i] *= 0.125f;
      if (CAUSAL && j > q0 + i) s[i] = kNegInf;
      sc[(size_t)i * n_keys + j] = s[i];
      mx[i] = fmaxf(mx[i], s[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < QPW; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], off, 64));
    for (int j = lane; j < nk; j += 64) {
      const float p = expf(sc[(size_t)i * n_keys + j] - mx[i]);
      sc[(size_t)i * n_keys + j] = p;
      sum[i] += p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum[i] += __shfl_xor(sum[i], off, 64);
  }
  __syncthreads();
  for (int j = 0; j < nk; ++j) {
    const float vf = (float)vb[(ANC ? (size_t)an[j] * kv_bs : 0) + (size_t)j * kv_rs + lane];
#pragma unroll
    for (int i = 0; i < QPW; ++i) o[i] += sc[(size_t)i * n_keys + j] * vf;
  }
#pragma unroll
  for (int i = 0; i < QPW; ++i) {
    const int qi = q0 + i;
    if (qi < n_q) O[(size_t)b * o_bs + (size_t)qi * o_rs + head * 64 + lane] = (h16)(o[i] / sum[i]);
  }
}

// ---- token selection ----------------------------------------------------------------------------------------------------
struct SelCfg {
  int vocab, eot, no_ts, tb, no_speech, max_init;
};
struct LaneState {  // per decode lane, on the device
  int n;            // tokens sampled so far
  int last, penult; // the last two sampled tokens (-1: none)
  int last_ts;      // the last sampled timestamp id (-1: none)
  int done;
  float sum;        // sum of the sampled tokens' log-probabilities
};
// per (lane, workgroup) partial over the workgroup's 64 vocabulary ids
constexpr int kNP = 10;  // max_text, arg_text, max_ts, arg_ts, m_all, s_all, s_ts (relative to max_ts), m_raw, s_raw, unused
constexpr int kFlagSuppress = 1, kFlagBegin = 2;  // flags[id]: bit 0 / 1, language index + 1 in bits 2..
// beam search: a beam partial is the kNP values above, then the block's best text ids and best timestamp ids as (value, id)
// pairs, kNC of each, best first, (-inf, -1) where there are fewer
constexpr int kMaxBeam = 8, kNC = kMaxBeam + 1, kMaxFinish = 16, kNPB = kNP + 4 * kNC;
// sampling (K20c): a sample partial is, per class (text ids, then timestamp ids), the block's best perturbed score, its id and
// that id's unperturbed masked logit, then max_text, max_ts, m_all, s_all, s_ts (relative to max_ts) as above, one unused
constexpr int kNPS = 12;

// Gumbel noise of sampled-token index idx and id n in the splitmix64 stream `seed`: element i = idx * vocab + n,
// u = ((z >> 41) + 0.5) * 2^-23 (23 bits: exact in fp32, never 0 or 1), g = -log(-log(u)) with the accurate logf.
__device__ __forceinline__ float gumbel_at(unsigned long long seed, int idx, int vocab, int n) {
  const unsigned long long z = splitmix64_at(seed, (unsigned long long)idx * (unsigned long long)vocab + (unsigned long long)n);
  const float u = ((float)(unsigned)(z >> 41) + 0.5f) * 1.1920928955078125e-07f;
  return -logf(-logf(u));
}

__device__ __forceinline__ bool rule_masks(int n, const SelCfg& c, unsigned flag, const LaneState& st) {
  const bool is_ts = n >= c.tb;
  bool mask = (flag & kFlagSuppress) != 0 || n == c.no_ts;
  if (st.n == 0) {
    mask = mask || (flag & kFlagBegin) != 0 || !is_ts;
    if (c.max_init >= 0 && n > c.tb + c.max_init) mask = true;
  }
  const bool last_ts = st.n >= 1 && st.last >= c.tb;
  const bool pen_ts = st.n < 2 || st.penult >= c.tb;
  if (last_ts) {
    if (pen_ts) mask = mask || is_ts;
    else mask = mask || n < c.eot;
  }
  if (st.last_ts >= 0) {
    const int limit = (last_ts && !pen_ts) ? st.last_ts : st.last_ts + 1;
    if (is_ts && n < limit) mask = true;
  }
  return mask;
}

// grid ceil(vocab / 64), 4 waves; wave w computes ids v0 + 16 w .. + 15 for 16 lanes at a time on the MFMA (or reads the
// supplied logits), masks them, and parks raw and masked values in LDS; thread b < 16 then folds the 64 ids of its lane
// in id order.  rules = 0: no masking (teacher-forced positions).
// BEAM: partials of kNPB values; the nc best masked text ids and the nc best masked timestamp ids of the block follow the
// kNP values.  Thread (lane tid & 15, ids 4 (tid >> 4) ..+ 3) ranks its ids within their class by (value, lower id first):
// an id's rank is the number of ids of its class that beat it, so every rank is written once and no order of threads matters.
// SAMPLE (never with BEAM): partials of kNPS values.  score = masked logit / temp + gumbel_at(seeds[lane], idx, vocab, id)
// is computed next to the mask and parked in LDS; the fold keeps the best score of each class (the lower id on equal
// scores), so no vocabulary-wide value reaches HBM.  idx = sidx[lane] when sidx is given, else sidx_all.
template <bool SUPPLIED, bool BEAM = false, bool SAMPLE = false>
__global__ __launch_bounds__(256) void k_logits(const h16* __restrict__ H, int d, const h16* __restrict__ E,
                                                const float* __restrict__ supplied, int B, SelCfg c,
                                                const uint16_t* __restrict__ flags, const LaneState* __restrict__ st, int rules,
                                                float* __restrict__ partial, int nblk, float* __restrict__ raw_out,
                                                long long raw_ld, float* __restrict__ masked_out, float* __restrict__ info,
                                                int nlang, int nc, float temp, const unsigned long long* __restrict__ seeds,
                                                const int* __restrict__ sidx, int sidx_all) {
  static_assert(!(BEAM && SAMPLE), "beam search does not sample");
  __shared__ float raw[64][17];
  __shared__ float msk[64][17];
  __shared__ float scr[SAMPLE ? 64 : 1][17];
  __shared__ float topv[BEAM ? 16 : 1][2][kNC];
  __shared__ int topi[BEAM ? 16 : 1][2][kNC];
  constexpr int NP = BEAM ? kNPB : (SAMPLE ? kNPS : kNP);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, u = lane >> 4;
  const int v0 = blockIdx.x * 64, n0 = v0 + wave * 16;
  for (int bt = 0; bt < B; bt += 16) {
    const int b = bt + r;
    float vals[4];
    if (SUPPLIED) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = n0 + 4 * u + t;
        vals[t] = (b < B && n < c.vocab) ? supplied[(size_t)b * c.vocab + n] : 0.f;
      }
    } else {
      const bool wl = n0 + r < c.vocab, al = b < B;
      const h16* wr = E + (size_t)(wl ? n0 + r : 0) * d + 8 * u;
      const h16* ar = H + (size_t)(al ? b : 0) * d + 8 * u;
      float4v acc = {0.f, 0.f, 0.f, 0.f};
      const half8 zero = {};
      for (int k = 0; k < d; k += 32) {
        const half8 w = wl ? __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(wr + k)) : zero;
        const half8 a = al ? __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(ar + k)) : zero;
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, a, acc, 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) vals[t] = acc[t];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + 4 * u + t, row = wave * 16 + 4 * u + t;
      float rv = kNegInf, mv = kNegInf;
      if (b < B && n < c.vocab) {
        rv = vals[t];
        const unsigned f = flags[n];
        mv = (rules && rule_masks(n, c, f, st[b])) ? kNegInf : rv;
        if (raw_out) raw_out[(size_t)b * raw_ld + n] = rv;
        if (masked_out) masked_out[(size_t)b * c.vocab + n] = mv;
        if (info) {
          if (n == c.no_speech) info[(size_t)b * (1 + nlang)] = rv;
          if ((f >> 2) > 0) info[(size_t)b * (1 + nlang) + (f >> 2)] = rv;
        }
      }
      raw[row][r] = rv;
      msk[row][r] = mv;
      if constexpr (SAMPLE)
        scr[row][r] = mv > kNegInf ? mv / temp + gumbel_at(seeds[b], sidx ? sidx[b] : sidx_all, c.vocab, n) : kNegInf;
    }
    __syncthreads();
    if constexpr (BEAM) {
      for (int i = tid; i < 16 * 2 * kNC; i += 256) (&topv[0][0][0])[i] = kNegInf, (&topi[0][0][0])[i] = -1;
      __syncthreads();
      const int bl = tid & 15, g = tid >> 4, split = c.tb - v0;  // block ids i < split are text
      if (bt + bl < B) {
        float mine[4];
        int rank[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) mine[t] = msk[4 * g + t][bl];
        for (int i = 0; i < 64; ++i) {
          const float o = msk[i][bl];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int me = 4 * g + t;
            if ((i >= split) == (me >= split) && (o > mine[t] || (o == mine[t] && i < me))) rank[t] += 1;
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int me = 4 * g + t;
          if (mine[t] > kNegInf && rank[t] < nc) topv[bl][me >= split][rank[t]] = mine[t], topi[bl][me >= split][rank[t]] = v0 + me;
        }
      }
      __syncthreads();
    }
    if (tid < 16 && bt + tid < B) {
      float max_text = kNegInf, max_ts = kNegInf, m_raw = kNegInf;
      int arg_text = -1, arg_ts = -1;
      float bs[2] = {kNegInf, kNegInf}, bl[2] = {kNegInf, kNegInf};  // SAMPLE: best score and its logit, text / timestamps
      int bi[2] = {-1, -1};
      for (int i = 0; i < 64; ++i) {
        const int n = v0 + i;
        const float mv = msk[i][tid];
        m_raw = fmaxf(m_raw, raw[i][tid]);
        if (n < c.tb) {
          if (mv > max_text) max_text = mv, arg_text = n;
        } else if (mv > max_ts) {
          max_ts = mv, arg_ts = n;
        }
        if constexpr (SAMPLE) {
          const int q = n < c.tb ? 0 : 1;
          if (mv > kNegInf && (bi[q] < 0 || scr[i][tid] > bs[q])) bs[q] = scr[i][tid], bi[q] = n, bl[q] = mv;
        }
      }
      const float m_all = fmaxf(max_text, max_ts);
      float s_all = 0.f, s_ts = 0.f, s_raw = 0.f;
      for (int i = 0; i < 64; ++i) {
        const float mv = msk[i][tid], rv = raw[i][tid];
        if (mv > kNegInf) {
          s_all += expf(mv - m_all);
          if (v0 + i >= c.tb) s_ts += expf(mv - max_ts);
        }
        if (rv > kNegInf) s_raw += expf(rv - m_raw);
      }
      float* p = partial + ((size_t)(bt + tid) * nblk + blockIdx.x) * NP;
      if constexpr (SAMPLE) {
        p[0] = bs[0], p[1] = __int_as_float(bi[0]), p[2] = bl[0], p[3] = bs[1], p[4] = __int_as_float(bi[1]), p[5] = bl[1];
        p[6] = max_text, p[7] = max_ts, p[8] = m_all, p[9] = s_all, p[10] = s_ts, p[11] = 0.f;
      } else {
        p[0] = max_text, p[1] = __int_as_float(arg_text), p[2] = max_ts, p[3] = __int_as_float(arg_ts);
        p[4] = m_all, p[5] = s_all, p[6] = s_ts, p[7] = m_raw, p[8] = s_raw, p[9] = 0.f;
      }
      if constexpr (BEAM) {
        for (int q = 0; q < 2; ++q)
          for (int r = 0; r < kNC; ++r)
            p[kNP + 2 * (q * kNC + r)] = topv[tid][q][r], p[kNP + 2 * (q * kNC + r) + 1] = __int_as_float(topi[tid][q][r]);
      }
    }
    __syncthreads();
  }
}

struct Acc {
  float max_text, max_ts, m_all, s_all, s_ts, m_raw, s_raw;
  int arg_text, arg_ts;
};

__device__ __forceinline__ void lse_merge(float& m, float& s, float pm, float ps) {
  if (pm == kNegInf) return;
  if (pm > m) {
    s = (m == kNegInf ? 0.f : s * expf(m - pm)) + ps;
    m = pm;
  } else {
    s += ps * expf(pm - m);
  }
}

__device__ __forceinline__ void acc_merge(Acc& a, const Acc& p) {
  if (p.max_text > a.max_text || (p.max_text == a.max_text && p.arg_text >= 0 && (a.arg_text < 0 || p.arg_text < a.arg_text)))
    a.max_text = p.max_text, a.arg_text = p.arg_text;
  lse_merge(a.m_all, a.s_all, p.m_all, p.s_all);
  lse_merge(a.m_raw, a.s_raw, p.m_raw, p.s_raw);
  // the timestamp sum is kept relative to the running timestamp max
  float mt = a.max_ts, st = a.s_ts;
  lse_merge(mt, st, p.max_ts, p.s_ts);
  if (p.max_ts > a.max_ts || (p.max_ts == a.max_ts && p.arg_ts >= 0 && (a.arg_ts < 0 || p.arg_ts < a.arg_ts))) a.arg_ts = p.arg_ts;
  a.max_ts = mt, a.s_ts = st;
}

// grid B, one wave: lanes fold the workgroup partials blk = lane, lane + 64, ...; thread 0 folds the 64 lanes in order and
// decides.  sample: pick a token, update the lane state, store it at tokens[b][idx].  do_info: no-speech probability and
// language argmax from the unmasked logits (prompt position 0).
__global__ __launch_bounds__(64) void k_select(const float* __restrict__ partial, int nblk, SelCfg c, LaneState* __restrict__ st,
                                               int sample, int idx, int do_info, const float* __restrict__ info, int nlang,
                                               const int* __restrict__ lang_ids, int* __restrict__ tokens, int tok_ld,
                                               int* __restrict__ cur_tok, float* __restrict__ nsp, int* __restrict__ lang_out,
                                               float* __restrict__ logprob_out) {
  __shared__ Acc sh[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  Acc a = {kNegInf, kNegInf, kNegInf, 0.f, 0.f, kNegInf, 0.f, -1, -1};
  for (int k = lane; k < nblk; k += 64) {
    const float* p = partial + ((size_t)b * nblk + k) * kNP;
    const Acc q = {p[0], p[2], p[4], p[5], p[6], p[7], p[8], __float_as_int(p[1]), __float_as_int(p[3])};
    acc_merge(a, q);
  }
  sh[lane] = a;
  __syncthreads();
  if (lane != 0) return;
  for (int i = 1; i < 64; ++i) acc_merge(a, sh[i]);
  if (do_info) {
    const float lse_raw = a.m_raw + logf(a.s_raw);
    const float* inf = info + (size_t)b * (1 + nlang);
    nsp[b] = expf(inf[0] - lse_raw);
    int best = -1;
    float bv = kNegInf;
    for (int i = 0; i < nlang; ++i)
      if (inf[1 + i] > bv) bv = inf[1 + i], best = i;
    lang_out[b] = best >= 0 ? lang_ids[best] : -1;
  }
  if (!sample) return;
  LaneState s = st[b];
  int tok = c.eot;
  float lp = 0.f;
  if (!s.done) {
    const float lse_all = a.m_all + logf(a.s_all);
    const float lse_ts = a.max_ts > kNegInf ? a.max_ts + logf(a.s_ts) : kNegInf;
    if (lse_ts > a.max_text) {
      tok = a.arg_ts, lp = a.max_ts - lse_ts;
    } else if (a.max_ts > a.max_text) {
      tok = a.arg_ts, lp = a.max_ts - lse_all;
    } else {
      tok = a.arg_text, lp = a.max_text - lse_all;
    }
    if (tok < 0) tok = c.eot, lp = 0.f;  // every id masked: cannot happen under the rules, end the lane
    s.sum += lp;
    s.penult = s.last;
    s.last = tok;
    if (tok >= c.tb) s.last_ts = tok;
    s.n += 1;
    if (tok == c.eot) s.done = 1;
    st[b] = s;
  }
  if (tokens) tokens[(size_t)b * tok_ld + idx] = tok;
  if (cur_tok) cur_tok[b] = tok;
  if (logprob_out) logprob_out[b] = lp;
}

// ---- sampling (K20c) ---------------------------------------------------------------------------------------------------------
struct SAcc {
  float bs[2], bl[2];  // per class (text, timestamps): the best perturbed score and that id's masked logit
  int bi[2];
  float max_text, max_ts, m_all, s_all, s_ts;
};

__device__ __forceinline__ void sacc_merge(SAcc& a, const SAcc& p) {
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (p.bi[q] >= 0 && (a.bi[q] < 0 || p.bs[q] > a.bs[q] || (p.bs[q] == a.bs[q] && p.bi[q] < a.bi[q])))
      a.bs[q] = p.bs[q], a.bi[q] = p.bi[q], a.bl[q] = p.bl[q];
  a.max_text = fmaxf(a.max_text, p.max_text);
  lse_merge(a.m_all, a.s_all, p.m_all, p.s_all);
  lse_merge(a.max_ts, a.s_ts, p.max_ts, p.s_ts);
}

// grid B, one wave: the fold of k_select over sample partials.  Rule 7 first (timestamp mass above every text id: text is
// out), then the best perturbed score of what is left, the lower id on equal scores.  The lane's sum gets the UNTEMPERED
// log-softmax of the masked logits at the token, as Whisper's GreedyDecoder accumulates.
__global__ __launch_bounds__(64) void k_sample_select(const float* __restrict__ partial, int nblk, SelCfg c, LaneState* __restrict__ st,
                                                      int idx, int* __restrict__ tokens, int tok_ld, int* __restrict__ cur_tok,
                                                      float* __restrict__ logprob_out) {
  __shared__ SAcc sh[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  SAcc a = {{kNegInf, kNegInf}, {kNegInf, kNegInf}, {-1, -1}, kNegInf, kNegInf, kNegInf, 0.f, 0.f};
  for (int k = lane; k < nblk; k += 64) {
    const float* p = partial + ((size_t)b * nblk + k) * kNPS;
    const SAcc q = {{p[0], p[3]}, {p[2], p[5]}, {__float_as_int(p[1]), __float_as_int(p[4])}, p[6], p[7], p[8], p[9], p[10]};
    sacc_merge(a, q);
  }
  sh[lane] = a;
  __syncthreads();
  if (lane != 0) return;
  for (int i = 1; i < 64; ++i) sacc_merge(a, sh[i]);
  LaneState s = st[b];
  int tok = c.eot;
  float lp = 0.f;
  if (!s.done) {
    const float lse_all = a.m_all + logf(a.s_all);
    const float lse_ts = a.max_ts > kNegInf ? a.max_ts + logf(a.s_ts) : kNegInf;
    if (lse_ts > a.max_text) {
      tok = a.bi[1], lp = a.bl[1] - lse_ts;
    } else if (a.bi[1] >= 0 && (a.bi[0] < 0 || a.bs[1] > a.bs[0])) {  // a text id is below every timestamp id
      tok = a.bi[1], lp = a.bl[1] - lse_all;
    } else {
      tok = a.bi[0], lp = a.bl[0] - lse_all;
    }
    if (tok < 0) tok = c.eot, lp = 0.f;  // every id masked: cannot happen under the rules, end the lane
    s.sum += lp;
    s.penult = s.last;
    s.last = tok;
    if (tok >= c.tb) s.last_ts = tok;
    s.n += 1;
    if (tok == c.eot) s.done = 1;
    st[b] = s;
  }
  if (tokens) tokens[(size_t)b * tok_ld + idx] = tok;
  if (cur_tok) cur_tok[b] = tok;
  if (logprob_out) logprob_out[b] = lp;
}

// ---- prompt prefill ------------------------------------------------------------------------------------------------------------
// x[(r, t)] = embed[ids[r * P + t]] + pos[t] for R rows of P prompt positions; grid R * P
__global__ __launch_bounds__(256) void k_embed_seq(const int* __restrict__ ids, int P, int vocab, int d, const h16* __restrict__ emb,
                                                   const float* __restrict__ pos, float* __restrict__ x) {
  const size_t row = blockIdx.x;
  int tok = ids[row];
  tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
  const int t = (int)(row % P);
  for (int i = threadIdx.x; i < d; i += 256) x[row * d + i] = (float)emb[(size_t)tok * d + i] + pos[(size_t)t * d + i];
}

// the prefill's keys and values [R][P][d] into the self-attention cache of lanes lane0 + r * lstride .. + G - 1 (row t of a
// lane's Tm rows); grid (P, R * G), 8 halves per thread
__global__ __launch_bounds__(256) void k_kv_to_cache(const h16* __restrict__ pk, const h16* __restrict__ pv, int P, int d, int G,
                                                     int lstride, int Tm, h16* __restrict__ ck, h16* __restrict__ cv) {
  const int t = blockIdx.x, r = blockIdx.y / G, lane = r * lstride + blockIdx.y % G;
  const size_t src = ((size_t)r * P + t) * d, dst = ((size_t)lane * Tm + t) * d;
  for (int i = threadIdx.x * 8; i < d; i += 256 * 8) {
    *reinterpret_cast<uint4*>(ck + dst + i) = *reinterpret_cast<const uint4*>(pk + src + i);
    *reinterpret_cast<uint4*>(cv + dst + i) = *reinterpret_cast<const uint4*>(pv + src + i);
  }
}

// out[l] = h[(l / G) * P + t]: one prefill position of every row, repeated for the G lanes of the row; grid L
__global__ __launch_bounds__(256) void k_gather_rows(const h16* __restrict__ h, int P, int t, int G, int d, h16* __restrict__ out) {
  const int l = blockIdx.x;
  const size_t src = ((size_t)(l / G) * P + t) * d;
  for (int i = threadIdx.x; i < d; i += 256) out[(size_t)l * d + i] = h[src + i];
}

// ---- beam search (K20b) ----------------------------------------------------------------------------------------------------
// Candidate order everywhere: the larger value first, the lower id on equal values.  (-inf, -1) is an empty entry.
__device__ __forceinline__ bool cand_better(float v, int i, float w, int k) { return v > w || (v == w && i < k); }

// sorted insert into a register-resident list of kNC entries (statically indexed: the loop is fully unrolled)
__device__ __forceinline__ void top_insert(float (&v)[kNC], int (&id)[kNC], float x, int xi) {
#pragma unroll
  for (int r = 0; r < kNC; ++r) {
    if (cand_better(x, xi, v[r], id[r])) {
      const float tv = v[r];
      const int ti = id[r];
      v[r] = x, id[r] = xi, x = tv, xi = ti;
    }
  }
}

// The wave's kNC best entries of 64 sorted per-thread lists, best first, into out_v / out_i [kNC] (LDS).  Round r: the best
// head of the wave by a butterfly over a total order (ids are unique, so every lane sees the same winner); its owner pops.
__device__ __forceinline__ void wave_top(float (&v)[kNC], int (&id)[kNC], int lane, float* out_v, int* out_i) {
#pragma unroll
  for (int r = 0; r < kNC; ++r) {
    float hv = v[0];
    int hi = id[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(hv, off, 64);
      const int oi = __shfl_xor(hi, off, 64);
      if (cand_better(ov, oi, hv, hi)) hv = ov, hi = oi;
    }
    if (hi >= 0 && id[0] == hi) {
#pragma unroll
      for (int q = 0; q + 1 < kNC; ++q) v[q] = v[q + 1], id[q] = id[q + 1];
      v[kNC - 1] = kNegInf, id[kNC - 1] = -1;
    }
    if (lane == r) out_v[r] = hv, out_i[r] = hi;
  }
}

// grid B (windows), W waves: wave j is beam slot j, lane b W + j.
//  1. the wave folds its lane's block partials (threads take blocks lane, lane + 64, ... in order, thread 0 then folds the
//     64 threads in order: the fold of k_select) and merges the blocks' best text and timestamp ids into the lane's best
//     nc = W + 1 of each class;
//  2. thread 0 of the wave decides the timestamp-mass rule and lists the slot's candidates (sum + log-probability, id),
//     best first; a dead slot (sum = -inf) has none;
//  3. thread 0 of the workgroup walks the candidates of all slots in (score, slot, id) order: EOT candidates finish, the
//     others fill the next slots, until W slots are filled;
//  4. all threads write the next lane states, input tokens, ancestry rows, token histories and the finished records.
// A complete window carries its slots over unchanged (identity permutation, no token, nothing recorded).
// s: the key row this step wrote; idx: the index of the token this step samples.  anc / hist may be NULL (test entry).
__global__ __launch_bounds__(64 * kMaxBeam) void k_beam_select(
    const float* __restrict__ partial, int nblk, SelCfg c, int W, int C, int s, int idx, LaneState* __restrict__ st,
    int* __restrict__ cur_tok, const uint8_t* __restrict__ anc, uint8_t* __restrict__ anc_next, int anc_ld,
    const int* __restrict__ hist, int* __restrict__ hist_next, int hist_ld, int* __restrict__ fin_tok, float* __restrict__ fin_sum,
    int* __restrict__ fin_n, int* __restrict__ fin_count, int* __restrict__ complete, int* __restrict__ out_src,
    int* __restrict__ out_tok, float* __restrict__ out_sum, int* __restrict__ out_nlive, int* __restrict__ out_fsrc,
    float* __restrict__ out_fsum, int* __restrict__ out_nfin) {
  __shared__ Acc sh[kMaxBeam][64];
  __shared__ float lv[kMaxBeam][2][kNC];
  __shared__ int li[kMaxBeam][2][kNC];
  __shared__ float cs[kMaxBeam][kNC];
  __shared__ int ct[kMaxBeam][kNC];
  __shared__ int cn[kMaxBeam], head[kMaxBeam];
  __shared__ LaneState old[kMaxBeam];
  __shared__ int n_src[kMaxBeam], n_tok[kMaxBeam], f_src[kMaxBeam];
  __shared__ float n_sum[kMaxBeam], f_sum[kMaxBeam];
  __shared__ int n_live, n_fin, fc_old, fc_new, carry;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, j = tid >> 6, nc = W + 1, L0 = b * W;
  if (tid < W) old[tid] = st[L0 + tid];
  // 1
  Acc a = {kNegInf, kNegInf, kNegInf, 0.f, 0.f, kNegInf, 0.f, -1, -1};
  float tv[kNC], sv[kNC];
  int ti[kNC], si[kNC];
#pragma unroll
  for (int r = 0; r < kNC; ++r) tv[r] = sv[r] = kNegInf, ti[r] = si[r] = -1;
  for (int k = lane; k < nblk; k += 64) {
    const float* p = partial + ((size_t)(L0 + j) * nblk + k) * kNPB;
    const Acc q = {p[0], p[2], p[4], p[5], p[6], p[7], p[8], __float_as_int(p[1]), __float_as_int(p[3])};
    acc_merge(a, q);
#pragma unroll
    for (int r = 0; r < kNC; ++r) {
      const float x = p[kNP + 2 * r], y = p[kNP + 2 * (kNC + r)];
      if (x > kNegInf) top_insert(tv, ti, x, __float_as_int(p[kNP + 2 * r + 1]));
      if (y > kNegInf) top_insert(sv, si, y, __float_as_int(p[kNP + 2 * (kNC + r) + 1]));
    }
  }
  sh[j][lane] = a;
  wave_top(tv, ti, lane, lv[j][0], li[j][0]);
  wave_top(sv, si, lane, lv[j][1], li[j][1]);
  __syncthreads();
  // 2
  if (lane == 0) {
    for (int i = 1; i < 64; ++i) acc_merge(a, sh[j][i]);
    const float lse_all = a.m_all + logf(a.s_all);
    const float lse_ts = a.max_ts > kNegInf ? a.max_ts + logf(a.s_ts) : kNegInf;
    const bool ts_only = lse_ts > a.max_text;
    const float lse = ts_only ? lse_ts : lse_all, sum = old[j].sum;
    int n = 0, pt = ts_only ? nc : 0, ps = 0;
    while (sum > kNegInf && n < nc) {
      const float x = pt < nc ? lv[j][0][pt] : kNegInf, y = ps < nc ? lv[j][1][ps] : kNegInf;
      if (!(x > kNegInf) && !(y > kNegInf)) break;
      const bool text = x >= y;  // a text id is below every timestamp id
      const float v = text ? x : y;
      ct[j][n] = text ? li[j][0][pt] : li[j][1][ps];
      cs[j][n] = sum + (v - lse);
      if (text) ++pt;
      else ++ps;
      ++n;
    }
    cn[j] = n;
    head[j] = 0;
  }
  __syncthreads();
  // 3
  if (tid == 0) {
    const int was = complete[b];
    int nl = 0, nf = 0;
    fc_old = fin_count[b];
    while (!was && nl < W) {
      int best = -1;
      float bs = kNegInf;
      for (int q = 0; q < W; ++q)
        if (head[q] < cn[q] && (best < 0 || cs[q][head[q]] > bs)) best = q, bs = cs[q][head[q]];
      if (best < 0) break;
      const int t = ct[best][head[best]];
      head[best] += 1;
      if (t == c.eot) {
        // a slot lists EOT at most once, so at most W <= kMaxBeam EOT candidates are walked: the guard never drops one
        if (nf < kMaxBeam) f_src[nf] = best, f_sum[nf] = bs, ++nf;
      } else {
        n_src[nl] = best, n_tok[nl] = t, n_sum[nl] = bs, ++nl;
      }
    }
    n_live = nl, n_fin = nf, carry = was;
    fc_new = was ? fc_old : (fc_old + nf < C ? fc_old + nf : C);
  }
  __syncthreads();
  // 4
  const int nl = n_live, cy = carry;
  if (tid < W) {
    const bool live = !cy && tid < nl;
    const int src = live ? n_src[tid] : tid;
    if (!cy) {
      LaneState ns = old[src];
      if (live) {
        ns.penult = ns.last;
        ns.last = n_tok[tid];
        if (n_tok[tid] >= c.tb) ns.last_ts = n_tok[tid];
        ns.n += 1;
        ns.sum = n_sum[tid];
        ns.done = 0;
      } else {
        ns.sum = kNegInf;
        ns.done = 1;
      }
      st[L0 + tid] = ns;
    }
    cur_tok[L0 + tid] = live ? n_tok[tid] : c.eot;
    if (out_src) {
      out_src[L0 + tid] = live ? src : -1;
      out_tok[L0 + tid] = live ? n_tok[tid] : c.eot;
      out_sum[L0 + tid] = live ? n_sum[tid] : kNegInf;
      out_fsrc[L0 + tid] = tid < n_fin ? f_src[tid] : -1;
      out_fsum[L0 + tid] = tid < n_fin ? f_sum[tid] : kNegInf;
    }
  }
  const int nt = 64 * W;
  if (anc) {
    for (int e = tid; e < W * (s + 1); e += nt) {
      const int q = e / (s + 1), t = e % (s + 1);
      const int src = (!cy && q < nl) ? n_src[q] : q;
      anc_next[(size_t)(L0 + q) * anc_ld + t] = anc[(size_t)(L0 + src) * anc_ld + t];
    }
  }
  if (hist) {
    for (int e = tid; e < W * (idx + 1); e += nt) {
      const int q = e / (idx + 1), t = e % (idx + 1);
      const bool live = !cy && q < nl;
      const int src = live ? n_src[q] : q;
      hist_next[(size_t)(L0 + q) * hist_ld + t] = (t == idx && live) ? n_tok[q] : hist[(size_t)(L0 + src) * hist_ld + t];
    }
    const int add = fc_new - fc_old;  // finished records: the history of the source slot, its score, its length
    for (int e = tid; e < add * (idx + 1); e += nt) {
      const int q = e / (idx + 1), t = e % (idx + 1);
      const size_t row = (size_t)b * kMaxFinish + fc_old + q;
      if (t < idx) fin_tok[row * hist_ld + t] = hist[(size_t)(L0 + f_src[q]) * hist_ld + t];
      else fin_sum[row] = f_sum[q], fin_n[row] = idx;
    }
  }
  if (tid == 0) {
    if (!cy) {
      fin_count[b] = fc_new;
      complete[b] = (fc_new >= C || nl == 0) ? 1 : 0;
    }
    if (out_nlive) out_nlive[b] = cy ? 0 : nl, out_nfin[b] = n_fin;
  }
}

// ---- word alignment (K21) ----------------------------------------------------------------------------------------------------
// Cross-attention probabilities of ONE head for every position of the alignment pass: the score and softmax half of k_attn
// (the same fp16 q and k, the same fp32 dot in the same order, x 0.125, running max, expf, lane sums folded by the same
// butterfly), without the V pass.  grid (ceil(n_q / 4), R), 4 waves, wave = query row qi of row b against all n_keys keys of
// window kvmap[b]; A[b * a_bs + qi * a_rs + f] = p_f / sum for f < nF[b].  Dynamic LDS: 4 (n_keys + 64) floats.
__global__ __launch_bounds__(256) void k_attn_weights(const h16* __restrict__ Q, long long q_bs, int q_rs, const h16* __restrict__ Kc,
                                                      long long kv_bs, int kv_rs, int n_q, int n_keys, int head,
                                                      const int* __restrict__ kvmap, const int* __restrict__ nF,
                                                      float* __restrict__ A, long long a_bs, long long a_rs) {
  extern __shared__ float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const int qi = blockIdx.x * 4 + wave;
  float* sc = smem + (size_t)wave * n_keys;
  float* qs = smem + (size_t)4 * n_keys + wave * 64;
  qs[lane] = qi < n_q ? (float)Q[(size_t)b * q_bs + (size_t)qi * q_rs + head * 64 + lane] : 0.f;
  __syncthreads();
  if (qi >= n_q) return;
  const h16* kb = Kc + (size_t)kvmap[b] * kv_bs + head * 64;
  float mx = kNegInf, sum = 0.f;
  for (int j = lane; j < n_keys; j += 64) {
    const uint4* kr = reinterpret_cast<const uint4*>(kb + (size_t)j * kv_rs);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const half8 kk = __builtin_bit_cast(half8, kr[c]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += qs[c * 8 + e] * (float)kk[e];
    }
    s *= 0.125f;
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  for (int j = lane; j < n_keys; j += 64) {
    const float p = expf(sc[j] - mx);
    sc[j] = p;
    sum += p;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  const int F = nF[b];
  float* out = A + (size_t)b * a_bs + (size_t)qi * a_rs;
  for (int j = lane; j < F; j += 64) out[j] = sc[j] / sum;
}

// Column statistics of A [R][H][T][ldf] over the token rows t < n_tok[r]: stat [R][H][2][ldf] = mean, population std, two
// passes with t in order.  The sums run in fp64: a frame that no token attends to holds probabilities around 1e-20 and
// below, whose squared deviations leave the fp32 range, and an fp32 std of such a column is off by a factor, not by an ulp.
// grid (ceil(ldf / 256), H, R), one thread per frame.
__global__ __launch_bounds__(256) void k_align_stats(const float* __restrict__ A, int H, int T, int ldf, const int* __restrict__ n_tok,
                                                     const int* __restrict__ nF, float* __restrict__ stat) {
  const int f = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, r = blockIdx.z;
  if (f >= nF[r]) return;
  const int n = n_tok[r];
  const float* a = A + ((size_t)r * H + h) * T * ldf + f;
  double s = 0.0;
  for (int t = 0; t < n; ++t) s += (double)a[(size_t)t * ldf];
  const double mean = s / (double)n;
  double q = 0.0;
  for (int t = 0; t < n; ++t) {
    const double c = (double)a[(size_t)t * ldf] - mean;
    q += c * c;
  }
  float* st = stat + ((size_t)r * H + h) * 2 * ldf;
  st[f] = (float)mean;
  st[ldf + f] = (float)sqrt(q / (double)n);
}

__device__ __forceinline__ void cswap(float& a, float& b) {
  const float lo = b < a ? b : a, hi = b < a ? a : b;
  a = lo, b = hi;
}

// the median of 7 values: the 16-exchange sorting network for 7 inputs, all in registers; a selection, so it adds no error
__device__ __forceinline__ float median7(float (&w)[7]) {
  cswap(w[0], w[6]), cswap(w[2], w[3]), cswap(w[4], w[5]);
  cswap(w[0], w[2]), cswap(w[1], w[4]), cswap(w[3], w[6]);
  cswap(w[0], w[1]), cswap(w[2], w[5]), cswap(w[3], w[4]);
  cswap(w[1], w[2]), cswap(w[4], w[6]);
  cswap(w[2], w[3]), cswap(w[4], w[5]);
  cswap(w[1], w[2]), cswap(w[3], w[4]), cswap(w[5], w[6]);
  return w[3];
}

// cost[r][i][f] = -mean_h median7_f((A[r][h][S + i][.] - mean) / std) for i < n_tok[r] - S - 1, f < nF[r]: normalise, width-7
// median along f with reflect indexing at both ends (skipped when nF[r] <= 3), heads summed in order and divided by H,
// negated.  grid (ceil(ldf / 256), Nmax, R), one thread per cost cell.
__global__ __launch_bounds__(256) void k_align_cost(const float* __restrict__ A, const float* __restrict__ stat, int H, int T, int ldf,
                                                    int S, const int* __restrict__ n_tok, const int* __restrict__ nF, int Nmax,
                                                    float* __restrict__ cost) {
  const int f = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, r = blockIdx.z;
  const int F = nF[r], N = n_tok[r] - S - 1;
  if (f >= F || i >= N) return;
  float acc = 0.f;
  for (int h = 0; h < H; ++h) {
    const float* row = A + (((size_t)r * H + h) * T + S + i) * ldf;
    const float* mean = stat + ((size_t)r * H + h) * 2 * ldf;
    const float* sd = mean + ldf;
    float v;
    if (F <= 3) {
      v = (row[f] - mean[f]) / sd[f];
    } else {
      float w[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        int g = f + k - 3;
        g = g < 0 ? -g : (g >= F ? 2 * (F - 1) - g : g);
        w[k] = (row[g] - mean[g]) / sd[g];
      }
      v = median7(w);
    }
    acc += v;
  }
  cost[((size_t)r * Nmax + i) * ldf + f] = -(acc / (float)H);
}

// Dynamic time warping of cost [R][ld_n][ldf], one workgroup per row r over its N = nN[r] token rows and F = nF[r] frames.
// D[i][j] = cost[i][j] + (D[i-1][j-1] if it is below both others, else D[i-1][j] if it is below both others, else
// D[i][j-1]), D[-1][-1] = 0 and +inf elsewhere outside, fp32, one add per cell.  Token rows go in bands of 256; in a band
// thread t owns row i = band + t and at step s computes column j = s - t, so the cells of a step lie on one anti-diagonal: its
// left value stays in a register, the value above comes from thread t - 1 through LDS (double-buffered, one barrier per
// step) and the value above-left is the one read the step before.  The last row of a band waits in `rowbuf` (dynamic LDS, F
// floats) for the first row of the next.  The trace takes 2 bits per cell (0 diagonal, 1 up, 2 left), 16 cells per word,
// trace [R][ld_n][tw] in global memory, each word written once by the thread that owns the row.  Thread 0 then walks back
// from (N - 1, F - 1): outside the matrix the trace is left along i = -1 and up along j = -1.  jump[r][i] = the frame of the
// first path cell of row i.  path (may be NULL) [R][2][ld_n + ldf]: the path's token rows, then its frames, last cell first.
constexpr int kDtwRows = 256;
__global__ __launch_bounds__(kDtwRows) void k_dtw(const float* __restrict__ cost, int ld_n, int ldf, const int* __restrict__ nN,
                                                   const int* __restrict__ nF, unsigned* __restrict__ trace, int tw,
                                                   int* __restrict__ jump, int* __restrict__ path, int* __restrict__ path_len) {
  extern __shared__ float rowbuf[];
  __shared__ float ex[2][kDtwRows];
  const int r = blockIdx.x, t = threadIdx.x, N = nN[r], F = nF[r];
  const float* C = cost + (size_t)r * ld_n * ldf;
  unsigned* tr = trace + (size_t)r * ld_n * tw;
  const float inf = INFINITY;
  for (int band = 0; band < N; band += kDtwRows) {
    const int i = band + t, rows = N - band < kDtwRows ? N - band : kDtwRows;
    float left = inf, diag = i == 0 ? 0.f : inf;
    unsigned word = 0;
    for (int s = 0; s < F + rows - 1; ++s) {
      const int j = s - t;
      if (t < rows && j >= 0 && j < F) {
        const float up = t > 0 ? ex[(s - 1) & 1][t - 1] : (band == 0 ? inf : rowbuf[j]);
        const float c0 = diag, c1 = up, c2 = left;
        float c;
        unsigned code;
        if (c0 < c1 && c0 < c2) c = c0, code = 0;
        else if (c1 < c0 && c1 < c2) c = c1, code = 1;
        else c = c2, code = 2;
        const float v = C[(size_t)i * ldf + j] + c;
        word |= code << (2 * (j & 15));
        if ((j & 15) == 15 || j == F - 1) {
          tr[(size_t)i * tw + (j >> 4)] = word;
          word = 0;
        }
        diag = up, left = v;
        ex[s & 1][t] = v;
        if (t == kDtwRows - 1) rowbuf[j] = v;  // read again by thread 0 of the next band only
      }
      __syncthreads();
    }
  }
  __threadfence();
  __syncthreads();
  if (t != 0) return;
  int* pt = path ? path + (size_t)r * 2 * (ld_n + ldf) : nullptr;
  int* pf = path ? pt + ld_n + ldf : nullptr;
  int i = N, j = F, n = 0;
  size_t cur = (size_t)-1;
  unsigned w = 0;
  while (i > 0 || j > 0) {
    if (pt) pt[n] = i - 1, pf[n] = j - 1;
    ++n;
    unsigned code;
    if (i == 0) code = 2;
    else if (j == 0) code = 1;
    else {
      const size_t at = (size_t)(i - 1) * tw + ((j - 1) >> 4);
      if (at != cur) cur = at, w = tr[at];
      code = (w >> (2 * ((j - 1) & 15))) & 3u;
    }
    if (code != 2 && i > 0) jump[(size_t)r * ld_n + i - 1] = j - 1;
    if (code == 0) --i, --j;
    else if (code == 1) --i;
    else --j;
  }
  if (path_len) path_len[r] = n;
}

// Forced-token logits against the tied embedding for M hidden rows H[hrow[b]][.]: grid ceil(eot / 64), the MFMA tile of
// k_logits; thread b < 16 folds the block's ids < eot in id order into partial [M][nblk][2] = (max, sum of exp relative to
// it) and, when target[b] is one of the block's ids, writes that logit to tgt[b] (one writer per row: a row's target lies
// in one block).  The vocabulary-wide logits are never written.
__global__ __launch_bounds__(256) void k_align_logits(const h16* __restrict__ H, int d, const h16* __restrict__ E,
                                                      const int* __restrict__ hrow, const int* __restrict__ target, int M, int eot,
                                                      float* __restrict__ partial, int nblk, float* __restrict__ tgt) {
  __shared__ float raw[64][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, u = lane >> 4;
  const int v0 = blockIdx.x * 64, n0 = v0 + wave * 16;
  for (int bt = 0; bt < M; bt += 16) {
    const int b = bt + r;
    const bool wl = n0 + r < eot, al = b < M;
    const h16* wr = E + (size_t)(wl ? n0 + r : 0) * d + 8 * u;
    const h16* ar = H + (size_t)(al ? hrow[b] : 0) * d + 8 * u;
    float4v acc = {0.f, 0.f, 0.f, 0.f};
    const half8 zero = {};
    for (int k = 0; k < d; k += 32) {
      const half8 w = wl ? __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(wr + k)) : zero;
      const half8 a = al ? __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(ar + k)) : zero;
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, a, acc, 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + 4 * u + t;
      raw[wave * 16 + 4 * u + t][r] = (b < M && n < eot) ? acc[t] : kNegInf;
    }
    __syncthreads();
    if (tid < 16 && bt + tid < M) {
      float mx = kNegInf, s = 0.f;
      for (int i = 0; i < 64; ++i) mx = fmaxf(mx, raw[i][tid]);
      for (int i = 0; i < 64; ++i)
        if (raw[i][tid] > kNegInf) s += expf(raw[i][tid] - mx);
      float* p = partial + ((size_t)(bt + tid) * nblk + blockIdx.x) * 2;
      p[0] = mx, p[1] = s;
      const int tg = target[bt + tid];
      if (tg >= v0 && tg < v0 + 64) tgt[bt + tid] = raw[tg - v0][tid];
    }
    __syncthreads();
  }
}

// grid M, one wave: prob[oidx[b]] = exp(tgt[b] - logsumexp of the block partials), folded as k_select folds its partials
__global__ __launch_bounds__(64) void k_align_prob(const float* __restrict__ partial, int nblk, const float* __restrict__ tgt,
                                                   const int* __restrict__ oidx, float* __restrict__ prob) {
  __shared__ float shm[64], shs[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  float mx = kNegInf, s = 0.f;
  for (int k = lane; k < nblk; k += 64) {
    const float* p = partial + ((size_t)b * nblk + k) * 2;
    lse_merge(mx, s, p[0], p[1]);
  }
  shm[lane] = mx, shs[lane] = s;
  __syncthreads();
  if (lane != 0) return;
  for (int i = 1; i < 64; ++i) lse_merge(mx, s, shm[i], shs[i]);
  prob[oidx[b]] = expf(tgt[b] - (mx + logf(s)));
}

// ---- the model ------------------------------------------------------------------------------------------------------------
struct Attn { int q, qb, k, v, vb, o, ob, ln_g, ln_b; };
struct Layer { Attn self, cross; int fc1, fc1b, fc2, fc2b, ln_g, ln_b; };

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The activations of one pass over a number of token rows: the residual stream x in fp32; the LayerNorm output h, the
// attention queries q, the attention output a and the MLP's hidden layer mid in fp16.
struct Work {
  DevBuf<float> x;
  DevBuf<h16> h, q, a, mid;
  int grow(size_t rows, size_t d, size_t ffn) {
    EIOKU_TRY(x.grow(rows * d));
    EIOKU_TRY(h.grow(rows * d));
    EIOKU_TRY(q.grow(rows * d));
    EIOKU_TRY(a.grow(rows * d));
    return mid.grow(rows * ffn);
  }
};

}  // namespace

struct eioku_whisper : TensorTable {
  eioku_whisper_cfg_t cfg{};
  SelCfg sel{};
  std::vector<Layer> enc, dec;
  int conv1 = 0, conv1b = 0, conv2 = 0, conv2b = 0, enc_pos = 0, enc_ln_g = 0, enc_ln_b = 0;
  int emb = 0, dec_pos = 0, dec_ln_g = 0, dec_ln_b = 0;
  int nlang = 0, nblk = 0, k1pad = 0;
  // constants
  DevBuf<double> hann, tw_cos, tw_sin, filt;
  DevBuf<uint16_t> flags;
  DevBuf<int> lang_ids;
  // audio + mel
  DevBuf<float> samples;
  long long n_samples = 0;
  DevBuf<long long> d_off;
  DevBuf<double> mel64, mel_mx;
  DevBuf<float> mel32;
  // encoder workspace (capacity cap windows; cap is the window stride of crossK / crossV)
  int cap = 0, enc_B = 0;
  DevBuf<h16> col1, h1, col2, ek, ev, enc_out, crossK, crossV;
  Work ew;
  // decoder workspace (capacity dcap lanes >= cap; dcap is the lane stride of selfK / selfV and the offset of the lane map
  // in kvmap)
  int dcap = 0;
  Work dw;
  DevBuf<h16> selfK, selfV;
  DevBuf<float> partial, info, nsp, d_logprob;
  DevBuf<LaneState> state;
  DevBuf<int> tokens, cur_tok, lang_out, d_ids;
  // beam search: lanes = windows * beam; ancestry table and token history double-buffered; finished records per window
  int beam_lanes = 0, beam_windows = 0;  // capacity of the beam buffers (0 until the first beam call)
  DevBuf<float> bpartial, fin_sum, b_sum, b_fsum;
  DevBuf<uint8_t> anc[2];
  DevBuf<int> hist[2], fin_tok, fin_n, fin_count, complete;
  DevBuf<int> b_src, b_tok, b_fsrc, b_nlive, b_nfin, tr_src, tr_tok;
  // sampling and prompt prefill: per-lane seeds and sample indices, the row -> window maps (rows, then lanes), and the
  // prefill workspace for prows = rows x prompt positions
  DevBuf<unsigned long long> d_seeds;
  DevBuf<int> d_sidx, kvmap;
  int prows = 0;
  Work pw;
  DevBuf<h16> pk, pv;
  DevBuf<float> ppartial;
  // word alignment (K21): the (layer, head) pairs (empty: every head of the upper half of the decoder layers), the
  // workspace of align(), each buffer grown on its own, and the device times of the last align() call
  std::vector<int> align_heads;
  DevBuf<float> al_A, al_stat, al_cost, al_part, al_tgt, al_prob;
  DevBuf<unsigned> al_trace;
  DevBuf<int> al_jump, al_meta, al_rows, al_path;
  double align_ms[3] = {0, 0, 0};
  double flops = 0;
  int launches = 0, steps = 0;
};

namespace {

void reset_counts(eioku_whisper* m) { m->flops = 0, m->launches = 0, m->steps = 0; }

// after a kernel launch: its error check, and the launch count of last_launches()
int launched(eioku_whisper* m) {
  EIOKU_LAUNCH_CHECK();
  m->launches += 1;
  return EIOKU_OK;
}

template <int MT, int EPI>
int gemm(eioku_whisper* m, const h16* A, int lda, const h16* W, int ldw, const float* bias, int M, int N, int K, void* out,
         long long ldc, const float* pos = nullptr, int pos_rows = 1) {
  EIOKU_TRY((launch_gemm<MT, EPI>(0, A, lda, W, ldw, bias, M, N, K, out, ldc, pos, pos_rows, nullptr, &m->flops)));
  m->launches += 1;
  return EIOKU_OK;
}

int ln(eioku_whisper* m, const float* x, int M, int d, int g, int b, h16* out) {
  hipLaunchKernelGGL(k_ln<h16>, dim3((M + 3) / 4), dim3(256), 0, 0, x, M, d, m->F(g), m->F(b), 1e-5f, (const int*)nullptr, out);
  return launched(m);
}

template <int QPW>
int attn(eioku_whisper* m, const h16* Q, long long q_bs, int q_rs, const h16* K, const h16* V, long long kv_bs, int kv_rs, int n_q,
         int n_keys, int B, h16* O, long long o_bs, int o_rs, int kv_div = 1, const uint8_t* anc = nullptr, int anc_ld = 0,
         const int* kvmap = nullptr, bool causal = false) {
  const size_t lds = (size_t)4 * QPW * (n_keys + 64) * sizeof(float);
  EIOKU_REQUIRE(lds <= 64 * 1024, "attention over %d keys needs %zu bytes of LDS", n_keys, lds);
  const dim3 grid((n_q + 4 * QPW - 1) / (4 * QPW), m->cfg.heads, B);
  if (causal) {
    EIOKU_REQUIRE(!anc && n_q == n_keys, "causal attention needs as many keys as queries and no ancestry table");
    hipLaunchKernelGGL((k_attn<QPW, false, true>), grid, dim3(256), lds, 0, Q, q_bs, q_rs, K, V, kv_bs, kv_rs, n_q, n_keys, O, o_bs,
                       o_rs, kv_div, (const uint8_t*)nullptr, 0, kvmap);
  } else if (anc) {
    hipLaunchKernelGGL((k_attn<QPW, true>), grid, dim3(256), lds, 0, Q, q_bs, q_rs, K, V, kv_bs, kv_rs, n_q, n_keys, O, o_bs, o_rs,
                       kv_div, anc, anc_ld, (const int*)nullptr);
  } else {
    hipLaunchKernelGGL((k_attn<QPW, false>), grid, dim3(256), lds, 0, Q, q_bs, q_rs, K, V, kv_bs, kv_rs, n_q, n_keys, O, o_bs, o_rs,
                       kv_div, (const uint8_t*)nullptr, 0, kvmap);
  }
  m->flops += 4.0 * B * m->cfg.heads * (double)n_q * n_keys * 64 * (causal ? 0.5 : 1.0);
  return launched(m);
}

// ---- the Whisper layer ------------------------------------------------------------------------------------------------------
// The sublayers that the encoder, the prompt prefill and the decoder step share, on a working set of M rows with GEMM tile
// MT.  What differs between the three - where self-attention keys and values go and how they are attended - stays with them.

// the head of an attention sublayer: LayerNorm of the residual stream into w.h, the query projection into w.q
template <int MT>
int ln_q(eioku_whisper* m, Work& w, int M, const Attn& A) {
  const int d = m->cfg.d_model;
  EIOKU_TRY(ln(m, w.x, M, d, A.ln_g, A.ln_b, w.h));
  return gemm<MT, EPI_F16>(m, w.h, d, m->H(A.q), d, m->F(A.qb), M, d, d, w.q, d);
}

// the key (no bias) and value projections of M rows of src into k and v, ldc elements from row to row
template <int MT>
int kv_proj(eioku_whisper* m, const h16* src, int M, const Attn& A, h16* k, h16* v, long long ldc) {
  const int d = m->cfg.d_model;
  EIOKU_TRY((gemm<MT, EPI_F16>(m, src, d, m->H(A.k), d, nullptr, M, d, d, k, ldc)));
  return gemm<MT, EPI_F16>(m, src, d, m->H(A.v), d, m->F(A.vb), M, d, d, v, ldc);
}

// the end of an attention sublayer: the out-projection of w.a added to the residual stream
template <int MT>
int out_proj(eioku_whisper* m, Work& w, int M, const Attn& A) {
  const int d = m->cfg.d_model;
  return gemm<MT, EPI_RESID>(m, w.a, d, m->H(A.o), d, m->F(A.ob), M, d, d, w.x, d);
}

// the MLP sublayer: LayerNorm, fc1 with GELU, fc2 added to the residual stream
template <int MT>
int mlp(eioku_whisper* m, Work& w, int M, const Layer& L, int ffn) {
  const int d = m->cfg.d_model;
  EIOKU_TRY(ln(m, w.x, M, d, L.ln_g, L.ln_b, w.h));
  EIOKU_TRY((gemm<MT, EPI_GELU_F16>(m, w.h, d, m->H(L.fc1), d, m->F(L.fc1b), M, ffn, d, w.mid, ffn)));
  return gemm<MT, EPI_RESID>(m, w.mid, ffn, m->H(L.fc2), ffn, m->F(L.fc2b), M, d, ffn, w.x, d);
}

// word alignment only: in every layer that has alignment heads, the cross-attention probabilities of those heads go to
// A [rows][n heads][positions][ldf] right after the cross q projection; the pass itself is unchanged.
struct AlignCapture {
  const int* heads;  // n (layer, head) pairs
  int n, ldf;
  const int* nF;     // device: frames kept per row
  float* A;
};

// the cross-attention sublayer of decoder layer l for R rows x P positions: row r (kv_div rows to a window, or window
// kvmap[r]) attends the window's crossK / crossV
template <int MT, int QPW>
int cross_attn(eioku_whisper* m, Work& w, int R, int P, int l, int kv_div, const int* kvmap, const AlignCapture* cap = nullptr) {
  const int d = m->cfg.d_model, ctx = m->cfg.max_source_positions;
  const long long bs = (long long)P * d;
  const Attn& A = m->dec[l].cross;
  const h16* ck = m->crossK + (size_t)l * m->cap * ctx * d;
  const h16* cv = m->crossV + (size_t)l * m->cap * ctx * d;
  EIOKU_TRY(ln_q<MT>(m, w, R * P, A));
  for (int hs = 0; cap && hs < cap->n; ++hs) {
    if (cap->heads[2 * hs] != l) continue;
    const size_t lds = (size_t)4 * (ctx + 64) * sizeof(float);
    hipLaunchKernelGGL(k_attn_weights, dim3((P + 3) / 4, R), dim3(256), lds, 0, w.q, bs, d, ck, (long long)ctx * d, d, P, ctx,
                       cap->heads[2 * hs + 1], kvmap, cap->nF, cap->A + (size_t)hs * P * cap->ldf, (long long)cap->n * P * cap->ldf,
                       (long long)cap->ldf);
    m->flops += 2.0 * R * (double)P * ctx * 64;
    EIOKU_TRY(launched(m));
  }
  EIOKU_TRY((attn<QPW>(m, w.q, bs, d, ck, cv, (long long)ctx * d, d, P, ctx, R, w.a, bs, d, kv_div, nullptr, 0, kvmap)));
  return out_proj<MT>(m, w, R * P, A);
}

// ---- workspaces -------------------------------------------------------------------------------------------------------------
// the decoder workspace for L lanes (greedy: one lane per window; beam search: beam lanes per window).  Growing it keeps
// the encoder's results.
int ensure_lanes(eioku_whisper* m, int L) {
  if (L <= m->dcap) return EIOKU_OK;
  const auto& c = m->cfg;
  const size_t d = c.d_model, Tm = c.max_target_positions, B = (size_t)L;
  m->dcap = 0;
  EIOKU_TRY(m->dw.grow(B, d, c.dec_ffn));
  for (DevBuf<h16>* b : {&m->selfK, &m->selfV}) EIOKU_TRY(b->grow(c.dec_layers * B * Tm * d));
  EIOKU_TRY(m->partial.grow(B * m->nblk * (kNPS > kNP ? kNPS : kNP)));
  EIOKU_TRY(m->info.grow(B * (1 + m->nlang)));
  EIOKU_TRY(m->kvmap.grow(2 * B));
  EIOKU_TRY(m->d_seeds.grow(B));
  EIOKU_TRY(m->state.grow(B));
  for (DevBuf<float>* b : {&m->nsp, &m->d_logprob}) EIOKU_TRY(b->grow(B));
  for (DevBuf<int>* b : {&m->d_sidx, &m->cur_tok, &m->lang_out}) EIOKU_TRY(b->grow(B));
  for (DevBuf<int>* b : {&m->tokens, &m->d_ids}) EIOKU_TRY(b->grow(B * Tm));
  m->dcap = L;
  return EIOKU_OK;
}

// beam search only: the decoder workspace for L lanes and the beam buffers for L lanes / B windows, made on the first beam
// call and grown as needed
int ensure_beam(eioku_whisper* m, int B, int L) {
  EIOKU_TRY(ensure_lanes(m, L));
  const size_t Tm = m->cfg.max_target_positions;
  if (L > m->beam_lanes) {
    const size_t n = (size_t)L;
    m->beam_lanes = 0;
    EIOKU_TRY(m->bpartial.grow(n * m->nblk * kNPB));
    for (int i = 0; i < 2; ++i) {
      EIOKU_TRY(m->anc[i].grow(n * Tm));
      EIOKU_TRY(m->hist[i].grow(n * Tm));
    }
    for (DevBuf<int>* b : {&m->b_src, &m->b_tok, &m->b_fsrc}) EIOKU_TRY(b->grow(n));
    for (DevBuf<float>* b : {&m->b_sum, &m->b_fsum}) EIOKU_TRY(b->grow(n));
    for (DevBuf<int>* b : {&m->tr_src, &m->tr_tok}) EIOKU_TRY(b->grow(n * Tm));
    m->beam_lanes = L;
  }
  if (B > m->beam_windows) {
    const size_t n = (size_t)B;
    m->beam_windows = 0;
    EIOKU_TRY(m->fin_tok.grow(n * kMaxFinish * Tm));
    EIOKU_TRY(m->fin_sum.grow(n * kMaxFinish));
    EIOKU_TRY(m->fin_n.grow(n * kMaxFinish));
    for (DevBuf<int>* b : {&m->fin_count, &m->complete, &m->b_nlive, &m->b_nfin}) EIOKU_TRY(b->grow(n));
    m->beam_windows = B;
  }
  return EIOKU_OK;
}

// the encoder workspace for B windows, and the decoder workspace for as many lanes.  Growing it drops the encoder's results.
int ensure_capacity(eioku_whisper* m, int B) {
  if (B <= m->cap) return ensure_lanes(m, B);
  const auto& c = m->cfg;
  const size_t T2 = 2 * (size_t)c.max_source_positions, ctx = c.max_source_positions, d = c.d_model;
  m->cap = 0;
  EIOKU_TRY(m->d_off.grow((size_t)B));
  EIOKU_TRY(m->mel64.grow(B * c.n_mels * T2));
  EIOKU_TRY(m->mel_mx.grow((size_t)B));
  EIOKU_TRY(m->mel32.grow(B * c.n_mels * T2));
  EIOKU_TRY(m->col1.grow(B * T2 * m->k1pad));
  EIOKU_TRY(m->h1.grow(B * T2 * d));
  EIOKU_TRY(m->col2.grow(B * ctx * 3 * d));
  EIOKU_TRY(m->ew.grow(B * ctx, d, c.enc_ffn > c.dec_ffn ? c.enc_ffn : c.dec_ffn));
  for (DevBuf<h16>* b : {&m->ek, &m->ev, &m->enc_out}) EIOKU_TRY(b->grow(B * ctx * d));
  for (DevBuf<h16>* b : {&m->crossK, &m->crossV}) EIOKU_TRY(b->grow(c.dec_layers * B * ctx * d));
  m->cap = B;
  m->enc_B = 0;
  return ensure_lanes(m, B);
}

// the prefill workspace for `rows` = rows x prompt positions
int ensure_prefill(eioku_whisper* m, int rows) {
  if (rows <= m->prows) return EIOKU_OK;
  const size_t n = (size_t)rows, d = m->cfg.d_model;
  m->prows = 0;
  EIOKU_TRY(m->pw.grow(n, d, m->cfg.dec_ffn));
  for (DevBuf<h16>* b : {&m->pk, &m->pv}) EIOKU_TRY(b->grow(n * d));
  EIOKU_TRY(m->ppartial.grow(n * m->nblk * kNP));
  m->prows = rows;
  return EIOKU_OK;
}

// ---- decoder passes ---------------------------------------------------------------------------------------------------------
// one decoder position s for B lanes: embedding -> layers -> final LayerNorm into m->dw.h.  Self-attention keys and values go
// straight into the cache at position s.  Beam search: kv_div lanes share a window's cross-attention K / V, and
// self-attention reads key t of a lane from the lane anc[lane][t].
int decoder_step(eioku_whisper* m, int B, int s, const int* toks, int tstride, int uniform, int kv_div = 1,
                 const uint8_t* anc = nullptr, const int* kvmap = nullptr) {
  const auto& c = m->cfg;
  const int d = c.d_model, Tm = c.max_target_positions;
  Work& w = m->dw;
  hipLaunchKernelGGL(k_embed, dim3(B), dim3(256), 0, 0, toks, tstride, uniform, c.vocab, d, s, m->H(m->emb), m->F(m->dec_pos), w.x);
  EIOKU_TRY(launched(m));
  for (int l = 0; l < c.dec_layers; ++l) {
    const Layer& L = m->dec[l];
    h16* sk = m->selfK + (size_t)l * m->dcap * Tm * d;
    h16* sv = m->selfV + (size_t)l * m->dcap * Tm * d;
    EIOKU_TRY(ln_q<1>(m, w, B, L.self));
    EIOKU_TRY(kv_proj<1>(m, w.h, B, L.self, sk + (size_t)s * d, sv + (size_t)s * d, (long long)Tm * d));
    EIOKU_TRY((attn<1>(m, w.q, d, d, sk, sv, (long long)Tm * d, d, 1, s + 1, B, w.a, d, d, 1, anc, Tm)));
    EIOKU_TRY(out_proj<1>(m, w, B, L.self));
    EIOKU_TRY((cross_attn<1, 1>(m, w, B, 1, l, kv_div, kvmap)));
    EIOKU_TRY(mlp<1>(m, w, B, L, c.dec_ffn));
  }
  return ln(m, w.x, B, d, m->dec_ln_g, m->dec_ln_b, w.h);
}

// One pass of the decoder over the P prompt positions of R rows (ids [R][P] on the device): the M-tiled GEMMs of the encoder,
// causal self-attention, cross-attention against window kvmap[r].  Leaves the final-LayerNorm hidden state of every position
// in m->pw.h [R][P][d] and the self-attention keys / values of positions 0 .. P - 1 in the cache of lanes r * lstride .. + G - 1.
int prefill(eioku_whisper* m, int R, int P, const int* ids, const int* kvmap, int G, int lstride, const AlignCapture* cap = nullptr) {
  const auto& c = m->cfg;
  const int d = c.d_model, Tm = c.max_target_positions, M = R * P;
  const long long bs = (long long)P * d;
  EIOKU_TRY(ensure_prefill(m, M));
  Work& w = m->pw;
  hipLaunchKernelGGL(k_embed_seq, dim3(M), dim3(256), 0, 0, ids, P, c.vocab, d, m->H(m->emb), m->F(m->dec_pos), w.x);
  EIOKU_TRY(launched(m));
  for (int l = 0; l < c.dec_layers; ++l) {
    const Layer& L = m->dec[l];
    h16* sk = m->selfK + (size_t)l * m->dcap * Tm * d;
    h16* sv = m->selfV + (size_t)l * m->dcap * Tm * d;
    EIOKU_TRY(ln_q<4>(m, w, M, L.self));
    EIOKU_TRY(kv_proj<4>(m, w.h, M, L.self, m->pk, m->pv, d));
    hipLaunchKernelGGL(k_kv_to_cache, dim3(P, R * G), dim3(256), 0, 0, m->pk, m->pv, P, d, G, lstride, Tm, sk, sv);
    EIOKU_TRY(launched(m));
    EIOKU_TRY((attn<2>(m, w.q, bs, d, m->pk, m->pv, bs, d, P, P, R, w.a, bs, d, 1, nullptr, 0, nullptr, true)));
    EIOKU_TRY(out_proj<4>(m, w, M, L.self));
    EIOKU_TRY((cross_attn<4, 2>(m, w, R, P, l, 1, kvmap, cap)));
    EIOKU_TRY(mlp<4>(m, w, M, L, c.dec_ffn));
  }
  return ln(m, w.x, M, d, m->dec_ln_g, m->dec_ln_b, w.h);
}

// m->dw.h[l] = the prefill's hidden state of row l / G at position t, for L lanes
int gather_hidden(eioku_whisper* m, int L, int P, int t, int G) {
  hipLaunchKernelGGL(k_gather_rows, dim3(L), dim3(256), 0, 0, m->pw.h, P, t, G, m->cfg.d_model, m->dw.h);
  return launched(m);
}

// ---- logits and selects -----------------------------------------------------------------------------------------------------
enum { SEL_GREEDY = 0, SEL_BEAM = 1, SEL_SAMPLE = 2 };

// what one launch of k_logits takes beyond the lanes; the defaults are the rules on the lanes' hidden state m->dw.h
struct LogitsArgs {
  const float* supplied = nullptr;  // the debug entries: logits [B][vocab] instead of the hidden state
  int rules = 1;
  float *raw_out = nullptr, *masked = nullptr;  // the rule-free logits (raw_ld from lane to lane) and the masked ones
  long long raw_ld = 0;
  bool info = false;                // the no-speech and language logits into m->info
  int nc = 0;                       // beam: candidates per block
  float temp = 1.f;                 // sample: the temperature, with m->d_seeds and a sample index per lane (sidx) or for all (idx)
  const int* sidx = nullptr;
  int idx = 0;
};

// masked logits of B lanes into the partials of KIND: greedy and sample share m->partial, beam has m->bpartial
template <int KIND>
int logits(eioku_whisper* m, int B, const LogitsArgs& a = {}) {
  constexpr bool BEAM = KIND == SEL_BEAM, SAMPLE = KIND == SEL_SAMPLE;
  float* partial = BEAM ? m->bpartial.p : m->partial.p;
  const unsigned long long* seeds = SAMPLE ? m->d_seeds.p : nullptr;
  float* info = a.info ? m->info.p : nullptr;
  if (a.supplied) {
    hipLaunchKernelGGL((k_logits<true, BEAM, SAMPLE>), dim3(m->nblk), dim3(256), 0, 0, (const h16*)nullptr, 0, (const h16*)nullptr,
                       a.supplied, B, m->sel, m->flags, m->state, a.rules, partial, m->nblk, a.raw_out, a.raw_ld, a.masked, info,
                       m->nlang, a.nc, a.temp, seeds, a.sidx, a.idx);
    EIOKU_LAUNCH_CHECK();
    return EIOKU_OK;
  }
  hipLaunchKernelGGL((k_logits<false, BEAM, SAMPLE>), dim3(m->nblk), dim3(256), 0, 0, m->dw.h, m->cfg.d_model, m->H(m->emb), nullptr, B,
                     m->sel, m->flags, m->state, a.rules, partial, m->nblk, a.raw_out, a.raw_ld, a.masked, info, m->nlang, a.nc,
                     a.temp, seeds, a.sidx, a.idx);
  m->flops += 2.0 * B * m->cfg.vocab * m->cfg.d_model;
  return launched(m);
}

// the greedy select of L lanes on m->partial.  sample: the token at index idx into tokens [L][Tm] and cur_tok (each may be
// NULL); info: the no-speech probability and the language into m->nsp / m->lang_out.
int greedy_select(eioku_whisper* m, int L, bool sample, int idx, bool info, int* tokens, int* cur_tok) {
  hipLaunchKernelGGL(k_select, dim3(L), dim3(64), 0, 0, m->partial, m->nblk, m->sel, m->state, sample ? 1 : 0, idx, info ? 1 : 0, m->info,
                     m->nlang, m->lang_ids, tokens, tokens ? m->cfg.max_target_positions : 0, cur_tok, m->nsp, m->lang_out,
                     (float*)nullptr);
  return launched(m);
}

// no-speech probability and language of L lanes from the rule-free logits of the hidden state in m->dw.h
int info_pair(eioku_whisper* m, int L, int* tokens = nullptr, int* cur_tok = nullptr) {
  LogitsArgs a;
  a.rules = 0, a.info = true;
  EIOKU_TRY(logits<SEL_GREEDY>(m, L, a));
  return greedy_select(m, L, false, 0, true, tokens, cur_tok);
}

// checks prompts [B][P] and windows [B] (NULL: identity, which needs B == the encoded windows); uploads the prompts to
// m->d_ids and the row -> window maps to m->kvmap (B rows) and m->kvmap + m->dcap (B * G lanes)
int prompted_args(eioku_whisper* m, const int32_t* prompts, int P, int sot_index, const int32_t* windows, int B, int G, int max_new) {
  EIOKU_REQUIRE(prompts && P >= 1 && max_new >= 1, "bad argument");
  EIOKU_REQUIRE(B > 0 && G >= 1 && B * G <= 64, "%d rows x %d = %d lanes: at most 64 lanes decode in lockstep", B, G, B * G);
  EIOKU_REQUIRE(sot_index >= 0 && sot_index < P, "sot_index %d outside the prompt of %d tokens", sot_index, P);
  EIOKU_REQUIRE(P + max_new <= m->cfg.max_target_positions, "prompt %d + %d new tokens exceed max_target_positions %d", P, max_new,
                m->cfg.max_target_positions);
  EIOKU_REQUIRE(m->enc_B > 0, "a prompted decode needs an encode first");
  if (!windows) EIOKU_REQUIRE(B == m->enc_B, "decode of %d rows without a window list needs an encode of the same %d windows", B, m->enc_B);
  for (int b = 0; windows && b < B; ++b)
    EIOKU_REQUIRE(windows[b] >= 0 && windows[b] < m->enc_B, "window %d outside the %d encoded windows", windows[b], m->enc_B);
  for (size_t i = 0; i < (size_t)B * P; ++i)
    EIOKU_REQUIRE(prompts[i] >= 0 && prompts[i] < m->cfg.vocab, "prompt id %d outside the vocabulary", prompts[i]);
  EIOKU_TRY(ensure_lanes(m, B * G));
  std::vector<int> map((size_t)2 * m->dcap, 0);
  for (int b = 0; b < B; ++b) map[b] = windows ? windows[b] : b;
  for (int l = 0; l < B * G; ++l) map[(size_t)m->dcap + l] = map[l / G];
  EIOKU_HIP_CHECK(hipMemcpy(m->kvmap, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->d_ids, prompts, (size_t)B * P * sizeof(int), hipMemcpyHostToDevice));
  return EIOKU_OK;
}

// ---- the start of a lockstep decode -----------------------------------------------------------------------------------------
// How B rows x G lanes get to the hidden state of their last prompt position (in m->dw.h), with the no-speech probability in
// m->nsp on the way.  Walked: `prompt` [P] is shared, every lane walks its first n_walk positions by decoder_step, and the
// info pair follows position 0 unless the caller merges it into its first select (info = false); nsp and the language are
// per lane.  Prefilled: `prompt` is [B][P], uploaded by prompted_args; one prefill per row fills the cache of `fill` lanes of
// the row, the info pair reads position sot_index, every lane starts from its row's last position; nsp is per row.
struct Start {
  const int32_t* prompt;
  int P;
  bool pre;
  int sot_index;
  int n_walk;
  bool info;
  int *tokens, *cur_tok;  // walked: what the info pair's select is handed (it stores nothing)
};

int start(eioku_whisper* m, const Start& st, int B, int G, int fill, int kv_div = 1, const uint8_t* anc = nullptr) {
  if (st.pre) {
    EIOKU_TRY(prefill(m, B, st.P, m->d_ids, m->kvmap, fill, G));
    EIOKU_TRY(gather_hidden(m, B, st.P, st.sot_index, 1));
    EIOKU_TRY(info_pair(m, B));
    return gather_hidden(m, B * G, st.P, st.P - 1, G);
  }
  for (int s = 0; s < st.n_walk; ++s) {
    EIOKU_TRY(decoder_step(m, B * G, s, nullptr, 1, st.prompt[s], kv_div, anc));
    m->steps += 1;
    if (s == 0 && st.info) EIOKU_TRY(info_pair(m, B * G, st.tokens, st.cur_tok));
  }
  return EIOKU_OK;
}

const LaneState kFreshLane{0, -1, -1, -1, 0, 0.f};

// The lockstep decode behind eioku_whisper_decode and eioku_whisper_decode_prompted: after the start, one select per new
// token - the greedy rule at temperature 0, Gumbel-max sampling with a seed per lane above it - and a decoder step between
// two selects.  Every sync_every tokens the lane states come back, and once every lane is done the rest is EOT.  Lane l's
// tokens go to tokens_out [l][max_new], its count and log-probability sum to n_out / sum_logprob, its final state to st.
int lane_decode(eioku_whisper* m, Start start_at, int B, int G, float temperature, const uint64_t* seeds, int max_new, int sync_every,
                int32_t* tokens_out, int32_t* n_out, float* sum_logprob, std::vector<LaneState>& st) {
  if (sync_every < 1) sync_every = 1;
  const int L = B * G, P = start_at.P, Tm = m->cfg.max_target_positions;
  const int* lane_map = start_at.pre ? m->kvmap + m->dcap : nullptr;
  reset_counts(m);
  st.assign(L, kFreshLane);
  EIOKU_HIP_CHECK(hipMemcpy(m->state, st.data(), (size_t)L * sizeof(LaneState), hipMemcpyHostToDevice));
  if (seeds) EIOKU_HIP_CHECK(hipMemcpy(m->d_seeds, seeds, (size_t)L * sizeof(uint64_t), hipMemcpyHostToDevice));
  // a walked one-token prompt that samples: step 0's select samples and reads the info in one launch pair
  const bool merged = !start_at.pre && P == 1 && max_new > 0;
  start_at.n_walk = max_new > 0 ? P : 1;
  start_at.info = !merged;
  start_at.tokens = m->tokens, start_at.cur_tok = m->cur_tok;
  EIOKU_TRY(start(m, start_at, B, G, G));
  for (int idx = 0; idx < max_new; ++idx) {
    if (idx > 0) {
      EIOKU_TRY(decoder_step(m, L, P - 1 + idx, m->cur_tok, 1, 0, 1, nullptr, lane_map));
      m->steps += 1;
    }
    LogitsArgs a;
    if (temperature == 0.f) {
      a.info = merged && idx == 0;
      EIOKU_TRY(logits<SEL_GREEDY>(m, L, a));
      EIOKU_TRY(greedy_select(m, L, true, idx, a.info, m->tokens, m->cur_tok));
    } else {
      a.temp = temperature, a.idx = idx;
      EIOKU_TRY(logits<SEL_SAMPLE>(m, L, a));
      hipLaunchKernelGGL(k_sample_select, dim3(L), dim3(64), 0, 0, m->partial, m->nblk, m->sel, m->state, idx, m->tokens, Tm, m->cur_tok,
                         (float*)nullptr);
      EIOKU_TRY(launched(m));
    }
    if ((idx + 1) % sync_every == 0 && idx + 1 < max_new) {  // read the lane states back: stop once every lane is done
      EIOKU_HIP_CHECK(hipMemcpy(st.data(), m->state, (size_t)L * sizeof(LaneState), hipMemcpyDeviceToHost));
      bool all = true;
      for (int l = 0; l < L; ++l) all = all && st[l].done;
      if (all) {  // the rest of every lane is EOT
        std::vector<int> row(Tm, m->cfg.eot);
        for (int l = 0; l < L; ++l)
          EIOKU_HIP_CHECK(hipMemcpy(m->tokens + (size_t)l * Tm + idx + 1, row.data(), (size_t)(max_new - idx - 1) * sizeof(int),
                                    hipMemcpyHostToDevice));
        break;
      }
    }
  }
  EIOKU_HIP_CHECK(hipMemcpy(st.data(), m->state, (size_t)L * sizeof(LaneState), hipMemcpyDeviceToHost));
  for (int l = 0; l < L && max_new > 0; ++l) {
    EIOKU_HIP_CHECK(hipMemcpy(tokens_out + (size_t)l * max_new, m->tokens + (size_t)l * Tm, (size_t)max_new * sizeof(int),
                              hipMemcpyDeviceToHost));
    n_out[l] = st[l].n;
    sum_logprob[l] = st[l].sum;
  }
  return EIOKU_OK;
}

// ---- the debug entries' shared parts ----------------------------------------------------------------------------------------
// positions s0 .. T - 1 of m->d_ids [B][T] walked by decoder_step, the rule-free logits of each into out [B][T][vocab]
int walked_logits(eioku_whisper* m, int B, int T, int s0, float* out) {
  LogitsArgs a;
  a.rules = 0, a.raw_ld = (long long)T * m->cfg.vocab;
  for (int s = s0; s < T; ++s) {
    EIOKU_TRY(decoder_step(m, B, s, m->d_ids + s, T, 0));
    a.raw_out = out + (size_t)s * m->cfg.vocab;
    EIOKU_TRY(logits<SEL_GREEDY>(m, B, a));
  }
  return EIOKU_OK;
}

LaneState state_of_prefix(const int32_t* prefix, int n, int tb) {
  LaneState s{n, -1, -1, -1, 0, 0.f};
  for (int i = 0; i < n; ++i) {
    s.penult = s.last;
    s.last = prefix[i];
    if (prefix[i] >= tb) s.last_ts = prefix[i];
  }
  return s;
}

// the state of L lanes after their prefixes [L][prefix_cap] (beam: with the lane's sum; -inf is a dead slot), uploaded
int upload_prefix_states(eioku_whisper* m, int L, const int32_t* prefix, int prefix_cap, const int32_t* prefix_len,
                         const float* sums = nullptr) {
  std::vector<LaneState> st(L);
  for (int l = 0; l < L; ++l) {
    const int n = prefix_len[l];
    EIOKU_REQUIRE(n >= 0 && n <= prefix_cap && (n == 0 || prefix), "bad prefix length %d", n);
    st[l] = state_of_prefix(n ? prefix + (size_t)l * prefix_cap : nullptr, n, m->cfg.timestamp_begin);
    if (sums) st[l].sum = sums[l], st[l].done = sums[l] > kNegInf ? 0 : 1;
  }
  EIOKU_HIP_CHECK(hipMemcpy(m->state, st.data(), (size_t)L * sizeof(LaneState), hipMemcpyHostToDevice));
  return EIOKU_OK;
}

struct Download {
  void* host;  // NULL: not wanted
  const void* dev;
  size_t bytes;
};

// supplied logits [L][vocab] up, `launch` on the device copy, the small results down
template <typename F>
int on_supplied_logits(eioku_whisper* m, const float* logits_in, int L, F launch, std::initializer_list<Download> results) {
  DevBuf<float> d_in;
  EIOKU_TRY(d_in.grow((size_t)L * m->cfg.vocab));
  EIOKU_HIP_CHECK(hipMemcpy(d_in, logits_in, (size_t)L * m->cfg.vocab * sizeof(float), hipMemcpyHostToDevice));
  EIOKU_TRY(launch(d_in.p));
  for (const Download& r : results)
    if (r.host) EIOKU_HIP_CHECK(hipMemcpy(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

}  // namespace

extern "C" {

int eioku_whisper_create(const eioku_whisper_cfg_t* cfg, eioku_whisper** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(cfg && out, "NULL argument");
  const eioku_whisper_cfg_t& c = *cfg;
  EIOKU_REQUIRE(c.d_model > 0 && c.d_model % 64 == 0 && c.heads * 64 == c.d_model, "head_dim must be 64 (d_model %d / heads %d)",
                c.d_model, c.heads);
  EIOKU_REQUIRE(c.enc_ffn > 0 && c.dec_ffn > 0 && c.enc_ffn % 32 == 0 && c.dec_ffn % 32 == 0, "ffn sizes must be multiples of 32");
  EIOKU_REQUIRE(c.n_mels > 0 && c.enc_layers > 0 && c.dec_layers > 0 && c.vocab > 0 && c.max_source_positions > 0 &&
                    c.max_target_positions > 0, "bad config");
  EIOKU_REQUIRE((size_t)4 * 2 * (c.max_source_positions + 64) * sizeof(float) <= 64 * 1024, "max_source_positions %d too large",
                c.max_source_positions);
  EIOKU_REQUIRE(c.eot >= 0 && c.eot < c.vocab && c.timestamp_begin > c.eot && c.timestamp_begin <= c.vocab &&
                    c.no_timestamps >= 0 && c.no_timestamps < c.vocab && c.no_speech >= 0 && c.no_speech < c.vocab,
                "special token ids outside the vocabulary");
  EIOKU_REQUIRE(c.n_suppress >= 0 && c.n_begin_suppress >= 0 && c.n_langs >= 0 && c.n_langs < 16000 && c.mel_filters, "bad lists");
  auto* m = new eioku_whisper();
  m->cfg = c;
  m->cfg.suppress = m->cfg.begin_suppress = m->cfg.lang_ids = nullptr;
  m->cfg.mel_filters = nullptr;
  m->sel = SelCfg{c.vocab, c.eot, c.no_timestamps, c.timestamp_begin, c.no_speech, c.max_initial_timestamp_index};
  m->nlang = c.n_langs;
  m->nblk = (c.vocab + 63) / 64;
  m->k1pad = round_up(3 * c.n_mels, 32);
  const int d = c.d_model;
  auto add_attn = [&](const std::string& p, const std::string& lnp) {
    Attn a;
    a.q = m->add(p + "q_proj.weight", d, d, T_F16);
    a.qb = m->add(p + "q_proj.bias", d, 1, T_F32);
    a.k = m->add(p + "k_proj.weight", d, d, T_F16);
    a.v = m->add(p + "v_proj.weight", d, d, T_F16);
    a.vb = m->add(p + "v_proj.bias", d, 1, T_F32);
    a.o = m->add(p + "out_proj.weight", d, d, T_F16);
    a.ob = m->add(p + "out_proj.bias", d, 1, T_F32);
    a.ln_g = m->add(lnp + ".weight", d, 1, T_F32);
    a.ln_b = m->add(lnp + ".bias", d, 1, T_F32);
    return a;
  };
  m->conv1 = m->add("model.encoder.conv1.weight", d, c.n_mels * 3, T_CONV);
  m->conv1b = m->add("model.encoder.conv1.bias", d, 1, T_F32);
  m->conv2 = m->add("model.encoder.conv2.weight", d, d * 3, T_CONV);
  m->conv2b = m->add("model.encoder.conv2.bias", d, 1, T_F32);
  m->enc_pos = m->add("model.encoder.embed_positions.weight", c.max_source_positions, d, T_F32);
  for (int l = 0; l < c.enc_layers + c.dec_layers; ++l) {
    const bool is_dec = l >= c.enc_layers;
    const std::string p = std::string("model.") + (is_dec ? "decoder" : "encoder") + ".layers." +
                          std::to_string(is_dec ? l - c.enc_layers : l) + ".";
    const int ffn = is_dec ? c.dec_ffn : c.enc_ffn;
    Layer L{};
    L.self = add_attn(p + "self_attn.", p + "self_attn_layer_norm");
    if (is_dec) L.cross = add_attn(p + "encoder_attn.", p + "encoder_attn_layer_norm");
    L.fc1 = m->add(p + "fc1.weight", ffn, d, T_F16);
    L.fc1b = m->add(p + "fc1.bias", ffn, 1, T_F32);
    L.fc2 = m->add(p + "fc2.weight", d, ffn, T_F16);
    L.fc2b = m->add(p + "fc2.bias", d, 1, T_F32);
    L.ln_g = m->add(p + "final_layer_norm.weight", d, 1, T_F32);
    L.ln_b = m->add(p + "final_layer_norm.bias", d, 1, T_F32);
    (is_dec ? m->dec : m->enc).push_back(L);
    if (l == c.enc_layers - 1) {
      m->enc_ln_g = m->add("model.encoder.layer_norm.weight", d, 1, T_F32);
      m->enc_ln_b = m->add("model.encoder.layer_norm.bias", d, 1, T_F32);
      m->emb = m->add("model.decoder.embed_tokens.weight", c.vocab, d, T_F16);
      m->dec_pos = m->add("model.decoder.embed_positions.weight", c.max_target_positions, d, T_F32);
    }
  }
  m->dec_ln_g = m->add("model.decoder.layer_norm.weight", d, 1, T_F32);
  m->dec_ln_b = m->add("model.decoder.layer_norm.bias", d, 1, T_F32);
  auto fail = [&](int rc) {
    eioku_whisper_destroy(m);
    return rc;
  };
  if (const int rc = m->finish()) return fail(rc);
  // constants: periodic Hann window, DFT twiddles, mel filterbank, per-id flags
  std::vector<double> hann(kNfft), tc(kNfft), ts(kNfft);
  const double two_pi = 6.283185307179586476925286766559;
  for (int n = 0; n < kNfft; ++n) {
    hann[n] = 0.5 - 0.5 * std::cos(two_pi * n / kNfft);
    tc[n] = std::cos(two_pi * n / kNfft);
    ts[n] = std::sin(two_pi * n / kNfft);
  }
  std::vector<uint16_t> flags(c.vocab, 0);
  for (int i = 0; i < c.n_suppress; ++i)
    if (c.suppress[i] >= 0 && c.suppress[i] < c.vocab) flags[c.suppress[i]] |= kFlagSuppress;
  for (int i = 0; i < c.n_begin_suppress; ++i)
    if (c.begin_suppress[i] >= 0 && c.begin_suppress[i] < c.vocab) flags[c.begin_suppress[i]] |= kFlagBegin;
  for (int i = 0; i < c.n_langs; ++i) {
    if (c.lang_ids[i] < 0 || c.lang_ids[i] >= c.vocab) {
      set_error("language id %d outside the vocabulary", c.lang_ids[i]);
      return fail(EIOKU_EINVAL);
    }
    flags[c.lang_ids[i]] |= (uint16_t)((i + 1) << 2);
  }
  if (m->hann.grow(kNfft) || m->tw_cos.grow(kNfft) || m->tw_sin.grow(kNfft) || m->filt.grow((size_t)c.n_mels * kBins) ||
      m->flags.grow((size_t)c.vocab) || m->lang_ids.grow((size_t)c.n_langs))
    return fail(EIOKU_ENOMEM);
  if (hipMemcpy(m->hann, hann.data(), kNfft * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->tw_cos, tc.data(), kNfft * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->tw_sin, ts.data(), kNfft * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->filt, c.mel_filters, (size_t)c.n_mels * kBins * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->flags, flags.data(), (size_t)c.vocab * 2, hipMemcpyHostToDevice) != hipSuccess ||
      (c.n_langs && hipMemcpy(m->lang_ids, c.lang_ids, (size_t)c.n_langs * 4, hipMemcpyHostToDevice) != hipSuccess)) {
    set_error("hipMemcpy of the Whisper constants failed");
    return fail(EIOKU_EHIP);
  }
  *out = m;
  return EIOKU_OK;
}

void eioku_whisper_destroy(eioku_whisper* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  delete m;  // every buffer frees itself
}

int eioku_whisper_num_tensors(const eioku_whisper* m) { return TensorTable::count(m); }

int eioku_whisper_tensor_info(const eioku_whisper* m, int idx, char* name, size_t cap, int* rows, int* cols) {
  return TensorTable::info(m, idx, name, cap, rows, cols);
}

int eioku_whisper_set_tensor(eioku_whisper* m, int idx, const float* host, size_t numel) { return TensorTable::set(m, idx, host, numel); }

int eioku_whisper_set_audio(eioku_whisper* m, const float* samples, long long n) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n >= 0 && (samples || n == 0), "bad argument");
  EIOKU_TRY(m->samples.grow((size_t)n));
  m->n_samples = n;
  if (n) EIOKU_HIP_CHECK(hipMemcpy(m->samples, samples, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  return EIOKU_OK;
}

int eioku_whisper_logmel(eioku_whisper* m, const long long* offsets, int B, float* out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && offsets && B > 0 && B <= 64, "bad argument (1 <= B <= 64)");
  EIOKU_REQUIRE(m->samples, "no audio: call eioku_whisper_set_audio first");
  for (int b = 0; b < B; ++b) EIOKU_REQUIRE(offsets[b] >= 0, "negative window offset");
  EIOKU_TRY(ensure_capacity(m, B));
  const auto& c = m->cfg;
  const int T = 2 * c.max_source_positions;
  const long long per = (long long)c.n_mels * T, total = per * B;
  EIOKU_HIP_CHECK(hipMemcpy(m->d_off, offsets, (size_t)B * sizeof(long long), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_mel_frames, dim3(T, B), dim3(256), 0, 0, m->samples, m->n_samples, m->d_off, T, c.n_mels, m->hann, m->tw_cos,
                     m->tw_sin, m->filt, m->mel64);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mel_max, dim3(B), dim3(256), 0, 0, m->mel64, per, m->mel_mx);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mel_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, m->mel64, per, m->mel_mx, total, m->mel32);
  EIOKU_LAUNCH_CHECK();
  if (out) EIOKU_HIP_CHECK(hipMemcpy(out, m->mel32, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
  else EIOKU_HIP_CHECK(hipDeviceSynchronize());
  return EIOKU_OK;
}

int eioku_whisper_encode(eioku_whisper* m, const float* mel, int B) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && B > 0 && B <= 64, "bad argument (1 <= B <= 64)");
  EIOKU_TRY(m->check());
  EIOKU_REQUIRE(mel || B <= m->cap, "no log-mel result for %d windows", B);
  EIOKU_TRY(ensure_capacity(m, B));
  const auto& c = m->cfg;
  const int d = c.d_model, ctx = c.max_source_positions, T2 = 2 * ctx, M = B * ctx;
  Work& w = m->ew;
  if (mel) EIOKU_HIP_CHECK(hipMemcpy(m->mel32, mel, (size_t)B * c.n_mels * T2 * sizeof(float), hipMemcpyHostToDevice));
  m->flops = 0;
  m->launches = 0;
  m->enc_B = 0;
  {
    const size_t n1 = (size_t)B * T2 * m->k1pad, n2 = (size_t)M * 3 * d;
    hipLaunchKernelGGL(k_im2col_mel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, 0, m->mel32, B, c.n_mels, T2, m->k1pad, m->col1);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY((gemm<4, EPI_GELU_F16>(m, m->col1, m->k1pad, m->H(m->conv1), m->k1pad, m->F(m->conv1b), B * T2, d, m->k1pad, m->h1, d)));
    hipLaunchKernelGGL(k_im2col_s2, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, 0, m->h1, B, d, T2, m->col2);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY((gemm<4, EPI_GELU_POS>(m, m->col2, 3 * d, m->H(m->conv2), 3 * d, m->F(m->conv2b), M, d, 3 * d, w.x, d, m->F(m->enc_pos), ctx)));
  }
  for (int l = 0; l < c.enc_layers; ++l) {
    const Layer& L = m->enc[l];
    EIOKU_TRY(ln_q<4>(m, w, M, L.self));
    EIOKU_TRY(kv_proj<4>(m, w.h, M, L.self, m->ek, m->ev, d));
    EIOKU_TRY((attn<2>(m, w.q, (long long)ctx * d, d, m->ek, m->ev, (long long)ctx * d, d, ctx, ctx, B, w.a, (long long)ctx * d, d)));
    EIOKU_TRY(out_proj<4>(m, w, M, L.self));
    EIOKU_TRY(mlp<4>(m, w, M, L, c.enc_ffn));
  }
  EIOKU_TRY(ln(m, w.x, M, d, m->enc_ln_g, m->enc_ln_b, m->enc_out));
  for (int l = 0; l < c.dec_layers; ++l)  // cross-attention keys and values, once per window
    EIOKU_TRY(kv_proj<4>(m, m->enc_out, M, m->dec[l].cross, m->crossK + (size_t)l * m->cap * ctx * d,
                     m->crossV + (size_t)l * m->cap * ctx * d, d));
  EIOKU_HIP_CHECK(hipDeviceSynchronize());
  m->enc_B = B;
  return EIOKU_OK;
}

int eioku_whisper_encoder_output(eioku_whisper* m, void* out_f16, size_t numel) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && out_f16 && m->enc_B > 0, "no encoder result");
  EIOKU_REQUIRE(numel == (size_t)m->enc_B * m->cfg.max_source_positions * m->cfg.d_model, "expected %zu elements",
                (size_t)m->enc_B * m->cfg.max_source_positions * m->cfg.d_model);
  EIOKU_HIP_CHECK(hipMemcpy(out_f16, m->enc_out, numel * sizeof(h16), hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

int eioku_whisper_decode(eioku_whisper* m, const int32_t* prompt, int prompt_len, int B, int max_new, int sync_every,
                         int32_t* tokens_out, int32_t* n_out, float* sum_logprob, float* no_speech_prob, int32_t* lang_out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && prompt && prompt_len >= 1 && max_new >= 0, "bad argument");
  EIOKU_REQUIRE(B > 0 && B == m->enc_B, "decode of %d lanes needs an encode of the same %d windows first", B, m->enc_B);
  EIOKU_REQUIRE(prompt_len + max_new <= m->cfg.max_target_positions, "prompt %d + %d new tokens exceed max_target_positions %d",
                prompt_len, max_new, m->cfg.max_target_positions);
  EIOKU_REQUIRE(max_new == 0 || (tokens_out && n_out && sum_logprob), "NULL output");
  for (int i = 0; i < prompt_len; ++i) EIOKU_REQUIRE(prompt[i] >= 0 && prompt[i] < m->cfg.vocab, "prompt id %d outside the vocabulary", prompt[i]);
  std::vector<LaneState> st;
  EIOKU_TRY(lane_decode(m, Start{prompt, prompt_len, false, 0}, B, 1, 0.f, nullptr, max_new, sync_every, tokens_out, n_out, sum_logprob, st));
  if (no_speech_prob) EIOKU_HIP_CHECK(hipMemcpy(no_speech_prob, m->nsp, (size_t)B * sizeof(float), hipMemcpyDeviceToHost));
  if (lang_out) EIOKU_HIP_CHECK(hipMemcpy(lang_out, m->lang_out, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

int eioku_whisper_decode_prompted(eioku_whisper* m, const int32_t* prompts, int P, int sot_index, const int32_t* windows, int B, int G,
                                  float temperature, const uint64_t* seeds, int max_new, int sync_every, int32_t* tokens_out,
                                  int32_t* n_out, float* sum_logprob, int32_t* best_out, float* no_speech_prob) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m, "NULL model");
  EIOKU_REQUIRE(temperature >= 0.f && std::isfinite(temperature), "temperature %g must be a finite number >= 0", (double)temperature);
  if (temperature == 0.f) EIOKU_REQUIRE(G == 1 && !seeds, "temperature 0 is the greedy rule: one row per window and no seeds");
  else EIOKU_REQUIRE(seeds, "sampling at temperature %g needs a seed per lane", (double)temperature);
  EIOKU_TRY(prompted_args(m, prompts, P, sot_index, windows, B, G, max_new));
  EIOKU_REQUIRE(tokens_out && n_out && sum_logprob && best_out, "NULL output");
  std::vector<LaneState> st;
  EIOKU_TRY(lane_decode(m, Start{prompts, P, true, sot_index}, B, G, temperature, seeds, max_new, sync_every, tokens_out, n_out, sum_logprob, st));
  for (int b = 0; b < B; ++b) {  // the row with the largest sum / max(1, tokens before EOT), the earlier row on a tie
    int best = 0;
    double best_score = 0;
    for (int g = 0; g < G; ++g) {
      const LaneState& ls = st[(size_t)b * G + g];
      const int n_text = ls.n - (ls.done ? 1 : 0);
      const double score = (double)ls.sum / (n_text > 1 ? n_text : 1);
      if (g == 0 || score > best_score) best = g, best_score = score;
    }
    best_out[b] = best;
  }
  if (no_speech_prob) EIOKU_HIP_CHECK(hipMemcpy(no_speech_prob, m->nsp, (size_t)B * sizeof(float), hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

int eioku_whisper_forced_logits(eioku_whisper* m, const int32_t* ids, int T, int B, float* out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && ids && out && T >= 1 && T <= m->cfg.max_target_positions, "bad argument");
  EIOKU_REQUIRE(B > 0 && B == m->enc_B, "forced_logits of %d lanes needs an encode of the same %d windows first", B, m->enc_B);
  const int V = m->cfg.vocab;
  for (size_t i = 0; i < (size_t)B * T; ++i) EIOKU_REQUIRE(ids[i] >= 0 && ids[i] < V, "id %d outside the vocabulary", ids[i]);
  EIOKU_HIP_CHECK(hipMemcpy(m->d_ids, ids, (size_t)B * T * sizeof(int), hipMemcpyHostToDevice));
  DevBuf<float> d_out;
  EIOKU_TRY(d_out.grow((size_t)B * T * V));
  const std::vector<LaneState> st(B, kFreshLane);
  EIOKU_HIP_CHECK(hipMemcpy(m->state, st.data(), (size_t)B * sizeof(LaneState), hipMemcpyHostToDevice));
  EIOKU_TRY(walked_logits(m, B, T, 0, d_out));
  EIOKU_HIP_CHECK(hipMemcpy(out, d_out, (size_t)B * T * V * sizeof(float), hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

int eioku_whisper_prefill_logits(eioku_whisper* m, const int32_t* ids, int T, int B, int n_prefill, float* out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && ids && out && T >= 1 && T <= m->cfg.max_target_positions, "bad argument");
  EIOKU_REQUIRE(n_prefill >= 1 && n_prefill <= T, "prefill of %d positions outside 1..%d", n_prefill, T);
  EIOKU_REQUIRE(B > 0 && B == m->enc_B, "prefill_logits of %d lanes needs an encode of the same %d windows first", B, m->enc_B);
  const int V = m->cfg.vocab, P = n_prefill;
  for (size_t i = 0; i < (size_t)B * T; ++i) EIOKU_REQUIRE(ids[i] >= 0 && ids[i] < V, "id %d outside the vocabulary", ids[i]);
  EIOKU_TRY(ensure_lanes(m, B));
  std::vector<int> head((size_t)B * P);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < P; ++t) head[(size_t)b * P + t] = ids[(size_t)b * T + t];
  DevBuf<int> d_head;
  DevBuf<float> d_out;
  EIOKU_TRY(d_head.grow(head.size()));
  EIOKU_TRY(d_out.grow((size_t)B * T * V));
  const std::vector<LaneState> st(B, kFreshLane);
  EIOKU_HIP_CHECK(hipMemcpy(m->state, st.data(), (size_t)B * sizeof(LaneState), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->d_ids, ids, (size_t)B * T * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(d_head, head.data(), head.size() * sizeof(int), hipMemcpyHostToDevice));
  reset_counts(m);
  EIOKU_TRY(prefill(m, B, P, d_head, nullptr, 1, 1));
  for (int b = 0; b < B; ++b) {  // the logits of row b's P positions: out[b][0 .. P - 1]; outside the launch and flop counts
    hipLaunchKernelGGL((k_logits<false>), dim3(m->nblk), dim3(256), 0, 0, m->pw.h + (size_t)b * P * m->cfg.d_model, m->cfg.d_model,
                       m->H(m->emb), nullptr, P, m->sel, m->flags, m->state, 0, m->ppartial, m->nblk, d_out + (size_t)b * T * V,
                       (long long)V, nullptr, nullptr, m->nlang, 0, 1.f, nullptr, nullptr, 0);
    EIOKU_LAUNCH_CHECK();
  }
  EIOKU_TRY(walked_logits(m, B, T, P, d_out));  // the positions after the prefill walk on its keys and values
  EIOKU_HIP_CHECK(hipMemcpy(out, d_out, (size_t)B * T * V * sizeof(float), hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

int eioku_whisper_select(eioku_whisper* m, const float* logits_in, int B, const int32_t* prefix, int prefix_cap,
                         const int32_t* prefix_len, int32_t* token_out, float* logprob_out, float* masked_out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && logits_in && B > 0 && B <= 64 && prefix_len && token_out && logprob_out && prefix_cap >= 0, "bad argument");
  EIOKU_TRY(ensure_capacity(m, B));
  EIOKU_TRY(upload_prefix_states(m, B, prefix, prefix_cap, prefix_len));
  const size_t V = m->cfg.vocab;
  DevBuf<float> d_msk;
  if (masked_out) EIOKU_TRY(d_msk.grow(B * V));
  auto launch = [&](const float* d_in) -> int {
    LogitsArgs a;
    a.supplied = d_in, a.masked = d_msk;
    EIOKU_TRY(logits<SEL_GREEDY>(m, B, a));
    hipLaunchKernelGGL(k_select, dim3(B), dim3(64), 0, 0, m->partial, m->nblk, m->sel, m->state, 1, 0, 0, m->info, m->nlang, m->lang_ids,
                       (int*)nullptr, 0, m->cur_tok, m->nsp, m->lang_out, m->d_logprob);
    EIOKU_LAUNCH_CHECK();
    return EIOKU_OK;
  };
  return on_supplied_logits(m, logits_in, B, launch, {{token_out, m->cur_tok, B * sizeof(int)}, {logprob_out, m->d_logprob, B * sizeof(float)},
                                                      {masked_out, d_msk, B * V * sizeof(float)}});
}

int eioku_whisper_sample(eioku_whisper* m, const float* logits_in, int B, const int32_t* prefix, int prefix_cap,
                         const int32_t* prefix_len, float temperature, const uint64_t* seeds, const int32_t* idx, int32_t* token_out,
                         float* logprob_out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && logits_in && B > 0 && B <= 64 && prefix_len && seeds && idx && token_out && logprob_out && prefix_cap >= 0,
                "bad argument");
  EIOKU_REQUIRE(temperature > 0.f && std::isfinite(temperature), "temperature %g must be a finite number > 0", (double)temperature);
  EIOKU_TRY(ensure_capacity(m, B));
  for (int b = 0; b < B; ++b)
    EIOKU_REQUIRE(idx[b] >= 0 && idx[b] < m->cfg.max_target_positions, "sample index %d outside 0..%d", idx[b],
                  m->cfg.max_target_positions - 1);
  EIOKU_TRY(upload_prefix_states(m, B, prefix, prefix_cap, prefix_len));
  EIOKU_HIP_CHECK(hipMemcpy(m->d_seeds, seeds, (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->d_sidx, idx, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
  auto launch = [&](const float* d_in) -> int {
    LogitsArgs a;
    a.supplied = d_in, a.temp = temperature, a.sidx = m->d_sidx;
    EIOKU_TRY(logits<SEL_SAMPLE>(m, B, a));
    hipLaunchKernelGGL(k_sample_select, dim3(B), dim3(64), 0, 0, m->partial, m->nblk, m->sel, m->state, 0, (int*)nullptr, 0, m->cur_tok,
                       m->d_logprob);
    EIOKU_LAUNCH_CHECK();
    return EIOKU_OK;
  };
  return on_supplied_logits(m, logits_in, B, launch, {{token_out, m->cur_tok, B * sizeof(int)}, {logprob_out, m->d_logprob, B * sizeof(float)}});
}

namespace {

int beam_args(const eioku_whisper* m, int B, int W, int C) {
  EIOKU_REQUIRE(W >= 1 && W <= kMaxBeam, "beam size %d outside 1..%d", W, kMaxBeam);
  EIOKU_REQUIRE(C >= 1 && C <= kMaxFinish, "%d finished hypotheses outside 1..%d (round(beam * patience))", C, kMaxFinish);
  EIOKU_REQUIRE(B > 0 && B * W <= 64, "%d windows x beam %d = %d lanes: at most 64 lanes decode in lockstep", B, W, B * W);
  return EIOKU_OK;
}

int beam_select(eioku_whisper* m, int B, int W, int C, int s, int idx, const uint8_t* anc, uint8_t* anc_next, const int* hist,
                int* hist_next, int* out_src, int* out_tok) {
  const int Tm = m->cfg.max_target_positions;  // out_src / out_tok NULL: no per-slot outputs
  hipLaunchKernelGGL(k_beam_select, dim3(B), dim3(64 * W), 0, 0, m->bpartial, m->nblk, m->sel, W, C, s, idx, m->state, m->cur_tok, anc,
                     anc_next, Tm, hist, hist_next, Tm, m->fin_tok, m->fin_sum, m->fin_n, m->fin_count, m->complete, out_src, out_tok,
                     m->b_sum, out_src ? m->b_nlive.p : nullptr, m->b_fsrc, m->b_fsum, m->b_nfin);
  return launched(m);
}

// The beam search behind both entries.  prefill = false: `prompt` [prompt_len] is shared and every lane walks it position by
// position.  prefill = true: `prompt` is [B][prompt_len], one prefill per window fills slot 0's cache, the ancestry table
// names that lane for every prompt position, the no-speech probability comes from position sot_index (per window, not per
// lane), and row b reads encoded window windows[b].
int beam_impl(eioku_whisper* m, const int32_t* prompt, int prompt_len, bool pre, int sot_index, const int32_t* windows, int B, int W,
              int C, int max_new, int sync_every, int32_t* tokens_out, int32_t* n_out, int32_t* ended_out, float* sum_logprob,
              int32_t* n_hyp, int32_t* best_out, float* no_speech_prob, int32_t* lang_out, int32_t* trace_src, int32_t* trace_tok) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && prompt && prompt_len >= 1 && max_new >= 1, "bad argument");
  EIOKU_TRY(beam_args(m, B, W, C));
  if (!pre) {
    EIOKU_REQUIRE(B == m->enc_B, "beam decode of %d windows needs an encode of the same %d windows first", B, m->enc_B);
    EIOKU_REQUIRE(prompt_len + max_new <= m->cfg.max_target_positions, "prompt %d + %d new tokens exceed max_target_positions %d",
                  prompt_len, max_new, m->cfg.max_target_positions);
  }
  EIOKU_REQUIRE(tokens_out && n_out && ended_out && sum_logprob && n_hyp && best_out, "NULL output");
  if (!pre)
    for (int i = 0; i < prompt_len; ++i)
      EIOKU_REQUIRE(prompt[i] >= 0 && prompt[i] < m->cfg.vocab, "prompt id %d outside the vocabulary", prompt[i]);
  if (sync_every < 1) sync_every = 1;
  const int L = B * W, Tm = m->cfg.max_target_positions, eot = m->cfg.eot, H = W > C ? W : C;
  EIOKU_TRY(ensure_beam(m, B, L));
  if (pre) EIOKU_TRY(prompted_args(m, prompt, prompt_len, sot_index, windows, B, W, max_new));
  const int* lane_map = pre ? m->kvmap + m->dcap : nullptr;
  reset_counts(m);
  // slot 0 of every window is live with sum 0, the others are dead; every ancestry row names its own lane
  std::vector<LaneState> st(L, LaneState{0, -1, -1, -1, 1, kNegInf});
  for (int b = 0; b < B; ++b) st[(size_t)b * W] = kFreshLane;
  std::vector<uint8_t> ident((size_t)L * Tm);
  for (int l = 0; l < L; ++l)
    for (int t = 0; t < Tm; ++t) ident[(size_t)l * Tm + t] = (uint8_t)((pre && t < prompt_len) ? l / W * W : l);
  std::vector<int> fill((size_t)L * Tm, eot), zeros(B, 0);
  EIOKU_HIP_CHECK(hipMemcpy(m->state, st.data(), (size_t)L * sizeof(LaneState), hipMemcpyHostToDevice));
  for (int i = 0; i < 2; ++i) {
    EIOKU_HIP_CHECK(hipMemcpy(m->anc[i], ident.data(), ident.size(), hipMemcpyHostToDevice));
    EIOKU_HIP_CHECK(hipMemcpy(m->hist[i], fill.data(), fill.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  EIOKU_HIP_CHECK(hipMemcpy(m->fin_count, zeros.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->complete, zeros.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
  const bool trace = trace_src && trace_tok;
  if (trace) {
    EIOKU_HIP_CHECK(hipMemset(m->tr_src, 0xFF, (size_t)L * Tm * sizeof(int)));
    EIOKU_HIP_CHECK(hipMemset(m->tr_tok, 0xFF, (size_t)L * Tm * sizeof(int)));
  }
  int cur = 0;
  std::vector<int> flags(B);
  // prefilled: the prompt in one pass per window; every slot starts from the window's hidden state at the last prompt position
  EIOKU_TRY(start(m, Start{prompt, prompt_len, pre, sot_index, prompt_len, true, nullptr, nullptr}, B, W, 1, W, m->anc[cur]));
  LogitsArgs beam;
  beam.nc = W + 1;
  for (int idx = 0; idx < max_new; ++idx) {
    const int s = prompt_len - 1 + idx;
    if (idx > 0) {
      EIOKU_TRY(decoder_step(m, L, s, m->cur_tok, 1, 0, W, m->anc[cur], lane_map));
      m->steps += 1;
    }
    EIOKU_TRY(logits<SEL_BEAM>(m, L, beam));
    EIOKU_TRY(beam_select(m, B, W, C, s, idx, m->anc[cur], m->anc[cur ^ 1], m->hist[cur], m->hist[cur ^ 1],
                      trace ? m->tr_src + (size_t)idx * L : nullptr, trace ? m->tr_tok + (size_t)idx * L : nullptr));
    cur ^= 1;
    if ((idx + 1) % sync_every == 0 && idx + 1 < max_new) {  // stop once every window is complete
      EIOKU_HIP_CHECK(hipMemcpy(flags.data(), m->complete, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
      bool all = true;
      for (int b = 0; b < B; ++b) all = all && flags[b];
      if (all) break;
    }
  }
  // hypotheses: the finished records, then live slots in slot order while there are fewer than W
  std::vector<int> hist((size_t)L * Tm), ftok((size_t)B * kMaxFinish * Tm), fn((size_t)B * kMaxFinish), fc(B);
  std::vector<float> fsum((size_t)B * kMaxFinish), nsp(L);
  std::vector<int> lang(L);
  EIOKU_HIP_CHECK(hipMemcpy(st.data(), m->state, (size_t)L * sizeof(LaneState), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(hist.data(), m->hist[cur], hist.size() * sizeof(int), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(ftok.data(), m->fin_tok, ftok.size() * sizeof(int), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(fn.data(), m->fin_n, fn.size() * sizeof(int), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(fsum.data(), m->fin_sum, fsum.size() * sizeof(float), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(fc.data(), m->fin_count, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(nsp.data(), m->nsp, (size_t)L * sizeof(float), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(lang.data(), m->lang_out, (size_t)L * sizeof(int), hipMemcpyDeviceToHost));
  if (trace) {
    EIOKU_HIP_CHECK(hipMemcpy(trace_src, m->tr_src, (size_t)max_new * L * sizeof(int), hipMemcpyDeviceToHost));
    EIOKU_HIP_CHECK(hipMemcpy(trace_tok, m->tr_tok, (size_t)max_new * L * sizeof(int), hipMemcpyDeviceToHost));
  }
  for (int b = 0; b < B; ++b) {
    int rows = 0, best = 0;
    double best_score = 0;
    auto put = [&](const int* toks, int n_text, bool ended, float sum) {
      const size_t row = (size_t)b * H + rows;
      int32_t* out = tokens_out + row * max_new;
      for (int t = 0; t < max_new; ++t) out[t] = t < n_text ? toks[t] : eot;
      n_out[row] = n_text + (ended ? 1 : 0);
      ended_out[row] = ended ? 1 : 0;
      sum_logprob[row] = sum;
      const double score = (double)sum / (n_text > 1 ? n_text : 1);
      if (rows == 0 || score > best_score) best = rows, best_score = score;
      ++rows;
    };
    const int nfin = fc[b] < C ? fc[b] : C;
    for (int i = 0; i < nfin && rows < H; ++i) {
      const size_t r = (size_t)b * kMaxFinish + i;
      const int n_text = fn[r] < max_new ? fn[r] : max_new;
      put(ftok.data() + r * Tm, n_text, true, fsum[r]);
    }
    for (int j = 0; j < W && rows < W; ++j) {
      const LaneState& ls = st[(size_t)b * W + j];
      if (!(ls.sum > kNegInf)) continue;
      put(hist.data() + ((size_t)b * W + j) * Tm, ls.n < max_new ? ls.n : max_new, false, ls.sum);
    }
    n_hyp[b] = rows;
    best_out[b] = best;
    for (; rows < H; ++rows) {
      const size_t row = (size_t)b * H + rows;
      for (int t = 0; t < max_new; ++t) tokens_out[row * max_new + t] = eot;
      n_out[row] = 0, ended_out[row] = 0, sum_logprob[row] = kNegInf;
    }
    // the prefilled start leaves one no-speech probability per window, the walked one per lane: slot 0's
    if (no_speech_prob) no_speech_prob[b] = nsp[pre ? (size_t)b : (size_t)b * W];
    if (lang_out) lang_out[b] = lang[pre ? (size_t)b : (size_t)b * W];
  }
  return EIOKU_OK;
}

}  // namespace

int eioku_whisper_decode_beam(eioku_whisper* m, const int32_t* prompt, int prompt_len, int B, int W, int C, int max_new,
                              int sync_every, int32_t* tokens_out, int32_t* n_out, int32_t* ended_out, float* sum_logprob,
                              int32_t* n_hyp, int32_t* best_out, float* no_speech_prob, int32_t* lang_out, int32_t* trace_src,
                              int32_t* trace_tok) {
  return beam_impl(m, prompt, prompt_len, false, 0, nullptr, B, W, C, max_new, sync_every, tokens_out, n_out, ended_out, sum_logprob,
                   n_hyp, best_out, no_speech_prob, lang_out, trace_src, trace_tok);
}

int eioku_whisper_decode_beam_prompted(eioku_whisper* m, const int32_t* prompts, int P, int sot_index, const int32_t* windows, int B,
                                       int W, int C, int max_new, int sync_every, int32_t* tokens_out, int32_t* n_out,
                                       int32_t* ended_out, float* sum_logprob, int32_t* n_hyp, int32_t* best_out, float* no_speech_prob,
                                       int32_t* trace_src, int32_t* trace_tok) {
  return beam_impl(m, prompts, P, true, sot_index, windows, B, W, C, max_new, sync_every, tokens_out, n_out, ended_out, sum_logprob,
                   n_hyp, best_out, no_speech_prob, nullptr, trace_src, trace_tok);
}

int eioku_whisper_beam_select(eioku_whisper* m, const float* logits_in, int B, int W, int C, const int32_t* prefix, int prefix_cap,
                              const int32_t* prefix_len, const float* sums, const int32_t* fin_count, int32_t* src_out,
                              int32_t* tok_out, float* sum_out, int32_t* n_live, int32_t* fsrc_out, float* fsum_out,
                              int32_t* n_fin, int32_t* fin_count_out, int32_t* complete_out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && logits_in && prefix_len && sums && fin_count && prefix_cap >= 0, "bad argument");
  EIOKU_REQUIRE(src_out && tok_out && sum_out && n_live && fsrc_out && fsum_out && n_fin && fin_count_out && complete_out, "NULL output");
  EIOKU_TRY(beam_args(m, B, W, C));
  const int L = B * W;
  EIOKU_TRY(ensure_beam(m, B, L));
  for (int b = 0; b < B; ++b) EIOKU_REQUIRE(fin_count[b] >= 0 && fin_count[b] < C, "finished count %d outside 0..%d", fin_count[b], C - 1);
  EIOKU_TRY(upload_prefix_states(m, L, prefix, prefix_cap, prefix_len, sums));
  const std::vector<int> zeros(B, 0);
  EIOKU_HIP_CHECK(hipMemcpy(m->fin_count, fin_count, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->complete, zeros.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
  auto launch = [&](const float* d_in) -> int {
    LogitsArgs a;
    a.supplied = d_in, a.nc = W + 1;
    EIOKU_TRY(logits<SEL_BEAM>(m, L, a));
    return beam_select(m, B, W, C, 0, 0, nullptr, nullptr, nullptr, nullptr, m->b_src, m->b_tok);
  };
  const size_t li = (size_t)L * sizeof(int), lf = (size_t)L * sizeof(float), bi = (size_t)B * sizeof(int);
  return on_supplied_logits(m, logits_in, L, launch,
                            {{src_out, m->b_src, li}, {tok_out, m->b_tok, li}, {sum_out, m->b_sum, lf}, {fsrc_out, m->b_fsrc, li},
                             {fsum_out, m->b_fsum, lf}, {n_live, m->b_nlive, bi}, {n_fin, m->b_nfin, bi},
                             {fin_count_out, m->fin_count, bi}, {complete_out, m->complete, bi}});
}

// ---- word alignment (K21) ----------------------------------------------------------------------------------------------------
extern "C++" {
namespace {

constexpr int kMaxDtw = 4096;  // token rows / frames the debug DTW entry takes

// mean / std over the token rows, then the cost; meta on the device: n_tok [R], nF [R]
int align_cost_launch(eioku_whisper* m, const float* A, int R, int H, int T, int ldf, int S, const int* d_ntok, const int* d_nF,
                      int Nmax, float* cost) {
  EIOKU_TRY(m->al_stat.grow((size_t)R * H * 2 * ldf));
  hipLaunchKernelGGL(k_align_stats, dim3((ldf + 255) / 256, H, R), dim3(256), 0, 0, A, H, T, ldf, d_ntok, d_nF, m->al_stat);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_align_cost, dim3((ldf + 255) / 256, Nmax, R), dim3(256), 0, 0, A, m->al_stat, H, T, ldf, S, d_ntok, d_nF, Nmax,
                     cost);
  EIOKU_LAUNCH_CHECK();
  m->launches += 2;
  return EIOKU_OK;
}

int dtw_launch(eioku_whisper* m, const float* cost, int R, int Nmax, int ldf, const int* d_nN, const int* d_nF, int* jump, int* path,
               int* path_len) {
  const int tw = (ldf + 15) / 16;
  EIOKU_TRY(m->al_trace.grow((size_t)R * Nmax * tw));
  hipLaunchKernelGGL(k_dtw, dim3(R), dim3(kDtwRows), (size_t)ldf * sizeof(float), 0, cost, Nmax, ldf, d_nN, d_nF, m->al_trace, tw, jump,
                     path, path_len);
  return launched(m);
}

}  // namespace
}  // extern "C++"

int eioku_whisper_set_alignment_heads(eioku_whisper* m, const int32_t* layer_head_pairs, int n) {
  EIOKU_REQUIRE(m && n >= 0 && (layer_head_pairs || n == 0), "bad argument");
  EIOKU_REQUIRE(n <= m->cfg.dec_layers * m->cfg.heads, "%d alignment heads: the decoder has %d", n, m->cfg.dec_layers * m->cfg.heads);
  for (int i = 0; i < n; ++i) {
    const int l = layer_head_pairs[2 * i], h = layer_head_pairs[2 * i + 1];
    EIOKU_REQUIRE(l >= 0 && l < m->cfg.dec_layers && h >= 0 && h < m->cfg.heads,
                  "alignment head (%d, %d) outside the decoder's %d layers x %d heads", l, h, m->cfg.dec_layers, m->cfg.heads);
  }
  m->align_heads.assign(layer_head_pairs, layer_head_pairs + 2 * (size_t)n);
  return EIOKU_OK;
}

int eioku_whisper_align(eioku_whisper* m, const int32_t* seq, int T, const int32_t* n_tok, int sot_len, const int32_t* windows,
                        const int32_t* n_frames, int R, int32_t* jump_out, float* prob_out, float* cost_out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && seq && n_tok && n_frames && jump_out && prob_out && sot_len >= 1, "bad argument");
  reset_counts(m);
  const auto& c = m->cfg;
  const int ctx = c.max_source_positions, d = c.d_model, S = sot_len;
  EIOKU_REQUIRE(R > 0 && R <= 64, "%d rows: an alignment pass takes 1..64", R);
  EIOKU_REQUIRE(T >= 1 && T <= c.max_target_positions, "sequence of %d tokens exceeds max_target_positions %d", T, c.max_target_positions);
  EIOKU_REQUIRE(m->enc_B > 0, "an alignment needs an encode first");
  if (!windows) EIOKU_REQUIRE(R == m->enc_B, "alignment of %d rows without a window list needs an encode of the same %d windows", R, m->enc_B);
  int Fmax = 0;
  size_t Mp = 0;
  for (int r = 0; r < R; ++r) {
    EIOKU_REQUIRE(!windows || (windows[r] >= 0 && windows[r] < m->enc_B), "window %d outside the %d encoded windows", windows[r], m->enc_B);
    EIOKU_REQUIRE(n_tok[r] >= S + 3 && n_tok[r] <= T, "row %d: %d tokens; an alignment needs sot_len %d + <|notimestamps|> + at least one "
                  "text token + EOT, within T = %d", r, n_tok[r], S, T);
    EIOKU_REQUIRE(n_frames[r] >= 2 && n_frames[r] <= 2 * ctx, "row %d: %d mel frames outside 2..%d", r, n_frames[r], 2 * ctx);
    for (int t = 0; t < T; ++t) {
      const int id = seq[(size_t)r * T + t];
      EIOKU_REQUIRE(id >= 0 && id < c.vocab, "id %d outside the vocabulary", id);
      if (t > S && t < n_tok[r] - 1) EIOKU_REQUIRE(id < c.eot, "row %d position %d: id %d is not a text token (< %d)", r, t, id, c.eot);
    }
    Fmax = n_frames[r] / 2 > Fmax ? n_frames[r] / 2 : Fmax;
    Mp += (size_t)(n_tok[r] - S - 2);
  }
  EIOKU_TRY(m->check());
  std::vector<int> heads = m->align_heads;
  if (heads.empty())
    for (int l = c.dec_layers / 2; l < c.dec_layers; ++l)
      for (int h = 0; h < c.heads; ++h) heads.push_back(l), heads.push_back(h);
  const int Hs = (int)heads.size() / 2, Nmax = T - S - 1, nblk = (c.eot + 63) / 64;
  EIOKU_REQUIRE(Hs > 0 && nblk > 0, "no alignment heads");
  EIOKU_TRY(ensure_lanes(m, R));
  // host lists: kvmap [R]; meta = n_tok, nF, nN [R each]; rows = hidden row, target id, output index [Mp each]
  std::vector<int> map((size_t)R), meta((size_t)3 * R), rows(3 * Mp);
  size_t k = 0;
  for (int r = 0; r < R; ++r) {
    map[r] = windows ? windows[r] : r;
    meta[r] = n_tok[r], meta[R + r] = n_frames[r] / 2, meta[2 * R + r] = n_tok[r] - S - 1;
    for (int i = 0; i < n_tok[r] - S - 2; ++i, ++k) {
      rows[k] = r * T + S + i;
      rows[Mp + k] = seq[(size_t)r * T + S + i + 1];
      rows[2 * Mp + k] = r * Nmax + i;
    }
  }
  const size_t nA = (size_t)R * Hs * T * Fmax, nC = (size_t)R * Nmax * Fmax, nJ = (size_t)R * Nmax;
  EIOKU_TRY(m->al_A.grow(nA));
  EIOKU_TRY(m->al_cost.grow(nC));
  EIOKU_TRY(m->al_jump.grow(nJ));
  EIOKU_TRY(m->al_prob.grow(nJ));
  EIOKU_TRY(m->al_meta.grow(meta.size()));
  EIOKU_TRY(m->al_rows.grow(rows.size()));
  EIOKU_TRY(m->al_part.grow(Mp * nblk * 2));
  EIOKU_TRY(m->al_tgt.grow(Mp));
  EIOKU_HIP_CHECK(hipMemcpy(m->kvmap, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->d_ids, seq, (size_t)R * T * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->al_meta, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->al_rows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemset(m->al_cost, 0, nC * sizeof(float)));
  EIOKU_HIP_CHECK(hipMemset(m->al_jump, 0xFF, nJ * sizeof(int)));
  EIOKU_HIP_CHECK(hipMemset(m->al_prob, 0, nJ * sizeof(float)));
  const int *d_ntok = m->al_meta, *d_nF = m->al_meta + R, *d_nN = m->al_meta + 2 * R;
  DevEvents ev;  // the four events that bracket the three stages: destroyed with the scope
  EIOKU_TRY(ev.ensure(4));
  EIOKU_TRY(ev.record(0, 0));
  const AlignCapture cap{heads.data(), Hs, Fmax, d_nF, m->al_A};
  EIOKU_TRY(prefill(m, R, T, m->d_ids, m->kvmap, 1, 1, &cap));
  hipLaunchKernelGGL(k_align_logits, dim3(nblk), dim3(256), 0, 0, m->pw.h, d, m->H(m->emb), m->al_rows, m->al_rows + Mp, (int)Mp, c.eot,
                     m->al_part, nblk, m->al_tgt);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_align_prob, dim3((unsigned)Mp), dim3(64), 0, 0, m->al_part, nblk, m->al_tgt, m->al_rows + 2 * Mp, m->al_prob);
  EIOKU_LAUNCH_CHECK();
  m->flops += 2.0 * (double)Mp * c.eot * d;
  m->launches += 2;
  EIOKU_TRY(ev.record(1, 0));
  EIOKU_TRY(align_cost_launch(m, m->al_A, R, Hs, T, Fmax, S, d_ntok, d_nF, Nmax, m->al_cost));
  EIOKU_TRY(ev.record(2, 0));
  EIOKU_TRY(dtw_launch(m, m->al_cost, R, Nmax, Fmax, d_nN, d_nF, m->al_jump, nullptr, nullptr));
  EIOKU_TRY(ev.record(3, 0));
  for (int i = 0; i < 3; ++i) EIOKU_TRY(ev.ms(i, i + 1, &m->align_ms[i]));  // waits for each stage's end
  EIOKU_HIP_CHECK(hipMemcpy(jump_out, m->al_jump, nJ * sizeof(int), hipMemcpyDeviceToHost));
  EIOKU_HIP_CHECK(hipMemcpy(prob_out, m->al_prob, nJ * sizeof(float), hipMemcpyDeviceToHost));
  if (cost_out) EIOKU_HIP_CHECK(hipMemcpy(cost_out, m->al_cost, nC * sizeof(float), hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

int eioku_whisper_align_cost(eioku_whisper* m, const float* A, int H, int T, int F, int sot_len, float* cost_out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && A && cost_out, "bad argument");
  EIOKU_REQUIRE(H >= 1 && H <= 4096 && F >= 1 && F <= kMaxDtw && sot_len >= 0 && T >= sot_len + 2 && T <= kMaxDtw,
                "align_cost: H %d, T %d, F %d, sot_len %d (T >= sot_len + 2, T and F <= %d)", H, T, F, sot_len, kMaxDtw);
  m->launches = 0;
  const int N = T - sot_len - 1;
  const int meta[2] = {T, F};
  EIOKU_TRY(m->al_A.grow((size_t)H * T * F));
  EIOKU_TRY(m->al_cost.grow((size_t)N * F));
  EIOKU_TRY(m->al_meta.grow(2));
  EIOKU_HIP_CHECK(hipMemcpy(m->al_A, A, (size_t)H * T * F * sizeof(float), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->al_meta, meta, sizeof(meta), hipMemcpyHostToDevice));
  EIOKU_TRY(align_cost_launch(m, m->al_A, 1, H, T, F, sot_len, m->al_meta, m->al_meta + 1, N, m->al_cost));
  EIOKU_HIP_CHECK(hipMemcpy(cost_out, m->al_cost, (size_t)N * F * sizeof(float), hipMemcpyDeviceToHost));
  return EIOKU_OK;
}

int eioku_whisper_dtw(eioku_whisper* m, const float* cost, int N, int F, int32_t* jump_out, int32_t* text_idx, int32_t* time_idx,
                      int* path_len) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && cost && jump_out, "bad argument");
  EIOKU_REQUIRE((text_idx && time_idx && path_len) || (!text_idx && !time_idx && !path_len), "the path outputs come together or not at all");
  EIOKU_REQUIRE(N >= 1 && N <= kMaxDtw && F >= 1 && F <= kMaxDtw, "dtw of %d token rows x %d frames: both 1..%d", N, F, kMaxDtw);
  m->launches = 0;
  const int meta[2] = {N, F};
  EIOKU_TRY(m->al_cost.grow((size_t)N * F));
  EIOKU_TRY(m->al_jump.grow((size_t)N));
  EIOKU_TRY(m->al_meta.grow(3));
  EIOKU_TRY(m->al_path.grow((size_t)2 * (N + F)));
  EIOKU_HIP_CHECK(hipMemcpy(m->al_cost, cost, (size_t)N * F * sizeof(float), hipMemcpyHostToDevice));
  EIOKU_HIP_CHECK(hipMemcpy(m->al_meta, meta, sizeof(meta), hipMemcpyHostToDevice));
  EIOKU_TRY(dtw_launch(m, m->al_cost, 1, N, F, m->al_meta, m->al_meta + 1, m->al_jump, m->al_path, m->al_meta + 2));
  EIOKU_HIP_CHECK(hipMemcpy(jump_out, m->al_jump, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
  if (path_len) {
    int n = 0;
    EIOKU_HIP_CHECK(hipMemcpy(&n, m->al_meta + 2, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> p((size_t)2 * (N + F));
    EIOKU_HIP_CHECK(hipMemcpy(p.data(), m->al_path, p.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) text_idx[i] = p[n - 1 - i], time_idx[i] = p[(size_t)N + F + n - 1 - i];
    *path_len = n;
  }
  return EIOKU_OK;
}

int eioku_whisper_last_align_ms(const eioku_whisper* m, double* pass_ms, double* cost_ms, double* dtw_ms) {
  EIOKU_REQUIRE(m && pass_ms && cost_ms && dtw_ms, "NULL argument");
  *pass_ms = m->align_ms[0], *cost_ms = m->align_ms[1], *dtw_ms = m->align_ms[2];
  return EIOKU_OK;
}

int eioku_whisper_last_flops(const eioku_whisper* m, double* flops) {
  EIOKU_REQUIRE(m && flops, "NULL argument");
  *flops = m->flops;
  return EIOKU_OK;
}

int eioku_whisper_last_launches(const eioku_whisper* m, int* launches, int* steps) {
  EIOKU_REQUIRE(m && launches && steps, "NULL argument");
  *launches = m->launches;
  *steps = m->steps;
  return EIOKU_OK;
}

}  // extern "C"

