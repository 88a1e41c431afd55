// K25: action recognition on gfx950 - TimeSformer with divided space-time attention (DESIGN.md "K25 action recognition").
//   k_clip_resize_h / k_clip_resize_v   (clip_resize.h, shared with clip.hip) Pillow's two-pass 8-bit bilinear resample of the
//                       centre-crop region only (22-bit fixed-point taps from the host, uint8 rounding between the passes), then BGR -> RGB,
//                       (v * (1 / 255) - mean) / std in fp32 and one rounding to fp16, written as patch rows
//                       [clip][patch][frame][c * 256 + ky * 16 + kx]: the patch embedding is one GEMM, no im2col pass
//   k_gemm<., EPI_POS>  (gemm_f16.h) patch projection + bias + (position + time) table into the fp32 residual stream
//   k_ln<h16>           (layernorm.h) LayerNorm, fp32 row -> fp16
//   k_attn_time         temporal attention: T <= 96 keys of one (clip, patch, head) per one-wave workgroup, q / k / v in LDS,
//                       fp32 scores
//   k_attn_tiles<SpaceTimeSeq, false>  (attn_f16.h) spatial attention: 1 + P keys of one (clip, frame, head); 64 queries per
//                       workgroup, keys / values staged through LDS 128 at a time, QK^T and PV on v_mfma_f32_16x16x32_f16
//                       with an online softmax
//   k_cls_mean          the CLS rule: mean over the frames (t = 0 .. T - 1, fp32) of the projected CLS outputs, added to CLS
//   k_action_head       softmax and top-k of the logits (block_argmax_256, layernorm.h), ties to the smaller class index
// The launch wrappers, the activation buffers and the MLP sublayer (LN -> fc1 + GELU -> fc2 EPI_RESID) are encoder.h's.
// Residual stream x, fp32: the B P T patch rows first, row (b P + p) T + t, then the B CLS rows.  The temporal GEMMs see the
// first B P T rows as one dense matrix, the spatial qkv and the MLP all B (P T + 1) rows; the CLS row of a clip goes
// through LayerNorm and qkv once for all its T frames.
// Precision points (tests/actions_oracle.py, fp16=True, rounds at the same places): linear / conv weights fp16; biases,
// LayerNorm parameters and the embedding tables fp32; the residual stream fp32; LayerNorm outputs, q / k / v, attention
// outputs, the temporal out-projection, GELU outputs and the patch rows are rounded to fp16; the spatial kernel rounds
// its softmax numerators exp(s - max) to fp16 for the PV MFMA.
#include "clip_resize.h"
#include "common.h"
#include "encoder.h"

#include <cmath>
#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kPatch = 16, kPatchK = 3 * kPatch * kPatch;
constexpr int kMaxFrames = 96, kMaxImage = 448;

// ---- clip preprocessing: k_clip_resize_h / k_clip_resize_v and their launch, clip_resize.h ----------------------------------

// ---- small kernels ------------------------------------------------------------------------------------------------------
// the embedding tables the GEMM epilogue and the CLS rows read: postime[p T + t] = position[1 + p] + time[t],
// cls = cls_token + position[0]
__global__ __launch_bounds__(256) void k_embed_tables(const float* __restrict__ pos, const float* __restrict__ time,
                                                      const float* __restrict__ cls_token, int P, int T, int d,
                                                      float* __restrict__ postime, float* __restrict__ cls) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n = (size_t)P * T * d;
  if (i < n) {
    const int c = (int)(i % d);
    const size_t row = i / d;
    const int t = (int)(row % T), p = (int)(row / T);
    postime[i] = pos[(size_t)(1 + p) * d + c] + time[(size_t)t * d + c];
  } else if (i < n + d) {
    const int c = (int)(i - n);
    cls[c] = cls_token[c] + pos[c];
  }
}

// x[first + b][:] = cls[:] for b < B
__global__ __launch_bounds__(256) void k_cls_rows(const float* __restrict__ cls, int B, int d, float* __restrict__ x) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)B * d) x[i] = cls[i % d];
}

// the CLS rule: x_cls[b] += (sum over t = 0 .. T - 1 of proj[b T + t]) / T, in fp32 and in frame order
__global__ __launch_bounds__(256) void k_cls_mean(const float* __restrict__ proj, int B, int T, int d, float* __restrict__ x_cls) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * d) return;
  const int c = (int)(i % d), b = (int)(i / d);
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += proj[((size_t)b * T + t) * d + c];
  x_cls[i] += s / (float)T;
}

// hidden_out [B][1 + P T][d] in the model's token order (CLS, then patch p at frame t in row 1 + p T + t) from the stream
__global__ __launch_bounds__(256) void k_hidden_out(const float* __restrict__ x, int B, int PT, int d, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * (PT + 1) * d) return;
  const int c = (int)(i % d);
  const size_t row = i / d;
  const int tok = (int)(row % (PT + 1)), b = (int)(row / (PT + 1));
  const size_t src = tok == 0 ? (size_t)B * PT + b : (size_t)b * PT + tok - 1;
  out[i] = x[src * d + c];
}

// ---- temporal attention -----------------------------------------------------------------------------------------------------
// qkv [rows][3 d] fp16 (q | k | v, head h in columns 64 h .. 64 h + 63 of each third); sequence s = rows s T .. s T + T - 1.
// grid (n_seq * heads), one wave = one (sequence, head).  q / k / v of the problem sit in LDS (rows of 66 halfs: lane j
// reads key row j without bank conflicts); per query, lane j scores keys j and j + 64, the wave reduces max and sum, and
// lane c accumulates output dimension c.  Dynamic LDS: 3 T 66 halfs + 96 floats (38.4 KB at T = 96).  out [rows][d] fp16.
__global__ __launch_bounds__(64) void k_attn_time(const h16* __restrict__ qkv, int T, int heads, h16* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x;
  const int head = (int)(blockIdx.x % heads);
  const size_t row0 = (size_t)(blockIdx.x / heads) * T;
  const int d = heads * 64;
  h16* sq = reinterpret_cast<h16*>(smem_raw);
  h16* sk = sq + T * 66;
  h16* sv = sk + T * 66;
  float* sp = reinterpret_cast<float*>(sv + T * 66);
  for (int i = lane; i < 3 * T * 8; i += 64) {  // 16-byte pieces: (third, row, piece)
    const int piece = i & 7, t = (i >> 3) % T, third = (i >> 3) / T;
    const uint4 v = *reinterpret_cast<const uint4*>(qkv + (row0 + t) * 3 * d + (size_t)third * d + head * 64 + piece * 8);
    unsigned* dst = reinterpret_cast<unsigned*>(sq + (third * T + t) * 66 + piece * 8);  // 4-byte aligned: 66 and 8 are even
    dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
  }
  __syncthreads();
  for (int qi = 0; qi < T; ++qi) {
    float s[2], mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = lane + 64 * e;
      s[e] = -INFINITY;
      if (j < T) {
        float acc = 0.f;
        for (int c = 0; c < 64; ++c) acc += (float)sq[qi * 66 + c] * (float)sk[j * 66 + c];
        s[e] = acc * 0.125f;
      }
      mx = fmaxf(mx, s[e]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = lane + 64 * e;
      if (j < T) {
        const float p = expf(s[e] - mx);
        sp[j] = p;
        sum += p;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    __syncthreads();
    float o = 0.f;
    for (int j = 0; j < T; ++j) o += sp[j] * (float)sv[j * 66 + lane];
    out[(row0 + qi) * d + head * 64 + lane] = (h16)(o / sum);
    __syncthreads();  // sp is rewritten by the next query
  }
}

// ---- head ---------------------------------------------------------------------------------------------------------------
// one workgroup per clip: probs = softmax(logits) in fp32 (each exponential and their sum computed in fp64 and rounded to
// fp32 once, so neither depends on the order of the sum or on the exp of a math library; one fp32 division), then top_k
// picks of the largest remaining probability, the smaller class index on a tie.  Dynamic LDS: nc floats.
__global__ __launch_bounds__(256) void k_action_head(const float* __restrict__ logits, int nc, int top_k, float* __restrict__ prob_out,
                                                     int* __restrict__ idx_out) {
  extern __shared__ float s_p[];
  __shared__ float s_f[4];
  __shared__ double s_d[4];
  __shared__ int s_i[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = logits + (size_t)b * nc;
  float m = -INFINITY;
  for (int j = tid; j < nc; j += 256) m = fmaxf(m, lg[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) s_f[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
  double sum = 0.0;
  for (int j = tid; j < nc; j += 256) {
    const float e = (float)exp((double)(lg[j] - m));  // the correctly rounded fp32 exponential
    s_p[j] = e;
    sum += (double)e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) s_d[wave] = sum;
  __syncthreads();
  const float total = (float)((s_d[0] + s_d[1]) + (s_d[2] + s_d[3]));
  for (int j = tid; j < nc; j += 256) s_p[j] = s_p[j] / total;
  __syncthreads();
  for (int k = 0; k < top_k; ++k) {
    Best best = block_argmax_256(s_p, nc, -1.f, s_f, s_i);  // -1: below every probability; taken entries are set to -2
    if (best.i >= nc) best.i = 0;  // NaN logits compare false everywhere
    if (tid == 0) {
      prob_out[(size_t)b * top_k + k] = best.v;
      idx_out[(size_t)b * top_k + k] = best.i;
      s_p[best.i] = -2.f;
    }
    __syncthreads();
  }
}

// ---- the model ------------------------------------------------------------------------------------------------------------
struct Layer {
  LNorm t_ln;
  Lin t_qkv, t_out, t_dense;
  EncLayer s;  // spatial attention (ln1, qkv, out) and the MLP (ln2, fc1, fc2)
};

}  // namespace

struct eioku_timesformer : TensorTable {
  int image = 0, frames = 0, d = 0, layers = 0, heads = 0, ffn = 0, labels = 0;
  int side = 0, P = 0;
  float eps = 1e-6f;
  Norm3 nrm{{0.45f, 0.45f, 0.45f}, {0.225f, 0.225f, 0.225f}};
  std::vector<Layer> L;
  int cls_token = 0, pos = 0, time = 0;
  Lin proj{}, classifier{};
  LNorm final_ln{};
  bool tables_ready = false;
  DevBuf<float> postime, cls;
  // preprocessing
  DevBuf<int> tables;
  DevBuf<uint8_t> src, tmp;
  DevBuf<h16> patches;
  // activations of one pass over B clips
  EncWork work;  // a: the B P T patch rows, then the B T per-frame CLS rows
  DevBuf<float> cls_proj, logits, probs;
  DevBuf<int> ids;
  StageClock<3> clock;  // preprocess / encoder / head
  double flops = 0;
};

namespace {

typedef eioku_timesformer Model;

int ensure_batch(Model* m, int B) {
  const size_t PT = (size_t)m->P * m->frames, d = m->d;
  EIOKU_TRY(m->work.grow((size_t)B * (PT + 1), d, m->ffn, (size_t)B * PT + (size_t)B * m->frames));
  EIOKU_TRY(grow_synced(m->cls_proj, (size_t)B * m->frames * d));
  EIOKU_TRY(grow_synced(m->logits, (size_t)B * m->labels));
  EIOKU_TRY(grow_synced(m->probs, (size_t)B * m->labels));
  return grow_synced(m->ids, (size_t)B * m->labels);
}

// patches [B P T][768] fp16 (device) -> the residual stream after every layer in m->work.x
int run_encoder(Model* m, const h16* patches, int B, hipStream_t st) {
  const Enc enc{m, st, m->d, m->eps, &m->flops};
  EncWork& w = m->work;
  const int d = m->d, T = m->frames, P = m->P, PT = P * T, Mp = B * PT, M = Mp + B;
  if (!m->tables_ready) {
    const size_t n = (size_t)PT * d + d;
    hipLaunchKernelGGL(k_embed_tables, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->F(m->pos), m->F(m->time),
                       m->F(m->cls_token), P, T, d, m->postime.p, m->cls.p);
    EIOKU_LAUNCH_CHECK();
    m->tables_ready = true;
  }
  float* x = w.x;
  float* x_cls = x + (size_t)Mp * d;
  EIOKU_TRY((enc.gemm<4, EPI_POS>(patches, kPatchK, m->proj, Mp, d, kPatchK, x, d, m->postime, PT)));
  hipLaunchKernelGGL(k_cls_rows, dim3((unsigned)(((size_t)B * d + 255) / 256)), dim3(256), 0, st, m->cls.p, B, d, x_cls);
  EIOKU_LAUNCH_CHECK();
  h16* a_cls = w.a.p + (size_t)Mp * d;
  for (const Layer& L : m->L) {
    // temporal: patch rows only
    EIOKU_TRY(enc.ln<h16>(x, Mp, L.t_ln, w.h.p));
    EIOKU_TRY((enc.gemm<4, EPI_F16>(w.h, d, L.t_qkv, Mp, 3 * d, d, w.qkv.p, 3 * d)));
    {
      const long long probs = (long long)B * P * m->heads;
      const size_t lds = (size_t)3 * T * 66 * sizeof(h16) + 96 * sizeof(float);
      hipLaunchKernelGGL(k_attn_time, dim3((unsigned)probs), dim3(64), lds, st, w.qkv.p, T, m->heads, w.a.p);
      EIOKU_LAUNCH_CHECK();
      m->flops += 4.0 * probs * T * T * 64;
    }
    EIOKU_TRY((enc.gemm<4, EPI_F16>(w.a, d, L.t_out, Mp, d, d, w.h.p, d)));
    EIOKU_TRY((enc.gemm<4, EPI_RESID>(w.h, d, L.t_dense, Mp, d, d, x, d)));
    // spatial: every row; the CLS row of a clip is normalised and projected once for its T frames
    EIOKU_TRY(enc.ln<h16>(x, M, L.s.ln1, w.h.p));
    EIOKU_TRY((enc.gemm<4, EPI_F16>(w.h, d, L.s.qkv, M, 3 * d, d, w.qkv.p, 3 * d)));
    {
      const int n = 1 + P;
      EIOKU_TRY(launch_attn<false>(st, w.qkv.p, SpaceTimeSeq{B, P, T, d, w.a.p, a_cls}, n, m->heads, B * T));
      m->flops += 4.0 * B * T * m->heads * (double)n * n * 64;
    }
    EIOKU_TRY((enc.gemm<4, EPI_RESID>(w.a, d, L.s.out, Mp, d, d, x, d)));
    EIOKU_TRY((enc.gemm<4, EPI_F32>(a_cls, d, L.s.out, B * T, d, d, m->cls_proj.p, d)));
    hipLaunchKernelGGL(k_cls_mean, dim3((unsigned)(((size_t)B * d + 255) / 256)), dim3(256), 0, st, m->cls_proj.p, B, T, d, x_cls);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY(mlp_sublayer(enc, w, M, L.s.ln2, L.s.fc1, L.s.fc2, m->ffn, false));
  }
  return EIOKU_OK;
}

// final LayerNorm and classifier on the CLS rows; top_k > 0 adds softmax and selection
int run_head(Model* m, int B, int top_k, hipStream_t st) {
  const Enc enc{m, st, m->d, m->eps, &m->flops};
  const int d = m->d;
  const float* x_cls = m->work.x.p + (size_t)B * m->P * m->frames * d;
  EIOKU_TRY(enc.ln<h16>(x_cls, B, m->final_ln, m->work.h.p));
  EIOKU_TRY((enc.gemm<1, EPI_F32>(m->work.h, d, m->classifier, B, m->labels, d, m->logits.p, m->labels)));
  if (top_k > 0) {
    hipLaunchKernelGGL(k_action_head, dim3(B), dim3(256), (size_t)m->labels * sizeof(float), st, m->logits.p, m->labels, top_k,
                       m->probs.p, m->ids.p);
    EIOKU_LAUNCH_CHECK();
  }
  return EIOKU_OK;
}

int preprocess(Model* m, const uint8_t* bgr, int n_clips, int h, int w, const int32_t* xbounds, const int32_t* xk, int kx,
               const int32_t* ybounds, const int32_t* yk, int ky, h16* patches, uint8_t* out_u8, int mem, hipStream_t stream) {
  return clip_resize(bgr, n_clips * m->frames, m->frames, h, w, m->image, xbounds, xk, kx, ybounds, yk, ky, m->nrm, kPatch, 0, kPatchK,
                     patches, out_u8, mem, m->tables, m->src, m->tmp, stream);
}

}  // namespace

extern "C" {

int eioku_timesformer_create(int image, int patch, int frames, int hidden, int layers, int heads, int ffn, int labels, float ln_eps,
                             eioku_timesformer** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL argument");
  EIOKU_REQUIRE(hidden > 0 && heads > 0 && heads * 64 == hidden, "head_dim must be 64 (hidden %d / heads %d)", hidden, heads);
  EIOKU_REQUIRE(patch == kPatch, "patch_size must be 16 (got %d)", patch);
  EIOKU_REQUIRE(image > 0 && image % kPatch == 0 && image <= kMaxImage, "image_size must be a multiple of 16, at most %d (got %d)",
                kMaxImage, image);
  EIOKU_REQUIRE(frames >= 1 && frames <= kMaxFrames, "num_frames must be in [1, %d] (got %d)", kMaxFrames, frames);
  EIOKU_REQUIRE(layers >= 0 && ffn > 0 && ffn % 32 == 0 && labels > 0 && labels <= 16000 && ln_eps > 0.f,
                "bad config (layers %d, ffn %d a multiple of 32, labels %d at most 16000, ln_eps %g)", layers, ffn, labels, (double)ln_eps);
  auto* m = new eioku_timesformer();
  m->image = image, m->frames = frames, m->d = hidden, m->layers = layers, m->heads = heads, m->ffn = ffn, m->labels = labels;
  m->side = image / kPatch, m->P = m->side * m->side, m->eps = ln_eps;
  const int d = hidden;
  const std::string e = "timesformer.embeddings.";
  m->cls_token = m->add(e + "cls_token", 1, d, T_F32);
  m->pos = m->add(e + "position_embeddings", 1 + m->P, d, T_F32);
  m->time = m->add(e + "time_embeddings", frames, d, T_F32);
  m->proj = m->lin(e + "patch_embeddings.projection", d, kPatchK);
  for (int l = 0; l < layers; ++l) {
    const std::string p = "timesformer.encoder.layer." + std::to_string(l) + ".";
    Layer L;
    L.t_ln = m->lnorm(p + "temporal_layernorm", d);
    L.t_qkv = m->lin(p + "temporal_attention.attention.qkv", 3 * d, d);
    L.t_out = m->lin(p + "temporal_attention.output.dense", d, d);
    L.t_dense = m->lin(p + "temporal_dense", d, d);
    L.s.ln1 = m->lnorm(p + "layernorm_before", d);
    L.s.qkv = m->lin(p + "attention.attention.qkv", 3 * d, d);
    L.s.out = m->lin(p + "attention.output.dense", d, d);
    L.s.ln2 = m->lnorm(p + "layernorm_after", d);
    L.s.fc1 = m->lin(p + "intermediate.dense", ffn, d);
    L.s.fc2 = m->lin(p + "output.dense", d, ffn);
    m->L.push_back(L);
  }
  m->final_ln = m->lnorm("timesformer.layernorm", d);
  m->classifier = m->lin("classifier", labels, d);
  auto fail = [&](int rc) {
    eioku_timesformer_destroy(m);
    return rc;
  };
  if (const int rc = m->finish()) return fail(rc);
  if (m->postime.grow((size_t)m->P * frames * d) || m->cls.grow((size_t)d)) return fail(EIOKU_ENOMEM);
  if (const int rc = m->clock.create()) return fail(rc);
  *out = m;
  return EIOKU_OK;
}

void eioku_timesformer_destroy(eioku_timesformer* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  delete m;  // every buffer and event frees itself
}

int eioku_timesformer_num_tensors(const eioku_timesformer* m) { return TensorTable::count(m); }

int eioku_timesformer_tensor_info(const eioku_timesformer* m, int idx, char* name, size_t cap, int* rows, int* cols) {
  return TensorTable::info(m, idx, name, cap, rows, cols);
}

int eioku_timesformer_set_tensor(eioku_timesformer* m, int idx, const float* host, size_t numel) {
  EIOKU_TRY(TensorTable::set(m, idx, host, numel));
  m->tables_ready = false;
  return EIOKU_OK;
}

int eioku_timesformer_set_norm(eioku_timesformer* m, const float* mean_rgb, const float* std_rgb) {
  EIOKU_REQUIRE(m && mean_rgb && std_rgb, "NULL argument");
  for (int c = 0; c < 3; ++c) {
    EIOKU_REQUIRE(std_rgb[c] > 0.f, "image_std must be positive");
    m->nrm.mean[c] = mean_rgb[c], m->nrm.std[c] = std_rgb[c];
  }
  return EIOKU_OK;
}

// n_clips clips of T BGR u8 frames (h x w, [clip][frame][h][w][3], host or device) -> patches_out [n_clips P T][768] fp16
// (device, optional) and / or out_rgb_u8 [n_clips T][S][S][3] (device, optional: the resized and cropped RGB image).  Tables
// from the host (eioku_amd/actions.py): the S rows of Pillow's tables that the centre crop keeps, per axis.
int eioku_timesformer_preprocess(eioku_timesformer* m, const uint8_t* bgr, int n_clips, int h, int w, const int32_t* xbounds,
                                 const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, void* patches_out,
                                 uint8_t* out_rgb_u8, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n_clips >= 0 && h > 0 && w > 0 && kx > 0 && ky > 0 && xbounds && xk && ybounds && yk, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (n_clips == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr, "NULL frames");
  hipStream_t stream = (hipStream_t)stream_;
  EIOKU_TRY(preprocess(m, bgr, n_clips, h, w, xbounds, xk, kx, ybounds, yk, ky, (h16*)patches_out, out_rgb_u8, mem, stream));
  if (mem == EIOKU_MEM_HOST) EIOKU_HIP_CHECK(hipStreamSynchronize(stream));  // the caller may reuse its host buffer
  return EIOKU_OK;
}

// The raw network: patches [n_clips P T][768] fp16 (device) -> logits_out [n_clips][labels] fp32 (device), and optionally
// hidden_out [n_clips][1 + P T][hidden] fp32 (device): the residual stream before the final LayerNorm, in the model's token
// order.  Asynchronous.
int eioku_timesformer_forward(eioku_timesformer* m, const void* patches, int n_clips, float* logits_out, float* hidden_out,
                              void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n_clips >= 0, "bad argument");
  if (n_clips == 0) return EIOKU_OK;
  EIOKU_REQUIRE(patches && logits_out, "NULL buffer");
  EIOKU_TRY(m->check());
  hipStream_t st = (hipStream_t)stream_;
  EIOKU_TRY(ensure_batch(m, n_clips));
  m->flops = 0;
  m->clock.begin(0b110);
  EIOKU_TRY(m->clock.mark(1, st));
  EIOKU_TRY(run_encoder(m, (const h16*)patches, n_clips, st));
  EIOKU_TRY(m->clock.mark(2, st));
  EIOKU_TRY(run_head(m, n_clips, 0, st));
  EIOKU_TRY(m->clock.mark(3, st));
  EIOKU_HIP_CHECK(hipMemcpyAsync(logits_out, m->logits, (size_t)n_clips * m->labels * 4, hipMemcpyDeviceToDevice, st));
  if (hidden_out) {
    const int PT = m->P * m->frames;
    const size_t n = (size_t)n_clips * (PT + 1) * m->d;
    hipLaunchKernelGGL(k_hidden_out, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->work.x.p, n_clips, PT, m->d, hidden_out);
    EIOKU_LAUNCH_CHECK();
  }
  return EIOKU_OK;
}

// detect_actions' per-clip arithmetic on n_clips clips (host or device): resize / crop / normalise -> network -> softmax ->
// top_k by (probability desc, class asc) -> prob_out [n_clips][top_k] fp32, class_out [n_clips][top_k] int32 (HOST when mem
// == EIOKU_MEM_HOST, else device); logits_out optional ([n_clips][labels], same side).  Host outputs synchronise the stream.
int eioku_timesformer_classify(eioku_timesformer* m, const uint8_t* bgr, int n_clips, int h, int w, const int32_t* xbounds,
                               const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, int top_k,
                               float* prob_out, int32_t* class_out, float* logits_out, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n_clips >= 0 && h > 0 && w > 0 && kx > 0 && ky > 0 && xbounds && xk && ybounds && yk, "bad argument");
  EIOKU_REQUIRE(top_k >= 1 && top_k <= m->labels, "bad argument (top_k %d of %d labels)", top_k, m->labels);
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (n_clips == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr && prob_out && class_out, "NULL buffer");
  EIOKU_TRY(m->check());
  hipStream_t st = (hipStream_t)stream_;
  EIOKU_TRY(ensure_batch(m, n_clips));
  EIOKU_TRY(grow_synced(m->patches, (size_t)n_clips * m->P * m->frames * kPatchK));
  m->flops = 0;
  m->clock.begin(0b111);
  EIOKU_TRY(m->clock.mark(0, st));
  EIOKU_TRY(preprocess(m, bgr, n_clips, h, w, xbounds, xk, kx, ybounds, yk, ky, m->patches.p, nullptr, mem, st));
  EIOKU_TRY(m->clock.mark(1, st));
  EIOKU_TRY(run_encoder(m, m->patches.p, n_clips, st));
  EIOKU_TRY(m->clock.mark(2, st));
  EIOKU_TRY(run_head(m, n_clips, top_k, st));
  EIOKU_TRY(m->clock.mark(3, st));
  const hipMemcpyKind kind = mem == EIOKU_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  EIOKU_HIP_CHECK(hipMemcpyAsync(prob_out, m->probs, (size_t)n_clips * top_k * 4, kind, st));
  EIOKU_HIP_CHECK(hipMemcpyAsync(class_out, m->ids, (size_t)n_clips * top_k * 4, kind, st));
  if (logits_out) EIOKU_HIP_CHECK(hipMemcpyAsync(logits_out, m->logits, (size_t)n_clips * m->labels * 4, kind, st));
  if (mem == EIOKU_MEM_HOST) EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

// softmax and top_k of logits [n][labels] fp32 (device) -> prob_out [n][top_k], class_out [n][top_k] (device): the head's
// selection on its own (parity helper).  Asynchronous.
int eioku_timesformer_topk(eioku_timesformer* m, const float* logits, int n, int top_k, float* prob_out, int32_t* class_out,
                           void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n >= 0 && top_k >= 1 && top_k <= m->labels, "bad argument (top_k %d of %d labels)", top_k, m ? m->labels : 0);
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(logits && prob_out && class_out, "NULL buffer");
  hipLaunchKernelGGL(k_action_head, dim3(n), dim3(256), (size_t)m->labels * sizeof(float), (hipStream_t)stream_, logits, m->labels, top_k,
                     prob_out, class_out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

int eioku_timesformer_last_flops(const eioku_timesformer* m, double* flops) {
  EIOKU_REQUIRE(m && flops, "NULL argument");
  *flops = m->flops;
  return EIOKU_OK;
}

// device milliseconds of the last forward / classify call per stage (0 for a stage that call did not run); waits for it
int eioku_timesformer_last_ms(const eioku_timesformer* m, double* preprocess_ms, double* encoder_ms, double* head_ms) {
  EIOKU_REQUIRE(m && preprocess_ms && encoder_ms && head_ms, "NULL argument");
  double* const out[3] = {preprocess_ms, encoder_ms, head_ms};
  return m->clock.last_ms(out);
}

}  // extern "C"
