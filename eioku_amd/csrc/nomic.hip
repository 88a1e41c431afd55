// K27: nomic-embed-text (Hugging Face NomicBertModel layout) over PACKED variable-length sequences on gfx950 (DESIGN.md "K27
// nomic-embed-text: ragged RoPE encoder").  Sequence b owns rows cu[b] .. cu[b + 1] - 1 of every [T][.] buffer; no row is padding.
//   k_nomic_embed_ln    word_embeddings[id] + token_type_embeddings[0], LayerNorm; writes the fp32 stream and the fp16 operand
//   k_gemm<., EPI_ROPE_F16>    (gemm_f16.h) one packed [3 d][d] GEMM: q and k are rotated in the epilogue from the [max_pos][64]
//                       cos | sin table and the row's position, v is stored as it is.  q_proj / k_proj rows are permuted when
//                       they are set (stored row 2j of a head = dimension j, 2j + 1 = dimension j + 32), so both partners of a
//                       rotation sit in one lane; q . k is the same under a permutation both carry, v and o_proj never see it
//   k_attn_ragged       k_attn_seq<false> of clip.hip with the sequence's first row and length read from cu[]: 64 queries per
//                       workgroup, keys / values through LDS 128 at a time, online softmax on v_mfma_f32_16x16x32_f16.  A sibling
//                       and not a shared header, so that CLIP's kernel stays byte for byte what its tests pinned
//   k_gemm<., EPI_RESID>       o_proj and down_proj into the fp32 stream
//   k_post_ln           post-LN: normalises the fp32 stream IN PLACE (the normalised value is the residual stream) and writes
//                       the fp16 operand of the next GEMM
//   k_gemm<., EPI_SWIGLU_F16>  one packed [2 F][d] GEMM (stored row 2i = gate_proj row i, 2i + 1 = up_proj row i) that writes
//                       silu(gate) * up as [T][F] fp16; the [T][2 F] intermediate never exists
//   k_nomic_pool        one workgroup per sequence: the token mean in row order, the optional affine-free LayerNorm (eps 1e-5)
//                       over the full width, the first `dim` columns, the L2 norm; fp32, no atomics
// Every output element is one fixed-order sum that involves only its own sequence's rows, so a text's bits do not depend on the
// batch around it.  Precision points (tests/nomic_oracle.py, fp16=True): matrix weights fp16; the tables, LayerNorm parameters and
// the residual stream fp32; q / k / v, the attention output, the SwiGLU output and the LayerNorm operands rounded once to fp16;
// softmax numerators fp16; pooling and norms fp32.
#include "common.h"
#include "gemm_f16.h"

#include <cmath>
#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kMaxPos = 8192, kMaxHidden = 8192;
constexpr int kKC = 128;           // keys per LDS stage of k_attn_ragged
constexpr int kKStride = 72;       // halfs per staged key row (64 + 8: 144 B, 16-byte aligned, spreads the banks)
constexpr int kVStride = kKC + 2;  // halfs per staged value column (65 words: a column starts one bank after its neighbour)

enum { ROWS_PLAIN = 0, ROWS_ROPE = 1, ROWS_EVEN = 2, ROWS_ODD = 3 };

// where source row i of a weight lands in its packed device tensor
__device__ __forceinline__ size_t stored_row(int i, int mode) {
  if (mode == ROWS_ROPE) {
    const int j = i & 63;
    return (size_t)(i - j) + (j < 32 ? 2 * j : 2 * (j - 32) + 1);
  }
  if (mode == ROWS_EVEN) return (size_t)2 * i;
  if (mode == ROWS_ODD) return (size_t)2 * i + 1;
  return (size_t)i;
}

// src [rows][cols] fp32 -> rows stored_row(i) of dst [.][cols] fp16
__global__ __launch_bounds__(256) void k_cvt_rows(const float* __restrict__ src, int rows, int cols, int mode, h16* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * cols) return;
  const int c = (int)(i % cols);
  dst[stored_row((int)(i / cols), mode) * cols + c] = (h16)src[i];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// x[row][:] = LayerNorm(word[ids[row]][:] + type0[:]) in fp32, h[row][:] its fp16 rounding; one wave per row
__global__ __launch_bounds__(256) void k_nomic_embed_ln(const int* __restrict__ ids, int T, int d, const float* __restrict__ word,
                                                        const float* __restrict__ type0, const float* __restrict__ g,
                                                        const float* __restrict__ b, float eps, float* __restrict__ x, h16* __restrict__ h) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* wr = word + (size_t)ids[row] * d;
  float s = 0.f;
  for (int i = lane; i < d; i += 64) s += wr[i] + type0[i];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float c = wr[i] + type0[i] - mean;
    q += c * c;
  }
  const float inv = 1.f / sqrtf(wave_sum(q) / (float)d + eps);
  for (int i = lane; i < d; i += 64) {
    const float v = (wr[i] + type0[i] - mean) * inv * g[i] + b[i];
    x[(size_t)row * d + i] = v;
    h[(size_t)row * d + i] = (h16)v;
  }
}

// x[row][:] = LayerNorm(x[row][:]) in place, h[row][:] its fp16 rounding; one wave per row, a lane rewrites only what it read
__global__ __launch_bounds__(256) void k_post_ln(float* __restrict__ x, int T, int d, const float* __restrict__ g,
                                                 const float* __restrict__ b, float eps, h16* __restrict__ h) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  float* xr = x + (size_t)row * d;
  float s = 0.f;
  for (int i = lane; i < d; i += 64) s += xr[i];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float c = xr[i] - mean;
    q += c * c;
  }
  const float inv = 1.f / sqrtf(wave_sum(q) / (float)d + eps);
  for (int i = lane; i < d; i += 64) {
    const float v = (xr[i] - mean) * inv * g[i] + b[i];
    xr[i] = v;
    h[(size_t)row * d + i] = (h16)v;
  }
}

// ---- attention over packed sequences ----------------------------------------------------------------------------------------
// qkv [T][3 d] fp16 (q | k | v, head h in columns 64 h .. 64 h + 63 of each third; q and k rotated, in the stored order),
// sequence b = rows cu[b] .. cu[b + 1] - 1.  grid (ceil(longest / 64), heads, B), 4 waves of 16 queries; a workgroup whose first
// query is at or past its sequence's length leaves before any barrier.  Otherwise k_attn_seq<false> (clip.hip): keys and values
// through LDS kKC at a time up to the sequence's length, per 32 keys S^T = K Q^T in two MFMA tiles, the online softmax, then O^T
// += V^T P^T with p = exp(s - max) rounded to fp16.  Keys at or past the length score -inf before the running maximum; groups
// start at multiples of 32 below the length, so every visited group holds a live key.  A query tile starts at a multiple of 64
// of its OWN sequence, so it never straddles two.  out [T][d] fp16.
__global__ __launch_bounds__(256) void k_attn_ragged(const h16* __restrict__ qkv, const int* __restrict__ cu, int heads,
                                                     h16* __restrict__ out) {
  __shared__ __align__(16) h16 sk[kKC * kKStride];
  __shared__ __align__(16) h16 svt[64 * kVStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, u = lane >> 4;
  const int head = blockIdx.y;
  const int d = heads * 64;
  const size_t ld = (size_t)3 * d, row0 = (size_t)cu[blockIdx.z];
  const int n = cu[blockIdx.z + 1] - cu[blockIdx.z];
  if ((int)blockIdx.x * 64 >= n) return;
  const int q = blockIdx.x * 64 + wave * 16 + r;  // this lane's query token
  half8 q0 = {}, q1 = {};
  if (q < n) {
    const h16* qr = qkv + (row0 + q) * ld + head * 64 + 8 * u;
    q0 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(qr));
    q1 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(qr + 32));
  }
  float4v acc[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc[f] = float4v{0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, sum = 0.f;  // sum: this lane's share, joined over u at the end
  for (int k0 = 0; k0 < n; k0 += kKC) {
    const int nk = n - k0 < kKC ? n - k0 : kKC, nk32 = (nk + 31) & ~31;
    __syncthreads();  // the previous stage has been read
    for (int i = threadIdx.x; i < nk32 * 8; i += 256) {
      const int piece = i & 7, key = i >> 3;
      uint4 kv = {0, 0, 0, 0}, vv = {0, 0, 0, 0};  // keys past the end: zeros (masked below; 0 * value adds nothing)
      if (key < nk) {
        const h16* row = qkv + (row0 + k0 + key) * ld + head * 64 + piece * 8;
        kv = *reinterpret_cast<const uint4*>(row + d);
        vv = *reinterpret_cast<const uint4*>(row + 2 * d);
      }
      *reinterpret_cast<uint4*>(sk + key * kKStride + piece * 8) = kv;
      const half8 vh = __builtin_bit_cast(half8, vv);
#pragma unroll
      for (int e = 0; e < 8; ++e) svt[(piece * 8 + e) * kVStride + key] = vh[e];
    }
    __syncthreads();
    for (int j0 = 0; j0 < nk32; j0 += 32) {
      float4v s[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const h16* kr = sk + (j0 + 16 * e + r) * kKStride + 8 * u;
        const half8 ka = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(kr));
        const half8 kb = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(kr + 32));
        s[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, q0, float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        s[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kb, q1, s[e], 0, 0, 0);
      }
      float m_new = mx;
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = j0 + 16 * e + 4 * u + i;
          s[e][i] = key < nk ? s[e][i] * 0.125f : -INFINITY;
          m_new = fmaxf(m_new, s[e][i]);
        }
      m_new = fmaxf(m_new, __shfl_xor(m_new, 16, 64));
      m_new = fmaxf(m_new, __shfl_xor(m_new, 32, 64));  // finite: the group's first key is below the length
      const float alpha = expf(mx - m_new);
      mx = m_new;
      half8 p;
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const h16 ph = (h16)expf(s[e][i] - m_new);
          p[4 * e + i] = ph;
          ps += (float)ph;
        }
      sum = sum * alpha + ps;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const h16* vr = svt + (16 * f + r) * kVStride + j0 + 4 * u;
        const unsigned* va = reinterpret_cast<const unsigned*>(vr);  // 4-byte aligned: kVStride, j0 and 4u are even
        const uint4 v4 = {va[0], va[1], va[8], va[9]};
        acc[f] = acc[f] * alpha;
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, v4), p, acc[f], 0, 0, 0);
      }
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (q >= n) return;
  h16* o = out + (row0 + q) * d + head * 64 + 4 * u;
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[16 * f + i] = (h16)(acc[f][i] / sum);
}

// ---- pooling ------------------------------------------------------------------------------------------------------------------
// the sum of v over the workgroup's 256 threads, the same value in every thread: lanes by xor, then the four waves in order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// out[b][0 .. dim) = l2norm(first dim columns of f(mean over the rows of sequence b of x)), f = LayerNorm without affine over all
// d columns (eps 1e-5) when layer_norm != 0, else the identity.  One workgroup per sequence; mean[] is d floats of dynamic LDS.
__global__ __launch_bounds__(256) void k_nomic_pool(const float* __restrict__ x, const int* __restrict__ cu, int d, int dim, int layer_norm,
                                                    float* __restrict__ out) {
  extern __shared__ float mean[];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t row0 = (size_t)cu[b];
  const int n = cu[b + 1] - cu[b];
  float s = 0.f;
  for (int c = tid; c < d; c += 256) {
    float a = 0.f;
    for (int t = 0; t < n; ++t) a += x[(row0 + t) * d + c];
    mean[c] = a / (float)n;
    s += mean[c];
  }
  if (layer_norm) {
    const float mu = block_sum(s, red) / (float)d;
    float q = 0.f;
    for (int c = tid; c < d; c += 256) {
      const float e = mean[c] - mu;
      q += e * e;
    }
    const float inv = 1.f / sqrtf(block_sum(q, red) / (float)d + 1e-5f);
    for (int c = tid; c < dim; c += 256) mean[c] = (mean[c] - mu) * inv;
  }
  float q = 0.f;
  for (int c = tid; c < dim; c += 256) q += mean[c] * mean[c];
  const float norm = sqrtf(block_sum(q, red));
  for (int c = tid; c < dim; c += 256) out[(size_t)b * dim + c] = mean[c] / norm;
}

// ---- the model ------------------------------------------------------------------------------------------------------------------
enum { T_F16 = 0, T_F32 = 1 };

// A named tensor of the state_dict().  Its device value is `dev`, or rows of tensor `into` starting at row0, placed by `mode`.
struct Tensor {
  std::string name;
  int rows = 0, cols = 0, kind = T_F16;
  int into = -1, row0 = 0, mode = ROWS_PLAIN;
  bool listed = true;  // packed targets are not part of the state_dict()
  DevBuf<uint8_t> dev;
  bool set = false;
  size_t numel() const { return (size_t)rows * cols; }
};

struct LNorm { int g, b; };
struct Layer {
  LNorm ln_attn, ln_mlp;
  int qkv, o, gate_up, down;
};

}  // namespace

struct eioku_nomic {
  int vocab = 0, d = 0, layers = 0, heads = 0, ffn = 0, max_pos = 0, type_vocab = 0;
  float eps = 1e-12f, theta = 1000.f;
  std::vector<Tensor> tensors;
  std::vector<int> listed;  // indices of the state_dict() tensors, in order
  int word = -1, type = -1;
  LNorm emb_ln{};
  std::vector<Layer> L;
  DevBuf<float> rope;  // [max_pos][64]: cos of (pos, j) in column j, sin in column 32 + j
  // one pass
  DevBuf<float> x, unit;
  DevBuf<h16> h, qkv, a, mid;
  DevBuf<int> ids, cu, pos;
  std::vector<int> ids_host, cu_host, pos_host;  // what the asynchronous uploads read: alive until the next call
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool timed = false;
  double flops = 0;

  const uint8_t* base(int i) const {
    const Tensor& t = tensors[i];
    return t.into < 0 ? t.dev.p : tensors[t.into].dev.p + (size_t)t.row0 * t.cols * 2;  // only fp16 weights are packed
  }
  const h16* H(int i) const { return (const h16*)base(i); }
  const float* F(int i) const { return (const float*)base(i); }
};

namespace {

typedef eioku_nomic Model;

template <int EPI>
int gemm(Model* m, hipStream_t st, const h16* A, int w, int M, int N, int K, void* out, long long ldc, const float* table = nullptr,
         int table_rows = 1, const int* row_pos = nullptr) {
  EIOKU_REQUIRE(K % 32 == 0 && N % 16 == 0 && ldc % 4 == 0, "GEMM K %d / N %d / ldc %lld misaligned", K, N, ldc);
  const dim3 grid((N + 63) / 64, (M + 63) / 64);
  hipLaunchKernelGGL((k_gemm<4, EPI>), grid, dim3(256), 0, st, A, K, m->H(w), K, (const float*)nullptr, M, N, K, out, ldc, table,
                     table_rows, row_pos);
  m->flops += 2.0 * M * N * K;
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// ids / cu / pos on the device, T rows, B sequences, the longest `longest` rows -> m->x after every layer, m->unit [B][dim]
int run(Model* m, int T, int B, int longest, int dim, int layer_norm, hipStream_t st) {
  const int d = m->d, F = m->ffn;
  const dim3 rows((T + 3) / 4);
  hipLaunchKernelGGL(k_nomic_embed_ln, rows, dim3(256), 0, st, m->ids.p, T, d, m->F(m->word), m->F(m->type), m->F(m->emb_ln.g),
                     m->F(m->emb_ln.b), m->eps, m->x.p, m->h.p);
  EIOKU_LAUNCH_CHECK();
  for (const Layer& L : m->L) {
    EIOKU_TRY((gemm<EPI_ROPE_F16>(m, st, m->h, L.qkv, T, 3 * d, d, m->qkv.p, 3 * d, m->rope.p, m->max_pos, m->pos.p)));
    hipLaunchKernelGGL(k_attn_ragged, dim3((longest + 63) / 64, m->heads, B), dim3(256), 0, st, m->qkv.p, m->cu.p, m->heads, m->a.p);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY((gemm<EPI_RESID>(m, st, m->a, L.o, T, d, d, m->x.p, d)));
    hipLaunchKernelGGL(k_post_ln, rows, dim3(256), 0, st, m->x.p, T, d, m->F(L.ln_attn.g), m->F(L.ln_attn.b), m->eps, m->h.p);
    EIOKU_LAUNCH_CHECK();
    EIOKU_TRY((gemm<EPI_SWIGLU_F16>(m, st, m->h, L.gate_up, T, 2 * F, d, m->mid.p, F)));
    EIOKU_TRY((gemm<EPI_RESID>(m, st, m->mid, L.down, T, d, F, m->x.p, d)));
    hipLaunchKernelGGL(k_post_ln, rows, dim3(256), 0, st, m->x.p, T, d, m->F(L.ln_mlp.g), m->F(L.ln_mlp.b), m->eps, m->h.p);
    EIOKU_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_nomic_pool, dim3(B), dim3(256), (size_t)d * sizeof(float), st, m->x.p, m->cu.p, d, dim, layer_norm, m->unit.p);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // namespace

extern "C" {

int eioku_nomic_create(int vocab, int hidden, int layers, int heads, int ffn, int max_pos, int type_vocab, float ln_eps, float rope_theta,
                       eioku_nomic** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL argument");
  EIOKU_REQUIRE(hidden > 0 && heads > 0 && heads * 64 == hidden, "head_dim must be 64 (hidden %d / heads %d)", hidden, heads);
  EIOKU_REQUIRE(hidden <= kMaxHidden, "hidden must be at most %d (got %d)", kMaxHidden, hidden);
  EIOKU_REQUIRE(ffn > 0 && ffn % 32 == 0, "intermediate_size must be a positive multiple of 32 (got %d)", ffn);
  EIOKU_REQUIRE(max_pos >= 1 && max_pos <= kMaxPos, "max_position_embeddings must be in [1, %d] (got %d)", kMaxPos, max_pos);
  EIOKU_REQUIRE(layers >= 0 && vocab > 0 && type_vocab > 0 && ln_eps > 0.f && rope_theta > 0.f,
                "bad config (layers %d, vocab %d, type_vocab %d, ln_eps %g, rope_theta %g)", layers, vocab, type_vocab, (double)ln_eps,
                (double)rope_theta);
  auto* m = new eioku_nomic();
  m->vocab = vocab, m->d = hidden, m->layers = layers, m->heads = heads, m->ffn = ffn, m->max_pos = max_pos, m->type_vocab = type_vocab;
  m->eps = ln_eps, m->theta = rope_theta;
  const int d = hidden;
  auto add = [&](const std::string& n, int rows, int cols, int kind) {
    Tensor t;
    t.name = n, t.rows = rows, t.cols = cols, t.kind = kind;
    m->tensors.push_back(std::move(t));
    return (int)m->tensors.size() - 1;
  };
  auto packed = [&](const std::string& n, int rows, int cols) {
    const int i = add(n, rows, cols, T_F16);
    m->tensors[i].listed = false;
    return i;
  };
  auto part = [&](const std::string& n, int rows, int cols, int into, int row0, int mode) {
    const int i = add(n, rows, cols, T_F16);
    m->tensors[i].into = into, m->tensors[i].row0 = row0, m->tensors[i].mode = mode;
    return i;
  };
  auto lnorm = [&](const std::string& p) {
    LNorm l;
    l.g = add(p + ".weight", d, 1, T_F32);
    l.b = add(p + ".bias", d, 1, T_F32);
    return l;
  };
  // the order of NomicBertModel.state_dict()
  m->word = add("embeddings.word_embeddings.weight", vocab, d, T_F32);
  m->type = add("embeddings.token_type_embeddings.weight", type_vocab, d, T_F32);
  m->emb_ln = lnorm("embeddings.LayerNorm");
  for (int l = 0; l < layers; ++l) {
    const std::string p = "layers." + std::to_string(l) + ".";
    Layer L;
    L.ln_attn = lnorm(p + "post_attention_layernorm");
    L.gate_up = packed(p + "mlp.gate_up.weight", 2 * ffn, d);
    part(p + "mlp.gate_proj.weight", ffn, d, L.gate_up, 0, ROWS_EVEN);
    part(p + "mlp.up_proj.weight", ffn, d, L.gate_up, 0, ROWS_ODD);
    L.down = add(p + "mlp.down_proj.weight", d, ffn, T_F16);
    L.qkv = packed(p + "self_attn.qkv.weight", 3 * d, d);
    part(p + "self_attn.q_proj.weight", d, d, L.qkv, 0, ROWS_ROPE);
    part(p + "self_attn.k_proj.weight", d, d, L.qkv, d, ROWS_ROPE);
    part(p + "self_attn.v_proj.weight", d, d, L.qkv, 2 * d, ROWS_PLAIN);
    L.o = add(p + "self_attn.o_proj.weight", d, d, T_F16);
    L.ln_mlp = lnorm(p + "post_mlp_layernorm");
    m->L.push_back(L);
  }
  auto fail = [&](int rc) {
    eioku_nomic_destroy(m);
    return rc;
  };
  for (size_t i = 0; i < m->tensors.size(); ++i) {
    Tensor& t = m->tensors[i];
    if (t.listed) m->listed.push_back((int)i);
    if (t.into >= 0) continue;
    if (t.dev.grow(t.numel() * (t.kind == T_F32 ? 4 : 2))) return fail(EIOKU_ENOMEM);
  }
  // the rotary table in fp32, as transformers computes it: inv_freq[j] = 1 / theta^(2j / 64), angle = pos * inv_freq[j]
  std::vector<float> table((size_t)max_pos * 64);
  for (int j = 0; j < 32; ++j) {
    const float inv_freq = 1.0f / powf(rope_theta, (float)(2 * j) / 64.0f);
    for (int p = 0; p < max_pos; ++p) {
      const float angle = (float)p * inv_freq;
      table[(size_t)p * 64 + j] = cosf(angle);
      table[(size_t)p * 64 + 32 + j] = sinf(angle);
    }
  }
  if (m->rope.upload(table.data(), table.size())) return fail(EIOKU_ENOMEM);
  for (auto& ev : m->ev)
    if (hipEventCreate(&ev) != hipSuccess) {
      ev = nullptr;
      set_error("hipEventCreate failed");
      return fail(EIOKU_EHIP);
    }
  *out = m;
  return EIOKU_OK;
}

void eioku_nomic_destroy(eioku_nomic* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  for (auto ev : m->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete m;  // every buffer frees itself
}

int eioku_nomic_num_tensors(const eioku_nomic* m) { return m ? (int)m->listed.size() : 0; }

int eioku_nomic_tensor_info(const eioku_nomic* m, int idx, char* name, size_t cap, int* rows, int* cols) {
  EIOKU_REQUIRE(m && idx >= 0 && idx < (int)m->listed.size(), "bad tensor index %d", idx);
  const auto& t = m->tensors[m->listed[idx]];
  if (name && cap) snprintf(name, cap, "%s", t.name.c_str());
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return EIOKU_OK;
}

int eioku_nomic_set_tensor(eioku_nomic* m, int idx, const float* host, size_t numel) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && idx >= 0 && idx < (int)m->listed.size() && host, "bad argument");
  auto& t = m->tensors[m->listed[idx]];
  EIOKU_REQUIRE(numel == t.numel(), "%s: expected %zu elements, got %zu", t.name.c_str(), t.numel(), numel);
  EIOKU_HIP_CHECK(hipDeviceSynchronize());  // no pass may still read the old value
  void* dst = const_cast<uint8_t*>(m->base(m->listed[idx]));
  if (t.kind == T_F32) {
    EIOKU_HIP_CHECK(hipMemcpy(dst, host, numel * sizeof(float), hipMemcpyHostToDevice));
  } else {
    DevBuf<float> stage;
    EIOKU_TRY(stage.grow(numel));
    EIOKU_HIP_CHECK(hipMemcpy(stage, host, numel * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_cvt_rows, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, 0, stage.p, t.rows, t.cols, t.mode, (h16*)dst);
    EIOKU_LAUNCH_CHECK();
    EIOKU_HIP_CHECK(hipDeviceSynchronize());
  }
  t.set = true;
  return EIOKU_OK;
}

// ids [T] and cu [B + 1] int32 on the side `mem` names (cu[0] = 0, T = cu[B]) -> out [B][dim] fp32 unit vectors and optionally
// hidden_out [T][hidden] fp32 (the stream after the last layer) on that side.  dim = matryoshka_dim, or hidden when that is 0.
// Device inputs are read back once: the lengths size the launches, and every id is checked before any kernel gathers with it.
int eioku_nomic_encode(eioku_nomic* m, const int32_t* ids, const int32_t* cu, int B, int matryoshka_dim, float* out, float* hidden_out,
                       int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && B >= 0, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  EIOKU_REQUIRE(matryoshka_dim >= 0 && matryoshka_dim <= m->d, "matryoshka_dim must be in [1, %d], or 0 for the full width (got %d)", m->d,
                matryoshka_dim);
  if (B == 0) return EIOKU_OK;
  EIOKU_REQUIRE(ids && cu && out, "NULL buffer");
  for (int i : m->listed) EIOKU_REQUIRE(m->tensors[i].set, "tensor %s has no weights", m->tensors[i].name.c_str());
  hipStream_t st = (hipStream_t)stream_;
  const bool dev = mem == EIOKU_MEM_DEVICE;
  if (dev) EIOKU_HIP_CHECK(hipStreamSynchronize(st));  // whatever on the caller's stream still writes ids / cu
  m->cu_host.resize((size_t)B + 1);
  EIOKU_HIP_CHECK(hipMemcpy(m->cu_host.data(), cu, ((size_t)B + 1) * 4, dev ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
  EIOKU_REQUIRE(m->cu_host[0] == 0, "cu[0] must be 0 (got %d)", m->cu_host[0]);
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    const long long n = (long long)m->cu_host[b + 1] - m->cu_host[b];
    EIOKU_REQUIRE(n >= 1, "sequence %d: length %lld, every sequence needs at least one token", b, n);
    EIOKU_REQUIRE(n <= m->max_pos, "sequence %d: length %lld exceeds max_position_embeddings %d", b, n, m->max_pos);
    if (n > longest) longest = (int)n;
  }
  const int T = m->cu_host[B];
  m->ids_host.resize((size_t)T);
  EIOKU_HIP_CHECK(hipMemcpy(m->ids_host.data(), ids, (size_t)T * 4, dev ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
  for (int i = 0; i < T; ++i)
    EIOKU_REQUIRE(m->ids_host[i] >= 0 && m->ids_host[i] < m->vocab, "token id %d at row %d outside the vocabulary of %d", m->ids_host[i], i,
                  m->vocab);
  m->pos_host.resize((size_t)T);
  for (int b = 0; b < B; ++b)
    for (int t = m->cu_host[b]; t < m->cu_host[b + 1]; ++t) m->pos_host[t] = t - m->cu_host[b];
  const int dim = matryoshka_dim ? matryoshka_dim : m->d;
  const size_t d = m->d;
  EIOKU_TRY(grow_synced(m->ids, (size_t)T));
  EIOKU_TRY(grow_synced(m->pos, (size_t)T));
  EIOKU_TRY(grow_synced(m->cu, (size_t)B + 1));
  EIOKU_TRY(grow_synced(m->x, T * d));
  EIOKU_TRY(grow_synced(m->h, T * d));
  EIOKU_TRY(grow_synced(m->qkv, T * 3 * d));
  EIOKU_TRY(grow_synced(m->a, T * d));
  EIOKU_TRY(grow_synced(m->mid, (size_t)T * m->ffn));
  EIOKU_TRY(grow_synced(m->unit, (size_t)B * dim));
  m->flops = 0;
  for (int b = 0; b < B; ++b) {
    const double n = m->cu_host[b + 1] - m->cu_host[b];
    m->flops += 4.0 * m->layers * m->heads * n * n * 64;
  }
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->ids, m->ids_host.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->pos, m->pos_host.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->cu, m->cu_host.data(), ((size_t)B + 1) * 4, hipMemcpyHostToDevice, st));
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[0], st));
  EIOKU_TRY(run(m, T, B, longest, dim, matryoshka_dim != 0, st));
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[1], st));
  m->timed = true;
  const hipMemcpyKind back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  EIOKU_HIP_CHECK(hipMemcpyAsync(out, m->unit, (size_t)B * dim * 4, back, st));
  if (hidden_out) EIOKU_HIP_CHECK(hipMemcpyAsync(hidden_out, m->x, T * d * 4, back, st));
  EIOKU_HIP_CHECK(hipStreamSynchronize(st));  // the host vectors and, for a host caller, the outputs are free again
  return EIOKU_OK;
}

int eioku_nomic_last_flops(const eioku_nomic* m, double* flops) {
  EIOKU_REQUIRE(m && flops, "NULL argument");
  *flops = m->flops;
  return EIOKU_OK;
}

// device milliseconds of the last encode call, from the first kernel to the pooled vectors (0 before any call)
int eioku_nomic_last_ms(const eioku_nomic* m, double* ms) {
  EIOKU_REQUIRE(m && ms, "NULL argument");
  *ms = 0.0;
  if (!m->timed) return EIOKU_OK;
  float v = 0.f;
  EIOKU_HIP_CHECK(hipEventSynchronize(m->ev[1]));
  EIOKU_HIP_CHECK(hipEventElapsedTime(&v, m->ev[0], m->ev[1]));
  *ms = v;
  return EIOKU_OK;
}

}  // extern "C"
