// K27: nomic-embed-text (Hugging Face NomicBertModel layout) over PACKED variable-length sequences on gfx950 (DESIGN.md "K27
// nomic-embed-text: ragged RoPE encoder").  Sequence b owns rows cu[b] .. cu[b + 1] - 1 of every [T][.] buffer; no row is padding.
//   k_nomic_embed_ln    word_embeddings[id] + token_type_embeddings[0], LayerNorm; writes the fp32 stream and the fp16 operand
//   k_gemm<., EPI_ROPE_F16>    (gemm_f16.h) one packed [3 d][d] GEMM: q and k are rotated in the epilogue from the [max_pos][64]
//                       cos | sin table and the row's position, v is stored as it is.  q_proj / k_proj rows are permuted when
//                       they are set (stored row 2j of a head = dimension j, 2j + 1 = dimension j + 32), so both partners of a
//                       rotation sit in one lane; q . k is the same under a permutation both carry, v and o_proj never see it
//   k_attn_tiles<RaggedSeq, false>  (attn_f16.h) the tiled MFMA attention with the sequence's first row and length read from
//                       cu[]: 64 queries per workgroup, keys / values through LDS 128 at a time, online softmax
//   k_gemm<., EPI_RESID>       o_proj and down_proj into the fp32 stream
//   k_post_ln           post-LN: normalises the fp32 stream IN PLACE (the normalised value is the residual stream) and writes
//                       the fp16 operand of the next GEMM; like k_nomic_embed_ln over row_stats (layernorm.h)
//   k_gemm<., EPI_SWIGLU_F16>  one packed [2 F][d] GEMM (stored row 2i = gate_proj row i, 2i + 1 = up_proj row i) that writes
//                       silu(gate) * up as [T][F] fp16; the [T][2 F] intermediate never exists
//   k_nomic_pool        one workgroup per sequence: the token mean in row order, the optional affine-free LayerNorm (eps 1e-5)
//                       over the full width, the first `dim` columns, the L2 norm; fp32, no atomics
// Every output element is one fixed-order sum that involves only its own sequence's rows, so a text's bits do not depend on the
// batch around it.  Precision points (tests/nomic_oracle.py, fp16=True): matrix weights fp16; the tables, LayerNorm parameters and
// the residual stream fp32; q / k / v, the attention output, the SwiGLU output and the LayerNorm operands rounded once to fp16;
// softmax numerators fp16; pooling and norms fp32.
#include "attn_f16.h"
#include "common.h"
#include "gemm_f16.h"
#include "layernorm.h"
#include "tensors.h"

#include <cmath>
#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kMaxPos = 8192, kMaxHidden = 8192;

// x[row][:] = LayerNorm(word[ids[row]][:] + type0[:]) in fp32, h[row][:] its fp16 rounding; one wave per row
__global__ __launch_bounds__(256) void k_nomic_embed_ln(const int* __restrict__ ids, int T, int d, const float* __restrict__ word,
                                                        const float* __restrict__ type0, const float* __restrict__ g,
                                                        const float* __restrict__ b, float eps, float* __restrict__ x, h16* __restrict__ h) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* wr = word + (size_t)ids[row] * d;
  const RowStats st = row_stats(lane, d, eps, [&](int i) { return wr[i] + type0[i]; });
  for (int i = lane; i < d; i += 64) {
    const float v = (wr[i] + type0[i] - st.mean) * st.inv * g[i] + b[i];
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
  const RowStats st = row_stats(lane, d, eps, [&](int i) { return xr[i]; });
  for (int i = lane; i < d; i += 64) {
    const float v = (xr[i] - st.mean) * st.inv * g[i] + b[i];
    xr[i] = v;
    h[(size_t)row * d + i] = (h16)v;
  }
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
struct Layer {
  LNorm ln_attn, ln_mlp;
  int qkv, o, gate_up, down;
};

}  // namespace

struct eioku_nomic : TensorTable {
  int vocab = 0, d = 0, layers = 0, heads = 0, ffn = 0, max_pos = 0, type_vocab = 0;
  float eps = 1e-12f, theta = 1000.f;
  int word = -1, type = -1;
  LNorm emb_ln{};
  std::vector<Layer> L;
  DevBuf<float> rope;  // [max_pos][64]: cos of (pos, j) in column j, sin in column 32 + j
  // one pass
  DevBuf<float> x, unit;
  DevBuf<h16> h, qkv, a, mid;
  DevBuf<int> ids, cu, pos;
  std::vector<int> ids_host, cu_host, pos_host;  // what the asynchronous uploads read: alive until the next call
  StageClock<1> clock;  // the encode, from the first kernel to the pooled vectors
  double flops = 0;
};

namespace {

typedef eioku_nomic Model;

template <int EPI>
int gemm(Model* m, hipStream_t st, const h16* A, int w, int M, int N, int K, void* out, long long ldc, const float* table = nullptr,
         int table_rows = 1, const int* row_pos = nullptr) {
  return launch_gemm<4, EPI>(st, A, K, m->H(w), K, nullptr, M, N, K, out, ldc, table, table_rows, row_pos, &m->flops);
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
    EIOKU_TRY(launch_attn<false>(st, m->qkv.p, RaggedSeq{m->cu.p, d, m->a.p}, longest, m->heads, B));
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
  // the order of NomicBertModel.state_dict()
  m->word = m->add("embeddings.word_embeddings.weight", vocab, d, T_F32);
  m->type = m->add("embeddings.token_type_embeddings.weight", type_vocab, d, T_F32);
  m->emb_ln = m->lnorm("embeddings.LayerNorm", d);
  for (int l = 0; l < layers; ++l) {
    const std::string p = "layers." + std::to_string(l) + ".";
    Layer L;
    L.ln_attn = m->lnorm(p + "post_attention_layernorm", d);
    L.gate_up = m->packed(p + "mlp.gate_up.weight", 2 * ffn, d, T_F16);
    m->part(p + "mlp.gate_proj.weight", ffn, d, L.gate_up, 0, ROWS_EVEN);
    m->part(p + "mlp.up_proj.weight", ffn, d, L.gate_up, 0, ROWS_ODD);
    L.down = m->add(p + "mlp.down_proj.weight", d, ffn, T_F16);
    L.qkv = m->packed(p + "self_attn.qkv.weight", 3 * d, d, T_F16);
    m->part(p + "self_attn.q_proj.weight", d, d, L.qkv, 0, ROWS_ROPE);
    m->part(p + "self_attn.k_proj.weight", d, d, L.qkv, d, ROWS_ROPE);
    m->part(p + "self_attn.v_proj.weight", d, d, L.qkv, 2 * d, ROWS_PLAIN);
    L.o = m->add(p + "self_attn.o_proj.weight", d, d, T_F16);
    L.ln_mlp = m->lnorm(p + "post_mlp_layernorm", d);
    m->L.push_back(L);
  }
  auto fail = [&](int rc) {
    eioku_nomic_destroy(m);
    return rc;
  };
  if (const int rc = m->finish()) return fail(rc);
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
  if (const int rc = m->clock.create()) return fail(rc);
  *out = m;
  return EIOKU_OK;
}

void eioku_nomic_destroy(eioku_nomic* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  delete m;  // every buffer and event frees itself
}

int eioku_nomic_num_tensors(const eioku_nomic* m) { return TensorTable::count(m); }

int eioku_nomic_tensor_info(const eioku_nomic* m, int idx, char* name, size_t cap, int* rows, int* cols) {
  return TensorTable::info(m, idx, name, cap, rows, cols);
}

int eioku_nomic_set_tensor(eioku_nomic* m, int idx, const float* host, size_t numel) { return TensorTable::set(m, idx, host, numel); }

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
  EIOKU_TRY(m->check());
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
  EIOKU_TRY(m->clock.mark(0, st));
  EIOKU_TRY(run(m, T, B, longest, dim, matryoshka_dim != 0, st));
  EIOKU_TRY(m->clock.mark(1, st));
  m->clock.begin(1);
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
  double* const out[1] = {ms};
  return m->clock.last_ms(out);
}

}  // extern "C"
