// K26: CLIP image and text towers on gfx950, in the Hugging Face CLIPModel layout (DESIGN.md "K26 CLIP frame and text embeddings").
//   k_clip_resize_h / k_clip_resize_v   (clip_resize.h) Pillow's two-pass 8-bit resample with the host's bicubic tables, the
//                       centre crop, BGR -> RGB, (v * (1 / 255) - mean) / std in fp32, one rounding to fp16, written as patch
//                       rows [image][1 + P][Kp]: token 0 and the columns past 3 p p stay zero (Kp = 3 p p rounded up to 32)
//   k_gemm<., EPI_POS>  (gemm_f16.h) patch projection over all B (1 + P) rows + the table {class_embedding + position[0],
//                       position[1 ..]} into the embedded fp32 stream; the convolution has no bias
//   k_ln<float>         pre_layrnorm: fp32 row -> fp32 residual stream;  k_ln<h16>: LayerNorm into the fp16 GEMM operand,
//                       optionally of picked rows only (the head)
//   k_text_embed        token_embedding[id] + position[i] into the fp32 stream, positions 0 .. n - 1 only
//   k_attn_seq<CAUSAL>  dense sequences of n tokens, row b n + i: 64 queries per workgroup (4 waves of 16), keys / values staged
//                       through LDS 128 at a time, QK^T and PV on v_mfma_f32_16x16x32_f16 with an online softmax; CAUSAL:
//                       query i sees keys 0 .. i, a wave's key loop ends at its last query's key
//   k_l2norm            the projected rows to unit length in fp32
// Layers are pre-LN: LN -> packed qkv GEMM -> attention -> out-projection (EPI_RESID) -> LN -> fc1 with the activation
// epilogue -> fc2 (EPI_RESID).  The text tower runs n = max(eot + 1) positions per text: under the causal mask no row up
// to EOT reads a later one, so the 77 - n pad positions are never computed.
// Precision points (tests/clip_oracle.py, fp16=True, rounds at the same places): matrix weights fp16; biases, LayerNorm
// parameters, the embedding and position tables fp32; the residual stream fp32 (pre_layrnorm writes it unrounded); LayerNorm
// outputs, q / k / v, attention outputs, activation outputs and the patch rows are rounded to fp16; the softmax numerators
// exp(s - max) are rounded to fp16 for the PV MFMA; the projection, the norm and the outputs are fp32.
#include "clip_resize.h"
#include "common.h"
#include "gemm_f16.h"

#include <cmath>
#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kMaxImage = 448, kMaxPositions = 77;
constexpr int kKC = 128;           // keys per LDS stage of k_attn_seq
constexpr int kKStride = 72;       // halfs per staged key row (64 + 8: 144 B, 16-byte aligned, spreads the banks)
constexpr int kVStride = kKC + 2;  // halfs per staged value column (65 words: a column starts one bank after its neighbour)

// ---- small kernels ------------------------------------------------------------------------------------------------------
// src [rows][cols] fp32 -> dst [rows][ld] fp16, columns cols .. ld - 1 zero
__global__ __launch_bounds__(256) void k_cvt_f16_pad(const float* __restrict__ src, int rows, int cols, int ld, h16* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * ld) return;
  const int c = (int)(i % ld);
  const size_t r = i / ld;
  dst[i] = c < cols ? (h16)src[r * cols + c] : (h16)0.f;
}

// the table the patch GEMM's epilogue reads: row 0 = class_embedding + position[0], row 1 + p = position[1 + p]
__global__ __launch_bounds__(256) void k_vision_table(const float* __restrict__ cls, const float* __restrict__ pos, int rows, int d,
                                                      float* __restrict__ table) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * d) return;
  table[i] = i < (size_t)d ? cls[i] + pos[i] : pos[i];
}

// x[b n + i][:] = token_embedding[ids[b positions + i]][:] + position[i][:] for i < n
__global__ __launch_bounds__(256) void k_text_embed(const int* __restrict__ ids, int B, int n, int positions, int d,
                                                    const float* __restrict__ tok, const float* __restrict__ pos, float* __restrict__ x) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * n * d) return;
  const int c = (int)(i % d);
  const size_t row = i / d;
  const int t = (int)(row % n), b = (int)(row / n);
  x[i] = tok[(size_t)ids[(size_t)b * positions + t] * d + c] + pos[(size_t)t * d + c];
}

// LayerNorm: fp32 row -> OUT (fp16 or fp32), one wave per row; pick != nullptr: output row r is the norm of x row pick[r]
template <typename OUT>
__global__ __launch_bounds__(256) void k_ln(const float* __restrict__ x, int M, int d, const float* __restrict__ g,
                                            const float* __restrict__ b, float eps, const int* __restrict__ pick, OUT* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (size_t)(pick ? pick[row] : row) * d;
  float s = 0.f;
  for (int i = lane; i < d; i += 64) s += xr[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / (float)d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float c = xr[i] - mean;
    q += c * c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float inv = 1.f / sqrtf(q / (float)d + eps);
  for (int i = lane; i < d; i += 64) out[(size_t)row * d + i] = (OUT)((xr[i] - mean) * inv * g[i] + b[i]);
}

// v[row][:] /= |v[row]| in fp32, one wave per row
__global__ __launch_bounds__(256) void k_l2norm(const float* __restrict__ v, int M, int d, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* vr = v + (size_t)row * d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) q += vr[i] * vr[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float norm = sqrtf(q);
  for (int i = lane; i < d; i += 64) out[(size_t)row * d + i] = vr[i] / norm;
}

// ---- attention over dense sequences ---------------------------------------------------------------------------------------
// qkv [B n][3 d] fp16 (q | k | v, head h in columns 64 h .. 64 h + 63 of each third), sequence b = rows b n .. b n + n - 1.
// grid (ceil(n / 64), heads, B), 4 waves of 16 queries.  Keys and values go through LDS kKC at a time (keys [key][72], values
// transposed [dim][kKC + 2]); the workgroup stages keys up to its last query (CAUSAL) or n.  Per 32 keys and wave: S^T = K Q^T
// in two 16-key MFMA tiles (lane (r, u): query r, keys 4u .. 4u + 3 of each tile), the online softmax per query across the
// lanes r, r + 16, r + 32, r + 48, then O^T += V^T P^T with the 32 keys in the order the lanes already hold them, p = exp(s -
// max) rounded to fp16.  CAUSAL: key > query scores -inf before the running maximum, and a wave stops after the 32-key group
// that holds its last query's key.  A wave's queries start at a multiple of 16 and groups at multiples of 32, so every group a
// wave visits starts at or before each of its queries: no query ever sees a group of masked keys only.  out [B n][d] fp16.
template <bool CAUSAL>
__global__ __launch_bounds__(256) void k_attn_seq(const h16* __restrict__ qkv, int n, int heads, h16* __restrict__ out) {
  __shared__ __align__(16) h16 sk[kKC * kKStride];
  __shared__ __align__(16) h16 svt[64 * kVStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, u = lane >> 4;
  const int head = blockIdx.y;
  const int d = heads * 64;
  const size_t ld = (size_t)3 * d, row0 = (size_t)blockIdx.z * n;
  const int q = blockIdx.x * 64 + wave * 16 + r;  // this lane's query token
  half8 q0 = {}, q1 = {};
  if (q < n) {
    const h16* qr = qkv + (row0 + q) * ld + head * 64 + 8 * u;
    q0 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(qr));
    q1 = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(qr + 32));
  }
  int kend_wg = n, kend_wave = n;  // one past the last key the workgroup stages / this wave scores
  if (CAUSAL) {
    const int last_wg = blockIdx.x * 64 + 63, last_wave = blockIdx.x * 64 + wave * 16 + 15;
    kend_wg = last_wg < n - 1 ? last_wg + 1 : n;
    kend_wave = last_wave < n - 1 ? last_wave + 1 : n;
  }
  float4v acc[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc[f] = float4v{0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, sum = 0.f;  // sum: this lane's share, joined over u at the end
  for (int k0 = 0; k0 < kend_wg; k0 += kKC) {
    const int nk = kend_wg - k0 < kKC ? kend_wg - k0 : kKC, nk32 = (nk + 31) & ~31;
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
    for (int j0 = 0; j0 < nk32 && k0 + j0 < kend_wave; j0 += 32) {
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
          const bool seen = key < nk && (!CAUSAL || k0 + key <= q);
          s[e][i] = seen ? s[e][i] * 0.125f : -INFINITY;
          m_new = fmaxf(m_new, s[e][i]);
        }
      m_new = fmaxf(m_new, __shfl_xor(m_new, 16, 64));
      m_new = fmaxf(m_new, __shfl_xor(m_new, 32, 64));  // finite from the first 32 keys on: key 0 is never masked
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

// ---- the model ------------------------------------------------------------------------------------------------------------
enum { T_F16 = 0, T_F32 = 1 };
enum { VISION = 0, TEXT = 1 };

// A named tensor of the state_dict().  Its device value is `dev`, or rows [row0, row0 + rows) of tensor `into` (q_proj,
// k_proj and v_proj land in one packed [3 d][d] weight and one [3 d] bias); ld is the device row length in elements.
struct Tensor {
  std::string name;
  int rows = 0, cols = 0, kind = T_F16, ld = 0, tower = VISION;
  int into = -1, row0 = 0;
  bool listed = true;  // packed targets are not part of the state_dict()
  DevBuf<uint8_t> dev;
  bool set = false;
  size_t numel() const { return (size_t)rows * cols; }
};

struct Lin { int w, b; };
struct LNorm { int g, b; };
struct Layer {
  LNorm ln1, ln2;
  Lin qkv, out, fc1, fc2;
};

struct Tower {
  int d = 0, layers = 0, heads = 0, ffn = 0;
  std::vector<Layer> L;
  LNorm final_ln{};
  int proj = -1;  // [projection_dim][d], no bias
};

}  // namespace

struct eioku_clip {
  int image = 0, patch = 0, side = 0, P = 0, K = 0, Kp = 0;  // K = 3 p p, Kp = K rounded up to 32
  int vocab = 0, positions = 0, proj_dim = 0, act = 0;
  float eps = 1e-5f;
  Norm3 nrm{{0.48145466f, 0.4578275f, 0.40821073f}, {0.26862954f, 0.26130258f, 0.27577711f}};
  Tower tw[2];
  std::vector<Tensor> tensors;
  std::vector<int> listed;  // indices of the state_dict() tensors, in order
  int cls = -1, patch_w = -1, vpos = -1, tok = -1, tpos = -1;
  LNorm pre_ln{};
  bool table_ready = false;
  DevBuf<float> vtable;
  // preprocessing
  DevBuf<int> tables;
  DevBuf<uint8_t> src, tmp;
  DevBuf<h16> patches;
  // activations of one pass
  DevBuf<float> x, x0, pooled, unit;
  DevBuf<h16> h, qkv, a, mid, hp;
  DevBuf<int> ids, pick;
  std::vector<int> ids_host, pick_host;  // what the asynchronous uploads read: alive until the next call
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool timed[3] = {false, false, false};  // which of preprocess / encoder / head the last call ran
  double flops = 0;

  const uint8_t* base(int i) const {
    const Tensor& t = tensors[i];
    if (t.into < 0) return t.dev.p;
    return tensors[t.into].dev.p + (size_t)t.row0 * t.ld * (t.kind == T_F32 ? 4 : 2);
  }
  const h16* H(int i) const { return (const h16*)base(i); }
  const float* F(int i) const { return (const float*)base(i); }
};

namespace {

typedef eioku_clip Model;

template <int MT, int EPI>
int gemm(Model* m, hipStream_t st, const h16* A, int lda, int w, int bias, int M, int N, int K, void* out, long long ldc,
         const float* pos = nullptr, int pos_rows = 1) {
  EIOKU_REQUIRE(K % 32 == 0 && lda % 8 == 0, "GEMM K %d / lda %d misaligned", K, lda);
  if (M == 0) return EIOKU_OK;
  const dim3 grid((N + 63) / 64, (M + 16 * MT - 1) / (16 * MT));
  hipLaunchKernelGGL((k_gemm<MT, EPI>), grid, dim3(256), 0, st, A, lda, m->H(w), K, bias >= 0 ? m->F(bias) : nullptr, M, N, K, out, ldc,
                     pos, pos_rows, nullptr);
  m->flops += 2.0 * M * N * K;
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

template <typename OUT>
int ln(Model* m, hipStream_t st, const float* x, int M, int d, const LNorm& p, const int* pick, OUT* out) {
  if (M == 0) return EIOKU_OK;
  hipLaunchKernelGGL(k_ln<OUT>, dim3((M + 3) / 4), dim3(256), 0, st, x, M, d, m->F(p.g), m->F(p.b), m->eps, pick, out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

int check_weights(const Model* m, int tower) {
  for (int i : m->listed) {
    const Tensor& t = m->tensors[i];
    EIOKU_REQUIRE(t.tower != tower || t.set, "tensor %s has no weights", t.name.c_str());
  }
  return EIOKU_OK;
}

int ensure_rows(Model* m, int tower, size_t M, int B) {
  const Tower& t = m->tw[tower];
  const size_t d = t.d;
  EIOKU_TRY(grow_synced(m->x, M * d));
  if (tower == VISION) EIOKU_TRY(grow_synced(m->x0, M * d));  // the embedded stream before pre_layrnorm
  EIOKU_TRY(grow_synced(m->h, M * d));
  EIOKU_TRY(grow_synced(m->qkv, M * 3 * d));
  EIOKU_TRY(grow_synced(m->a, M * d));
  EIOKU_TRY(grow_synced(m->mid, M * t.ffn));
  EIOKU_TRY(grow_synced(m->hp, (size_t)B * d));
  EIOKU_TRY(grow_synced(m->pick, (size_t)B));
  EIOKU_TRY(grow_synced(m->pooled, (size_t)B * m->proj_dim));
  return grow_synced(m->unit, (size_t)B * m->proj_dim);
}

// the residual stream m->x [B n][d] through the tower's layers
template <bool CAUSAL>
int run_layers(Model* m, int tower, int B, int n, hipStream_t st) {
  const Tower& t = m->tw[tower];
  const int d = t.d, M = B * n;
  float* x = m->x;
  for (const Layer& L : t.L) {
    EIOKU_TRY(ln<h16>(m, st, x, M, d, L.ln1, nullptr, m->h.p));
    EIOKU_TRY((gemm<4, EPI_F16>(m, st, m->h, d, L.qkv.w, L.qkv.b, M, 3 * d, d, m->qkv.p, 3 * d)));
    hipLaunchKernelGGL(k_attn_seq<CAUSAL>, dim3((n + 63) / 64, t.heads, B), dim3(256), 0, st, m->qkv.p, n, t.heads, m->a.p);
    EIOKU_LAUNCH_CHECK();
    m->flops += 4.0 * B * t.heads * (double)n * n * 64 * (CAUSAL ? 0.5 : 1.0);
    EIOKU_TRY((gemm<4, EPI_RESID>(m, st, m->a, d, L.out.w, L.out.b, M, d, d, x, d)));
    EIOKU_TRY(ln<h16>(m, st, x, M, d, L.ln2, nullptr, m->h.p));
    if (m->act == 0)
      EIOKU_TRY((gemm<4, EPI_QGELU_F16>(m, st, m->h, d, L.fc1.w, L.fc1.b, M, t.ffn, d, m->mid.p, t.ffn)));
    else
      EIOKU_TRY((gemm<4, EPI_GELU_F16>(m, st, m->h, d, L.fc1.w, L.fc1.b, M, t.ffn, d, m->mid.p, t.ffn)));
    EIOKU_TRY((gemm<4, EPI_RESID>(m, st, m->mid, t.ffn, L.fc2.w, L.fc2.b, M, d, t.ffn, x, d)));
  }
  return EIOKU_OK;
}

// rows pick_host[b] of the stream -> final LayerNorm -> projection -> unit vectors in m->unit [B][projection_dim]
int run_head(Model* m, int tower, int B, const int* pick_host, hipStream_t st) {
  const Tower& t = m->tw[tower];
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->pick, pick_host, (size_t)B * 4, hipMemcpyHostToDevice, st));
  EIOKU_TRY(ln<h16>(m, st, m->x, B, t.d, t.final_ln, m->pick.p, m->hp.p));
  EIOKU_TRY((gemm<1, EPI_F32>(m, st, m->hp, t.d, t.proj, -1, B, m->proj_dim, t.d, m->pooled.p, m->proj_dim)));
  hipLaunchKernelGGL(k_l2norm, dim3((B + 3) / 4), dim3(256), 0, st, m->pooled.p, B, m->proj_dim, m->unit.p);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// patch rows [B][1 + P][Kp] fp16 (device) -> m->x after every layer, m->unit
int run_vision(Model* m, const h16* patches, int B, hipStream_t st) {
  const Tower& t = m->tw[VISION];
  const int d = t.d, n = 1 + m->P, M = B * n;
  if (!m->table_ready) {
    const size_t e = (size_t)n * d;
    hipLaunchKernelGGL(k_vision_table, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st, m->F(m->cls), m->F(m->vpos), n, d, m->vtable.p);
    EIOKU_LAUNCH_CHECK();
    m->table_ready = true;
  }
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[1], st));
  EIOKU_TRY((gemm<4, EPI_POS>(m, st, patches, m->Kp, m->patch_w, -1, M, d, m->Kp, m->x0.p, d, m->vtable, n)));
  EIOKU_TRY(ln<float>(m, st, m->x0, M, d, m->pre_ln, nullptr, m->x.p));
  EIOKU_TRY(run_layers<false>(m, VISION, B, n, st));
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[2], st));
  m->pick_host.resize(B);
  for (int b = 0; b < B; ++b) m->pick_host[b] = b * n;
  EIOKU_TRY(run_head(m, VISION, B, m->pick_host.data(), st));
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[3], st));
  return EIOKU_OK;
}

int copy_out(const float* src, size_t n, float* dst, int mem, hipStream_t st) {
  EIOKU_HIP_CHECK(hipMemcpyAsync(dst, src, n * 4, mem == EIOKU_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
  return EIOKU_OK;
}

int preprocess(Model* m, const uint8_t* bgr, int n, int h, int w, const int32_t* xbounds, const int32_t* xk, int kx, const int32_t* ybounds,
               const int32_t* yk, int ky, h16* patches, uint8_t* out_u8, int mem, hipStream_t st) {
  if (patches) EIOKU_HIP_CHECK(hipMemsetAsync(patches, 0, (size_t)n * (1 + m->P) * m->Kp * sizeof(h16), st));  // token 0, the K padding
  return clip_resize(bgr, n, 1, h, w, m->image, xbounds, xk, kx, ybounds, yk, ky, m->nrm, m->patch, 1, m->Kp, patches, out_u8, mem,
                     m->tables, m->src, m->tmp, st);
}

}  // namespace

extern "C" {

int eioku_clip_create(int image, int patch, int v_hidden, int v_layers, int v_heads, int v_ffn, int vocab, int positions, int t_hidden,
                      int t_layers, int t_heads, int t_ffn, int projection_dim, float ln_eps, int act, eioku_clip** out) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(out, "NULL argument");
  EIOKU_REQUIRE(v_hidden > 0 && v_heads > 0 && v_heads * 64 == v_hidden, "vision head_dim must be 64 (hidden %d / heads %d)", v_hidden,
                v_heads);
  EIOKU_REQUIRE(t_hidden > 0 && t_heads > 0 && t_heads * 64 == t_hidden, "text head_dim must be 64 (hidden %d / heads %d)", t_hidden,
                t_heads);
  EIOKU_REQUIRE(image > 0 && image <= kMaxImage, "image_size must be in [1, %d] (got %d)", kMaxImage, image);
  EIOKU_REQUIRE(patch > 0 && image % patch == 0, "image_size %d must be a multiple of patch_size %d", image, patch);
  EIOKU_REQUIRE(positions >= 1 && positions <= kMaxPositions, "max_position_embeddings must be in [1, %d] (got %d)", kMaxPositions,
                positions);
  EIOKU_REQUIRE(v_layers >= 0 && t_layers >= 0 && v_ffn > 0 && v_ffn % 32 == 0 && t_ffn > 0 && t_ffn % 32 == 0 && vocab > 0 &&
                    projection_dim > 0 && ln_eps > 0.f && (act == 0 || act == 1),
                "bad config (layers %d / %d, ffn %d / %d multiples of 32, vocab %d, projection_dim %d, ln_eps %g, act %d)", v_layers,
                t_layers, v_ffn, t_ffn, vocab, projection_dim, (double)ln_eps, act);
  auto* m = new eioku_clip();
  m->image = image, m->patch = patch, m->side = image / patch, m->P = m->side * m->side;
  m->K = 3 * patch * patch, m->Kp = (m->K + 31) / 32 * 32;
  m->vocab = vocab, m->positions = positions, m->proj_dim = projection_dim, m->act = act, m->eps = ln_eps;
  m->tw[VISION].d = v_hidden, m->tw[VISION].layers = v_layers, m->tw[VISION].heads = v_heads, m->tw[VISION].ffn = v_ffn;
  m->tw[TEXT].d = t_hidden, m->tw[TEXT].layers = t_layers, m->tw[TEXT].heads = t_heads, m->tw[TEXT].ffn = t_ffn;
  int tower = TEXT;
  auto add = [&](const std::string& n, int rows, int cols, int kind, int ld = 0) {
    Tensor t;
    t.name = n, t.rows = rows, t.cols = cols, t.kind = kind, t.ld = ld ? ld : cols, t.tower = tower;
    m->tensors.push_back(std::move(t));
    return (int)m->tensors.size() - 1;
  };
  auto part = [&](const std::string& n, int rows, int cols, int kind, int into, int row0) {
    const int i = add(n, rows, cols, kind);
    m->tensors[i].into = into, m->tensors[i].row0 = row0;
    return i;
  };
  auto lin = [&](const std::string& p, int rows, int cols) {
    Lin l;
    l.w = add(p + ".weight", rows, cols, T_F16);
    l.b = add(p + ".bias", rows, 1, T_F32);
    return l;
  };
  auto lnorm = [&](const std::string& p, int d) {
    LNorm l;
    l.g = add(p + ".weight", d, 1, T_F32);
    l.b = add(p + ".bias", d, 1, T_F32);
    return l;
  };
  // the order of CLIPModel.state_dict(): text_model, vision_model, visual_projection, text_projection
  auto layers = [&](const std::string& model, Tower& t) {
    for (int l = 0; l < t.layers; ++l) {
      const std::string p = model + ".encoder.layers." + std::to_string(l) + ".";
      Layer L;
      L.qkv.w = add(p + "self_attn.qkv.weight", 3 * t.d, t.d, T_F16);
      L.qkv.b = add(p + "self_attn.qkv.bias", 3 * t.d, 1, T_F32);
      m->tensors[L.qkv.w].listed = m->tensors[L.qkv.b].listed = false;
      const char* names[3] = {"k_proj", "v_proj", "q_proj"};  // state_dict() order; packed as q | k | v
      const int third[3] = {1, 2, 0};
      for (int j = 0; j < 3; ++j) {
        part(p + "self_attn." + names[j] + ".weight", t.d, t.d, T_F16, L.qkv.w, third[j] * t.d);
        part(p + "self_attn." + names[j] + ".bias", t.d, 1, T_F32, L.qkv.b, third[j] * t.d);
      }
      L.out = lin(p + "self_attn.out_proj", t.d, t.d);
      L.ln1 = lnorm(p + "layer_norm1", t.d);
      L.fc1 = lin(p + "mlp.fc1", t.ffn, t.d);
      L.fc2 = lin(p + "mlp.fc2", t.d, t.ffn);
      L.ln2 = lnorm(p + "layer_norm2", t.d);
      t.L.push_back(L);
    }
  };
  {
    Tower& t = m->tw[TEXT];
    m->tok = add("text_model.embeddings.token_embedding.weight", vocab, t.d, T_F32);
    m->tpos = add("text_model.embeddings.position_embedding.weight", positions, t.d, T_F32);
    layers("text_model", t);
    t.final_ln = lnorm("text_model.final_layer_norm", t.d);
  }
  tower = VISION;
  {
    Tower& t = m->tw[VISION];
    m->cls = add("vision_model.embeddings.class_embedding", 1, t.d, T_F32);
    m->patch_w = add("vision_model.embeddings.patch_embedding.weight", t.d, m->K, T_F16, m->Kp);
    m->vpos = add("vision_model.embeddings.position_embedding.weight", 1 + m->P, t.d, T_F32);
    m->pre_ln = lnorm("vision_model.pre_layrnorm", t.d);
    layers("vision_model", t);
    t.final_ln = lnorm("vision_model.post_layernorm", t.d);
    t.proj = add("visual_projection.weight", projection_dim, t.d, T_F16);
  }
  tower = TEXT;
  m->tw[TEXT].proj = add("text_projection.weight", projection_dim, m->tw[TEXT].d, T_F16);
  auto fail = [&](int rc) {
    eioku_clip_destroy(m);
    return rc;
  };
  for (size_t i = 0; i < m->tensors.size(); ++i) {
    Tensor& t = m->tensors[i];
    if (t.listed) m->listed.push_back((int)i);
    if (t.into >= 0) continue;
    if (t.dev.grow((size_t)t.rows * t.ld * (t.kind == T_F32 ? 4 : 2))) return fail(EIOKU_ENOMEM);
  }
  if (m->vtable.grow((size_t)(1 + m->P) * v_hidden)) return fail(EIOKU_ENOMEM);
  for (auto& ev : m->ev)
    if (hipEventCreate(&ev) != hipSuccess) {
      ev = nullptr;
      set_error("hipEventCreate failed");
      return fail(EIOKU_EHIP);
    }
  *out = m;
  return EIOKU_OK;
}

void eioku_clip_destroy(eioku_clip* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  for (auto ev : m->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete m;  // every buffer frees itself
}

int eioku_clip_num_tensors(const eioku_clip* m) { return m ? (int)m->listed.size() : 0; }

int eioku_clip_tensor_info(const eioku_clip* m, int idx, char* name, size_t cap, int* rows, int* cols) {
  EIOKU_REQUIRE(m && idx >= 0 && idx < (int)m->listed.size(), "bad tensor index %d", idx);
  const auto& t = m->tensors[m->listed[idx]];
  if (name && cap) snprintf(name, cap, "%s", t.name.c_str());
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return EIOKU_OK;
}

int eioku_clip_set_tensor(eioku_clip* m, int idx, const float* host, size_t numel) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && idx >= 0 && idx < (int)m->listed.size() && host, "bad argument");
  auto& t = m->tensors[m->listed[idx]];
  EIOKU_REQUIRE(numel == t.numel(), "%s: expected %zu elements, got %zu", t.name.c_str(), t.numel(), numel);
  EIOKU_HIP_CHECK(hipDeviceSynchronize());  // no pass may still read the old value
  void* dst = const_cast<uint8_t*>(m->base(m->listed[idx]));
  if (t.kind == T_F32) {
    EIOKU_HIP_CHECK(hipMemcpy(dst, host, numel * sizeof(float), hipMemcpyHostToDevice));  // fp32 tensors have ld == cols
  } else {
    DevBuf<float> stage;
    EIOKU_TRY(stage.grow(numel));
    EIOKU_HIP_CHECK(hipMemcpy(stage, host, numel * sizeof(float), hipMemcpyHostToDevice));
    const size_t e = (size_t)t.rows * t.ld;
    hipLaunchKernelGGL(k_cvt_f16_pad, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, 0, stage.p, t.rows, t.cols, t.ld, (h16*)dst);
    EIOKU_LAUNCH_CHECK();
    EIOKU_HIP_CHECK(hipDeviceSynchronize());
  }
  t.set = true;
  m->table_ready = false;
  return EIOKU_OK;
}

int eioku_clip_set_norm(eioku_clip* m, const float* mean_rgb, const float* std_rgb) {
  EIOKU_REQUIRE(m && mean_rgb && std_rgb, "NULL argument");
  for (int c = 0; c < 3; ++c) {
    EIOKU_REQUIRE(std_rgb[c] > 0.f, "image_std must be positive");
    m->nrm.mean[c] = mean_rgb[c], m->nrm.std[c] = std_rgb[c];
  }
  return EIOKU_OK;
}

// n BGR u8 frames (h x w, [n][h][w][3], host or device) -> patches_out [n][1 + P][Kp] fp16 (device, optional) and / or
// out_rgb_u8 [n][S][S][3] (device, optional: the resized and cropped RGB image).  Tables from the host (eioku_amd/visual.py):
// the S rows of Pillow's bicubic tables that the centre crop keeps, per axis.
int eioku_clip_preprocess(eioku_clip* m, const uint8_t* bgr, int n, int h, int w, const int32_t* xbounds, const int32_t* xk, int kx,
                          const int32_t* ybounds, const int32_t* yk, int ky, void* patches_out, uint8_t* out_rgb_u8, int mem,
                          void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n >= 0 && h > 0 && w > 0 && kx > 0 && ky > 0 && xbounds && xk && ybounds && yk, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr, "NULL frames");
  hipStream_t st = (hipStream_t)stream_;
  EIOKU_TRY(preprocess(m, bgr, n, h, w, xbounds, xk, kx, ybounds, yk, ky, (h16*)patches_out, out_rgb_u8, mem, st));
  if (mem == EIOKU_MEM_HOST) EIOKU_HIP_CHECK(hipStreamSynchronize(st));  // the caller may reuse its host buffer
  return EIOKU_OK;
}

// The vision tower on patch rows [n][1 + P][Kp] fp16 (device) -> out [n][projection_dim] fp32 unit vectors (device) and
// optionally hidden_out [n][1 + P][hidden] fp32 (device): the residual stream after the last layer, before post_layernorm.
// Asynchronous.
int eioku_clip_encode_patches(eioku_clip* m, const void* patches, int n, float* out, float* hidden_out, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n >= 0, "bad argument");
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(patches && out, "NULL buffer");
  EIOKU_TRY(check_weights(m, VISION));
  hipStream_t st = (hipStream_t)stream_;
  const size_t M = (size_t)n * (1 + m->P);
  EIOKU_TRY(ensure_rows(m, VISION, M, n));
  m->flops = 0;
  m->timed[0] = false, m->timed[1] = m->timed[2] = true;
  EIOKU_TRY(run_vision(m, (const h16*)patches, n, st));
  EIOKU_TRY(copy_out(m->unit, (size_t)n * m->proj_dim, out, EIOKU_MEM_DEVICE, st));
  if (hidden_out) EIOKU_TRY(copy_out(m->x, M * m->tw[VISION].d, hidden_out, EIOKU_MEM_DEVICE, st));
  return EIOKU_OK;
}

// preprocess + the vision tower on n frames (host or device) -> out [n][projection_dim] fp32 unit vectors on the side `mem`
// names.  A host output synchronises the stream.
int eioku_clip_encode_images(eioku_clip* m, const uint8_t* bgr, int n, int h, int w, const int32_t* xbounds, const int32_t* xk, int kx,
                             const int32_t* ybounds, const int32_t* yk, int ky, float* out, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n >= 0 && h > 0 && w > 0 && kx > 0 && ky > 0 && xbounds && xk && ybounds && yk, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(bgr && out, "NULL buffer");
  EIOKU_TRY(check_weights(m, VISION));
  hipStream_t st = (hipStream_t)stream_;
  const size_t M = (size_t)n * (1 + m->P);
  EIOKU_TRY(ensure_rows(m, VISION, M, n));
  EIOKU_TRY(grow_synced(m->patches, M * m->Kp));
  m->flops = 0;
  m->timed[0] = m->timed[1] = m->timed[2] = true;
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[0], st));
  EIOKU_TRY(preprocess(m, bgr, n, h, w, xbounds, xk, kx, ybounds, yk, ky, m->patches.p, nullptr, mem, st));
  EIOKU_TRY(run_vision(m, m->patches.p, n, st));
  EIOKU_TRY(copy_out(m->unit, (size_t)n * m->proj_dim, out, mem, st));
  if (mem == EIOKU_MEM_HOST) EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

// The text tower: ids [n_texts][positions] int32 and eot [n_texts] int32 (HOST; eot = the position whose row is pooled), run
// over positions 0 .. n - 1 (every eot < n <= positions) -> out [n_texts][projection_dim] fp32 unit vectors and optionally
// hidden_out [n_texts][n][hidden] fp32 (the residual stream after the last layer, before final_layer_norm), both on the side
// `mem` names.  Host outputs synchronise the stream.
int eioku_clip_encode_text(eioku_clip* m, const int32_t* ids, const int32_t* eot, int n_texts, int n, float* out, float* hidden_out,
                           int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && n_texts >= 0, "bad argument");
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  if (n_texts == 0) return EIOKU_OK;
  EIOKU_REQUIRE(ids && eot && out, "NULL buffer");
  EIOKU_REQUIRE(n >= 1 && n <= m->positions, "n must be in [1, %d] (got %d)", m->positions, n);
  for (int b = 0; b < n_texts; ++b) {
    EIOKU_REQUIRE(eot[b] >= 0 && eot[b] < n, "text %d: eot position %d outside the %d positions run", b, eot[b], n);
    for (int i = 0; i < n; ++i) {
      const int id = ids[(size_t)b * m->positions + i];
      EIOKU_REQUIRE(id >= 0 && id < m->vocab, "text %d: token id %d outside the vocabulary of %d", b, id, m->vocab);
    }
  }
  EIOKU_TRY(check_weights(m, TEXT));
  hipStream_t st = (hipStream_t)stream_;
  const Tower& t = m->tw[TEXT];
  const size_t M = (size_t)n_texts * n;
  EIOKU_TRY(ensure_rows(m, TEXT, M, n_texts));
  EIOKU_TRY(grow_synced(m->ids, (size_t)n_texts * m->positions));
  m->flops = 0;
  m->timed[0] = false, m->timed[1] = m->timed[2] = true;
  m->ids_host.assign(ids, ids + (size_t)n_texts * m->positions);
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->ids, m->ids_host.data(), m->ids_host.size() * 4, hipMemcpyHostToDevice, st));
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[1], st));
  hipLaunchKernelGGL(k_text_embed, dim3((unsigned)((M * t.d + 255) / 256)), dim3(256), 0, st, m->ids.p, n_texts, n, m->positions, t.d,
                     m->F(m->tok), m->F(m->tpos), m->x.p);
  EIOKU_LAUNCH_CHECK();
  EIOKU_TRY(run_layers<true>(m, TEXT, n_texts, n, st));
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[2], st));
  m->pick_host.resize(n_texts);
  for (int b = 0; b < n_texts; ++b) m->pick_host[b] = b * n + eot[b];
  EIOKU_TRY(run_head(m, TEXT, n_texts, m->pick_host.data(), st));
  EIOKU_HIP_CHECK(hipEventRecord(m->ev[3], st));
  EIOKU_TRY(copy_out(m->unit, (size_t)n_texts * m->proj_dim, out, mem, st));
  if (hidden_out) EIOKU_TRY(copy_out(m->x, M * t.d, hidden_out, mem, st));
  if (mem == EIOKU_MEM_HOST) EIOKU_HIP_CHECK(hipStreamSynchronize(st));
  return EIOKU_OK;
}

int eioku_clip_last_flops(const eioku_clip* m, double* flops) {
  EIOKU_REQUIRE(m && flops, "NULL argument");
  *flops = m->flops;
  return EIOKU_OK;
}

// device milliseconds of the last encode call per stage (0 for a stage that call did not run); waits for it
int eioku_clip_last_ms(const eioku_clip* m, double* preprocess_ms, double* encoder_ms, double* head_ms) {
  EIOKU_REQUIRE(m && preprocess_ms && encoder_ms && head_ms, "NULL argument");
  double* out[3] = {preprocess_ms, encoder_ms, head_ms};
  for (int i = 0; i < 3; ++i) {
    *out[i] = 0.0;
    if (!m->timed[i]) continue;
    float ms = 0.f;
    EIOKU_HIP_CHECK(hipEventSynchronize(m->ev[i + 1]));
    EIOKU_HIP_CHECK(hipEventElapsedTime(&ms, m->ev[i], m->ev[i + 1]));
    *out[i] = ms;
  }
  return EIOKU_OK;
}

}  // extern "C"
