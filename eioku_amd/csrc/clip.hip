// K26: CLIP image and text towers on gfx950, in the Hugging Face CLIPModel layout (DESIGN.md "K26 CLIP frame and text embeddings").
//   k_clip_resize_h / k_clip_resize_v   (clip_resize.h) Pillow's two-pass 8-bit resample with the host's bicubic tables, the
//                       centre crop, BGR -> RGB, (v * (1 / 255) - mean) / std in fp32, one rounding to fp16, written as patch
//                       rows [image][1 + P][Kp]: token 0 and the columns past 3 p p stay zero (Kp = 3 p p rounded up to 32)
//   k_gemm<., EPI_POS>  (gemm_f16.h) patch projection over all B (1 + P) rows + the table {class_embedding + position[0],
//                       position[1 ..]} into the embedded fp32 stream; the convolution has no bias
//   k_ln<float>         (layernorm.h) pre_layrnorm: fp32 row -> fp32 residual stream;  k_ln<h16>: LayerNorm into the fp16 GEMM
//                       operand, optionally of picked rows only (the head)
//   k_text_embed        token_embedding[id] + position[i] into the fp32 stream, positions 0 .. n - 1 only
//   k_attn_tiles<DenseSeq, CAUSAL>  (attn_f16.h) dense sequences of n tokens, row b n + i: 64 queries per workgroup (4 waves
//                       of 16), keys / values staged through LDS 128 at a time, QK^T and PV on v_mfma_f32_16x16x32_f16 with an
//                       online softmax; CAUSAL: query i sees keys 0 .. i, a wave's key loop ends at its last query's key
//   k_l2norm            the projected rows to unit length in fp32
// Layers are pre-LN, attn_sublayer and mlp_sublayer of encoder.h: LN -> packed qkv GEMM -> attention -> out-projection
// (EPI_RESID) -> LN -> fc1 with the activation epilogue -> fc2 (EPI_RESID).  The text tower runs n = max(eot + 1) positions per text: under the causal mask no row up
// to EOT reads a later one, so the 77 - n pad positions are never computed.
// Precision points (tests/clip_oracle.py, fp16=True, rounds at the same places): matrix weights fp16; biases, LayerNorm
// parameters, the embedding and position tables fp32; the residual stream fp32 (pre_layrnorm writes it unrounded); LayerNorm
// outputs, q / k / v, attention outputs, activation outputs and the patch rows are rounded to fp16; the softmax numerators
// exp(s - max) are rounded to fp16 for the PV MFMA; the projection, the norm and the outputs are fp32.
#include "clip_resize.h"
#include "common.h"
#include "encoder.h"

#include <cmath>
#include <string>
#include <vector>

using namespace eioku;

namespace {

constexpr int kMaxImage = 448, kMaxPositions = 77;

// ---- small kernels ------------------------------------------------------------------------------------------------------
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

// v[row][:] /= |v[row]| in fp32, one wave per row
__global__ __launch_bounds__(256) void k_l2norm(const float* __restrict__ v, int M, int d, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* vr = v + (size_t)row * d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) q += vr[i] * vr[i];
  const float norm = sqrtf(wave_sum(q));
  for (int i = lane; i < d; i += 64) out[(size_t)row * d + i] = vr[i] / norm;
}

// ---- the model ------------------------------------------------------------------------------------------------------------
enum { VISION = 0, TEXT = 1 };

struct Tower {
  int d = 0, layers = 0, heads = 0, ffn = 0;
  std::vector<EncLayer> L;
  LNorm final_ln{};
  int proj = -1;  // [projection_dim][d], no bias
};

}  // namespace

struct eioku_clip : TensorTable {  // tag: the tower
  int image = 0, patch = 0, side = 0, P = 0, K = 0, Kp = 0;  // K = 3 p p, Kp = K rounded up to 32
  int vocab = 0, positions = 0, proj_dim = 0, act = 0;
  float eps = 1e-5f;
  Norm3 nrm{{0.48145466f, 0.4578275f, 0.40821073f}, {0.26862954f, 0.26130258f, 0.27577711f}};
  Tower tw[2];
  int cls = -1, patch_w = -1, vpos = -1, tok = -1, tpos = -1;
  LNorm pre_ln{};
  bool table_ready = false;
  DevBuf<float> vtable;
  // preprocessing
  DevBuf<int> tables;
  DevBuf<uint8_t> src, tmp;
  DevBuf<h16> patches;
  // activations of one pass
  EncWork work;
  DevBuf<float> x0, pooled, unit;
  DevBuf<h16> hp;
  DevBuf<int> ids, pick;
  std::vector<int> ids_host, pick_host;  // what the asynchronous uploads read: alive until the next call
  StageClock<3> clock;  // preprocess / encoder / head
  double flops = 0;
};

namespace {

typedef eioku_clip Model;

Enc enc_of(Model* m, int tower, hipStream_t st) { return Enc{m, st, m->tw[tower].d, m->eps, &m->flops}; }

int ensure_rows(Model* m, int tower, size_t M, int B) {
  const Tower& t = m->tw[tower];
  const size_t d = t.d;
  EIOKU_TRY(m->work.grow(M, d, t.ffn));
  if (tower == VISION) EIOKU_TRY(grow_synced(m->x0, M * d));  // the embedded stream before pre_layrnorm
  EIOKU_TRY(grow_synced(m->hp, (size_t)B * d));
  EIOKU_TRY(grow_synced(m->pick, (size_t)B));
  EIOKU_TRY(grow_synced(m->pooled, (size_t)B * m->proj_dim));
  return grow_synced(m->unit, (size_t)B * m->proj_dim);
}

// the residual stream m->work.x [B n][d] through the tower's layers
template <bool CAUSAL>
int run_layers(Model* m, int tower, int B, int n, hipStream_t st) {
  const Tower& t = m->tw[tower];
  const Enc enc = enc_of(m, tower, st);
  for (const EncLayer& L : t.L) {
    EIOKU_TRY(attn_sublayer<CAUSAL>(enc, m->work, L, B, n, t.heads));
    EIOKU_TRY(mlp_sublayer(enc, m->work, B * n, L.ln2, L.fc1, L.fc2, t.ffn, m->act == 0));
  }
  return EIOKU_OK;
}

// rows pick_host[b] of the stream -> final LayerNorm -> projection -> unit vectors in m->unit [B][projection_dim]
int run_head(Model* m, int tower, int B, const int* pick_host, hipStream_t st) {
  const Tower& t = m->tw[tower];
  const Enc enc = enc_of(m, tower, st);
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->pick, pick_host, (size_t)B * 4, hipMemcpyHostToDevice, st));
  EIOKU_TRY(enc.ln<h16>(m->work.x, B, t.final_ln, m->hp.p, m->pick.p));
  EIOKU_TRY((enc.gemm<1, EPI_F32>(m->hp, t.d, Lin{t.proj, -1}, B, m->proj_dim, t.d, m->pooled.p, m->proj_dim)));
  hipLaunchKernelGGL(k_l2norm, dim3((B + 3) / 4), dim3(256), 0, st, m->pooled.p, B, m->proj_dim, m->unit.p);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// patch rows [B][1 + P][Kp] fp16 (device) -> m->work.x after every layer, m->unit
int run_vision(Model* m, const h16* patches, int B, hipStream_t st) {
  const Enc enc = enc_of(m, VISION, st);
  const int d = enc.d, n = 1 + m->P, M = B * n;
  if (!m->table_ready) {
    const size_t e = (size_t)n * d;
    hipLaunchKernelGGL(k_vision_table, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st, m->F(m->cls), m->F(m->vpos), n, d, m->vtable.p);
    EIOKU_LAUNCH_CHECK();
    m->table_ready = true;
  }
  EIOKU_TRY(m->clock.mark(1, st));
  EIOKU_TRY((enc.gemm<4, EPI_POS>(patches, m->Kp, Lin{m->patch_w, -1}, M, d, m->Kp, m->x0.p, d, m->vtable, n)));
  EIOKU_TRY(enc.ln<float>(m->x0, M, m->pre_ln, m->work.x.p));
  EIOKU_TRY(run_layers<false>(m, VISION, B, n, st));
  EIOKU_TRY(m->clock.mark(2, st));
  m->pick_host.resize(B);
  for (int b = 0; b < B; ++b) m->pick_host[b] = b * n;
  EIOKU_TRY(run_head(m, VISION, B, m->pick_host.data(), st));
  EIOKU_TRY(m->clock.mark(3, st));
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
  // the order of CLIPModel.state_dict(): text_model, vision_model, visual_projection, text_projection
  auto layers = [&](const std::string& model, Tower& t) {
    for (int l = 0; l < t.layers; ++l) {
      const std::string p = model + ".encoder.layers." + std::to_string(l) + ".";
      EncLayer L;
      L.qkv.w = m->packed(p + "self_attn.qkv.weight", 3 * t.d, t.d, T_F16);
      L.qkv.b = m->packed(p + "self_attn.qkv.bias", 3 * t.d, 1, T_F32);
      const char* names[3] = {"k_proj", "v_proj", "q_proj"};  // state_dict() order; packed as q | k | v
      const int third[3] = {1, 2, 0};
      for (int j = 0; j < 3; ++j) {
        m->part(p + "self_attn." + names[j] + ".weight", t.d, t.d, L.qkv.w, third[j] * t.d);
        m->part(p + "self_attn." + names[j] + ".bias", t.d, 1, L.qkv.b, third[j] * t.d);
      }
      L.out = m->lin(p + "self_attn.out_proj", t.d, t.d);
      L.ln1 = m->lnorm(p + "layer_norm1", t.d);
      L.fc1 = m->lin(p + "mlp.fc1", t.ffn, t.d);
      L.fc2 = m->lin(p + "mlp.fc2", t.d, t.ffn);
      L.ln2 = m->lnorm(p + "layer_norm2", t.d);
      t.L.push_back(L);
    }
  };
  m->tag = TEXT;
  {
    Tower& t = m->tw[TEXT];
    m->tok = m->add("text_model.embeddings.token_embedding.weight", vocab, t.d, T_F32);
    m->tpos = m->add("text_model.embeddings.position_embedding.weight", positions, t.d, T_F32);
    layers("text_model", t);
    t.final_ln = m->lnorm("text_model.final_layer_norm", t.d);
  }
  m->tag = VISION;
  {
    Tower& t = m->tw[VISION];
    m->cls = m->add("vision_model.embeddings.class_embedding", 1, t.d, T_F32);
    m->patch_w = m->add("vision_model.embeddings.patch_embedding.weight", t.d, m->K, T_F16, m->Kp);
    m->vpos = m->add("vision_model.embeddings.position_embedding.weight", 1 + m->P, t.d, T_F32);
    m->pre_ln = m->lnorm("vision_model.pre_layrnorm", t.d);
    layers("vision_model", t);
    t.final_ln = m->lnorm("vision_model.post_layernorm", t.d);
    t.proj = m->add("visual_projection.weight", projection_dim, t.d, T_F16);
  }
  m->tag = TEXT;
  m->tw[TEXT].proj = m->add("text_projection.weight", projection_dim, m->tw[TEXT].d, T_F16);
  auto fail = [&](int rc) {
    eioku_clip_destroy(m);
    return rc;
  };
  if (const int rc = m->finish()) return fail(rc);
  if (m->vtable.grow((size_t)(1 + m->P) * v_hidden)) return fail(EIOKU_ENOMEM);
  if (const int rc = m->clock.create()) return fail(rc);
  *out = m;
  return EIOKU_OK;
}

void eioku_clip_destroy(eioku_clip* m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  delete m;  // every buffer and event frees itself
}

int eioku_clip_num_tensors(const eioku_clip* m) { return TensorTable::count(m); }

int eioku_clip_tensor_info(const eioku_clip* m, int idx, char* name, size_t cap, int* rows, int* cols) {
  return TensorTable::info(m, idx, name, cap, rows, cols);
}

int eioku_clip_set_tensor(eioku_clip* m, int idx, const float* host, size_t numel) {
  EIOKU_TRY(TensorTable::set(m, idx, host, numel));
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
  EIOKU_TRY(m->check(VISION));
  hipStream_t st = (hipStream_t)stream_;
  const size_t M = (size_t)n * (1 + m->P);
  EIOKU_TRY(ensure_rows(m, VISION, M, n));
  m->flops = 0;
  m->clock.begin(0b110);
  EIOKU_TRY(run_vision(m, (const h16*)patches, n, st));
  EIOKU_TRY(copy_out(m->unit, (size_t)n * m->proj_dim, out, EIOKU_MEM_DEVICE, st));
  if (hidden_out) EIOKU_TRY(copy_out(m->work.x, M * m->tw[VISION].d, hidden_out, EIOKU_MEM_DEVICE, st));
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
  EIOKU_TRY(m->check(VISION));
  hipStream_t st = (hipStream_t)stream_;
  const size_t M = (size_t)n * (1 + m->P);
  EIOKU_TRY(ensure_rows(m, VISION, M, n));
  EIOKU_TRY(grow_synced(m->patches, M * m->Kp));
  m->flops = 0;
  m->clock.begin(0b111);
  EIOKU_TRY(m->clock.mark(0, st));
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
  EIOKU_TRY(m->check(TEXT));
  hipStream_t st = (hipStream_t)stream_;
  const Tower& t = m->tw[TEXT];
  const size_t M = (size_t)n_texts * n;
  EIOKU_TRY(ensure_rows(m, TEXT, M, n_texts));
  EIOKU_TRY(grow_synced(m->ids, (size_t)n_texts * m->positions));
  m->flops = 0;
  m->clock.begin(0b110);
  m->ids_host.assign(ids, ids + (size_t)n_texts * m->positions);
  EIOKU_HIP_CHECK(hipMemcpyAsync(m->ids, m->ids_host.data(), m->ids_host.size() * 4, hipMemcpyHostToDevice, st));
  EIOKU_TRY(m->clock.mark(1, st));
  hipLaunchKernelGGL(k_text_embed, dim3((unsigned)((M * t.d + 255) / 256)), dim3(256), 0, st, m->ids.p, n_texts, n, m->positions, t.d,
                     m->F(m->tok), m->F(m->tpos), m->work.x.p);
  EIOKU_LAUNCH_CHECK();
  EIOKU_TRY(run_layers<true>(m, TEXT, n_texts, n, st));
  EIOKU_TRY(m->clock.mark(2, st));
  m->pick_host.resize(n_texts);
  for (int b = 0; b < n_texts; ++b) m->pick_host[b] = b * n + eot[b];
  EIOKU_TRY(run_head(m, TEXT, n_texts, m->pick_host.data(), st));
  EIOKU_TRY(m->clock.mark(3, st));
  EIOKU_TRY(copy_out(m->unit, (size_t)n_texts * m->proj_dim, out, mem, st));
  if (hidden_out) EIOKU_TRY(copy_out(m->work.x, M * t.d, hidden_out, mem, st));
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
  double* const out[3] = {preprocess_ms, encoder_ms, head_ms};
  return m->clock.last_ms(out);
}

}  // extern "C"
