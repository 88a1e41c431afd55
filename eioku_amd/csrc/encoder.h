// The host side of a pre-LN transformer encoder layer over gemm_f16.h, layernorm.h, attn_f16.h and tensors.h: the layer's
// tensors, the activation buffers of one pass, the two launch wrappers a forward pass is written in, and the two sublayers
//   LN -> packed qkv GEMM -> k_attn_tiles<DenseSeq, CAUSAL> -> out-projection (EPI_RESID)
//   LN -> fc1 with the GELU / quick_gelu epilogue -> fc2 (EPI_RESID)
// K26 CLIP's two towers and K29 AST run both per layer; K25 TimeSformer runs the MLP sublayer and builds its temporal and
// spatial attention from Enc::gemm / Enc::ln (k_attn_time, the CLS mean and SpaceTimeSeq are its own).  Two models stay
// outside on purpose: K27 nomic-embed-text is post-LN with RoPE and SwiGLU epilogues and a ragged batch, and K20 Whisper runs
// on stream 0, counts its launches and has its own attention kernel.  Included by actions.hip, clip.hip and sounds.hip;
// everything here has internal linkage.
#pragma once

#include "attn_f16.h"
#include "common.h"
#include "gemm_f16.h"
#include "layernorm.h"
#include "tensors.h"

namespace {

struct EncLayer {
  LNorm ln1, ln2;
  Lin qkv, out, fc1, fc2;
};

// activations of one pass: the fp32 residual stream x [rows][d] and the fp16 GEMM operands h [rows][d], qkv [rows][3 d],
// a [a_rows][d] (attention outputs) and mid [rows][ffn]
struct EncWork {
  eioku::DevBuf<float> x;
  eioku::DevBuf<h16> h, qkv, a, mid;
  int grow(size_t rows, size_t d, size_t ffn, size_t a_rows = 0) {
    EIOKU_TRY(eioku::grow_synced(x, rows * d));
    EIOKU_TRY(eioku::grow_synced(h, rows * d));
    EIOKU_TRY(eioku::grow_synced(qkv, rows * 3 * d));
    EIOKU_TRY(eioku::grow_synced(a, (a_rows ? a_rows : rows) * d));
    return eioku::grow_synced(mid, rows * ffn);
  }
};

// what every launch of a pass shares: the weights, the stream, the width, the LayerNorm eps and the FLOP counter
struct Enc {
  const TensorTable* tt;
  hipStream_t st;
  int d;
  float eps;
  double* flops;

  // w.b < 0: no bias
  template <int MT, int EPI>
  int gemm(const h16* A, int lda, const Lin& w, int M, int N, int K, void* out, long long ldc, const float* pos = nullptr,
           int pos_rows = 1) const {
    return launch_gemm<MT, EPI>(st, A, lda, tt->H(w.w), K, tt->F(w.b), M, N, K, out, ldc, pos, pos_rows, nullptr, flops);
  }

  template <typename OUT>
  int ln(const float* x, int M, const LNorm& p, OUT* out, const int* pick = nullptr) const {
    if (M == 0) return EIOKU_OK;
    hipLaunchKernelGGL(k_ln<OUT>, dim3((M + 3) / 4), dim3(256), 0, st, x, M, d, tt->F(p.g), tt->F(p.b), eps, pick, out);
    EIOKU_LAUNCH_CHECK();
    return EIOKU_OK;
  }
};

// w.x [B n][d] += out(attention(qkv(ln1(w.x)))) over B dense sequences of n tokens
template <bool CAUSAL>
int attn_sublayer(const Enc& e, EncWork& w, const EncLayer& L, int B, int n, int heads) {
  const int d = e.d, M = B * n;
  EIOKU_TRY(e.ln<h16>(w.x, M, L.ln1, w.h.p));
  EIOKU_TRY((e.gemm<4, EPI_F16>(w.h, d, L.qkv, M, 3 * d, d, w.qkv.p, 3 * d)));
  EIOKU_TRY(launch_attn<CAUSAL>(e.st, w.qkv.p, DenseSeq{n, d, w.a.p}, n, heads, B));
  *e.flops += 4.0 * B * heads * (double)n * n * 64 * (CAUSAL ? 0.5 : 1.0);
  return e.gemm<4, EPI_RESID>(w.a, d, L.out, M, d, d, w.x.p, d);
}

// w.x [M][d] += fc2(act(fc1(ln(w.x)))), act = GELU or CLIP's quick_gelu
int mlp_sublayer(const Enc& e, EncWork& w, int M, const LNorm& ln, const Lin& fc1, const Lin& fc2, int ffn, bool quick_gelu) {
  const int d = e.d;
  EIOKU_TRY(e.ln<h16>(w.x, M, ln, w.h.p));
  if (quick_gelu)
    EIOKU_TRY((e.gemm<4, EPI_QGELU_F16>(w.h, d, fc1, M, ffn, d, w.mid.p, ffn)));
  else
    EIOKU_TRY((e.gemm<4, EPI_GELU_F16>(w.h, d, fc1, M, ffn, d, w.mid.p, ffn)));
  return e.gemm<4, EPI_RESID>(w.mid, ffn, fc2, M, d, ffn, w.x.p, d);
}

}  // namespace
