// libeioku_hip_probe.so: the three shared kernels of the transformer models (gemm_f16.h, attn_f16.h, layernorm.h), each behind
// one entry point that takes device pointers, so that tests/test_transformer_core_gpu.py can compare them with a float64
// restatement one kernel at a time.  Test infrastructure: linked with core.o only, never loaded by the product, and not
// declared in include/eioku_hip.h.  The headers are included unchanged: what is tested here is what the models run.
#include "../attn_f16.h"
#include "../gemm_f16.h"
#include "../layernorm.h"

namespace {

// Every (MT, EPI) pair that whisper.hip, actions.hip, clip.hip or nomic.hip instantiates, and no other:
// tests/test_transformer_core_host.py compares this list with the models' sources.
#define EIOKU_PROBE_GEMM_TABLE(X) \
  X(1, EPI_F16)                   \
  X(4, EPI_F16)                   \
  X(1, EPI_GELU_F16)              \
  X(4, EPI_GELU_F16)              \
  X(1, EPI_RESID)                 \
  X(4, EPI_RESID)                 \
  X(4, EPI_GELU_POS)              \
  X(1, EPI_F32)                   \
  X(4, EPI_F32)                   \
  X(4, EPI_POS)                   \
  X(4, EPI_QGELU_F16)             \
  X(4, EPI_ROPE_F16)              \
  X(4, EPI_SWIGLU_F16)

enum { kDense = 0, kRagged = 1, kSpaceTime = 2 };

}  // namespace

extern "C" {

int eioku_probe_gemm(int mt, int epi, const void* A, int lda, const void* W, int ldw, const float* bias, int M, int N, int K, void* out,
                     long long ldc, const float* pos, int pos_rows, const int* row_pos, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(A && W && out && M >= 0 && N > 0 && K > 0, "probe GEMM: NULL argument or bad shape (M %d, N %d, K %d)", M, N, K);
  EIOKU_REQUIRE(lda >= K && ldw >= K, "probe GEMM: lda %d / ldw %d below K %d", lda, ldw, K);
  EIOKU_REQUIRE(ldc >= (epi == EPI_SWIGLU_F16 ? N / 2 : N), "probe GEMM: ldc %lld below the output's %d columns", ldc, N);
  if (epi == EPI_POS || epi == EPI_GELU_POS || epi == EPI_ROPE_F16) EIOKU_REQUIRE(pos && pos_rows >= 1, "probe GEMM: no pos table");
  if (epi == EPI_ROPE_F16) EIOKU_REQUIRE(row_pos, "probe GEMM: ROPE needs row_pos");
  double flops = 0;
  const h16 *a = (const h16*)A, *w = (const h16*)W;
#define X(MT, EPI) \
  if (mt == MT && epi == EPI) return launch_gemm<MT, EPI>(stream, a, lda, w, ldw, bias, M, N, K, out, ldc, pos, pos_rows, row_pos, &flops);
  EIOKU_PROBE_GEMM_TABLE(X)
#undef X
  EIOKU_REQUIRE(false, "probe GEMM: no model instantiates k_gemm<%d, %d>", mt, epi);
}

// policy 0 DenseSeq: `sequences` sequences of `longest` tokens; 1 RaggedSeq: cu [sequences + 1] on the device; 2 SpaceTimeSeq:
// B T sequences of 1 + P tokens, out = out_patch.  len, cu and out_cls are read by their own policy alone.
int eioku_probe_attn(int policy, int causal, const void* qkv, int heads, int sequences, int longest, int len, const int* cu, int B, int P,
                     int T, void* out, void* out_cls, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(qkv && out && heads >= 1 && sequences >= 1 && longest >= 1, "probe attention: NULL argument or bad shape");
  const h16* x = (const h16*)qkv;
  const int d = 64 * heads;
  if (policy == kDense) {
    EIOKU_REQUIRE(len == longest, "probe attention: dense len %d != longest %d", len, longest);
    const DenseSeq s{len, d, (h16*)out};
    return causal ? launch_attn<true>(stream, x, s, longest, heads, sequences) : launch_attn<false>(stream, x, s, longest, heads, sequences);
  }
  if (policy == kRagged) {
    EIOKU_REQUIRE(cu, "probe attention: ragged needs cu");
    const RaggedSeq s{cu, d, (h16*)out};
    return causal ? launch_attn<true>(stream, x, s, longest, heads, sequences) : launch_attn<false>(stream, x, s, longest, heads, sequences);
  }
  if (policy == kSpaceTime) {
    EIOKU_REQUIRE(!causal && out_cls && B >= 1 && P >= 1 && T >= 1 && sequences == B * T && longest == 1 + P,
                  "probe attention: space-time needs out_cls, sequences = B T and longest = 1 + P, not causal");
    return launch_attn<false>(stream, x, SpaceTimeSeq{B, P, T, d, (h16*)out, (h16*)out_cls}, longest, heads, sequences);
  }
  EIOKU_REQUIRE(false, "probe attention: unknown policy %d", policy);
}

// the grid of the models' ln helpers: four rows (waves) per workgroup
int eioku_probe_ln(int out_is_f16, const float* x, int M, int d, const float* g, const float* b, float eps, const int* pick, void* out,
                   hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(x && g && b && out && M >= 1 && d >= 1, "probe LayerNorm: NULL argument or bad shape (M %d, d %d)", M, d);
  if (out_is_f16)
    hipLaunchKernelGGL(k_ln<h16>, dim3((M + 3) / 4), dim3(256), 0, stream, x, M, d, g, b, eps, pick, (h16*)out);
  else
    hipLaunchKernelGGL(k_ln<float>, dim3((M + 3) / 4), dim3(256), 0, stream, x, M, d, g, b, eps, pick, (float*)out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // extern "C"
