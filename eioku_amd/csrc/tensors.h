// The named-tensor table of the transformer models (K20 Whisper, K25 TimeSformer, K26 CLIP, K27 nomic-embed-text, K29 AST): the
// tensors of a state_dict() in its order, their device copies, and what *_num_tensors / *_tensor_info / *_set_tensor do with
// them.  A model's handle derives from TensorTable and lists its tensors in its create function.  Included by whisper.hip and
// nomic.hip, and through encoder.h by actions.hip, clip.hip and sounds.hip; everything here has internal linkage.
#pragma once

#include "common.h"
#include "gemm_f16.h"

#include <string>
#include <vector>

namespace {

// how a tensor is kept on the device: T_F16 one rounding to fp16, T_F32 as it is, T_CONV a [rows][cin][3] convolution weight as
// fp16 [rows][ld] with column tap * cin + c
enum { T_F16 = 0, T_F32 = 1, T_CONV = 2 };
// where source row i lands among the stored rows (ROWS_ROPE, ROWS_EVEN, ROWS_ODD: the pair epilogues of gemm_f16.h)
enum { ROWS_PLAIN = 0, ROWS_ROPE = 1, ROWS_EVEN = 2, ROWS_ODD = 3 };

__device__ __forceinline__ size_t stored_row(int i, int mode) {
  if (mode == ROWS_ROPE) {  // within a 64-row head: stored row 2j = dimension j, 2j + 1 = dimension j + 32
    const int j = i & 63;
    return (size_t)(i - j) + (j < 32 ? 2 * j : 2 * (j - 32) + 1);
  }
  if (mode == ROWS_EVEN) return (size_t)2 * i;
  if (mode == ROWS_ODD) return (size_t)2 * i + 1;
  return (size_t)i;
}

// src [rows][cols] fp32 (conv: [rows][cols / 3][3]) -> rows stored_row(i) of dst [.][ld] fp16, columns cols .. ld - 1 zero
__global__ __launch_bounds__(256) void k_cvt(const float* __restrict__ src, int rows, int cols, int ld, int conv, int mode,
                                             h16* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * ld) return;
  const int c = (int)(i % ld), cin = cols / 3;
  const size_t r = i / ld;
  float v = 0.f;
  if (c < cols) v = conv ? src[(r * cin + c % cin) * 3 + c / cin] : src[r * cols + c];
  dst[stored_row((int)r, mode) * ld + c] = (h16)v;
}

// A named tensor.  Its device value is `dev` ([rows][ld] elements), or rows of tensor `into` from row0 on, placed by `mode`
// (q_proj, k_proj and v_proj land in one packed weight).
struct Tensor {
  std::string name;
  int rows = 0, cols = 0, kind = T_F16, ld = 0;
  int into = -1, row0 = 0, mode = ROWS_PLAIN;
  int tag = 0;         // the part of the model it belongs to (CLIP's tower)
  bool listed = true;  // packed targets are not part of the state_dict()
  eioku::DevBuf<uint8_t> dev;
  bool set = false;
  size_t numel() const { return (size_t)rows * cols; }
  size_t elem() const { return kind == T_F32 ? 4 : 2; }
};

struct Lin { int w, b; };
struct LNorm { int g, b; };

struct TensorTable {
  std::vector<Tensor> tensors;
  std::vector<int> listed;  // indices of the state_dict() tensors, in order
  int tag = 0;              // given to the tensors added from here on

  // ld: the device row length in elements; 0 = cols, for T_CONV cols rounded up to 32
  int add(const std::string& name, int rows, int cols, int kind, int ld = 0) {
    Tensor t;
    t.name = name, t.rows = rows, t.cols = cols, t.kind = kind, t.tag = tag;
    t.ld = ld ? ld : kind == T_CONV ? (cols + 31) / 32 * 32 : cols;
    tensors.push_back(std::move(t));
    return (int)tensors.size() - 1;
  }
  // a device tensor that state_dict() tensors are packed into
  int packed(const std::string& name, int rows, int cols, int kind) {
    const int i = add(name, rows, cols, kind);
    tensors[i].listed = false;
    return i;
  }
  int part(const std::string& name, int rows, int cols, int into, int row0, int mode = ROWS_PLAIN) {
    const int i = add(name, rows, cols, tensors[into].kind);
    tensors[i].into = into, tensors[i].row0 = row0, tensors[i].mode = mode;
    return i;
  }
  Lin lin(const std::string& prefix, int rows, int cols) {
    Lin l;
    l.w = add(prefix + ".weight", rows, cols, T_F16);
    l.b = add(prefix + ".bias", rows, 1, T_F32);
    return l;
  }
  LNorm lnorm(const std::string& prefix, int d) {
    LNorm l;
    l.g = add(prefix + ".weight", d, 1, T_F32);
    l.b = add(prefix + ".bias", d, 1, T_F32);
    return l;
  }
  // after the last add: the list of state_dict() tensors, and the device memory of every tensor that is not a part
  int finish() {
    for (size_t i = 0; i < tensors.size(); ++i) {
      Tensor& t = tensors[i];
      if (t.listed) listed.push_back((int)i);
      if (t.into < 0) EIOKU_TRY(t.dev.grow((size_t)t.rows * t.ld * t.elem()));
    }
    return EIOKU_OK;
  }

  const uint8_t* base(int i) const {
    const Tensor& t = tensors[i];
    return t.into < 0 ? t.dev.p : tensors[t.into].dev.p + (size_t)t.row0 * t.ld * t.elem();
  }
  const h16* H(int i) const { return (const h16*)base(i); }
  const float* F(int i) const { return i < 0 ? nullptr : (const float*)base(i); }

  // every state_dict() tensor, or those with this tag, has been set
  int check(int only_tag = -1) const {
    for (int i : listed) {
      const Tensor& t = tensors[i];
      EIOKU_REQUIRE((only_tag >= 0 && t.tag != only_tag) || t.set, "tensor %s has no weights", t.name.c_str());
    }
    return EIOKU_OK;
  }

  // the bodies of *_num_tensors, *_tensor_info and *_set_tensor; tt is NULL for a NULL handle
  static int count(const TensorTable* tt) { return tt ? (int)tt->listed.size() : 0; }

  static int info(const TensorTable* tt, int idx, char* name, size_t cap, int* rows, int* cols) {
    EIOKU_REQUIRE(tt && idx >= 0 && idx < (int)tt->listed.size(), "bad tensor index %d", idx);
    const Tensor& t = tt->tensors[tt->listed[idx]];
    if (name && cap) snprintf(name, cap, "%s", t.name.c_str());
    if (rows) *rows = t.rows;
    if (cols) *cols = t.cols;
    return EIOKU_OK;
  }

  static int set(TensorTable* tt, int idx, const float* host, size_t numel) {
    EIOKU_REQUIRE_INIT();
    EIOKU_REQUIRE(tt && idx >= 0 && idx < (int)tt->listed.size() && host, "bad argument");
    Tensor& t = tt->tensors[tt->listed[idx]];
    EIOKU_REQUIRE(numel == t.numel(), "%s: expected %zu elements, got %zu", t.name.c_str(), t.numel(), numel);
    EIOKU_HIP_CHECK(hipDeviceSynchronize());  // no pass may still read the old value
    void* dst = const_cast<uint8_t*>(tt->base(tt->listed[idx]));
    if (t.kind == T_F32) {
      EIOKU_HIP_CHECK(hipMemcpy(dst, host, numel * sizeof(float), hipMemcpyHostToDevice));  // fp32 tensors have ld == cols
    } else {
      eioku::DevBuf<float> stage;
      EIOKU_TRY(stage.grow(numel));
      EIOKU_HIP_CHECK(hipMemcpy(stage, host, numel * sizeof(float), hipMemcpyHostToDevice));
      const size_t e = (size_t)t.rows * t.ld;
      hipLaunchKernelGGL(k_cvt, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, 0, stage.p, t.rows, t.cols, t.ld, t.kind == T_CONV,
                         t.mode, (h16*)dst);
      EIOKU_LAUNCH_CHECK();
      EIOKU_HIP_CHECK(hipDeviceSynchronize());
    }
    t.set = true;
    return EIOKU_OK;
  }
};

}  // namespace
