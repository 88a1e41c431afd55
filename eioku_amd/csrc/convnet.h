// Host plumbing shared by the handles of the convolutional networks (YOLO, ResNet18, IResNet, WeSpeaker, CRAFT, CRNN):
// the table of named convolutions with their packed weights, the staging of host frames, and the torchvision
// BasicBlock over four rotating buffers.  Internal: nothing here is part of the C ABI.
#pragma once

#include <string>
#include <vector>

#include "conv.h"

namespace eioku {

struct ConvLayer {
  std::string name;
  int cout, cin, k, stride = 1;  // as the checkpoint has them; the packed form in ConvStack::w may differ
};

// The convolutions of one network in checkpoint order: layer i's shape, its packed weights and whether it has any.
struct ConvStack {
  std::vector<ConvLayer> layers;
  std::vector<ConvWeights> w;
  std::vector<bool> set;

  int size() const { return (int)layers.size(); }
  int add(ConvLayer l) {
    layers.push_back(std::move(l));
    w.emplace_back();
    set.push_back(false);
    return size() - 1;
  }
  void add_all(std::initializer_list<ConvLayer> ls) {
    for (const ConvLayer& l : ls) add(l);
  }
  int check_idx(int idx) const {
    EIOKU_REQUIRE(idx >= 0 && idx < size(), "bad convolution index %d", idx);
    return EIOKU_OK;
  }
  // every output is optional
  int info(int idx, char* name, size_t cap, int* cout, int* cin, int* k, int* stride) const {
    EIOKU_TRY(check_idx(idx));
    const ConvLayer& l = layers[idx];
    if (name && cap) snprintf(name, cap, "%s", l.name.c_str());
    if (cout) *cout = l.cout;
    if (cin) *cin = l.cin;
    if (k) *k = l.k;
    if (stride) *stride = l.stride;
    return EIOKU_OK;
  }
  int all_set() const {
    for (int i = 0; i < size(); ++i) EIOKU_REQUIRE(set[i], "convolution %s has no weights", layers[i].name.c_str());
    return EIOKU_OK;
  }
  // the outcome of packing layer idx's weights: the layer counts as set only when that succeeded
  int mark(int idx, int rc) {
    set[idx] = rc == EIOKU_OK;
    return rc;
  }
};

// *dev = the frames on the device: frames the caller holds on the host are copied (asynchronously) into `stage`, grown
// on demand; device frames are used where they are.
inline int stage_host(DevBuf<uint8_t>& stage, const uint8_t* ptr, size_t bytes, int mem, hipStream_t stream, const uint8_t** dev) {
  *dev = ptr;
  if (mem != EIOKU_MEM_HOST) return EIOKU_OK;
  EIOKU_TRY(stage.grow(bytes));
  EIOKU_HIP_CHECK(hipMemcpyAsync(stage, ptr, bytes, hipMemcpyHostToDevice, stream));
  *dev = stage;
  return EIOKU_OK;
}

// One torchvision BasicBlock on buf[*x] (N x *H x *W x c1.cin): conv1 + ReLU into buf[*x + 1], the shortcut convolution
// (`down`, or nullptr for the identity) into buf[*x + 2], conv2 + shortcut + ReLU into buf[*x + 3], indices modulo 4.
// *x, *H and *W move on to the block's output.
inline int basic_block(const ConvWeights& c1, const ConvWeights& c2, const ConvWeights* down, const DevBuf<__half> (&buf)[4],
                       int* x, int N, int* H, int* W, hipStream_t stream) {
  const int t = (*x + 1) & 3, idn = (*x + 2) & 3, y = (*x + 3) & 3;
  const int Ho = conv_out_dim(*H, 3, c1.stride), Wo = conv_out_dim(*W, 3, c1.stride);
  Slice in{buf[*x], c1.cin, 0}, mid{buf[t], c1.cout, 0}, out{buf[y], c2.cout, 0}, res = in;
  EIOKU_TRY(conv_forward(c1, in, N, *H, *W, mid, nullptr, Slice{}, kActReLU, stream));
  if (down) {
    res = Slice{buf[idn], c2.cout, 0};
    EIOKU_TRY(conv_forward(*down, in, N, *H, *W, res, nullptr, Slice{}, kActNone, stream));
  }
  EIOKU_TRY(conv_forward(c2, mid, N, Ho, Wo, out, nullptr, res, kActResReLU, stream));
  *x = y;
  *H = Ho;
  *W = Wo;
  return EIOKU_OK;
}

}  // namespace eioku
