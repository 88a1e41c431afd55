// libeioku_hip_probe.so: the hand-written kernels around the conv family in resnet.hip (k_stem7x7, k_maxpool3s2, k_places_head),
// each behind one entry point that takes device pointers, so that tests/test_convnet_glue_gpu.py can compare them with a float64
// restatement one kernel at a time.  Test infrastructure as transformer_probe.hip: not declared in include/eioku_hip.h, never
// loaded by the product.  The model's source is included unchanged, so the kernels are the ones the model runs and the library
// carries its own eioku_resnet18_*: the tests create their handles through it.  The grids are run_network's
// (tests/test_convnet_glue_host.py compares the launch lines).
#include "../resnet.hip"

extern "C" {

// in224 [n][224][224][4] fp16 -> out112 [n][112][112][64] fp16, weights as eioku_resnet18_set_conv(handle, 0, ...) packed them
int eioku_probe_places_stem(eioku_resnet_t* r, const void* in224, int n, void* out112, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && in224 && out112, "probe stem: NULL argument");
  EIOKU_REQUIRE(n >= 1 && n <= 65535, "probe stem: n = %d outside [1, 65535]", n);
  EIOKU_REQUIRE(r->stem_w && r->stem_b, "probe stem: conv 0 has no weights");
  const int N = n;
  hipLaunchKernelGGL(k_stem7x7, dim3(112 / kSTW, 112 / kSTH, (unsigned)N), dim3(256), 0, stream, (const __half*)in224, N, r->stem_w.p, r->stem_b.p,
                     (__half*)out112);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// in [n][h][w][c] fp16 -> out [n][(h - 1) / 2 + 1][(w - 1) / 2 + 1][c] fp16
int eioku_probe_places_maxpool(const void* in, int n, int h, int w, int c, void* out, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(in && out, "probe max pool: NULL argument");
  EIOKU_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 8 && c % 8 == 0, "probe max pool: bad shape (n %d, h %d, w %d, c %d; c %% 8 == 0)", n, h, w,
                c);
  const int N = n;
  const long long work = (long long)N * ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1) * (c / 8);
  EIOKU_REQUIRE(work <= (1ll << 31), "probe max pool: %lld threads", work);
  hipLaunchKernelGGL(k_maxpool3s2, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, (const __half*)in, N, h, w, c, (__half*)out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// x [n][hw][512] fp16 -> logits [n][nc] fp32 (optional), probs / idx [n][top_k]; fc as eioku_resnet18_set_fc uploaded it
int eioku_probe_places_head(eioku_resnet_t* r, const void* x, int n, int hw, int top_k, float* logits, float* probs, int* idx,
                            hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && x && probs && idx, "probe head: NULL argument");
  EIOKU_REQUIRE(r->fc_set, "probe head: fc has no weights");
  EIOKU_REQUIRE(n >= 1 && hw >= 1, "probe head: bad shape (n %d, hw %d)", n, hw);
  EIOKU_REQUIRE(r->nc >= 1 && r->nc <= 512, "probe head: %d classes, more than the sort's 512", r->nc);
  EIOKU_REQUIRE(top_k >= 1 && top_k <= r->nc, "probe head: top_k %d of %d classes", top_k, r->nc);
  const int N = n;
  hipLaunchKernelGGL(k_places_head, dim3((unsigned)N), dim3(256), 0, stream, (const __half*)x, hw, r->fc_w.p, r->fc_b.p, r->nc, top_k,
                     logits, probs, idx);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // extern "C"
