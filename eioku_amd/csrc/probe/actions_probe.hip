// libeioku_hip_probe.so: TimeSformer's temporal attention (k_attn_time in actions.hip) behind one entry point that takes device
// pointers, so that tests/test_bespoke_attn_gpu.py can compare it with a float64 restatement on its own.  Test infrastructure as
// places_probe.hip: not declared in include/eioku_hip.h, never loaded by the product.  The model's source is included unchanged;
// the launch line repeats the layer loop's under the same names (tests/test_bespoke_attn_host.py compares grid, block and LDS
// size as text).
#include "../actions.hip"

extern "C" {

// qkv [n_seq T][3 * 64 heads] fp16 (q | k | v) -> out [n_seq T][64 heads] fp16; the model's n_seq is B * P
int eioku_probe_attn_time(const void* qkv, int n_seq, int T, int heads, void* out, hipStream_t st) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(qkv && out, "probe temporal attention: NULL argument");
  EIOKU_REQUIRE(n_seq >= 1 && heads >= 1 && T >= 1 && T <= kMaxFrames, "probe temporal attention: bad shape (n_seq %d, T %d in [1, %d], heads %d)",
                n_seq, T, kMaxFrames, heads);
  const long long probs = (long long)n_seq * heads;
  EIOKU_REQUIRE(probs <= 0x7fffffffll, "probe temporal attention: %lld workgroups", probs);
  const size_t lds = (size_t)3 * T * 66 * sizeof(h16) + 96 * sizeof(float);
  hipLaunchKernelGGL(k_attn_time, dim3((unsigned)probs), dim3(64), lds, st, (const h16*)qkv, T, heads, (h16*)out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // extern "C"
