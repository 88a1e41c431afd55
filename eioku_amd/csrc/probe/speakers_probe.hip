// libeioku_hip_probe.so: the pooling and the head of speakers.hip (k_spk_pool, k_spk_head) behind entry points that take device
// pointers (tests/test_convnet_glue_gpu.py).  Test infrastructure as places_probe.hip: the model's source is included unchanged,
// the library carries its own eioku_spk_*, and the grids are run_pool_head's.
#include "../speakers.hip"

extern "C" {

// x [m][10][wf][256] fp16, valid HOST int32 [m] (frames, 9 .. 8 wf) -> stats [m][5120] fp32.  Synchronous (valid is staged).
int eioku_probe_spk_pool(const void* x, const int* valid, int m, int wf, float* stats, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(x && valid && stats, "probe speaker pool: NULL argument");
  EIOKU_REQUIRE(m >= 1 && m <= kPass && wf >= 2, "probe speaker pool: bad shape (m %d of at most %d, wf %d)", m, kPass, wf);
  for (int i = 0; i < m; ++i)
    EIOKU_REQUIRE(valid[i] >= 9 && valid[i] <= 8 * wf, "probe speaker pool: window %d: %d valid frames outside [9, %d]", i, valid[i], 8 * wf);
  DevBuf<int> d_valid;
  EIOKU_TRY(d_valid.grow((size_t)m));
  EIOKU_HIP_CHECK(hipMemcpyAsync(d_valid, valid, (size_t)m * 4, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_spk_pool, dim3(kFreq, (unsigned)m), dim3(256), 0, stream, (const __half*)x, d_valid.p, wf, stats);
  EIOKU_LAUNCH_CHECK();
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  return EIOKU_OK;
}

// stats [m][5120] fp32 -> out [m][256] fp32, weights as eioku_spk_set_head uploaded them
int eioku_probe_spk_head(eioku_spk_t* s, const float* stats, int m, float* out, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(s && stats && out, "probe speaker head: NULL argument");
  EIOKU_REQUIRE(m >= 1 && m <= kPass, "probe speaker head: m = %d outside [1, %d]", m, kPass);
  EIOKU_REQUIRE(s->seg_set, "probe speaker head: seg_1 has no weights");
  hipLaunchKernelGGL(k_spk_head, dim3(kEmb), dim3(256), 0, stream, stats, m, s->seg_w.p, s->seg_b.p, out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // extern "C"
