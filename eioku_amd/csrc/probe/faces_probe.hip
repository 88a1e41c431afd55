// libeioku_hip_probe.so: the hand-written kernels around the conv family in faces.hip (k_chan_ops, k_face_fc, k_face_norm) behind
// entry points that take device pointers (tests/test_convnet_glue_gpu.py).  Test infrastructure as places_probe.hip: the model's
// source is included unchanged, the library carries its own eioku_iresnet_*, and the grids are chan_ops' and run_iresnet's.
#include "../faces.hip"

extern "C" {

// in [pixels][c] fp16; slope [c], scale_shift [2 c] (scale | shift) fp32; each of slope, out_act, scale_shift, out_bn may be
// NULL, as in chan_ops; out_act may alias in
int eioku_probe_face_chan_ops(const void* in, long long pixels, int c, const float* slope, void* out_act, const float* scale_shift,
                              void* out_bn, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(in, "probe chan_ops: NULL input");
  EIOKU_REQUIRE(pixels >= 0 && c >= 8 && c % 8 == 0, "probe chan_ops: bad shape (pixels %lld, c %d; c %% 8 == 0)", pixels, c);
  EIOKU_REQUIRE(!out_bn || scale_shift, "probe chan_ops: out_bn without scale_shift");
  EIOKU_REQUIRE(pixels * (c / 8) <= (1ll << 31), "probe chan_ops: %lld threads", pixels * (c / 8));
  return chan_ops((const __half*)in, pixels, c, slope, (__half*)out_act, scale_shift, (__half*)out_bn, stream);
}

// x [m][7][7][512] fp16 -> partial_out [16][m][512] fp32 (k_face_fc), emb_out [m][512] fp32 (k_face_norm); weights as
// eioku_iresnet_set_head uploaded them
int eioku_probe_face_head(eioku_iresnet_t* r, const void* x, int m, float* partial_out, float* emb_out, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(r && x && partial_out && emb_out, "probe face head: NULL argument");
  EIOKU_REQUIRE(m >= 1 && m <= kChunk, "probe face head: m = %d outside [1, %d]", m, kChunk);
  EIOKU_REQUIRE(r->fc_w && r->fc_b, "probe face head: head has no weights");
  hipLaunchKernelGGL(k_face_fc, dim3(kFeat / 64, (unsigned)((m + 15) / 16), kFcSplit), dim3(256), 0, stream, (const __half*)x, m, r->fc_w.p,
                     partial_out);
  EIOKU_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_face_norm, dim3((unsigned)m), dim3(256), 0, stream, partial_out, m, r->fc_b.p, emb_out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // extern "C"
