// libeioku_hip_probe.so: Whisper's own attention (k_attn through the model's attn<QPW> wrapper, k_attn_weights) and the index
// movers around it (k_embed, k_embed_seq, k_kv_to_cache, k_gather_rows, k_im2col_mel, k_im2col_s2), each behind one entry point
// that takes device pointers, so that tests/test_bespoke_attn_gpu.py can compare them with a float64 restatement one kernel at
// a time.  Test infrastructure as places_probe.hip: not declared in include/eioku_hip.h, never loaded by the product.  The
// model's source is included unchanged, so the kernels are the ones the model runs and the library carries its own
// eioku_whisper_*: the tests create their handle through it (a tiny config: attn<QPW> reads cfg.heads alone).  k_attn keeps the
// wrapper's LDS size, grid, causal / anc dispatch and refusals; the other launch lines repeat the model's, under the model's
// own names (tests/test_bespoke_attn_host.py compares grid, block and LDS size as text).
#include "../whisper.hip"

extern "C" {

// attn<QPW> launches on the null stream, as every Whisper kernel does: a stream of the caller's is refused, not ignored
int eioku_probe_wh_attn(eioku_whisper* m, int qpw, const void* Q, long long q_bs, int q_rs, const void* K, const void* V, long long kv_bs,
                        int kv_rs, int n_q, int n_keys, int B, void* O, long long o_bs, int o_rs, int kv_div, const uint8_t* anc, int anc_ld,
                        const int* kvmap, int causal, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(m && Q && K && V && O, "probe attention: NULL argument");
  EIOKU_REQUIRE(!stream, "probe attention: the model's wrapper launches on the null stream");
  EIOKU_REQUIRE(n_q >= 1 && n_keys >= 1 && B >= 1 && B <= 65535 && kv_div >= 1, "probe attention: bad shape (n_q %d, n_keys %d, B %d, kv_div %d)",
                n_q, n_keys, B, kv_div);
  EIOKU_REQUIRE(q_rs >= 64 * m->cfg.heads && kv_rs >= 64 * m->cfg.heads && o_rs >= 64 * m->cfg.heads && kv_rs % 8 == 0 && kv_bs % 8 == 0,
                "probe attention: row strides below %d or keys off 16 bytes", 64 * m->cfg.heads);
  EIOKU_REQUIRE(!anc || anc_ld >= n_keys, "probe attention: anc_ld %d below n_keys %d", anc_ld, n_keys);
  const h16 *q = (const h16*)Q, *k = (const h16*)K, *v = (const h16*)V;
  if (qpw == 1) return attn<1>(m, q, q_bs, q_rs, k, v, kv_bs, kv_rs, n_q, n_keys, B, (h16*)O, o_bs, o_rs, kv_div, anc, anc_ld, kvmap, causal != 0);
  if (qpw == 2) return attn<2>(m, q, q_bs, q_rs, k, v, kv_bs, kv_rs, n_q, n_keys, B, (h16*)O, o_bs, o_rs, kv_div, anc, anc_ld, kvmap, causal != 0);
  EIOKU_REQUIRE(false, "probe attention: the model instantiates attn<1> and attn<2>, not attn<%d>", qpw);
}

// cross_attn's capture launch: R rows of P positions against the ctx keys of window kvmap[r], one head
int eioku_probe_wh_attn_weights(const void* Q, long long q_bs, int q_rs, const void* K, long long kv_bs, int kv_rs, int P, int ctx, int R,
                                int head, const int* kvmap, const int* nF, float* A, long long a_bs, long long a_rs, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(Q && K && kvmap && nF && A, "probe attention weights: NULL argument");
  EIOKU_REQUIRE(P >= 1 && ctx >= 1 && R >= 1 && R <= 65535 && head >= 0, "probe attention weights: bad shape (P %d, ctx %d, R %d, head %d)", P,
                ctx, R, head);
  EIOKU_REQUIRE(q_rs >= 64 * (head + 1) && kv_rs >= 64 * (head + 1) && kv_rs % 8 == 0 && kv_bs % 8 == 0,
                "probe attention weights: row strides below head %d or keys off 16 bytes", head);
  const size_t lds = (size_t)4 * (ctx + 64) * sizeof(float);
  EIOKU_REQUIRE(lds <= 64 * 1024, "probe attention weights: %d keys need %zu bytes of LDS", ctx, lds);
  hipLaunchKernelGGL(k_attn_weights, dim3((P + 3) / 4, R), dim3(256), lds, stream, (const h16*)Q, q_bs, q_rs, (const h16*)K, kv_bs, kv_rs, P,
                     ctx, head, kvmap, nF, A, a_bs, a_rs);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// decoder_step's embedding: x [B][d] fp32 = emb[token of lane b] + pos[s]
int eioku_probe_wh_embed(const int* toks, int tstride, int uniform, int vocab, int d, int s, const void* emb, const float* pos, float* x, int B,
                         hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(emb && pos && x, "probe embed: NULL argument");
  EIOKU_REQUIRE(B >= 1 && vocab >= 1 && d >= 1 && s >= 0 && tstride >= 0, "probe embed: bad shape (B %d, vocab %d, d %d, s %d)", B, vocab, d, s);
  hipLaunchKernelGGL(k_embed, dim3(B), dim3(256), 0, stream, toks, tstride, uniform, vocab, d, s, (const h16*)emb, pos, x);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// prefill's embedding: ids [R][P] -> x [R P][d] fp32
int eioku_probe_wh_embed_seq(const int* ids, int R, int P, int vocab, int d, const void* emb, const float* pos, float* x, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(ids && emb && pos && x, "probe embed_seq: NULL argument");
  EIOKU_REQUIRE(R >= 1 && P >= 1 && vocab >= 1 && d >= 1, "probe embed_seq: bad shape (R %d, P %d, vocab %d, d %d)", R, P, vocab, d);
  const int M = R * P;
  hipLaunchKernelGGL(k_embed_seq, dim3(M), dim3(256), 0, stream, ids, P, vocab, d, (const h16*)emb, pos, x);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// prefill's keys and values pk / pv [R][P][d] into rows 0 .. P - 1 of lanes r * lstride .. + G - 1 of ck / cv [lanes][Tm][d]
int eioku_probe_wh_kv_to_cache(const void* pk, const void* pv, int R, int P, int d, int G, int lstride, int Tm, void* ck, void* cv,
                               hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(pk && pv && ck && cv, "probe kv_to_cache: NULL argument");
  EIOKU_REQUIRE(R >= 1 && G >= 1 && lstride >= G && P >= 1 && P <= Tm && d >= 8 && d % 8 == 0 && R * G <= 65535,
                "probe kv_to_cache: bad shape (R %d, G %d, lstride %d, P %d, Tm %d, d %d; d %% 8 == 0)", R, G, lstride, P, Tm, d);
  hipLaunchKernelGGL(k_kv_to_cache, dim3(P, R * G), dim3(256), 0, stream, (const h16*)pk, (const h16*)pv, P, d, G, lstride, Tm, (h16*)ck,
                     (h16*)cv);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// gather_hidden: out [L][d] = h[(l / G) * P + t]
int eioku_probe_wh_gather_rows(const void* h, int L, int P, int t, int G, int d, void* out, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(h && out, "probe gather_rows: NULL argument");
  EIOKU_REQUIRE(L >= 1 && P >= 1 && t >= 0 && t < P && G >= 1 && d >= 1, "probe gather_rows: bad shape (L %d, P %d, t %d, G %d, d %d)", L, P, t,
                G, d);
  hipLaunchKernelGGL(k_gather_rows, dim3(L), dim3(256), 0, stream, (const h16*)h, P, t, G, d, (h16*)out);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// encode's first im2col: mel [B][C][T2] fp32 -> col [B T2][k1pad] fp16
int eioku_probe_wh_im2col_mel(const float* mel, int B, int C, int T2, int k1pad, void* col, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(mel && col, "probe im2col_mel: NULL argument");
  EIOKU_REQUIRE(B >= 1 && C >= 1 && T2 >= 1 && k1pad >= 3 * C, "probe im2col_mel: bad shape (B %d, C %d, T %d, ldk %d)", B, C, T2, k1pad);
  const size_t n1 = (size_t)B * T2 * k1pad;
  hipLaunchKernelGGL(k_im2col_mel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, stream, mel, B, C, T2, k1pad, (h16*)col);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

// encode's second im2col: h [B][T2][d] fp16 -> col [B ctx][3 d] fp16, ctx = T2 / 2
int eioku_probe_wh_im2col_s2(const void* h, int B, int d, int T2, void* col, hipStream_t stream) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(h && col, "probe im2col_s2: NULL argument");
  EIOKU_REQUIRE(B >= 1 && d >= 1 && T2 >= 2 && T2 % 2 == 0, "probe im2col_s2: bad shape (B %d, C %d, T %d; T even as 2 ctx is)", B, d, T2);
  const int ctx = T2 / 2, M = B * ctx;
  const size_t n2 = (size_t)M * 3 * d;
  hipLaunchKernelGGL(k_im2col_s2, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, stream, (const h16*)h, B, d, T2, (h16*)col);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

}  // extern "C"
