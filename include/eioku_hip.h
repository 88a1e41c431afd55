/*
 * eioku_hip.h - C ABI of libeioku_hip.so: the MI355X (gfx950) implementation of the
 * ml-service hot path of codihuston/eioku (scene scoring, YOLOv8 detection,
 * all-MiniLM-L6-v2 segment embedding, flat-L2 kNN).
 *
 * The reference (pure Python, /root/reference @ 2026-01-28) has no FFI for this path:
 * its arithmetic happens inside ffmpeg / OpenCV / Ultralytics / torchvision calls made
 * from ml-service/src/services/model_manager.py.  Each entry point below names the
 * reference call site whose work it replaces, so a maintainer can bind it (ctypes, see
 * INTEGRATION.md) behind the unchanged ModelManager.detect_* / process_ml_task API.
 *
 * Conventions
 *   - every function returns 0 on success or a negative EIOKU_E* code; the message for the
 *     calling thread's last failure is eioku_last_error().
 *   - `mem` says where the data pointers of THAT call live: EIOKU_MEM_HOST (the library
 *     stages through its own device buffers; PCIe-inclusive) or EIOKU_MEM_DEVICE (HBM
 *     pointers, zero copy).  Small result arrays follow the same flag.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls with
 *     EIOKU_MEM_DEVICE are asynchronous on that stream unless stated; EIOKU_MEM_HOST calls
 *     return after the results are in the host buffers.
 *   - handles are thread-compatible: one handle per thread, no internal locking.
 *   - no callbacks, no torch types, plain pointers and sizes only.
 */
#ifndef EIOKU_HIP_H
#define EIOKU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EIOKU_ABI_VERSION 1

enum {
  EIOKU_OK = 0,
  EIOKU_EINVAL = -1,   /* bad argument (shape, alignment, NULL) */
  EIOKU_ENOMEM = -2,   /* device or host allocation failed */
  EIOKU_EHIP = -3,     /* a HIP runtime call failed; see eioku_last_error() */
  EIOKU_ENODEV = -4,   /* no gfx950 device / library not initialised */
  EIOKU_ESTATE = -5    /* handle used in the wrong state */
};

enum { EIOKU_MEM_HOST = 0, EIOKU_MEM_DEVICE = 1 };

/* ---- lifecycle ------------------------------------------------------------------------
 * Replaces: ModelManager._get_device()/gpu_available (model_manager.py:23-42): the Python
 * host keeps returning "cuda"; this selects the HIP device the worker process is pinned to.
 */
int eioku_abi_version(void);
int eioku_init(int device_id);
void eioku_shutdown(void);
const char* eioku_last_error(void);
/* name, CU count, HBM bytes of the active device (any pointer may be NULL). */
int eioku_device_info(char* name, size_t name_cap, int* compute_units, uint64_t* hbm_bytes);

/* ---- in-library kernel timing (bench.py roofline block) -------------------------------
 * When enabled, the launch sites of the tagged kernels are bracketed with hipEvents on the
 * stream they are launched on.  eioku_prof_read synchronises those events and returns the
 * summed duration and the number of launches since the last reset.
 */
enum {
  EIOKU_PROF_SCENE_SAD = 0,
  EIOKU_PROF_SCENE_HSV = 1,
  EIOKU_PROF_CONV = 2,
  EIOKU_PROF_KNN = 3,
  EIOKU_PROF_GEMM = 4,
  EIOKU_PROF_IVFPQ = 5, /* k_lscan, the list-major ADC scan */
  EIOKU_PROF_NUM_TAGS = 8
};
int eioku_prof_enable(int on); /* 0 off, 1 all tags, else mask: bit (tag + 1) enables that tag only */
int eioku_prof_reset(void);
int eioku_prof_read(int tag, double* total_ms, uint64_t* launches);

/* ---- synthetic inputs (bench / tests) ------------------------------------
 * Counter-based splitmix64, identical to oracle/prng.py.  Device pointers only.
 */
int eioku_synth_u64(uint64_t seed, uint64_t offset, uint64_t n, uint64_t* out_dev, void* stream);
int eioku_synth_bytes(uint64_t seed, uint64_t n, uint8_t* out_dev, void* stream);
/* approx-normal float32 (Irwin-Hall 4), optionally L2-normalised per row of `dim`. */
int eioku_synth_normal_f32(uint64_t seed, uint64_t rows, int dim, int l2_normalise,
                           float* out_dev, void* stream);
/* n BGR frames h x w; params_dev = n x 5 int32 {base_b,base_g,base_r,gx,gy}. */
int eioku_synth_frames_bgr(uint64_t seed, uint64_t first_frame, int n, int h, int w,
                           const int32_t* params_dev, uint8_t* out_dev, void* stream);

/* ---- scene scoring ---------------------------------------------------------------------
 * K1. Replaces the `ffmpeg -vf select='gt(scene\,T)',showinfo` child process of
 * ModelManager.detect_scenes (model_manager.py:736-755): per-frame luma SAD against the
 * previous frame, exact uint64.  y_frames: n planes of h rows, `row_stride` bytes apart,
 * planes `frame_stride` bytes apart.  prev (nullable): the plane preceding frame 0 (same
 * row_stride); without it sad_out[0] = 0.  sad_out: n uint64.
 */
int eioku_scene_sad_luma(const uint8_t* y_frames, int n, int h, int w, size_t row_stride,
                         size_t frame_stride, const uint8_t* prev, uint64_t* sad_out,
                         int mem, void* stream);

/* K2. PySceneDetect ContentDetector frame deltas (BASELINE.json north_star; the reference
 * holds intent only, .kiro/specs/semantic-video-search/design.md:59-61): OpenCV 8-bit
 * BGR->HSV, then per-frame sums of |c_t - c_{t-1}| for c = hue, sat, val, exact uint64.
 * bgr_frames: n packed frames (h*w*3 bytes each, `frame_stride` bytes apart).
 * sums_out: n x 3 uint64 (row 0 = 0 unless prev given).
 */
int eioku_scene_hsv_sums(const uint8_t* bgr_frames, int n, int h, int w, size_t frame_stride,
                         const uint8_t* prev, uint64_t* sums_out, int mem, void* stream);

/* K1 on decoded BGR frames, for the single-pass ingest entry (one upload of a frame serves scene + objects + faces):
 * luma = OpenCV's 8-bit COLOR_BGR2YUV_I420 luma of each pixel (BT.601 studio range, 20-bit fixed point - what
 * cv2.cvtColor gives for the frames cv2.VideoCapture.read() returns at model_manager.py:263), then the per-frame SAD of
 * eioku_scene_sad_luma.  Exact uint64.  h * w must be a multiple of 4.  The DECODER's own Y plane differs from this by
 * the YUV -> BGR -> Y round trip (+-1-2 codes on some pixels): use eioku_scene_sad_luma when that plane is available. */
int eioku_scene_sad_luma_bgr(const uint8_t* bgr_frames, int n, int h, int w, size_t frame_stride, const uint8_t* prev,
                             uint64_t* sad_out, int mem, void* stream);

/* ---- scene scores and cut rules (host arithmetic behind the ABI; csrc/scene_host.hip) ----
 * What the reference reads from its ffmpeg child (`select='gt(scene,T)'`: /root/reference/ml-service/src/services/
 * model_manager.py:736-786) and the ContentDetector the north star names, restated once, in the libraries' own float
 * order, so that a binder in any language gets the bits eioku_amd/scene.py gets.  Outputs are HOST doubles / ints.
 *   eioku_scene_scores_from_sad : libavfilter get_scene_score over a SAD series (mafd, clip(float32(min(mafd,
 *                                 |mafd - prev|) / 100))); count = pixels per plane.
 *   eioku_scene_scores_luma     : K1 + the above on luma planes (host or device); synchronises the stream.
 *   eioku_scene_content_scores  : ContentDetector score (dh + ds + dl + 0) / 3 from K2's sums [n][3].
 *   eioku_scene_content_cuts    : PySceneDetect cut filter; mode 0 = 0.6.0-0.6.3 / SUPPRESS, 1 = 0.6.4+ MERGE.
 *   eioku_scene_content         : K2 + score + cuts on BGR frames (host or device); synchronises the stream. */
int eioku_scene_scores_from_sad(const uint64_t* sad, int n, double count, int bitdepth, double prev_mafd, int first_has_prev,
                                double* mafd_out, double* score_out);
int eioku_scene_scores_luma(const uint8_t* y_frames, int n, int h, int w, size_t row_stride, size_t frame_stride,
                            const uint8_t* prev, double prev_mafd, double* mafd_out, double* score_out, int mem,
                            void* stream);
int eioku_scene_content_scores(const uint64_t* sums, int n, double num_pixels, int first_has_prev, double* score_out);
int eioku_scene_content_cuts(const double* scores, int n, double threshold, int min_scene_len, int mode, int32_t* cuts_out,
                             int cap, int* n_cuts);
int eioku_scene_content(const uint8_t* bgr_frames, int n, int h, int w, const uint8_t* prev, double threshold,
                        int min_scene_len, int mode, int32_t* cuts_out, int cap, int* n_cuts, double* score_out, int mem,
                        void* stream);

/* ---- decoder planes in, BGR on the device (csrc/yuv.hip) ----
 * OpenCV's 8-bit COLOR_YUV2BGR_I420 / _NV12 (BT.601 studio range, 20-bit fixed point): the conversion cap.read() runs on
 * the CPU inside the reference's frame loops (model_manager.py:237-297,331-398).  yuv: n frames of (3h/2) x w bytes in
 * OpenCV's planar Mat layout (layout 0 = I420: Y | U | V, 1 = NV12: Y | interleaved UV); bgr_out [n][h][w][3]; both on
 * the side `mem` names.  h even, w a multiple of 4.  The Y plane itself (rows 0 .. h-1 of every frame) is what
 * eioku_scene_sad_luma scores with frame_stride = 3 h w / 2. */
int eioku_yuv420_to_bgr(const uint8_t* yuv, int n, int h, int w, int layout, uint8_t* bgr_out, int mem, void* stream);

/* Debug / parity helper: the HSV image itself (same layout as the input). */
int eioku_bgr2hsv(const uint8_t* bgr, size_t n_pixels, uint8_t* hsv_out, int mem, void* stream);

/* ---- detection: YOLOv8 -----------------------------------------------------------------
 * K4 building block.  One NHWC fp16 convolution (k in {1,3}, stride in {1,2} (2 only for k=3),
 * pad k/2) as implicit GEMM on MFMA with fused bias + optional SiLU + optional residual.  This is
 * the arithmetic that `model(frame, ...)` (ultralytics, called at model_manager.py:270-275 and
 * :364-369) spends its time in (Conv2d + folded BatchNorm + SiLU).  Device pointers only.
 *   in_nhwc   : fp16, n x h x w pixels, `in_cstride` channels per pixel; the conv reads the `cin`
 *               channels starting at `in_coff` (a concat/chunk slice).  cin, strides, offsets % 8 == 0.
 *   weight    : HOST fp32 [cout][cin][k][k] (torch layout), bias HOST fp32 [cout] or NULL; rounded
 *               to fp16 like tensor.half().
 *   act_silu  : 0 none, 1 SiLU, 2 ReLU, 3 ReLU AFTER the residual sum (relu(fp16(conv + bias) + res): ResNet blocks).
 *   residual  : optional fp16 slice added after activation: out = fp16(fp16(act(..)) + res).
 *   out_nhwc  : fp16 slice (cstride/coff % 4 == 0), or out_f32 != NULL: dense fp32 [n,ho,wo,cout].
 * Synchronous (packs weights per call): a test / building-block entry, not the fast path.
 */
int eioku_conv2d_f16(const void* in_nhwc, int n, int h, int w, int in_cstride, int in_coff, int cin,
                     const float* weight_oihw, const float* bias, int cout, int ksize, int stride,
                     int act_silu, const void* residual, int res_cstride, int res_coff,
                     void* out_nhwc, int out_cstride, int out_coff, float* out_f32, void* stream);

/* Bounds-check instrumentation of the conv family (libeioku_hip_bc.so = the same sources with -DEIOKU_BOUNDS_CHECK: every
 * global access of an activation / residual / image / output tensor is compared with the tensor's extent, a violation is
 * counted, not performed).  violations = -1 in the regular library.  selftest != 0: first make 3 violations on purpose. */
int eioku_debug_bounds(int* violations, int* line, int reset, int selftest);

/* Route log of the conv family: one line per distinct kernel instantiation launched in this process since the last
 * reset, "family<FIELDvalue,...> count\n" with the launching template's own arguments, e.g.
 * "persist<NF3,S1,NCH3,DB0,POST0,NWV8> 4" (families: igemm, flat, persist, chain, c8, stem_chain, 1x1, gather).  The
 * launch sites bump a host counter; nothing is formatted and no device work is added until this call.  buf receives
 * the NUL-terminated text (EIOKU_EINVAL when cap is too small; buf NULL with cap 0 only resets); reset != 0 clears the
 * counters after reading them.  Thread safe; needs no eioku_init. */
int eioku_debug_conv_routes(char* buf, size_t cap, int reset);
/* The plan of one layer as eioku_conv2d_f16 would run it on dense tensors of this shape (with / without a residual, fp16 or
 * fp32 output): `route` receives the instantiation in the route log's format ("persist<NF3,S1,NCH3,DB0,POST0,NWV8>"),
 * *lds_bytes the dynamic LDS of its launch.  A shape no kernel runs returns the error eioku_conv2d_f16 would return and
 * no route.  Host arithmetic only: launches nothing, needs no device and no eioku_init. */
int eioku_debug_conv_plan(int n, int h, int w, int cin, int cout, int ksize, int stride, int has_residual, int out_f32,
                          char* route, size_t cap, size_t* lds_bytes);
/* k_conv3x3_flat launches since the last reset whose straight-line epilogue (EIOKU_CONV_EPI) ran on at least the first cout tile */
int eioku_debug_conv_epi(int* launches, int reset);

/* YOLOv8 detector handle.  Replaces `YOLO(model_path); model.to(device)` + `model(frame, conf=..)`
 * of ModelManager.detect_objects / detect_faces (model_manager.py:252-254,270-275 / :346-348,
 * :364-369).  The graph is the Ultralytics yolov8 layout parameterised by its backbone widths
 * ch5 = {c1..c5} and C2f repeats depth4 (n: {16,32,64,128,256},{1,2,2,1}; s: {32,..,512},{1,2,2,1};
 * m: {48,96,192,384,576},{2,4,4,2}); nc = 80 for COCO models, 1 for yolov8n-face.
 * Weights are set per convolution (BatchNorm already folded: conv + bias), indexed in module order;
 * eioku_yolo_conv_info returns the Ultralytics state-dict prefix ("model.2.m.0.cv1.conv", ...;
 * the three Detect output convs are "model.22.cv2.<l>.2" / "model.22.cv3.<l>.2") and the shape.
 * Convolution 0 takes 8 input channels: RGB in channels 0..2, channels 3..7 must be zero weights.
 */
typedef struct eioku_yolo eioku_yolo_t;
int eioku_yolo_create(const int* ch5, const int* depth4, int nc, eioku_yolo_t** out);
/* The same with an Ultralytics Pose head (the community yolov8n-face.pt: kpt_shape [5, 3]): nk = K * 3 keypoint channels
 * (x, y, visibility; K <= 17), nine more convolutions "model.22.cv4.<l>.{0.conv,1.conv,2}" behind the Detect ones, of width
 * c4 = max(c3 / 4, nk).  nk = 0 is eioku_yolo_create. */
int eioku_yolo_create_pose(const int* ch5, const int* depth4, int nc, int nk, eioku_yolo_t** out);
void eioku_yolo_destroy(eioku_yolo_t* y);
int eioku_yolo_num_convs(const eioku_yolo_t* y);
int eioku_yolo_conv_info(const eioku_yolo_t* y, int idx, char* name, size_t name_cap, int* cout, int* cin,
                         int* ksize, int* stride);
int eioku_yolo_set_conv(eioku_yolo_t* y, int idx, const float* weight_oihw, const float* bias);

/* Raw network: fp16 NHWC8 input (device, n x h x w x 8, h,w % 32 == 0) -> the six Detect maps
 * (device fp32): box_out[l] [n,h/s,w/s,64], cls_out[l] [n,h/s,w/s,nc], s = 8,16,32.  NULL entries
 * are skipped.  Asynchronous on `stream`. */
int eioku_yolo_forward(eioku_yolo_t* y, const void* in_nhwc8_f16, int n, int h, int w,
                       float* const* box_out, float* const* cls_out, void* stream);
/* ... plus the raw keypoint maps of a Pose handle, kpt_out[l] [n,h/s,w/s,nk] (device fp32).  kpt_out == NULL: the
 * keypoint branch does not run (eioku_yolo_forward). */
int eioku_yolo_forward_pose(eioku_yolo_t* y, const void* in_nhwc8_f16, int n, int h, int w,
                            float* const* box_out, float* const* cls_out, float* const* kpt_out, void* stream);
/* Algorithmic conv FLOPs (2*Cout*Cin*k*k per output pixel, unpadded) of the last forward. */
int eioku_yolo_last_conv_flops(const eioku_yolo_t* y, double* flops);

/* One detection, ORIGINAL-frame pixels (after scale_boxes + clip), 32 bytes. */
typedef struct {
  float x1, y1, x2, y2;
  float conf;
  int32_t cls;
  int32_t anchor; /* index into the concatenated P3|P4|P5 anchor list: the "post-NMS box index" */
  int32_t pad;
} eioku_det_t;

/* Full per-frame pipeline on n BGR frames (u8, n x h x w x 3): K3 letterbox (cv2.resize
 * INTER_LINEAR fixed point / 2x2 area / copy, 114 padding, RGB, /255) -> network -> K6 decode ->
 * K7 class-aware NMS (IoU > iou suppresses, <= max_det kept, score order) -> scale_boxes + clip.
 * The letterbox geometry and the resize coefficient tables are produced by the host in the
 * reference's Python float semantics (eioku_amd/detect.py):
 *   lb_geom[9] = {new_h, new_w, top, left, out_h, out_w, mode(0 copy,1 bilinear,2 area), pad_x, pad_y}
 *   xofs[new_w], yofs[new_h] : first source column / row;  xalpha[new_w][2], ybeta[new_h][2] :
 *   11-bit fixed point tap weights (HOST pointers; may be NULL unless mode == 1).
 * dets_out: n x max_det eioku_det_t, counts_out: n int32 (host or device per `mem`; frames too).
 */
int eioku_yolo_detect(eioku_yolo_t* y, const uint8_t* bgr, int n, int h, int w, const int32_t* lb_geom,
                      const int32_t* xofs, const int32_t* yofs, const int16_t* xalpha,
                      const int16_t* ybeta, float gain, float conf, float iou, int max_det,
                      void* dets_out, int32_t* counts_out, int mem, void* stream);
/* The same on a Pose handle, plus kpts_out [n][max_det][nk] fp32 (host or device per `mem`): per kept detection its K
 * keypoints as (x, y, confidence), decoded after NMS from the anchor the detection came from (K6p: Ultralytics'
 * kpts_decode, then scale_coords with the unrounded padding, clipped to the frame); rows past counts_out[i] are zero.
 * kpts_out == NULL is eioku_yolo_detect: the keypoint branch does not run. */
int eioku_yolo_detect_pose(eioku_yolo_t* y, const uint8_t* bgr, int n, int h, int w, const int32_t* lb_geom,
                           const int32_t* xofs, const int32_t* yofs, const int16_t* xalpha,
                           const int16_t* ybeta, float gain, float conf, float iou, int max_det,
                           void* dets_out, int32_t* counts_out, int mem, void* stream, float* kpts_out);

/* Stage entry points (device pointers, asynchronous): K3 alone and K6+K7 alone.
 * eioku_letterbox_f16: BGR u8 frames -> fp16 NHWC8 (n x out_h x out_w x 8) network input.
 * eioku_yolo_postprocess: the six Detect maps -> detections, same semantics as eioku_yolo_detect
 * (hl/wl: map sizes of P3,P4,P5; gain/pad/src: scale_boxes parameters). */
int eioku_letterbox_f16(const uint8_t* bgr_dev, int n, int h, int w, const int32_t* lb_geom,
                        const int32_t* xofs, const int32_t* yofs, const int16_t* xalpha,
                        const int16_t* ybeta, void* out_nhwc8_dev, void* stream);
int eioku_yolo_postprocess(const float* const* box_dev, const float* const* cls_dev, int n, const int* hl,
                           const int* wl, int nc, float conf, float iou, int max_det, float gain,
                           int pad_x, int pad_y, int src_w, int src_h, void* dets_dev,
                           int32_t* counts_dev, void* stream);
/* K6 + K7 + K6p alone: ... plus the three keypoint maps kpt_dev[l] [n,hl,wl,nk] -> kpts_dev [n][max_det][nk] (device).
 * kpad_x / kpad_y: scale_coords' unrounded padding ((out_w - src_w * gain) / 2, (out_h - src_h * gain) / 2). */
int eioku_yolo_postprocess_pose(const float* const* box_dev, const float* const* cls_dev, const float* const* kpt_dev,
                                int n, const int* hl, const int* wl, int nc, int nk, float conf, float iou, int max_det,
                                float gain, int pad_x, int pad_y, float kpad_x, float kpad_y, int src_w, int src_h,
                                void* dets_dev, int32_t* counts_dev, float* kpts_dev, void* stream);

/* ---- semantic search: exact kNN (FAISS IndexFlatL2 semantics) -----------------------------
 * The reference holds intent only for this stage (.kiro/specs/semantic-video-search/design.md:
 * 35-40,1105-1113; tasks.md:304-313 unchecked); BASELINE.json's north_star names FAISS IndexFlatL2.
 * search() returns SQUARED L2 distances ascending and int64 ids (-1 / FLT_MAX when fewer than k
 * vectors exist), ties broken by the smaller id.  d in {64,128,256,384,512}, k <= 32.
 * HBM layout: the fp32 rows [N][d] (+ fp32 norms) and, built lazily by the first search with nq > 64 over
 * >= scan_min_rows rows, a bf16 copy of the rows in MFMA-fragment order (2 d bytes per row).
 */
typedef struct eioku_index eioku_index_t;
int eioku_index_flat_create(int d, eioku_index_t** out);
void eioku_index_destroy(eioku_index_t* ix);
long long eioku_index_ntotal(const eioku_index_t* ix);
int eioku_index_reset(eioku_index_t* ix);
/* append n vectors (host: staged; device: copied into the index' own HBM buffer) */
int eioku_index_add(eioku_index_t* ix, const float* x, long long n, int mem, void* stream);
/* zero-copy: search an existing 16-byte aligned device buffer of n x d floats (bench: 10M x 384) */
int eioku_index_attach(eioku_index_t* ix, float* x_dev, long long n, void* stream);
int eioku_index_search(eioku_index_t* ix, const float* q, int nq, int k, float* D, int64_t* I, int mem,
                       void* stream);
/* the next k results AFTER a previous answer: only rows with (distance, id) > (after_D[q], after_I[q]) in the
 * result order are candidates (FAISS has no such call; IndexIVFPQ's probe selection uses it to lift nprobe above
 * the k <= 32 of one search: successive rounds on the exact-fp32 kernels see bit-identical distances). */
int eioku_index_search_after(eioku_index_t* ix, const float* q, int nq, int k, const float* after_D,
                             const int64_t* after_I, float* D, int64_t* I, int mem, void* stream);
/* Row selectors and removal (K9f, see csrc/knn.hip).  Eligible rows of a search = live rows AND selector; the answer
 * is the exact top-k of the eligible rows in the conventions above (-1 / FLT_MAX padding when fewer than k are eligible).
 * sel_words: ceil(ntotal/32) 32-bit words, bit r % 32 of word r / 32 set = row r eligible (one word = one 32-row MFMA
 *   tile); bits at or beyond ntotal are ignored and no word at or beyond ceil(ntotal/32) is read.  One selector per call,
 *   shared by all nq queries (FAISS SearchParameters.sel).  sel_mem: EIOKU_MEM_HOST (staged) or EIOKU_MEM_DEVICE,
 *   independently of `mem`.  NULL = every live row.
 * after_D / after_I: the exclusive lower bound of eioku_index_search_after, both NULL = none; k up to 32 per call, so a
 *   filtered top_k > 32 chains calls exactly as the unfiltered one does.
 * Selector searches run on the exact-fp32 register-tile kernels: a tile-list route that stages only the non-empty
 * tiles when at most "sel_list_ppm" millionths of the tiles are non-empty (decided on the device, no host round trip),
 * else a masked walk over all rows.  They never take the scan path (its bound would have to be taken over eligible
 * rows only). */
int eioku_index_search_sel(eioku_index_t* ix, const float* q, int nq, int k, const uint32_t* sel_words, int sel_mem,
                           const float* after_D, const int64_t* after_I, float* D, int64_t* I, int mem, void* stream);
/* Take rows out of every later search.  Ids NEVER shift (unlike FAISS remove_ids): eioku_index_ntotal keeps counting
 * the rows ever added (ids are < ntotal), later add() calls continue with fresh ids, eioku_index_nlive counts what a
 * search can still return.  Nothing is rebuilt: the rows' norms become +inf, which no candidate test of any kernel
 * passes.  Unknown (< 0, >= ntotal) and repeated ids are ignored.  Allowed on an attached buffer (the norms are the
 * index' own; the buffer is not written).  ids: int64, host or device per `mem`.  Returns after the stream has drained.
 * eioku_index_reset makes every id available again. */
int eioku_index_remove_ids(eioku_index_t* ix, const int64_t* ids, long long n_ids, int mem, void* stream);
long long eioku_index_nlive(const eioku_index_t* ix);
/* Tuning / test knobs, see csrc/knn.hip.  "sel_list_ppm": selector searches take the tile-list route when
 * non-empty tiles * 1e6 <= sel_list_ppm * tiles (0 = never, 1000000 = always).  The wide-search ("scan") path: "scan_mode" 0 = register-tile kernels only,
 * 1 (default) = searches of >= "scan_min_nq" (default 1) queries over >= "scan_min_rows" rows keep row tiles stationary, filter with one bf16
 * product term and re-rank the candidates in fp32; "scan_cap" candidate slots per query (a list that overflows falls
 * back to the register-tile kernels); "scan_sample" rows of the bounding sample (0 = automatic); "scan_prescan" stride of the row tiles the
 * scan visits FIRST to tighten that bound (default 32; 0 = off, the sample alone bounds the scan); "scan_rt" 1 or 2
 * row tiles per wave (12 / 8 waves per workgroup). */
int eioku_index_set_param(eioku_index_t* ix, const char* name, long long value);
/* C1 helper: merge nlists per-shard results [nlists][nq][k] (ids already global) -> [nq][k].
 * Device pointers.  Used after the RCCL all-gather of per-rank (D, I). */
int eioku_topk_merge(const float* d_lists, const int64_t* i_lists, int nlists, int nq, int k, float* D,
                     int64_t* I, void* stream);

/* ---- C1 without a torch process group: sharded exact search over RCCL ----------------------------------
 * The reference holds intent only (.kiro/specs/semantic-video-search/design.md:58-61: one FAISS index per node);
 * BASELINE.json's north_star asks for "per-GPU FAISS-style shards ... merged via a single RCCL all-gather" behind
 * the C ABI.  Rank 0 makes an id (eioku_comm_unique_id) and ships the 128 bytes to its peers out of band (the
 * service's own RPC, a file, MPI ...); every rank, one process per GPU, then calls eioku_comm_create -- a
 * collective, like ncclCommInitRank, which it wraps -- and from then on eioku_index_search_sharded with the same
 * nq and k: local shard search, ONE all-gather of nq*k*12 bytes per rank over xGMI, local merge.  Every rank
 * receives the same global answer.  q / D / I are DEVICE pointers; ids are id_base + the shard's local row.
 * RCCL is bound with dlopen at first use (EIOKU_ENODEV if librccl.so is absent). */
#define EIOKU_COMM_ID_BYTES 128
typedef struct eioku_comm eioku_comm_t;
int eioku_comm_unique_id(unsigned char* id128);
int eioku_comm_create(const unsigned char* id128, int rank, int world, eioku_comm_t** out);
void eioku_comm_destroy(eioku_comm_t* comm);
int eioku_comm_rank(const eioku_comm_t* comm, int* rank, int* world);
int eioku_index_search_sharded(eioku_index_t* ix, eioku_comm_t* comm, long long id_base, const float* q, int nq,
                               int k, float* D, int64_t* I, void* stream);

/* ---- segment embedding: all-MiniLM-L6-v2 (BERT encoder + mean pooling + L2 norm) ----------
 * The reference holds intent only (.kiro/specs/semantic-video-search/design.md:54-57,1096-1103;
 * tasks.md:297-302 unchecked); BASELINE.json's north_star names all-MiniLM-L6-v2: vocab 30522,
 * hidden 384, 6 layers, 12 heads, ffn 1536, 512 positions, 2 token types, LayerNorm eps 1e-12.
 * Tensors carry the Hugging Face BertModel state-dict names ("embeddings.word_embeddings.weight",
 * "encoder.layer.0.attention.self.query.weight", ...), fp32, row-major [out][in].
 * Tokenisation (WordPiece) stays on the host.  head_dim must be 32; hidden, ffn % 128 == 0.
 */
typedef struct eioku_bert eioku_bert_t;
int eioku_bert_create(int vocab, int hidden, int layers, int heads, int ffn, int max_pos, int type_vocab,
                      float ln_eps, eioku_bert_t** out);
void eioku_bert_destroy(eioku_bert_t* m);
int eioku_bert_num_tensors(const eioku_bert_t* m);
int eioku_bert_tensor_info(const eioku_bert_t* m, int idx, char* name, size_t name_cap, int* rows, int* cols);
int eioku_bert_set_tensor(eioku_bert_t* m, int idx, const float* host_data, size_t numel);
/* ids int32 [B][S], mask uint8 [B][S] (1 = token) -> out float32 [B][hidden], unit L2 norm. */
int eioku_bert_embed(eioku_bert_t* m, const int32_t* ids, const uint8_t* mask, int B, int S, float* out,
                     int mem, void* stream);
int eioku_bert_last_flops(const eioku_bert_t* m, double* flops);
/* Route log of the encoder: one line "name count\n" for EVERY kernel route eioku_bert_embed can launch, zeros included,
 * counted by the launch sites in this process since the last reset: attn_bf / attn8 / attn1,
 * gemm_bf<EPI0|1,T64|T128,AS0|1>, gemm_f32<EPI0|1,T64|T128>, gemm_f32_s<EPI0|1>, add_ln_fixed<6> / add_ln_fixed<12> /
 * add_ln, pool<G1|G2>, and splits<1..4> (GEMM launches by split-K factor).  Host counters only: no device work, no
 * allocation, no eioku_init.  buf receives the NUL-terminated text (EIOKU_EINVAL when cap is too small; buf NULL with
 * cap 0 only resets); reset != 0 clears the counters after reading them.  Thread safe. */
int eioku_debug_bert_routes(char* buf, size_t cap, int reset);

/* as eioku_topk_merge, for lists that carry k_in >= k entries each ([nlists][nq][k_in]) */
int eioku_topk_merge_ex(const float* d_lists, const int64_t* i_lists, int nlists, int nq, int k_in, int k,
                        float* D, int64_t* I, void* stream);

/* ---- approximate kNN: IVF-PQ building blocks (FAISS IndexIVFPQ semantics: L2, by_residual, 8 bit) ----
 * BASELINE.json cfg5.  Host orchestration (k-means / PQ training loops, list bookkeeping) lives in
 * eioku_amd/ivfpq.py; coarse assignment and probe selection reuse eioku_index_search (k = 1 / nprobe).
 * All pointers are DEVICE pointers; calls are asynchronous on `stream`.
 *   eioku_kmeans_update : centroids[k][d] <- mean of assigned rows (64-bit fixed-point atomics: bit
 *                         reproducible); empty clusters keep their centroid; counts_out optional.
 *   eioku_pq_assign     : nearest of 256 sub-centroids per (vector, sub-quantiser) of x - coarse[list]
 *                         (coarse may be NULL); codes_out [n][m] u8 and/or resid_out [n][d], d/m in {4,8,16}.
 *   eioku_ivf_histogram / eioku_ivf_scatter : counting sort of encoded vectors into inverted lists.
 *   eioku_ivfpq_scan    : ADC over the probed lists; partial results [nprobe][nq][K], K = 16 (k <= 16)
 *                         or 32, to be merged with eioku_topk_merge_ex.
 */
int eioku_kmeans_update(const float* x_dev, long long n, int d, const long long* assign_dev, int k,
                        float* centroids_dev, int* counts_out_dev, void* stream);
/* the two halves of eioku_kmeans_update for a build sharded over GPUs: every rank adds its rows
 * into caller-zeroed integer sums (int64 [k][d], 2^-32 fixed point) and counts (int32 [k]), the host all-reduces them
 * (RCCL; integers: exact, order independent) and every rank finalises the same centroids. */
int eioku_kmeans_accumulate(const float* x_dev, long long n, int d, const long long* assign_dev, int k,
                            long long* sums_dev, int* counts_dev, void* stream);
int eioku_kmeans_finalize(const long long* sums_dev, const int* counts_dev, int k, int d, float* centroids_dev,
                          void* stream);
int eioku_pq_assign(const float* x_dev, long long n, int d, int m, const float* coarse_dev,
                    const long long* list_dev, const float* pq_dev, uint8_t* codes_out_dev,
                    float* resid_out_dev, void* stream);
int eioku_ivf_histogram(const long long* list_dev, long long n, int nlist, int* counts_dev, void* stream);
int eioku_ivf_scatter(const long long* list_dev, long long n, int m, const uint8_t* codes_dev, long long id_base,
                      int* cursor_dev, uint8_t* list_codes_dev, long long* list_ids_dev, void* stream);
int eioku_ivfpq_scan(const float* q_dev, int nq, int d, int m, const long long* probes_dev, int nprobe,
                     const float* coarse_dev, const float* pq_dev, const int* offsets_dev,
                     const int* sizes_dev, const uint8_t* list_codes_dev, const long long* list_ids_dev,
                     int k, float* pd_dev, long long* pi_dev, void* stream);
/* FAISS' precomputed-table form of the same scan (IndexIVFPQ::use_precomputed_table): eioku_ivfpq_tables writes
 * out[v][j][c] = alpha ||pq[j][c]||^2 + beta (vecs[v]_j . pq[j][c]) as [nvec][m][256] floats - once per index over the
 * coarse centroids (alpha 1, beta 2: nlist x m x 1 KB) and once per search over the queries (alpha 0, beta -2) - and
 * eioku_ivfpq_scan_tables assembles each (query, list) look-up table as the sum of two rows + ||q - c||^2 instead of
 * m x 256 x dsub multiply-adds over the codebook.  Same results up to fp32 rounding of the decomposition. */
int eioku_ivfpq_tables(const float* vecs_dev, int nvec, int d, int m, const float* pq_dev, float alpha, float beta,
                       float* out_dev, void* stream);
int eioku_ivfpq_scan_tables(const float* q_dev, int nq, int d, int m, const long long* probes_dev, int nprobe,
                            const float* coarse_dev, const float* pq_dev, const int* offsets_dev,
                            const int* sizes_dev, const uint8_t* list_codes_dev, const long long* list_ids_dev,
                            const float* list_tables_dev, const float* query_tables_dev, int k, float* pd_dev,
                            long long* pi_dev, void* stream);

/* List-major form of the scan (round 3; d/m = 8, d in {64, 128, 256, 384}): the (query -> probes) relation is inverted per
 * search, a workgroup decodes a segment of ONE list once into bf16 MFMA operands and multiplies it with every query that
 * probes the list; the products only FILTER (rigorous bf16 margin against the k-th exact distance of the query's
 * nearest list), survivors are re-ranked with eioku_ivfpq_scan_tables' own fp32 arithmetic: (D, I) are bit-identical
 * to eioku_ivfpq_scan_tables + eioku_topk_merge_ex, codes cross HBM once per search instead of once per (query, probe).
 *   eioku_ivfpq_lists_aux       : index-side tables, once per pack: pqh_out [m * 256 * 16 B] (bf16 codebook),
 *                                 hx_out [ntotal] floats, pmax2_out [nlist] floats.
 *   eioku_ivfpq_lists_workspace : bytes of device workspace one search of nq queries needs (-1: bad argument).
 *   eioku_ivfpq_search_lists    : the whole search; probes [nq][nprobe] from the coarse quantiser; cand_cap = per-query
 *                                 candidate capacity (0: 8192); a query whose list overflows is redone by the gated
 *                                 query-major scan (same results, slower).  stats_out (optional, device, 6 ints): overflow
 *                                 bits (1: every query redone, 2: some), work items, largest per-query candidate list,
 *                                 candidates of all queries, the query holding the largest list, its size.
 * Replaces: FAISS IndexIVFPQ::search as planned by /root/reference/.kiro/specs/semantic-video-search/design.md:35-40,1105-1113. */
int eioku_ivfpq_lists_aux(const uint8_t* list_codes_dev, const int* offsets_dev, const int* sizes_dev, int nlist, int d, int m,
                          const float* list_tables_dev, const float* pq_dev, void* pqh_out_dev, float* hx_out_dev,
                          float* pmax2_out_dev, void* stream);
long long eioku_ivfpq_lists_workspace(int nq, int d, int nprobe, int nlist, long long ntotal, int k, int cand_cap);
int eioku_ivfpq_search_lists(const float* q_dev, int nq, int d, int m, const long long* probes_dev, int nprobe, int nlist,
                             long long ntotal, const float* coarse_dev, const float* pq_dev, const int* offsets_dev, const int* sizes_dev,
                             const uint8_t* list_codes_dev, const long long* list_ids_dev, const float* list_tables_dev,
                             const float* query_tables_dev, const void* pqh_dev, const float* hx_dev,
                             const float* pmax2_dev, int k, int cand_cap, void* workspace_dev, long long workspace_bytes,
                             float* D_dev, long long* I_dev, int* stats_out_dev, void* stream);

/* Row selectors and removed rows for IVF-PQ (K10f): the SELECTED VIEW of the probed lists.  keep [(ntotal + 31) / 32]
 * little-endian 32-bit words by row id (bit set = the row may be returned: selector AND NOT removed; NULL is an error,
 * an unfiltered search takes the lists as they are).  For the lists that probes [nq][nprobe] touch, the call writes a
 * compact copy holding exactly their rows whose bit is set, in their order within the list: v_offsets / v_sizes [nlist]
 * ints (v_sizes[l] = 0 for a list nobody probes), v_codes [cap_rows][m], v_ids [cap_rows], and v_hx [cap_rows] from hx
 * (eioku_ivfpq_lists_aux; both NULL when no list-major scan follows).  eioku_ivfpq_scan, eioku_ivfpq_scan_tables and
 * eioku_ivfpq_search_lists (with the UNCHANGED pmax2) then run on the v_* pointers in place of the pack's: same
 * distance bits per row as an unfiltered search, k best of the eligible rows.  No atomics: the view is deterministic.
 * cap_rows: rows the v_* arrays hold; min(ntotal, bits set in the selector) always suffices.  The eligible rows are
 * known on the device only: when they exceed cap_rows nothing is written past the end - the view comes out EMPTY (all
 * sizes 0) and status_out[0] = 1; status_out (device, 2 ints) = {1 if the capacity was too small else 0, eligible rows
 * of the probed lists}.  EIOKU_EINVAL: NULL buffer, hx without v_hx, ntotal outside [1, 2^31), nq x nprobe >= 2^30.
 * All pointers are DEVICE pointers; asynchronous on `stream`. */
int eioku_ivfpq_select_view(const long long* probes_dev, int nq, int nprobe, int nlist, int m, long long ntotal,
                            const int* offsets_dev, const int* sizes_dev, const uint8_t* list_codes_dev,
                            const long long* list_ids_dev, const float* hx_dev, const uint32_t* keep_dev,
                            long long cap_rows, int* v_offsets_dev, int* v_sizes_dev, uint8_t* v_codes_dev,
                            long long* v_ids_dev, float* v_hx_dev, int* status_out_dev, void* stream);

/* ---- place classification: Places365 ResNet18 (csrc/resnet.hip) --------------------------------------------------
 * Replaces the per-frame arithmetic of ModelManager.classify_places
 * (/root/reference/ml-service/src/services/model_manager.py:560-713): `transforms.Resize((224, 224))` on the PIL image
 * (Pillow's antialiased bilinear resample, bit-exact: model_manager.py:630-640), ToTensor + Normalize,
 * `models.resnet18` with a 365-way fc (:609-624), softmax + descending sort + top_k (:672-687).
 * Weights are set per convolution with BatchNorm folded in (eioku_resnet18_conv_info names them as torchvision's
 * state dict does: "conv1", "layer1.0.conv1", ..., "layer2.0.downsample.0"); fp16 storage, fp32 accumulation.
 * The resize tables are Pillow's precompute_coeffs output for (w -> 224) and (h -> 224), computed by the host
 * (eioku_amd/places.py): bounds [224][2] = {first input index, taps}, k [224][ksize] int32 taps x 2^22. */
typedef struct eioku_resnet eioku_resnet_t;
int eioku_resnet18_create(int num_classes, eioku_resnet_t** out);
void eioku_resnet18_destroy(eioku_resnet_t* r);
int eioku_resnet18_num_convs(const eioku_resnet_t* r);
int eioku_resnet18_conv_info(const eioku_resnet_t* r, int idx, char* name, size_t name_cap, int* cout, int* cin, int* ksize,
                             int* stride);
int eioku_resnet18_set_conv(eioku_resnet_t* r, int idx, const float* weight_oihw, const float* bias);
int eioku_resnet18_set_fc(eioku_resnet_t* r, const float* weight, const float* bias);
/* resize + normalise only: out_f16 [n][224][224][4] fp16 (R, G, B, 0) and / or out_rgb_u8 [n][224][224][3], DEVICE */
int eioku_places_preprocess(eioku_resnet_t* r, const uint8_t* bgr, int n, int h, int w, const int32_t* xbounds,
                            const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, void* out_f16,
                            uint8_t* out_rgb_u8, int mem, void* stream);
/* the raw network: in [n][224][224][4] fp16 -> logits [n][num_classes] fp32; device pointers, asynchronous */
int eioku_resnet18_forward(eioku_resnet_t* r, const void* in_nhwc4_f16, int n, float* logits_out, void* stream);
/* n BGR frames (host or device) -> per frame the top_k (probability, class) of softmax(logits) in descending order
 * (ties: lower class); outputs on the side `mem` names (host outputs synchronise); logits_out optional */
int eioku_resnet18_classify(eioku_resnet_t* r, const uint8_t* bgr, int n, int h, int w, const int32_t* xbounds,
                            const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, int top_k,
                            float* prob_out, int32_t* class_out, float* logits_out, int mem, void* stream);
int eioku_resnet18_last_flops(const eioku_resnet_t* r, double* flops);

/* ---- face clustering: ArcFace IResNet embeddings + cosine DBSCAN (csrc/faces.hip) ------------------------------------
 * Fills the cluster_id of ModelManager.detect_faces.  The embedder is insightface arcface_torch's `iresnet` (112 x 112
 * input, stem conv3x3 + BN + PReLU, four stages 64 / 128 / 256 / 512 each opening with a stride 2, IBasicBlock =
 * bn1 -> conv3x3 -> bn2 -> PReLU -> conv3x3(stride) -> bn3 + identity or 1x1 / s2 conv + BN, head bn2 -> fc -> features).
 * depths = blocks per stage ([2,2,2,2] r18, [3,4,14,3] r50, [3,13,30,3] r100).  Convolutions are named as the
 * state dict's prefixes ("conv1", "layer1.0.conv1", "layer1.0.downsample.0", ...) and take BatchNorm folded in (conv1 <-
 * bn1, block conv1 <- bn2, conv2 <- bn3, downsample.0 <- downsample.1).  PReLU unit 0 is the stem's, unit 1 + b block
 * b's; set_bn takes block b's leading bn1 as per-channel (scale, shift).  set_head: bn2, fc and features folded into
 * weight [512][25088] (columns in NHWC order: (y * 7 + x) * 512 + c) and bias [512].  Boxes: HOST fp32 [m][5] = (frame
 * slot, x1, y1, x2, y2); the crop is a square of side max(w, h, 1) centred on the box, bilinear to 112 x 112.
 * fp16 storage, fp32 accumulation.  All calls are synchronous. */
typedef struct eioku_iresnet eioku_iresnet_t;
int eioku_iresnet_create(const int* depths, eioku_iresnet_t** out);
void eioku_iresnet_destroy(eioku_iresnet_t* r);
int eioku_iresnet_num_convs(const eioku_iresnet_t* r);
int eioku_iresnet_num_blocks(const eioku_iresnet_t* r);
int eioku_iresnet_conv_info(const eioku_iresnet_t* r, int idx, char* name, size_t name_cap, int* cout, int* cin, int* ksize,
                            int* stride);
int eioku_iresnet_set_conv(eioku_iresnet_t* r, int idx, const float* weight_oihw, const float* bias);
int eioku_iresnet_set_prelu(eioku_iresnet_t* r, int unit, const float* slope);
int eioku_iresnet_set_bn(eioku_iresnet_t* r, int block, const float* scale, const float* shift);
int eioku_iresnet_set_head(eioku_iresnet_t* r, const float* weight, const float* bias);
/* crop only: out_f16 [m][112][112][8] fp16 (R, G, B as (v / 255 - 0.5) / 0.5, 5 zero channels), DEVICE */
int eioku_iresnet_crop(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const float* boxes, int m, void* out_f16,
                       int mem, void* stream);
/* the raw network on crops (DEVICE, m <= 256) -> emb_out [m][512]; upto_block >= 0: that block's NHWC fp16 output to
 * act_out instead */
int eioku_iresnet_forward(eioku_iresnet_t* r, const void* in_f16, int m, int upto_block, void* act_out, float* emb_out,
                          void* stream);
/* n BGR frames (host or device) + m boxes -> out [m][512] fp32 unit vectors on the side `mem` names */
int eioku_iresnet_embed(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const float* boxes, int m, float* out,
                        int mem, void* stream);
/* K13c, the aligned crop, alone: face i of frame slots[i] (HOST int32 [m]) warped by M[i] (HOST float64 [m][6], the
 * matrix cv2.warpAffine takes: frame -> 112 x 112 crop) as cv2.warpAffine(frame, M, (112, 112), flags = INTER_LINEAR,
 * borderValue = 0) computes it in fixed point, then eioku_iresnet_crop's normalisation and layout */
int eioku_iresnet_crop_aligned(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const int32_t* slots, const double* M,
                               int m, void* out_f16, int mem, void* stream);
/* eioku_iresnet_embed on aligned crops: face i is warped by M[i] unless use_box[i] != 0 (HOST int32 [m]), which keeps the
 * box crop of boxes[i]; the frame slot is boxes[i][0] either way */
int eioku_iresnet_embed_aligned(eioku_iresnet_t* r, const uint8_t* bgr, int n, int h, int w, const float* boxes, const double* M,
                                const int32_t* use_box, int m, float* out, int mem, void* stream);
int eioku_iresnet_last_flops(const eioku_iresnet_t* r, double* flops);
/* scikit-learn DBSCAN(eps, min_samples, metric="cosine") on unit-norm rows emb [n][d] fp32: j is a neighbour of i iff
 * 1 - e_i . e_j <= eps (i is its own), core iff >= min_samples neighbours, clusters = components of the core-core graph
 * numbered by smallest core index, a border point takes the smallest label among its core neighbours, -1 = noise.
 * n <= 65536, d % 32 == 0, eps in [0, 2], min_samples >= 1; labels_out [n] int32 on the side `mem` names. */
int eioku_dbscan_cosine(const float* emb, int n, int d, float eps, int min_samples, int32_t* labels_out, int mem, void* stream);
/* K14h, the device half of HDBSCAN(metric="cosine") (csrc/hdbscan.hip; the tree code is eioku_amd/hdbscan.py): rows emb
 * [n][d] fp32 are taken to float64 and normalised, d_ij = 1 - x_i . x_j in float64 (clipped to [0, 2], 0 on the diagonal),
 * core_out[i] = the min_samples-th smallest d_ij of row i (i itself included), and the n - 1 edges are a minimum spanning
 * tree of the weights max(core_i, core_j, d_ij) under the total order (w, min(i, j), max(i, j)), found by Boruvka rounds on
 * the device, in no particular order.  n in [0, 65536] (n <= 1: no edges), d % 32 == 0, 1 <= min_samples <= min(n, 32).
 * core_out [n] f64 and edge_u / edge_v int32 / edge_w f64 [n - 1] on the side `mem` names; rounds_out HOST: the rounds
 * taken, at most ceil(log2 n) + 1 -- with components left after that many the call fails rather than going on.
 * Synchronous; its own grow-only workspace. */
int eioku_hdbscan_mst_cosine(const float* emb, int n, int d, int min_samples, double* core_out, int32_t* edge_u, int32_t* edge_v,
                             double* edge_w, int32_t* rounds_out, int mem, void* stream);
/* device milliseconds of the last eioku_hdbscan_mst_cosine call: ms_out[0] the core-distance pass, ms_out[1 + r] Boruvka
 * round r; returns the number of stages (it may exceed cap; at most cap are written) */
int eioku_hdbscan_last_stage_ms(double* ms_out, int cap);

/* ---- OCR: EasyOCR's CRAFT detector and english_g2 CRNN recogniser (csrc/ocr.hip) -------------------------------------
 * Fills ModelManager.extract_ocr.  Convolutions are named as the state dicts' prefixes ("basenet.slice1.0", ...,
 * "upconv1.conv.0", "conv_cls.8"; "FeatureExtraction.ConvNet.0", ..., "Prediction") and take the following BatchNorm
 * folded in.  fc6 ("basenet.slice5.1") is the 3x3 / dilation 6 conv.  craft_forward: n BGR u8 frames (host or device per
 * mem) -> text / link score maps [n][H/2][W/2] fp32 and their (text > low_text) | (link > link_threshold) u8 map, DEVICE
 * and each optional, H x W = the canvas (frame, or INTER_LINEAR to canvas_size on the long side, padded to multiples of
 * 32).  crnn_forward: m normalised grey crops imgs HOST fp32 [64][widths[i]] (packed) -> per sequence step (T_i =
 * widths[i] / 4 - 1, rows in crop order) the argmax class and its probability after softmax with the `ignore` classes
 * zeroed and renormalised, HOST; logits_out optional; at most 262,144 steps per call.  CRAFT and the recogniser's VGG store
 * fp16 and accumulate in fp32; the recogniser is fp32 from its row mean on (GEMMs, BiLSTMs, logits).
 * All calls are synchronous. */
typedef struct eioku_craft eioku_craft_t;
int eioku_craft_create(eioku_craft_t** out);
void eioku_craft_destroy(eioku_craft_t* r);
int eioku_craft_num_convs(const eioku_craft_t* r);
int eioku_craft_conv_info(const eioku_craft_t* r, int idx, char* name, size_t name_cap, int* cout, int* cin, int* ksize);
int eioku_craft_set_conv(eioku_craft_t* r, int idx, const float* weight_oihw, const float* bias);
int eioku_craft_forward(eioku_craft_t* r, const uint8_t* bgr, int n, int h, int w, int canvas_size, float low_text,
                        float link_threshold, float* text_out, float* link_out, uint8_t* bin_out, int mem, void* stream);
int eioku_craft_last_flops(const eioku_craft_t* r, double* flops);
typedef struct eioku_crnn eioku_crnn_t;
int eioku_crnn_create(int num_class, eioku_crnn_t** out);
void eioku_crnn_destroy(eioku_crnn_t* r);
int eioku_crnn_num_convs(const eioku_crnn_t* r);
int eioku_crnn_conv_info(const eioku_crnn_t* r, int idx, char* name, size_t name_cap, int* cout, int* cin, int* ksize);
int eioku_crnn_set_conv(eioku_crnn_t* r, int idx, const float* weight_oihw, const float* bias);
/* BiLSTM layer 0 / 1: w_ih, w_hh [2][1024][256] and b_ih, b_hh [2][1024] (forward, reverse), w_lin [256][512], b_lin [256] */
int eioku_crnn_set_lstm(eioku_crnn_t* r, int layer, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                        const float* w_lin, const float* b_lin);
int eioku_crnn_forward(eioku_crnn_t* r, const float* imgs, const int* widths, int m, const uint8_t* ignore, int32_t* idx_out,
                       float* prob_out, float* logits_out, void* stream);
int eioku_crnn_last_flops(const eioku_crnn_t* r, double* flops);
/* Stage entry points: the code eioku_craft_forward / eioku_crnn_forward run, one stage at a time (tests hold each stage to a
 * reference of its own).
 * eioku_craft_canvas: frames (host or device per mem) -> out DEVICE fp16 [n][H][W][8], the network's input (the frame, or
 *   INTER_LINEAR to canvas_size; zero padded to multiples of 32, then normalised; channels 3..7 zero).  The handle lends its
 *   staging buffers and needs no weights.  Synchronous.
 * eioku_crnn_tail: the recogniser from its packed sequences on.  seq HOST fp32 [sum len][256], m sequences of len[i] >= 1
 *   steps one after another -> two BiLSTMs, Prediction, softmax / ignore / argmax; outputs as eioku_crnn_forward.  Needs the
 *   BiLSTM and "Prediction" weights only.  Synchronous.
 * eioku_ctc_probs: logits DEVICE fp32 [rows][C], ignore DEVICE u8 [C] (at least one class kept), 2 <= C <= 4096 -> per row
 *   the argmax over the kept classes (ties: the lower class) and its probability p / sum of kept p, DEVICE.  Asynchronous.
 * eioku_ocr_maxpool_f16 / _im2col_dil_f16 / _up2x_f16: CRAFT's glue kernels over caller DEVICE fp16 NHWC tensors (c % 8 == 0;
 *   a slice = channels coff .. coff + c of a tensor of cstride channels, both 8-aligned; 16-byte aligned pointers; every
 *   tensor below 2^31 elements).  Max pool: [n][h][w] -> [n][(h + 2 ph - kh) / sh + 1][(w + 2 pw - kw) / sw + 1], padding
 *   never wins (2 ph <= kh, 2 pw <= kw).  im2col: dense [n][h][w][c] -> dense [n][h][w][9][c], tap (ky, kx) =
 *   in[y + d (ky - 1)][x + d (kx - 1)] or zero.  up2x: dense [n][h][w][c] -> slice of [n][2h][2w], bilinear with
 *   align_corners=False, fp32 arithmetic rounded once to fp16.  Asynchronous. */
int eioku_craft_canvas(eioku_craft_t* r, const uint8_t* bgr, int n, int h, int w, int canvas_size, void* out_nhwc8_dev, int mem,
                       void* stream);
int eioku_crnn_tail(eioku_crnn_t* r, const float* seq, const int* len, int m, const uint8_t* ignore, int32_t* idx_out,
                    float* prob_out, float* logits_out, void* stream);
int eioku_ctc_probs(const float* logits, int rows, int C, const uint8_t* ignore, int32_t* idx_out, float* prob_out, void* stream);
int eioku_ocr_maxpool_f16(const void* in, int in_cstride, int in_coff, int n, int h, int w, int c, int kh, int kw, int sh, int sw,
                          int ph, int pw, void* out, int out_cstride, int out_coff, void* stream);
int eioku_ocr_im2col_dil_f16(const void* in, int n, int h, int w, int c, int d, void* out, void* stream);
int eioku_ocr_up2x_f16(const void* in, int n, int h, int w, int c, void* out, int out_cstride, int out_coff, void* stream);

/* ---- topics: KeyBERT keyword selection (csrc/topics.hip, K17) -------------------------------------------------------
 * Fills the topic_extraction stage the reference schedules but never built.  rows: x [n_rows][d] fp32; terms [n_terms][d]
 * fp32 (both unit vectors, 16-byte aligned); CSR row_ptr [n_rows+1], cand [nnz] int32 (term ids, read at
 * cand[row_ptr[r] .. row_ptr[r+1])).  s = dot(x, w_t).  diversity < 0: plain, the min(top_n, |row|) largest s; else MMR
 * with lambda = diversity (<= 1): argmax s, then argmax (1 - lambda) * s_t - lambda * max_k dot(w_t, w_k) over the picked
 * k, in fp32.  Every argmax breaks ties by the smaller term id.  -> idx [n_rows][top_n] int32 (picked term ids ordered
 * by s descending, ties by the smaller id; -1 pad), score [n_rows][top_n] fp32 (their s; 0 pad), count [n_rows] int32.
 * 1 <= top_n <= 32, d % 4 == 0, d <= 1024, else EIOKU_EINVAL before the device is touched; a term id outside
 * [0, n_terms) is EIOKU_EINVAL after the launch.  Fixed summation order, no atomics: repeated calls, and host- and
 * device-memory calls, give the same bytes.  Synchronous: returns after the outputs are written. */
int eioku_keyword_select(const float* x, int n_rows, const float* terms, int n_terms, int d, const int32_t* row_ptr,
                         const int32_t* cand, int top_n, float diversity, int32_t* idx, float* score, int32_t* count,
                         int mem, void* stream);

/* ---- thumbnails: Pillow's bicubic resize and libjpeg's baseline encoder (csrc/thumbs.hip, K18) ------------------------
 * Fills the thumbnail_generation stage.  Every image pointer is a DEVICE pointer, every table a HOST pointer.  At most 64
 * images per call and 1024 pixels per thumbnail side, else EIOKU_EINVAL before the device is touched (the handle stays
 * usable).  All stages are integer arithmetic: the results are the bytes Pillow 12 / libjpeg-turbo produce.
 * resize: n BGR u8 frames [n][h][w][3] -> rgb_out [n][th][tw][3] (RGB), Image.resize((tw, th), BICUBIC): horizontal pass,
 *   8-bit intermediate, vertical pass.  Tables from the host (eioku_amd/thumbs.py: bicubic_tables): bounds [out][2] =
 *   {first input index, taps}, k [out][ksize] int32 taps x 2^22.  Asynchronous on `stream`.
 * jpeg: n RGB u8 images [n][th][tw][3] -> per image the 4:2:0 baseline scan's quantised coefficients (coef_out, HOST,
 *   optional: [n][mcus][6][64] int16, per 16x16 MCU in scan order Y00 Y01 Y10 Y11 Cb Cr, zigzag) and its Huffman-coded
 *   bitstream without padding, byte stuffing and markers, kept on the device.  qtab: [2][64] luma / chroma divisors in
 *   natural order, each 1..255.  nbits_out [n]: bits per image; *bytes_out: size of the packed streams, where image i
 *   starts at the byte offset sum_{j<i} 4 * ceil(nbits[j] / 32) and unused trailing bits are 0.  Synchronous.
 * read: the packed streams of the last jpeg call -> out (HOST, cap >= *bytes_out).  Synchronous.
 * last_ms: device milliseconds of the last resize, block stage, entropy stage and read (0 for a stage not yet run). */
typedef struct eioku_thumbs eioku_thumbs_t;
int eioku_thumbs_create(eioku_thumbs_t** out);
void eioku_thumbs_destroy(eioku_thumbs_t* t);
int eioku_thumbs_resize(eioku_thumbs_t* t, const uint8_t* bgr, int n, int h, int w, int th, int tw, const int32_t* xbounds,
                        const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, uint8_t* rgb_out,
                        void* stream);
int eioku_thumbs_jpeg(eioku_thumbs_t* t, const uint8_t* rgb, int n, int th, int tw, const uint16_t* qtab, int16_t* coef_out,
                      uint32_t* nbits_out, uint64_t* bytes_out, void* stream);
int eioku_thumbs_read(eioku_thumbs_t* t, uint8_t* out, size_t cap, void* stream);
int eioku_thumbs_last_ms(eioku_thumbs_t* t, double* ms4);

/* ---- transcription: Whisper log-mel front end (K19), greedy decode (K20), beam search (K20b), csrc/whisper.hip --------
 * Fills ModelManager.transcribe_video (the reference calls faster_whisper.WhisperModel.transcribe on the CPU).  fp16
 * weights and activations, fp32 accumulation, fp32 residual stream / LayerNorm / softmax; head dimension 64.  All data
 * pointers are HOST pointers, every call is synchronous on the null stream.  Every dimension and every special-token id
 * comes from the config struct (config.json / generation_config.json of the checkpoint).
 * create: d_model % 64 == 0, d_model == 64 * heads, ffn % 32 == 0, else EIOKU_EINVAL.  suppress / begin_suppress / lang_ids
 *   are copied.  Tensors carry the Hugging Face WhisperForConditionalGeneration names; tensor_info gives rows x cols with
 *   rows * cols = numel (conv weights: rows = out channels, cols = in channels * 3); set_tensor takes fp32 in the
 *   checkpoint's own layout and converts on the device.  mel_filters: [n_mels][201] float64 (Slaney, made by the host).
 * set_audio: fp32 mono 16 kHz samples, uploaded once per video.
 * logmel: B windows starting at sample offsets[b] -> [B][n_mels][2 * max_source_positions] fp32, kept on the device for
 *   encode and copied to `out` when it is not NULL.  DFT and mel product in fp64.
 * encode: the encoder and the cross-attention K/V of every decoder layer for B windows; mel NULL = the last logmel result.
 * decode: greedy, temperature 0, timestamp rules, B lanes in lockstep over the last encode.  prompt_ids [prompt_len] is
 *   shared by the lanes.  tokens_out [B][max_new_tokens] (EOT-filled after a lane ends), n_out [B] = tokens sampled up to
 *   and including EOT, sum_logprob [B] over those, no_speech_prob [B] and lang_out [B] from the logits at prompt position
 *   0.  Tokens are read back at most every sync_every sampled steps (the loop ends early once every lane is done).
 * forced_logits (tests): teacher-forced, rule-free logits [B][T][vocab] for ids [B][T].
 * select (tests): the rule + argmax stage on supplied logits [B][vocab]; prefix [B][prefix_cap] with prefix_len [B] are the
 *   tokens sampled so far.  token_out [B], logprob_out [B], masked_out [B][vocab] (rules 1-6 applied; may be NULL).
 * encoder_output (tests): the final-LayerNorm output of the last encode, raw fp16 [B][ctx][d_model].
 * decode_beam: beam search (K20b) over the last encode of B windows: beam W in 1..8, lane b * W + j is slot j of window b,
 *   B * W <= 64.  n_finish = C, the number of finished hypotheses that ends a window's search (max(1, round(W * patience)),
 *   1..16).  Per window H = max(W, C) hypothesis rows: first the finished ones in the order they finished, then live
 *   slots in slot order while fewer than W.  tokens_out [B][H][max_new_tokens] (EOT-filled), n_out [B][H] = tokens
 *   sampled up to and including EOT, ended_out [B][H] = 1 when the row ended on EOT, sum_logprob [B][H], n_hyp [B] = rows
 *   in use, best_out [B] = the row with the largest sum_logprob / max(1, tokens before EOT) (ties: the earlier row).  The
 *   complete flags are read back at most every sync_every sampled steps.  trace_src / trace_tok (tests; may be NULL)
 *   [max_new_tokens][B][W]: per sampled step the source slot and token of every next slot, -1 where a slot stays
 *   empty, the window was complete, or the step was not run.
 * beam_select (tests): one beam step on supplied logits [B * W][vocab]; prefix [B * W][prefix_cap] with prefix_len [B * W]
 *   and sums [B * W] (-inf = a dead slot) describe the slots, fin_count [B] the finished hypotheses each window has.
 *   src_out / tok_out / sum_out [B][W] with n_live [B]: the next slots; fsrc_out / fsum_out [B][W] with n_fin [B]: the
 *   candidates that ended on EOT in walk order; fin_count_out [B] = min(C, fin_count + n_fin); complete_out [B].
 * decode_prompted (K20c): B rows with prompts [B][P] of one common length, each run through the decoder in ONE pass (the
 *   prompt prefill), then G lanes per row decoded in lockstep, B * G <= 64 and P + max_new_tokens <= max_target_positions.
 *   Row b reads encoded window windows[b]; windows NULL = identity, which needs B == the encoded windows.  temperature == 0:
 *   the greedy rule of `decode`, G == 1 and seeds NULL.  temperature > 0: every lane samples by Gumbel-max inside the
 *   selection path: score = masked logit / temperature - log(-log(u)), u = ((z >> 41) + 0.5) * 2^-23, z = element
 *   idx * vocab + id of the splitmix64 stream seeds[lane] (idx: the index of the sampled token); the token is the best
 *   score of the unmasked ids after the timestamp-mass rule, the lower id on equal scores.  sum_logprob adds the
 *   untempered log-softmax of the masked logits.  tokens_out [B][G][max_new_tokens] (EOT-filled), n_out / sum_logprob
 *   [B][G], best_out [B] = the row with the largest sum_logprob / max(1, tokens before EOT) (ties: the earlier row),
 *   no_speech_prob [B] from the logits at prompt position sot_index (may be NULL).
 * decode_beam_prompted: decode_beam with prompts [B][P], sot_index and windows as above; the prompt is prefilled once per
 *   window and the ancestry table names slot 0's lane for every prompt position.  Outputs as decode_beam (no language).
 * sample (tests): the rule + sampling stage on supplied logits [B][vocab] at temperature > 0 with seeds [B] and sample
 *   indices idx [B]; token_out [B], logprob_out [B].
 * prefill_logits (tests): rule-free logits [B][T][vocab] for ids [B][T]: positions 0 .. n_prefill - 1 in one prefill pass,
 *   the others walked position by position on the keys and values the prefill left.
 * last_launches: kernel launches of the last decode and its number of decoder steps.
 * Word alignment (K21; Whisper's find_alignment on the device):
 * set_alignment_heads: n (layer, head) pairs, generation_config.json's "alignment_heads"; n == 0 restores the default, every
 *   head of the upper half of the decoder layers.  A pair outside the decoder is EIOKU_EINVAL.
 * align: R rows over the last encode.  seq [R][T] = sot sequence (sot_len ids), <|notimestamps|>, the text ids (< eot), EOT,
 *   padded with EOT to the common T; n_tok [R] the true lengths; row r reads encoded window windows[r] (NULL: identity)
 *   and keeps F[r] = n_frames[r] / 2 frames.  One teacher-forced causal pass; the cross-attention probabilities of the
 *   alignment heads are normalised over the n_tok[r] token rows (population std, no guard against 0), median-filtered
 *   (width 7, reflect; skipped when F[r] <= 3), averaged over the heads and negated into the cost of the N[r] = n_tok[r] -
 *   sot_len - 1 rows sot_len .. n_tok[r] - 2; dynamic time warping (fp32; diagonal if below both others, else up if below
 *   both others, else left) gives jump_out [R][Nmax], Nmax = T - sot_len - 1: the frame index of the first path cell of
 *   each row, -1 past N[r].  prob_out [R][Nmax]: for i < N[r] - 1 the softmax over the ids < eot of the logits at position
 *   sot_len + i, taken at text id i; 0 elsewhere.  cost_out (tests; may be NULL) [R][Nmax][Fmax], Fmax = max F[r], 0 outside
 *   a row's N[r] x F[r].  EIOKU_EINVAL before any launch: no encode, R outside 1..64, T > max_target_positions, n_tok[r] <
 *   sot_len + 3 or > T, n_frames[r] outside 2 .. 2 * max_source_positions, an id outside the vocabulary, a text id >= eot.
 * align_cost (tests): normalise + filter + head mean on supplied probabilities A [H][T][F] -> cost_out [T - sot_len - 1][F].
 * dtw (tests): the warping on a supplied cost [N][F] (both 1..4096) -> jump_out [N]; text_idx / time_idx [N + F] with
 *   path_len: the path from (0, 0) to (N - 1, F - 1) (all three NULL: not wanted).
 * last_align_ms: device milliseconds of the last align: the pass with the probabilities, the cost kernels, the warping. */
typedef struct {
  int n_mels, d_model, heads, enc_layers, dec_layers, enc_ffn, dec_ffn, vocab, max_source_positions, max_target_positions;
  int eot, no_timestamps, timestamp_begin, no_speech, max_initial_timestamp_index;
  int n_suppress, n_begin_suppress, n_langs;
  const int32_t* suppress;
  const int32_t* begin_suppress;
  const int32_t* lang_ids;
  const double* mel_filters;
} eioku_whisper_cfg_t;
typedef struct eioku_whisper eioku_whisper_t;
int eioku_whisper_create(const eioku_whisper_cfg_t* cfg, eioku_whisper_t** out);
void eioku_whisper_destroy(eioku_whisper_t* m);
int eioku_whisper_num_tensors(const eioku_whisper_t* m);
int eioku_whisper_tensor_info(const eioku_whisper_t* m, int idx, char* name, size_t name_cap, int* rows, int* cols);
int eioku_whisper_set_tensor(eioku_whisper_t* m, int idx, const float* host_data, size_t numel);
int eioku_whisper_set_audio(eioku_whisper_t* m, const float* samples, long long n_samples);
int eioku_whisper_logmel(eioku_whisper_t* m, const long long* offsets, int B, float* out);
int eioku_whisper_encode(eioku_whisper_t* m, const float* mel, int B);
int eioku_whisper_decode(eioku_whisper_t* m, const int32_t* prompt_ids, int prompt_len, int B, int max_new_tokens,
                         int sync_every, int32_t* tokens_out, int32_t* n_out, float* sum_logprob, float* no_speech_prob,
                         int32_t* lang_out);
int eioku_whisper_forced_logits(eioku_whisper_t* m, const int32_t* ids, int T, int B, float* logits_out);
int eioku_whisper_select(eioku_whisper_t* m, const float* logits, int B, const int32_t* prefix, int prefix_cap,
                         const int32_t* prefix_len, int32_t* token_out, float* logprob_out, float* masked_out);
int eioku_whisper_decode_beam(eioku_whisper_t* m, const int32_t* prompt_ids, int prompt_len, int B, int beam, int n_finish,
                              int max_new_tokens, int sync_every, int32_t* tokens_out, int32_t* n_out, int32_t* ended_out,
                              float* sum_logprob, int32_t* n_hyp, int32_t* best_out, float* no_speech_prob,
                              int32_t* lang_out, int32_t* trace_src, int32_t* trace_tok);
int eioku_whisper_beam_select(eioku_whisper_t* m, const float* logits, int B, int beam, int n_finish, const int32_t* prefix,
                              int prefix_cap, const int32_t* prefix_len, const float* sums, const int32_t* fin_count,
                              int32_t* src_out, int32_t* tok_out, float* sum_out, int32_t* n_live, int32_t* fsrc_out,
                              float* fsum_out, int32_t* n_fin, int32_t* fin_count_out, int32_t* complete_out);
int eioku_whisper_decode_prompted(eioku_whisper_t* m, const int32_t* prompts, int prompt_len, int sot_index,
                                  const int32_t* windows, int B, int G, float temperature, const uint64_t* seeds,
                                  int max_new_tokens, int sync_every, int32_t* tokens_out, int32_t* n_out, float* sum_logprob,
                                  int32_t* best_out, float* no_speech_prob);
int eioku_whisper_decode_beam_prompted(eioku_whisper_t* m, const int32_t* prompts, int prompt_len, int sot_index,
                                       const int32_t* windows, int B, int beam, int n_finish, int max_new_tokens,
                                       int sync_every, int32_t* tokens_out, int32_t* n_out, int32_t* ended_out,
                                       float* sum_logprob, int32_t* n_hyp, int32_t* best_out, float* no_speech_prob,
                                       int32_t* trace_src, int32_t* trace_tok);
int eioku_whisper_sample(eioku_whisper_t* m, const float* logits, int B, const int32_t* prefix, int prefix_cap,
                         const int32_t* prefix_len, float temperature, const uint64_t* seeds, const int32_t* idx,
                         int32_t* token_out, float* logprob_out);
int eioku_whisper_prefill_logits(eioku_whisper_t* m, const int32_t* ids, int T, int B, int n_prefill, float* logits_out);
int eioku_whisper_encoder_output(eioku_whisper_t* m, void* out_f16, size_t numel);
int eioku_whisper_set_alignment_heads(eioku_whisper_t* m, const int32_t* layer_head_pairs, int n);
int eioku_whisper_align(eioku_whisper_t* m, const int32_t* seq, int T, const int32_t* n_tok, int sot_len,
                        const int32_t* windows, const int32_t* n_frames, int R, int32_t* jump_out, float* prob_out,
                        float* cost_out);
int eioku_whisper_align_cost(eioku_whisper_t* m, const float* A, int H, int T, int F, int sot_len, float* cost_out);
int eioku_whisper_dtw(eioku_whisper_t* m, const float* cost, int N, int F, int32_t* jump_out, int32_t* text_idx,
                      int32_t* time_idx, int* path_len);
int eioku_whisper_last_align_ms(const eioku_whisper_t* m, double* pass_ms, double* cost_ms, double* dtw_ms);
int eioku_whisper_last_flops(const eioku_whisper_t* m, double* flops);
int eioku_whisper_last_launches(const eioku_whisper_t* m, int* launches, int* steps);

/* ---- transcription: voice activity (K22), csrc/vad.hip -----------------------------------------------------------------
 * The 16 kHz branch of Silero VAD v5/v6 in fp32: one speech probability per chunk of 512 samples (the last 64 samples of
 * the previous chunk are its context, zeros before the first).  A handle owns its stream, its weights and its buffers, and
 * can live next to any other handle.  Files longer than slab_chunks chunks run slab by slab; the context samples and the
 * LSTM state are carried on the device, so the result does not depend on slab_chunks.
 *   tensor_info / set_tensor: fp32, row-major rows x cols, under the names stft.forward_basis_buffer (258 x 256),
 *     encoder.{0..3}.weight (out x 3 in, the Conv1d weight flattened) / .bias, decoder.rnn.weight_ih / weight_hh (512 x 128,
 *     gate order i f g o) / bias_ih / bias_hh, decoder.out.weight (1 x 128) / .bias.
 *   probs: host samples in, host probabilities out.  The audio is padded with 512 - n_samples % 512 zeros (a whole zero
 *     chunk when n_samples is a multiple of 512), so n_probs = n_samples / 512 + 1; *n_probs is written even when
 *     n_probs_cap is too small (EIOKU_EINVAL).  Every tensor must have been set.
 *   last_ms: kernel time of the last probs call, summed over its slabs (batched stages; recurrence). */
typedef struct eioku_vad eioku_vad_t;
int eioku_vad_create(int slab_chunks, eioku_vad_t** out);
void eioku_vad_destroy(eioku_vad_t* v);
int eioku_vad_num_tensors(const eioku_vad_t* v);
int eioku_vad_tensor_info(const eioku_vad_t* v, int idx, char* name, size_t name_cap, int* rows, int* cols);
int eioku_vad_set_tensor(eioku_vad_t* v, int idx, const float* host_data, size_t numel);
int eioku_vad_probs(eioku_vad_t* v, const float* samples, long long n_samples, float* probs_out, long long n_probs_cap,
                    long long* n_probs);
int eioku_vad_last_ms(const eioku_vad_t* v, double* encode_ms, double* lstm_ms);

/* ---- transcription: audio front end (K23), csrc/audio.hip ---------------------------------------------------------------
 * Interleaved PCM of any rate -> 16 kHz mono fp32: decode, downmix (fp32 sum in channel order, one IEEE division by the
 * channel count) and the polyphase form of scipy.signal.resample_poly(x, up, down), up / down = 16000 / rate in lowest
 * terms.  With half = 10 max(up, down) and L = 2 half + 1 taps h, the bank is B[p][q] = h[p + q up] (zero from L on),
 * taps_per_phase = ceil(L / up) values per phase, row-major [up][taps_per_phase]; output n is
 * sum_q B[t mod up][q] x[t div up - q] at t = n down + half, in fp32 from 0 in ascending q with a separate multiply and add.
 * n_out = ceil(n_frames up / down).  up == down == 1 (taps_per_phase 0, bank NULL) decodes and downmixes only.
 *   create: copies the bank.  L above 14336, or a bank that leaves no room for a tile's input in 64 KiB of LDS, is
 *     EIOKU_EINVAL.  slab_out (1..2^26) bounds device memory: longer results run slab by slab, and do not depend on it.
 *   resample: host PCM in, host samples out; *n_out is written even when n_out_cap is too small (EIOKU_EINVAL).
 *   plan: slab `slab` of a file of n_frames, host only, as resample walks it: out_start, n_out, first_frame, frames,
 *     lead, trail (zero frames in front of and behind the input), phase (t mod up of the first output); returns 1 past
 *     the last slab.  Every position is 64-bit here; the kernel sees the slab-relative ones.
 *   tile: outputs per workgroup tile.  last_ms: kernel time of the last resample call, summed over its slabs. */
enum { EIOKU_PCM_U8 = 0, EIOKU_PCM_S16 = 1, EIOKU_PCM_S24 = 2, EIOKU_PCM_S32 = 3, EIOKU_PCM_F32 = 4 };
typedef struct eioku_audio eioku_audio_t;
int eioku_audio_create(int up, int down, int taps_per_phase, const float* bank, long long slab_out, eioku_audio_t** out);
void eioku_audio_destroy(eioku_audio_t* a);
int eioku_audio_resample(eioku_audio_t* a, const void* pcm, int format, int channels, long long n_frames, float* samples_out,
                         long long n_out_cap, long long* n_out);
int eioku_audio_plan(int up, int down, int taps_per_phase, long long slab_out, long long n_frames, long long slab,
                     long long* plan7);
int eioku_audio_tile(const eioku_audio_t* a, int* tile);
int eioku_audio_last_ms(const eioku_audio_t* a, double* kernel_ms);

/* ---- transcription: speaker labels (K24), csrc/speakers.hip ---------------------------------------------------------------
 * WeSpeaker ResNet speaker embeddings per window of a transcript segment, clustered per video by K14 (dbscan_cosine).
 * [PUBLIC-LIB]: restated from the public WeSpeaker / Kaldi sources.  A window is (first sample, valid frames) over the
 * uploaded 16 kHz audio: frame t covers samples first + 160 t .. + 399, valid <= win_frames.
 *   create: depths = BasicBlocks per stage (r18 2,2,2,2; r34 3,4,6,3), base width 32; win_frames a multiple of 8, >= 16;
 *     window HOST fp64 [400] (Povey), mel HOST fp64 [80][256] (Kaldi triangles over FFT bins 0..255).
 *   conv_info / set_conv: conv1, layer<L>.<b>.conv1 / .conv2 / .shortcut.0; weight HOST fp32 [cout][cin][k][k] with the
 *     BatchNorm that follows folded in, bias HOST fp32 [cout].
 *   set_head: seg_1, weight HOST fp32 [256][5120] with columns in the device's order (means, then standard deviations,
 *     each at frequency * 256 + channel), bias [256].
 *   set_audio: the video's samples (host or device per mem), kept on the device.
 *   features: plan HOST int32 [m][2], m <= 64 -> fp16 [m][80][win][8] (NHWC: mel bin, frame, channel 0) and, optionally,
 *     the fp32 values before that rounding [m][80][win]; frames at or past valid are 0.  Device outputs.
 *   forward: the network on such features, m <= 64; upto_block >= 0 -> that block's NHWC fp16 output; otherwise the 5120
 *     pooled statistics (optional) and the unnormalised 256-vectors over the first ceil(valid / 8) columns (valid >= 9).
 *   embed: features + network + pooling + seg_1 for any m, in passes of 64 -> device [m][256].
 *   segments: mean of each segment's window rows (seg_first HOST [n_seg + 1]) in row order, L2 normalised -> device.
 *   assign: centroid per DBSCAN label (normalised sum of its rows in row order); a noise row takes the nearest centroid's
 *     label when 1 - cos <= assign_max (ties: the smaller label).  Device in and out; *n_labels = labels seen.
 *   last_ms: device time of the last embed (features, network, pooling + seg_1), summed over its passes. */
typedef struct eioku_spk eioku_spk_t;
int eioku_spk_create(const int* depths, int win_frames, const double* window, const double* mel, eioku_spk_t** out);
void eioku_spk_destroy(eioku_spk_t* s);
int eioku_spk_num_convs(const eioku_spk_t* s);
int eioku_spk_conv_info(const eioku_spk_t* s, int idx, char* name, size_t name_cap, int* cout, int* cin, int* ksize, int* stride);
int eioku_spk_set_conv(eioku_spk_t* s, int idx, const float* weight_oihw, const float* bias);
int eioku_spk_set_head(eioku_spk_t* s, const float* weight, const float* bias);
int eioku_spk_set_audio(eioku_spk_t* s, const float* samples, long long n_samples, int mem, void* stream);
int eioku_spk_features(eioku_spk_t* s, const int* plan, int m, void* out_f16, float* out_f32, void* stream);
int eioku_spk_forward(eioku_spk_t* s, const void* in_f16, const int* valid, int m, int upto_block, void* act_out, float* stats_out,
                      float* emb_out, void* stream);
int eioku_spk_embed(eioku_spk_t* s, const int* plan, int m, float* emb_out, void* stream);
int eioku_spk_last_ms(const eioku_spk_t* s, double* features_ms, double* network_ms, double* head_ms);
int eioku_spk_segments(const float* win_emb, const int* seg_first, int n_seg, float* out, void* stream);
int eioku_spk_assign(const float* emb, int n, const int32_t* labels, float assign_max, int32_t* labels_out, float* centroids_out,
                     int* n_labels, void* stream);

/* ---- action recognition (K25), csrc/actions.hip ----------------------------------------------------------------------------
 * Hugging Face TimesformerForVideoClassification with attention_type "divided_space_time" on clips of `frames` frames:
 * fp16 weights and activations, fp32 residual stream and accumulators.  [PUBLIC-LIB]: restated from the public
 * transformers / TimeSformer sources.  P = (image / 16)^2 patches; token 0 is CLS, patch p at frame t is token 1 + p T + t.
 *   create: head dimension (hidden / heads) 64, patch 16, image a multiple of 16 up to 448, 1 <= frames <= 96, ffn a
 *     multiple of 32; anything else is EIOKU_EINVAL.  layers may be 0 (embedding and head only).
 *   tensor_info / set_tensor: fp32, row-major rows x cols, under the names of the model's state_dict():
 *     timesformer.embeddings.cls_token (1 x hidden), .position_embeddings (1 + P x hidden), .time_embeddings (frames x
 *     hidden), .patch_embeddings.projection.weight (hidden x 768, column c 256 + ky 16 + kx) / .bias, per layer
 *     timesformer.encoder.layer.<l>.{temporal_layernorm, temporal_attention.attention.qkv, temporal_attention.output.dense,
 *     temporal_dense, layernorm_before, attention.attention.qkv, attention.output.dense, layernorm_after,
 *     intermediate.dense, output.dense}.{weight, bias}, then timesformer.layernorm and classifier.  Biases are rows x 1.
 *   set_norm: per-channel (R, G, B) mean and std of the preprocessing; 0.45 and 0.225 until set.
 *   preprocess: n_clips x frames BGR u8 frames of h x w (host or device per mem) -> Pillow's antialiased bilinear resize
 *     and centre crop to image x image, BGR -> RGB, (v * (1 / 255) - mean) / std, as fp16 patch rows
 *     [clip][patch][frame][c 256 + ky 16 + kx] (device, optional), and / or the cropped RGB u8 image [clip frame][image]
 *     [image][3] (device, optional).  Tables: HOST int32, the `image` rows of Pillow's coefficient tables (bounds [.][2] =
 *     first source index, taps; k [.][kx] taps x 2^22) that the crop keeps, per axis.
 *   forward: patch rows -> logits [n_clips][labels] fp32 and optionally hidden_out [n_clips][1 + P frames][hidden] fp32,
 *     the residual stream before the final LayerNorm in token order.  Device buffers, asynchronous.
 *   classify: preprocess + forward + softmax + the top_k classes by (probability descending, class ascending); outputs on
 *     the side `mem` names ([n_clips][top_k]; logits optional).  topk: that selection alone, on device logits.
 *   last_flops: GEMM and attention FLOPs of the last forward / classify.  last_ms: its device time per stage. */
typedef struct eioku_timesformer eioku_timesformer_t;
int eioku_timesformer_create(int image, int patch, int frames, int hidden, int layers, int heads, int ffn, int labels, float ln_eps,
                             eioku_timesformer_t** out);
void eioku_timesformer_destroy(eioku_timesformer_t* m);
int eioku_timesformer_num_tensors(const eioku_timesformer_t* m);
int eioku_timesformer_tensor_info(const eioku_timesformer_t* m, int idx, char* name, size_t name_cap, int* rows, int* cols);
int eioku_timesformer_set_tensor(eioku_timesformer_t* m, int idx, const float* host_data, size_t numel);
int eioku_timesformer_set_norm(eioku_timesformer_t* m, const float* mean_rgb, const float* std_rgb);
int eioku_timesformer_preprocess(eioku_timesformer_t* m, const uint8_t* bgr, int n_clips, int h, int w, const int32_t* xbounds,
                                 const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, void* patches_out,
                                 uint8_t* out_rgb_u8, int mem, void* stream);
int eioku_timesformer_forward(eioku_timesformer_t* m, const void* patches, int n_clips, float* logits_out, float* hidden_out,
                              void* stream);
int eioku_timesformer_classify(eioku_timesformer_t* m, const uint8_t* bgr, int n_clips, int h, int w, const int32_t* xbounds,
                               const int32_t* xk, int kx, const int32_t* ybounds, const int32_t* yk, int ky, int top_k,
                               float* prob_out, int32_t* class_out, float* logits_out, int mem, void* stream);
int eioku_timesformer_topk(eioku_timesformer_t* m, const float* logits, int n, int top_k, float* prob_out, int32_t* class_out,
                           void* stream);
int eioku_timesformer_last_flops(const eioku_timesformer_t* m, double* flops);
int eioku_timesformer_last_ms(const eioku_timesformer_t* m, double* preprocess_ms, double* encoder_ms, double* head_ms);

/* ---- CLIP frame and text embeddings (K26), csrc/clip.hip -------------------------------------------------------------------
 * Hugging Face CLIPModel (openai/clip-vit-base-patch32, -patch16, -large-patch14 and checkpoints converted to that layout):
 * fp16 matrix weights and activations, fp32 residual stream, accumulators, projection and outputs.  [PUBLIC-LIB]: restated
 * from the public transformers / CLIP sources.  P = (image / patch)^2 patches; vision token 0 is CLS.
 *   create: both head dimensions (hidden / heads) 64, image a multiple of patch and at most 448, positions at most 77, both
 *     ffn multiples of 32, act 0 = quick_gelu, 1 = gelu; anything else is EIOKU_EINVAL.  layers may be 0.
 *   tensor_info / set_tensor: fp32, row-major rows x cols, under the names and in the order of the model's state_dict()
 *     (text_model.*, vision_model.*, visual_projection.weight, text_projection.weight; no logit_scale, no position_ids).
 *     q_proj / k_proj / v_proj are stored as one packed [3 hidden][hidden] weight; patch_embedding.weight is hidden x 3 p p
 *     (column c p p + ky p + kx), stored with its rows zero-padded to a multiple of 32.  Biases are rows x 1.
 *   set_norm: per-channel (R, G, B) mean and std of the preprocessing; OpenAI's CLIP values until set.
 *   preprocess: n BGR u8 frames of h x w (host or device per mem) -> Pillow's bicubic resize and centre crop to image x
 *     image, BGR -> RGB, (v * (1 / 255) - mean) / std, as fp16 patch rows [frame][1 + P][Kp] with token 0 and the columns
 *     past 3 p p zero (Kp = 3 p p rounded up to 32; device, optional), and / or the cropped RGB u8 image [frame][image]
 *     [image][3] (device, optional).  Tables: HOST int32, as for eioku_timesformer_preprocess, from the bicubic filter.
 *   encode_patches: patch rows -> unit vectors [n][projection_dim] fp32 and optionally hidden_out [n][1 + P][hidden] fp32,
 *     the residual stream before post_layernorm.  Device buffers, asynchronous.
 *   encode_images: preprocess + encode_patches; the vectors arrive on the side `mem` names.
 *   encode_text: HOST ids [n_texts][positions] and eot [n_texts] (the pooled position of each text); positions 0 .. n - 1
 *     are run under the causal mask (every eot < n <= positions) -> unit vectors and optionally hidden_out [n_texts][n]
 *     [hidden] (before final_layer_norm), on the side `mem` names.
 *   last_flops: GEMM and attention FLOPs of the last encode call.  last_ms: its device time per stage. */
typedef struct eioku_clip eioku_clip_t;
int eioku_clip_create(int image, int patch, int v_hidden, int v_layers, int v_heads, int v_ffn, int vocab, int positions, int t_hidden,
                      int t_layers, int t_heads, int t_ffn, int projection_dim, float ln_eps, int act, eioku_clip_t** out);
void eioku_clip_destroy(eioku_clip_t* m);
int eioku_clip_num_tensors(const eioku_clip_t* m);
int eioku_clip_tensor_info(const eioku_clip_t* m, int idx, char* name, size_t name_cap, int* rows, int* cols);
int eioku_clip_set_tensor(eioku_clip_t* m, int idx, const float* host_data, size_t numel);
int eioku_clip_set_norm(eioku_clip_t* m, const float* mean_rgb, const float* std_rgb);
int eioku_clip_preprocess(eioku_clip_t* m, const uint8_t* bgr, int n, int h, int w, const int32_t* xbounds, const int32_t* xk, int kx,
                          const int32_t* ybounds, const int32_t* yk, int ky, void* patches_out, uint8_t* out_rgb_u8, int mem,
                          void* stream);
int eioku_clip_encode_patches(eioku_clip_t* m, const void* patches, int n, float* out, float* hidden_out, void* stream);
int eioku_clip_encode_images(eioku_clip_t* m, const uint8_t* bgr, int n, int h, int w, const int32_t* xbounds, const int32_t* xk,
                             int kx, const int32_t* ybounds, const int32_t* yk, int ky, float* out, int mem, void* stream);
int eioku_clip_encode_text(eioku_clip_t* m, const int32_t* ids, const int32_t* eot, int n_texts, int n, float* out,
                           float* hidden_out, int mem, void* stream);
int eioku_clip_last_flops(const eioku_clip_t* m, double* flops);
int eioku_clip_last_ms(const eioku_clip_t* m, double* preprocess_ms, double* encoder_ms, double* head_ms);

/* ---- nomic-embed-text sentence vectors over packed sequences (K27), csrc/nomic.hip ------------------------------------------
 * Hugging Face NomicBertModel (nomic-ai/nomic-embed-text-v1.5): no position table, rotary q / k (rotate_half, head_dim 64),
 * post-LN layers, SwiGLU, no Linear bias; fp16 matrix weights and activations, fp32 tables, residual stream, pooling and
 * outputs.  [PUBLIC-LIB]: restated from the public transformers sources.
 *   create: head_dim (hidden / heads) 64, hidden <= 8192, ffn a multiple of 32, max_pos in [1, 8192], plain RoPE with base
 *     rope_theta; anything else is EIOKU_EINVAL.  layers may be 0.
 *   tensor_info / set_tensor: fp32, row-major rows x cols, under the names and in the order of the model's state_dict()
 *     (embeddings.*, layers.N.*).  q_proj / k_proj / v_proj are stored as one packed [3 hidden][hidden] weight with the rows of
 *     q and k permuted inside each head (stored row 2j = row j, 2j + 1 = row j + 32); gate_proj / up_proj as one interleaved
 *     [2 ffn][hidden] weight.  LayerNorm parameters are rows x 1.
 *   encode: ids [T] and cu [B + 1] int32 (sequence b = rows cu[b] .. cu[b + 1] - 1, cu[0] = 0, T = cu[B]); every length in
 *     [1, max_pos], every id inside the vocabulary, else EIOKU_EINVAL.  -> out [B][dim] fp32: the token mean, then for
 *     matryoshka_dim > 0 the affine-free LayerNorm (eps 1e-5) over the full width and the first matryoshka_dim columns, then
 *     L2-normalised (dim = matryoshka_dim, or hidden when it is 0); optionally hidden_out [T][hidden] fp32, the last hidden
 *     state.  All four buffers on the side `mem` names.  Synchronises the stream.
 *   last_flops: GEMM and attention FLOPs of the last encode call.  last_ms: its device time. */
typedef struct eioku_nomic eioku_nomic_t;
int eioku_nomic_create(int vocab, int hidden, int layers, int heads, int ffn, int max_pos, int type_vocab, float ln_eps, float rope_theta,
                       eioku_nomic_t** out);
void eioku_nomic_destroy(eioku_nomic_t* m);
int eioku_nomic_num_tensors(const eioku_nomic_t* m);
int eioku_nomic_tensor_info(const eioku_nomic_t* m, int idx, char* name, size_t name_cap, int* rows, int* cols);
int eioku_nomic_set_tensor(eioku_nomic_t* m, int idx, const float* host_data, size_t numel);
int eioku_nomic_encode(eioku_nomic_t* m, const int32_t* ids, const int32_t* cu, int B, int matryoshka_dim, float* out, float* hidden_out,
                       int mem, void* stream);
int eioku_nomic_last_flops(const eioku_nomic_t* m, double* flops);
int eioku_nomic_last_ms(const eioku_nomic_t* m, double* ms);

/* ---- Motion-JPEG: baseline JPEG decode (csrc/mjpeg.hip, K28) -----------------------------------------------------------
 * n frames of one geometry from their entropy-coded bytes to pixels in device memory, bit for bit libjpeg's default
 * decode ("islow" IDCT, fancy upsampling, 16-bit colour tables).  The host (eioku_amd/mjpeg.py) parses the markers.
 *   entropy (HOST, entropy_bytes % 4 == 0): the restart segments of all frames, unstuffed (FF 00 -> FF), each starting
 *     on a 4-byte boundary.  seg (HOST) [nseg][5] = {frame, first MCU, MCU count, byte offset, bit length}: frames in
 *     order, and the segments of a frame own its MCUs in order and without gaps.
 *   qtab (HOST) [n][4][64] divisors 1..255 in natural order; huff (HOST) [n][4][16 + 256]: the tables DC 0, DC 1, AC 0,
 *     AC 1 as DHT carries them (16 counts, then the symbols; unused tables all zero); comp (HOST) [n][3][3] = per
 *     component {quantisation table, DC table, AC table}.  Tables may differ from frame to frame.
 *   h, w in [1, 8192]; ncomp 1, or 3 with luma sampling hs x vs of 1x1, 2x1 or 2x2 and 1x1 chroma; n <= 4096.
 *   decode: -> out (DEVICE) [n][h][w][3] u8 for EIOKU_MJPEG_BGR / _RGB, [n][h][w] for _LUMA (the decoded Y plane; chroma
 *     is not touched).  status (HOST) [n]: non-zero where a segment of the frame closed fewer blocks than it owns.
 *   coefficients: -> coef (HOST) [n][blocks][64] int16 in natural order, DC already predicted; blocks in scan order
 *     (MCU by MCU, luma blocks row by row, then Cb, Cr).
 *   set_subseq_bits: the size of the subsequences one thread decodes, a multiple of 32 in [32, 4096].
 *   set_batch_frames: frames per internal sub-batch (0: as many as a 96 MiB coefficient buffer holds).  The results do
 *     not depend on either setting.
 *   last: device milliseconds of the last call's upload, synchronisation rounds, coefficient write (scan, write, DC),
 *     IDCT and colour stage, and the number of synchronisation rounds that decoded something (the largest over the
 *     sub-batches).
 * Anything outside the limits is EIOKU_EINVAL before the device is touched; the handle stays usable.  Synchronous. */
typedef struct eioku_mjpeg eioku_mjpeg_t;
enum { EIOKU_MJPEG_BGR = 0, EIOKU_MJPEG_RGB = 1, EIOKU_MJPEG_LUMA = 2 };
int eioku_mjpeg_create(eioku_mjpeg_t** out);
void eioku_mjpeg_destroy(eioku_mjpeg_t* m);
int eioku_mjpeg_set_subseq_bits(eioku_mjpeg_t* m, int bits);
int eioku_mjpeg_set_batch_frames(eioku_mjpeg_t* m, int frames);
int eioku_mjpeg_decode(eioku_mjpeg_t* m, const uint8_t* entropy, size_t entropy_bytes, const uint32_t* seg, int nseg,
                       const uint16_t* qtab, const uint8_t* huff, const uint8_t* comp, int n, int h, int w, int ncomp, int hs, int vs,
                       int fmt, uint8_t* out, int32_t* status, void* stream);
int eioku_mjpeg_coefficients(eioku_mjpeg_t* m, const uint8_t* entropy, size_t entropy_bytes, const uint32_t* seg, int nseg,
                             const uint16_t* qtab, const uint8_t* huff, const uint8_t* comp, int n, int h, int w, int ncomp, int hs,
                             int vs, int16_t* coef, int32_t* status, void* stream);
int eioku_mjpeg_last(eioku_mjpeg_t* m, double* ms5, int* rounds);

/* ---- sound tagging (K29), csrc/sounds.hip ------------------------------------------------------------------------------------
 * Hugging Face ASTForAudioClassification (MIT/ast-finetuned-audioset-10-10-0.4593) on windows of 16 kHz audio: fp16 matrix
 * weights and activations, fp32 residual stream, accumulators and head.  [PUBLIC-LIB]: restated from the public transformers
 * sources.  A window is max_length frames of 400 samples, 160 apart; its spectrogram [max_length][num_mel_bins] is cut into
 * P = f t overlapping 16 x 16 patches, f = (num_mel_bins - 16) / fstride + 1, t = (max_length - 16) / tstride + 1, patch
 * fi t + ti (frequency-major); the tokens are CLS, the distillation token, then the patches.
 *   create: head dimension (hidden / heads) 64, 16 <= num_mel_bins <= 128, max_length >= 16 and at most 4094 tokens, both
 *     strides in [1, 16], labels in [1, 8192], ffn a multiple of 32; anything else is EIOKU_EINVAL, each with its own message.
 *     layers may be 0.  window HOST fp64 [400] (symmetric Hann), mel HOST fp64 [257][num_mel_bins] (Kaldi-scale triangles),
 *     mean and std of the normalisation (x - mean) / (2 std).
 *   tensor_info / set_tensor: fp32, row-major rows x cols, under the names and in the order of the model's state_dict():
 *     audio_spectrogram_transformer.embeddings.{cls_token, distillation_token (1 x hidden), position_embeddings (P + 2 x
 *     hidden), patch_embeddings.projection.weight (hidden x 256, column 16 df + dt) / .bias}, per layer
 *     audio_spectrogram_transformer.layers.<l>.{attention.q_proj, .k_proj, .v_proj (stored as one packed [3 hidden][hidden]
 *     weight), attention.o_proj, layernorm_before, layernorm_after, mlp.fc1, mlp.fc2}.{weight, bias}, then
 *     audio_spectrogram_transformer.layernorm, classifier.layernorm and classifier.dense.  Biases are rows x 1.
 *   set_audio: the file's mono samples in [-1, 1] (host or device per mem), kept on the device.  Synchronous.
 *   features: HOST plan [n_windows][2] = (first sample, valid frames in [1, max_length]) -> the normalised log-mel
 *     spectrogram [n_windows][max_length][num_mel_bins] fp32 (fp64 arithmetic, one rounding; rows from the valid frames on
 *     hold the normalised zero) and / or the patch rows [n_windows][P][256] fp16, element 16 df + dt = spec[tstride ti + dt]
 *     [fstride fi + df].  Device buffers, each optional.  Synchronous.
 *   forward: patch rows -> logits [n_windows][labels] fp32 and optionally hidden_out [n_windows][P + 2][hidden] fp32, the
 *     residual stream before the final LayerNorm.  Device buffers, asynchronous.
 *   topk: sigmoid scores and labels of the top_k largest logits (logit descending, label ascending), on device logits.
 *   classify: features + forward + topk for n_windows windows of the uploaded audio; outputs on the side `mem` names
 *     ([n_windows][top_k]; logits and hidden optional).
 *   At most 64 windows per features / forward / classify call.
 *   last_flops: GEMM, attention and head FLOPs of the last forward / classify.  last_ms: its device time per stage. */
typedef struct eioku_ast eioku_ast_t;
int eioku_ast_create(int num_mel_bins, int max_length, int fstride, int tstride, int hidden, int layers, int heads, int ffn, int labels,
                     float ln_eps, const double* window, const double* mel, double mean, double std, eioku_ast_t** out);
void eioku_ast_destroy(eioku_ast_t* m);
int eioku_ast_num_tensors(const eioku_ast_t* m);
int eioku_ast_tensor_info(const eioku_ast_t* m, int idx, char* name, size_t name_cap, int* rows, int* cols);
int eioku_ast_set_tensor(eioku_ast_t* m, int idx, const float* host_data, size_t numel);
int eioku_ast_set_audio(eioku_ast_t* m, const float* samples, long long n, int mem, void* stream);
int eioku_ast_features(eioku_ast_t* m, const int32_t* plan, int n_windows, float* spec_out, void* patches_out, void* stream);
int eioku_ast_forward(eioku_ast_t* m, const void* patches, int n_windows, float* logits_out, float* hidden_out, void* stream);
int eioku_ast_topk(eioku_ast_t* m, const float* logits, int n, int top_k, float* score_out, int32_t* id_out, void* stream);
int eioku_ast_classify(eioku_ast_t* m, const int32_t* plan, int n_windows, int top_k, float* score_out, int32_t* id_out,
                       float* logits_out, float* hidden_out, int mem, void* stream);
int eioku_ast_last_flops(const eioku_ast_t* m, double* flops);
int eioku_ast_last_ms(const eioku_ast_t* m, double* features_ms, double* encoder_ms, double* head_ms);

#ifdef __cplusplus
}
#endif
#endif /* EIOKU_HIP_H */
