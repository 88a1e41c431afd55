"""ctypes binding of ``libeioku_hip.so`` (the C ABI declared in ``include/eioku_hip.h``).

The product path has no CPU fallback: if the shared library is missing, or a GPU call is made
without a gfx950 device, this module raises - it never routes around the HIP kernels.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

_PKG_DIR = Path(__file__).resolve().parent
# EIOKU_HIP_LIB: another build of the same ABI (tests load libeioku_hip_bc.so, the bounds-check build, in a child process)
LIB_PATH = Path(os.environ["EIOKU_HIP_LIB"]) if os.environ.get("EIOKU_HIP_LIB") else _PKG_DIR / "libeioku_hip.so"

MEM_HOST = 0
MEM_DEVICE = 1


class EiokuHipError(RuntimeError):
    """A libeioku_hip call returned a non-zero code (message from ``eioku_last_error``)."""


_c_u8p = C.c_void_p  # all data pointers travel as integers (host ndarray / torch data_ptr)

# name -> (restype, argtypes).  Kept in one table so tests can compare it with the header.
SIGNATURES = {
    "eioku_abi_version": (C.c_int, []),
    "eioku_init": (C.c_int, [C.c_int]),
    "eioku_shutdown": (None, []),
    "eioku_last_error": (C.c_char_p, []),
    "eioku_device_info": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "eioku_prof_enable": (C.c_int, [C.c_int]),
    "eioku_prof_reset": (C.c_int, []),
    "eioku_prof_read": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "eioku_synth_u64": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "eioku_synth_bytes": (C.c_int, [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "eioku_synth_normal_f32": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_synth_frames_bgr": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "eioku_scene_sad_luma": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_scene_hsv_sums": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_scene_sad_luma_bgr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p]),
    "eioku_scene_scores_from_sad": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_scene_scores_luma": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_double,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_scene_content_scores": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "eioku_scene_content_cuts": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                           C.POINTER(C.c_int)]),
    "eioku_scene_content": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                      C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_yuv420_to_bgr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_bgr2hsv": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_conv2d_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "eioku_debug_bounds": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int]),
    "eioku_debug_conv_routes": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int]),
    "eioku_debug_conv_epi": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "eioku_debug_conv_plan": (C.c_int, [C.c_int] * 9 + [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "eioku_yolo_create": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_yolo_create_pose": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_yolo_destroy": (None, [C.c_void_p]),
    "eioku_yolo_num_convs": (C.c_int, [C.c_void_p]),
    "eioku_yolo_conv_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_yolo_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_yolo_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p), C.c_void_p]),
    "eioku_yolo_forward_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "eioku_yolo_last_conv_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_yolo_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_yolo_detect_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_yolo_postprocess_pose": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                              C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_float, C.c_float,
                                              C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_letterbox_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_yolo_postprocess": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.c_int, C.c_float, C.c_float, C.c_int, C.c_float,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_index_flat_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_index_destroy": (None, [C.c_void_p]),
    "eioku_index_ntotal": (C.c_longlong, [C.c_void_p]),
    "eioku_index_reset": (C.c_int, [C.c_void_p]),
    "eioku_index_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "eioku_index_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "eioku_index_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p]),
    "eioku_index_search_after": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_index_search_sel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_index_remove_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "eioku_index_nlive": (C.c_longlong, [C.c_void_p]),
    "eioku_index_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_longlong]),
    "eioku_topk_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "eioku_comm_unique_id": (C.c_int, [C.c_void_p]),
    "eioku_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_comm_destroy": (None, [C.c_void_p]),
    "eioku_comm_rank": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_index_search_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_bert_create": (C.c_int, [C.c_int] * 7 + [C.c_float, C.POINTER(C.c_void_p)]),
    "eioku_bert_destroy": (None, [C.c_void_p]),
    "eioku_bert_num_tensors": (C.c_int, [C.c_void_p]),
    "eioku_bert_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int)]),
    "eioku_bert_set_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "eioku_bert_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                   C.c_void_p]),
    "eioku_bert_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_debug_bert_routes": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int]),
    "eioku_topk_merge_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "eioku_kmeans_update": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "eioku_kmeans_accumulate": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "eioku_kmeans_finalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_pq_assign": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_ivf_histogram": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_ivf_scatter": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "eioku_ivfpq_scan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "eioku_ivfpq_tables": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                                     C.c_void_p]),
    "eioku_ivfpq_scan_tables": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_resnet18_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_resnet18_destroy": (None, [C.c_void_p]),
    "eioku_resnet18_num_convs": (C.c_int, [C.c_void_p]),
    "eioku_resnet18_conv_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_resnet18_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_resnet18_set_fc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_places_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_resnet18_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_resnet18_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p]),
    "eioku_resnet18_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_iresnet_create": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "eioku_iresnet_destroy": (None, [C.c_void_p]),
    "eioku_iresnet_num_convs": (C.c_int, [C.c_void_p]),
    "eioku_iresnet_num_blocks": (C.c_int, [C.c_void_p]),
    "eioku_iresnet_conv_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_iresnet_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_iresnet_set_prelu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_iresnet_set_bn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_iresnet_set_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_iresnet_crop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p]),
    "eioku_iresnet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_iresnet_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p]),
    "eioku_iresnet_crop_aligned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_iresnet_embed_aligned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_iresnet_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_craft_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "eioku_craft_destroy": (None, [C.c_void_p]),
    "eioku_craft_num_convs": (C.c_int, [C.c_void_p]),
    "eioku_craft_conv_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    "eioku_craft_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_craft_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_craft_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_crnn_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_crnn_destroy": (None, [C.c_void_p]),
    "eioku_crnn_num_convs": (C.c_int, [C.c_void_p]),
    "eioku_crnn_conv_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]),
    "eioku_crnn_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_crnn_set_lstm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "eioku_crnn_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "eioku_crnn_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_craft_canvas": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_crnn_tail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "eioku_ctc_probs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_ocr_maxpool_f16": (C.c_int, [C.c_void_p] + [C.c_int] * 12 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "eioku_ocr_im2col_dil_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_ocr_up2x_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "eioku_dbscan_cosine": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_hdbscan_mst_cosine": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_hdbscan_last_stage_ms": (C.c_int, [C.c_void_p, C.c_int]),
    "eioku_ivfpq_lists_aux": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_ivfpq_lists_workspace": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int]),
    "eioku_ivfpq_search_lists": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_ivfpq_select_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_keyword_select": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_thumbs_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "eioku_thumbs_destroy": (None, [C.c_void_p]),
    "eioku_thumbs_resize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_thumbs_jpeg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_uint64), C.c_void_p]),
    "eioku_thumbs_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "eioku_thumbs_last_ms": (C.c_int, [C.c_void_p, C.c_void_p]),
    "eioku_whisper_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "eioku_whisper_destroy": (None, [C.c_void_p]),
    "eioku_whisper_num_tensors": (C.c_int, [C.c_void_p]),
    "eioku_whisper_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int),
                                            C.POINTER(C.c_int)]),
    "eioku_whisper_set_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "eioku_whisper_set_audio": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong]),
    "eioku_whisper_logmel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_whisper_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "eioku_whisper_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_whisper_forced_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "eioku_whisper_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "eioku_whisper_decode_beam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] +
                                  [C.c_void_p] * 10),
    "eioku_whisper_beam_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int] +
                                  [C.c_void_p] * 12),
    "eioku_whisper_decode_prompted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5),
    "eioku_whisper_decode_beam_prompted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                     C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9),
    "eioku_whisper_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float] +
                             [C.c_void_p] * 4),
    "eioku_whisper_prefill_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "eioku_whisper_encoder_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "eioku_whisper_set_alignment_heads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "eioku_whisper_align": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_whisper_align_cost": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "eioku_whisper_dtw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_int)]),
    "eioku_whisper_last_align_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "eioku_whisper_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_whisper_last_launches": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_vad_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_vad_destroy": (None, [C.c_void_p]),
    "eioku_vad_num_tensors": (C.c_int, [C.c_void_p]),
    "eioku_vad_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_vad_set_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "eioku_vad_probs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]),
    "eioku_vad_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "eioku_audio_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_void_p)]),
    "eioku_audio_destroy": (None, [C.c_void_p]),
    "eioku_audio_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_longlong,
                                       C.POINTER(C.c_longlong)]),
    "eioku_audio_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p]),
    "eioku_audio_tile": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "eioku_audio_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_spk_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "eioku_spk_destroy": (None, [C.c_void_p]),
    "eioku_spk_num_convs": (C.c_int, [C.c_void_p]),
    "eioku_spk_conv_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_spk_set_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_spk_set_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_spk_set_audio": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "eioku_spk_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_spk_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "eioku_spk_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_spk_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "eioku_spk_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "eioku_spk_assign": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                   C.c_void_p]),
    "eioku_timesformer_create": (C.c_int, [C.c_int] * 8 + [C.c_float, C.POINTER(C.c_void_p)]),
    "eioku_timesformer_destroy": (None, [C.c_void_p]),
    "eioku_timesformer_num_tensors": (C.c_int, [C.c_void_p]),
    "eioku_timesformer_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int),
                                                C.POINTER(C.c_int)]),
    "eioku_timesformer_set_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "eioku_timesformer_set_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_timesformer_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_timesformer_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_timesformer_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p]),
    "eioku_timesformer_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_timesformer_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_timesformer_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "eioku_clip_create": (C.c_int, [C.c_int] * 13 + [C.c_float, C.c_int, C.POINTER(C.c_void_p)]),
    "eioku_clip_destroy": (None, [C.c_void_p]),
    "eioku_clip_num_tensors": (C.c_int, [C.c_void_p]),
    "eioku_clip_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_clip_set_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "eioku_clip_set_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_clip_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_clip_encode_patches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_clip_encode_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "eioku_clip_encode_text": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p]),
    "eioku_clip_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_clip_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "eioku_nomic_create": (C.c_int, [C.c_int] * 7 + [C.c_float, C.c_float, C.POINTER(C.c_void_p)]),
    "eioku_nomic_destroy": (None, [C.c_void_p]),
    "eioku_nomic_num_tensors": (C.c_int, [C.c_void_p]),
    "eioku_nomic_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_nomic_set_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "eioku_nomic_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p]),
    "eioku_nomic_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_nomic_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_mjpeg_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "eioku_mjpeg_destroy": (None, [C.c_void_p]),
    "eioku_mjpeg_set_subseq_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "eioku_mjpeg_set_batch_frames": (C.c_int, [C.c_void_p, C.c_int]),
    "eioku_mjpeg_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] +
                           [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_mjpeg_coefficients": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] +
                                 [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_mjpeg_last": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "eioku_ast_create": (C.c_int, [C.c_int] * 9 + [C.c_float, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "eioku_ast_destroy": (None, [C.c_void_p]),
    "eioku_ast_num_tensors": (C.c_int, [C.c_void_p]),
    "eioku_ast_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "eioku_ast_set_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "eioku_ast_set_audio": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "eioku_ast_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_ast_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_ast_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "eioku_ast_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p]),
    "eioku_ast_last_flops": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "eioku_ast_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}


class WhisperCfg(C.Structure):
    """``eioku_whisper_cfg_t`` (include/eioku_hip.h)."""

    _fields_ = [(n, C.c_int) for n in (
        "n_mels", "d_model", "heads", "enc_layers", "dec_layers", "enc_ffn", "dec_ffn", "vocab", "max_source_positions",
        "max_target_positions", "eot", "no_timestamps", "timestamp_begin", "no_speech", "max_initial_timestamp_index",
        "n_suppress", "n_begin_suppress", "n_langs")] + [
        ("suppress", C.c_void_p), ("begin_suppress", C.c_void_p), ("lang_ids", C.c_void_p), ("mel_filters", C.c_void_p)]


_lib = None
_lock = threading.Lock()
_initialised_device: int | None = None


def load() -> C.CDLL:
    """dlopen the library and attach prototypes (no GPU needed for this step)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not LIB_PATH.exists():
            raise EiokuHipError(
                f"{LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C eioku_amd/csrc`; there is no CPU fallback for the hot path")
        # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7,
        # the soname this library links against).  Loading torch FIRST makes the dynamic linker
        # resolve our dependency to that already-loaded copy; the other order leaves two runtimes
        # in the process and the second one sees no device.  torch owns device memory and streams
        # for the Python host anyway, so it is always present here.
        import torch  # noqa: F401

        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.eioku_abi_version() != 1:
            raise EiokuHipError(f"ABI version mismatch: library reports {lib.eioku_abi_version()}")
        _lib = lib
    return _lib


def last_error() -> str:
    return (load().eioku_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise EiokuHipError(f"{what} failed (code {rc}): {last_error()}")


def init(device_id: int | None = None) -> int:
    """Select the worker's HIP device (``EIOKU_HIP_DEVICE`` / ``LOCAL_RANK`` / 0)."""
    global _initialised_device
    lib = load()
    if device_id is None:
        device_id = int(os.environ.get("EIOKU_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if _initialised_device == device_id:
        return device_id
    check(lib.eioku_init(device_id), f"eioku_init({device_id})")
    _initialised_device = device_id
    return device_id


def device_info() -> dict:
    lib = load()
    init()
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    hbm = C.c_uint64(0)
    check(lib.eioku_device_info(name, 256, C.byref(cus), C.byref(hbm)), "eioku_device_info")
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}


PROF_SCENE_SAD, PROF_SCENE_HSV, PROF_CONV, PROF_KNN, PROF_GEMM, PROF_IVFPQ = 0, 1, 2, 3, 4, 5


def prof_enable(on: bool, tags=None) -> None:
    """hipEvent brackets on/off; ``tags`` (iterable of PROF_* ids) restricts them to those kernels."""
    flag = int(bool(on))
    if on and tags is not None:
        flag = 0
        for t in tags:
            flag |= 1 << (int(t) + 1)
    check(load().eioku_prof_enable(flag), "eioku_prof_enable")


def prof_reset() -> None:
    check(load().eioku_prof_reset(), "eioku_prof_reset")


def prof_read(tag: int) -> tuple[float, int]:
    """(summed kernel milliseconds, launches) for one tagged kernel since the last reset."""
    ms = C.c_double(0)
    cnt = C.c_uint64(0)
    check(load().eioku_prof_read(tag, C.byref(ms), C.byref(cnt)), "eioku_prof_read")
    return ms.value, cnt.value
