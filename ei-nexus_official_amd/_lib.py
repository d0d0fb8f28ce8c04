"""ctypes binding of libeinx_hip.so (C ABI: include/einx.h).

The library is the product: if it is missing or a symbol is absent this module raises --
there is no Python/torch fallback for any kernel.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EINX_LIB") or os.path.join(_HERE, "libeinx_hip.so")  # EINX_LIB: A/B builds when tuning

c_void_p, c_int, c_float, c_size_t, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_char_p


class ConvDesc(ctypes.Structure):
    _fields_ = [("w_native", c_void_p), ("bias", c_void_p), ("scale", c_void_p), ("shift", c_void_p),
                ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("ks", ctypes.c_int32), ("relu", ctypes.c_int32),
                ("pool", ctypes.c_int32)]


class ConvDescF16(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t), ("w_f16", c_void_p), ("bias", c_void_p), ("scale", c_void_p), ("shift", c_void_p),
                ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("ks", ctypes.c_int32), ("relu", ctypes.c_int32),
                ("pool", ctypes.c_int32)]


class DetectParams(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("Hp", ctypes.c_int32), ("Wp", ctypes.c_int32), ("H", ctypes.c_int32),
                ("W", ctypes.c_int32), ("h0", ctypes.c_int32), ("w0", ctypes.c_int32), ("radius", ctypes.c_int32),
                ("top_k", ctypes.c_int32), ("det_thr", c_float), ("ordering_xy", ctypes.c_int32), ("cap", ctypes.c_int32),
                ("nms_iters", ctypes.c_int32)]


class ExtractorDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t), ("cell", ctypes.c_int32), ("n_backbone", ctypes.c_int32), ("n_det", ctypes.c_int32), ("n_desc", ctypes.c_int32),
                ("backbone", ctypes.POINTER(ConvDesc)), ("det_head", ctypes.POINTER(ConvDesc)), ("desc_head", ctypes.POINTER(ConvDesc)),
                ("dilate_mask", ctypes.c_int32), ("border", ctypes.c_int32), ("nms_radius", ctypes.c_int32), ("top_k", ctypes.c_int32),
                ("det_thr", c_float), ("ordering_xy", ctypes.c_int32), ("desc_scale", c_float), ("input_div", c_float),
                ("merged_head0", ctypes.POINTER(ConvDesc))]


class ExtractShapes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("Hp", "Wp", "h0", "w0", "hc", "wc", "feat_channels", "det_channels", "desc_dim", "cap")]


class ExtractOut(ctypes.Structure):
    _names = ("feats", "logits", "raw", "prob", "score", "coarse", "raw_cl", "nms", "positions", "indices", "counts", "thr", "not_converged",
              "sparse_desc")
    _fields_ = [(n, c_void_p) for n in _names] + [("cap", ctypes.c_int32), ("score_crop", c_void_p)]


class WeightWatch(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t), ("n", ctypes.c_int32), ("table", c_void_p), ("ref", c_void_p), ("scratch", c_void_p), ("stale", c_void_p)]


class MetricParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "cap0", "cap1", "D", "cols", "H0", "W0", "H1", "W1", "kp_yx", "n_mma", "n_vdd")] + \
               [("mma_thr", c_float * 4), ("vdd_thr", c_float * 4), ("rep_nan_if_empty", ctypes.c_int32)]


class PoseMetricParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + \
               [(n, ctypes.c_int32) for n in ("B", "cap0", "cap1", "D", "cols", "H0", "W0", "H1", "W1", "dH0", "dW0", "dH1", "dW1", "kp_yx",
                                              "n_mma", "n_vdd", "n_epi")] + \
               [("mma_thr", c_float * 4), ("vdd_thr", c_float * 4), ("epi_thr", c_float * 4), ("occlusion_th", c_float)]


class PoseParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "cap", "cols", "kp_yx", "k_f64", "max_iters")] + \
               [("thresh", ctypes.c_double), ("conf", ctypes.c_double), ("seed", ctypes.c_uint64)]


class PoseRefineParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "cap", "cols", "kp_yx", "k_f64", "rounds", "lm_iters")] + \
               [("thresh", ctypes.c_double)]


class HomographyParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "cap", "cols", "kp_yx", "max_iters", "n_thr")] + \
               [("thresh", ctypes.c_double), ("conf", ctypes.c_double), ("he_thr", c_float * 4), ("seed", ctypes.c_uint64)]


class AbsPoseParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "cap", "cols", "kp_yx", "H", "W", "max_iters", "refine")] + \
               [("thresh", ctypes.c_double), ("conf", ctypes.c_double), ("seed", ctypes.c_uint64)]


class GtMatchesParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "cap0", "cap1", "cols0", "cols1", "kp_yx", "H0", "W0", "H1", "W1",
                                                                            "homography")] + [("pos_sq", c_float), ("neg_sq", c_float)]


class GtDenseParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "F0", "F1", "H0", "W0", "H1", "W1")] + [("pos_sq", c_float),
                                                                                                                      ("neg_sq", c_float)]


class GeomSide(ctypes.Structure):
    _ptrs = ("kp", "count", "depth", "d_in", "valid_in", "depth_other", "dj_in", "validj_in", "K", "K_other", "T", "T_other", "d_out", "valid_out",
             "proj", "visible")
    _fields_ = [(n, c_void_p) for n in _ptrs] + [(n, ctypes.c_int32) for n in ("cap", "cols", "H", "W", "Ho", "Wo")]


class GeomProjectParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "sides", "kp_yx", "cc")] + [("cc_bound", c_float),
                                                                                                          ("side", GeomSide * 2)]


class GeomDenseSide(ctypes.Structure):
    _ptrs = ("depth", "depth_other", "K", "K_other", "T", "T_other", "warp", "visible")
    _fields_ = [(n, c_void_p) for n in _ptrs] + [(n, ctypes.c_int32) for n in ("H", "W", "Ho", "Wo")]


class GeomDenseParams(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t)] + [(n, ctypes.c_int32) for n in ("B", "sides", "cc")] + [("cc_bound", c_float), ("counts", c_void_p),
                                                                                                  ("side", GeomDenseSide * 2)]


class EventArrays(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("y", c_void_p), ("t", c_void_p), ("p", c_void_p), ("x_type", ctypes.c_int32), ("y_type", ctypes.c_int32),
                ("t_type", ctypes.c_int32), ("p_type", ctypes.c_int32), ("n", ctypes.c_int64)]


class LgLayer(ctypes.Structure):
    _names = ("Wqkv", "bqkv", "Wo", "bo", "sf0_w", "sf0_b", "sln_g", "sln_b", "sf3_w", "sf3_b",
              "Wqk", "bqk", "Wv", "bv", "Wco", "bco", "cf0_w", "cf0_b", "cln_g", "cln_b", "cf3_w", "cf3_b", "Wqk_v", "bqk_v",
              "Wqkv_h", "Wo_h", "sf0_h", "sf3_h", "Wqk_h", "Wv_h", "Wco_h", "cf0_h", "cf3_h", "Wqk_v_h")  # *_h: binary16 images (conf.mp)
    _fields_ = [(n, c_void_p) for n in _names]


class LgWeights(ctypes.Structure):
    _fields_ = [("struct_size", c_size_t), ("layer_size", c_size_t), ("in_w", c_void_p), ("in_b", c_void_p), ("Wr", c_void_p), ("proj_w", c_void_p), ("proj_b", c_void_p),
                ("match_w", c_void_p), ("match_b", c_void_p), ("n_layers", ctypes.c_int32), ("heads", ctypes.c_int32),
                ("d", ctypes.c_int32), ("input_dim", ctypes.c_int32), ("filter_threshold", c_float),
                ("layers", ctypes.POINTER(LgLayer))]


class LgHead(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("proj_w", "proj_b", "match_w", "match_b", "token_w", "token_b")]


# name -> (restype, argtypes); every symbol include/einx.h declares
SIGNATURES = {
    "einx_version": (c_char_p, []),
    "einx_abi_version": (c_int, []),
    "einx_build_flags": (c_char_p, []),
    "einx_params_hash": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "einx_last_error": (c_char_p, []),
    "einx_math_eval": (c_int, [c_int, c_void_p, ctypes.c_longlong, c_void_p, c_void_p]),
    "einx_fork_stream_of": (c_void_p, [c_void_p]),
    "einx_fork_stream_prepare_beside": (c_int, [c_void_p, ctypes.POINTER(c_void_p), c_int]),
    "einx_stream_overlap_us": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(ctypes.c_float)]),
    "einx_device_count": (c_int, []),
    "einx_profile_enable": (c_int, [c_int]),
    "einx_profile_report": (c_int, [c_char_p, c_size_t]),
    "einx_extractor_create": (c_void_p, [ctypes.POINTER(ExtractorDesc)]),
    "einx_extractor_destroy": (None, [c_void_p]),
    "einx_fork_stream_prepare": (c_int, [c_void_p]),
    "einx_fork_stream_release": (c_int, [c_void_p]),
    "einx_fork_stream_count": (c_int, []),
    "einx_side_stream": (c_void_p, [c_void_p, c_int, ctypes.POINTER(c_void_p), c_int]),
    "einx_extract_shapes": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(ExtractShapes)]),
    "einx_extract_ws_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "einx_extract": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(ExtractOut), c_void_p]),
    "einx_extract_watch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(ExtractOut),
                           ctypes.POINTER(WeightWatch), c_void_p]),
    "einx_extract_pad": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(ExtractOut),
                         ctypes.POINTER(WeightWatch), c_void_p]),
    "einx_conv_last_kernel": (c_char_p, []),
    "einx_conv_plan": (c_char_p, [c_int] * 11),
    "einx_conv_weight_elems": (c_size_t, [c_int, c_int, c_int]),
    "einx_conv_repack": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "einx_bn_fold": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_conv_block": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(ConvDesc), c_void_p, c_void_p]),
    "einx_conv_first_two_fused_ok": (c_int, [ctypes.POINTER(ConvDesc), ctypes.POINTER(ConvDesc), c_int, c_int, c_int]),
    "einx_conv_first_two_fused": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(ConvDesc), ctypes.POINTER(ConvDesc),
                                  c_void_p, c_void_p]),
    "einx_conv_weight_elems_f16": (c_size_t, [c_int, c_int, c_int]),
    "einx_conv_repack_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "einx_conv_block_f16": (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(ConvDescF16), c_void_p, c_void_p]),
    "einx_conv_f16_plan": (c_char_p, [c_int] * 7),
    "einx_conv_f16_last_kernel": (c_char_p, []),
    "einx_extractor_set_conv_f16": (c_int, [c_void_p, ctypes.POINTER(ctypes.POINTER(ConvDescF16)), ctypes.POINTER(ctypes.POINTER(ConvDescF16)),
                                            ctypes.POINTER(ctypes.POINTER(ConvDescF16)), ctypes.POINTER(ConvDescF16)]),
    "einx_div_inplace": (c_int, [c_void_p, c_size_t, c_float, c_void_p]),
    "einx_image_prepare": (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                           c_float, c_void_p, c_void_p]),
    "einx_score_map": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                               c_void_p, c_void_p]),
    "einx_score_map_pad": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p]),
    "einx_remove_border": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "einx_detect_ws_bytes": (c_size_t, [ctypes.POINTER(DetectParams)]),
    "einx_detect": (c_int, [c_void_p, ctypes.POINTER(DetectParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p]),
    "einx_desc_sample": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_float,
                                 c_void_p, c_void_p]),
    "einx_desc_sample_pos": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_float,
                                     c_void_p, c_void_p]),
    "einx_refine_keypoints": (c_int, [c_void_p] + [c_int] * 8 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                      c_float, c_void_p, c_void_p]),
    "einx_normalize_map": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "einx_upsample_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "einx_upsample_normalize": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "einx_mnn_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "einx_mnn": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p, c_void_p]),
    "einx_mnn_gather": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "einx_mnn_thresh": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_float, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "einx_gather_matches": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "einx_events_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "einx_voxel_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, ctypes.c_int64]),
    "einx_voxel_grid": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                c_size_t, c_void_p]),
    "einx_events_mask": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_time_surface_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, ctypes.c_int64]),
    "einx_event_stack_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, ctypes.c_int64]),
    "einx_distance_map_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, ctypes.c_int64]),
    "einx_time_surface": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "einx_event_stack": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "einx_distance_map": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "einx_distance_map_plan": (c_char_p, [c_int, c_int]),
    "einx_events_windows_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "einx_voxel_windows_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, ctypes.c_int64]),
    "einx_voxel_grid_windows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "einx_events_mask_windows": (c_int, [c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p,
                                         c_void_p]),
    "einx_events_pack": (c_int, [ctypes.POINTER(EventArrays), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "einx_rectify_map_fisheye": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_rectify_map_radtan": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_undistort_points_map_radtan": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_remap_bilinear": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "einx_events_remap_ws_bytes": (c_size_t, [ctypes.c_int64]),
    "einx_events_remap": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_int, c_int, c_float, c_float,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "einx_events_remap_chunk": (c_int, []),
    "einx_warp_perspective": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_pose_interp": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_pose_relative": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "einx_nearest_stamp": (c_int, [c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, c_void_p, c_void_p]),
    "einx_metrics_ws_bytes": (c_size_t, [ctypes.POINTER(MetricParams)]),
    "einx_pair_metrics": (c_int, [ctypes.POINTER(MetricParams)] + [c_void_p] * 13),
    "einx_pair_metrics_pose_ws_bytes": (c_size_t, [ctypes.POINTER(PoseMetricParams)]),
    "einx_pair_metrics_pose": (c_int, [ctypes.POINTER(PoseMetricParams)] + [c_void_p] * 18),
    "einx_relative_pose_ws_bytes": (c_size_t, [ctypes.POINTER(PoseParams)]),
    "einx_relative_pose": (c_int, [ctypes.POINTER(PoseParams)] + [c_void_p] * 13),
    "einx_essential_5pt": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_relative_pose_refine_ws_bytes": (c_size_t, [ctypes.POINTER(PoseRefineParams)]),
    "einx_relative_pose_refine": (c_int, [ctypes.POINTER(PoseRefineParams)] + [c_void_p] * 18),
    "einx_homography_ws_bytes": (c_size_t, [ctypes.POINTER(HomographyParams)]),
    "einx_homography": (c_int, [ctypes.POINTER(HomographyParams)] + [c_void_p] * 11),
    "einx_homography_dlt": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_absolute_pose_ws_bytes": (c_size_t, [ctypes.POINTER(AbsPoseParams)]),
    "einx_absolute_pose": (c_int, [ctypes.POINTER(AbsPoseParams)] + [c_void_p] * 16),
    "einx_p3p": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "einx_gt_matches_ws_bytes": (c_size_t, [ctypes.POINTER(GtMatchesParams)]),
    "einx_gt_project": (c_int, [ctypes.POINTER(GtMatchesParams)] + [c_void_p] * 23),
    "einx_gt_warp": (c_int, [ctypes.POINTER(GtMatchesParams)] + [c_void_p] * 8),
    "einx_gt_label": (c_int, [ctypes.POINTER(GtMatchesParams)] + [c_void_p] * 17),
    "einx_gt_matches": (c_int, [ctypes.POINTER(GtMatchesParams)] + [c_void_p] * 30),
    "einx_gt_dense_ws_bytes": (c_size_t, [ctypes.POINTER(GtDenseParams)]),
    "einx_gt_dense": (c_int, [ctypes.POINTER(GtDenseParams)] + [c_void_p] * 23),
    "einx_geom_project": (c_int, [ctypes.POINTER(GeomProjectParams), c_void_p]),
    "einx_geom_dense_warp": (c_int, [ctypes.POINTER(GeomDenseParams), c_void_p]),
    "einx_geom_sample": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_epipolar_all": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "einx_match_pr": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "einx_desc_loss_ws_bytes": (c_size_t, [c_int] * 11),
    "einx_desc_loss": (c_int, [c_void_p, c_float, c_void_p, c_float] + [c_int] * 11 + [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "einx_map_loss_ws_bytes": (c_size_t, [c_int, c_int]),
    "einx_map_loss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "einx_logits_loss": (c_int, [c_void_p, c_void_p] + [c_int] * 9 + [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "einx_linear": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "einx_lg_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "einx_lg_ws_bytes_heads": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "einx_lightglue": (c_int, [ctypes.POINTER(LgWeights), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                               c_int, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_int, c_void_p]),
    "einx_lightglue_early_stop_ws_bytes": (c_size_t, [c_int] * 7),
    "einx_lightglue_early_stop": (c_int, [ctypes.POINTER(LgWeights), ctypes.POINTER(LgHead), c_size_t, c_float, c_void_p, c_void_p, c_void_p,
                                          c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_float] + [c_void_p] * 10),
    "einx_lightglue_adaptive_ws_bytes": (c_size_t, [c_int] * 7),
    "einx_lightglue_adaptive": (c_int, [ctypes.POINTER(LgWeights), ctypes.POINTER(LgHead), c_size_t, c_float, ctypes.c_double, c_int, c_void_p,
                                        c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_float]
                                + [c_void_p] * 15),
    "einx_lightglue_flash_ws_bytes": (c_size_t, [c_int] * 7),
    "einx_lightglue_flash": (c_int, [ctypes.POINTER(LgWeights), ctypes.POINTER(LgHead), c_size_t, c_float, ctypes.c_double, c_int, c_void_p,
                                     c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_float]
                             + [c_void_p] * 8 + [c_int] + [c_void_p] * 7),
    "einx_lg_attention_f16": (c_int, [c_void_p] * 6 + [c_int] * 7 + [c_void_p]),
    "einx_lightglue_mp_ws_bytes": (c_size_t, [c_int] * 7),
    "einx_lightglue_mp": (c_int, [ctypes.POINTER(LgWeights), ctypes.POINTER(LgHead), c_size_t, c_float, ctypes.c_double, c_int, c_void_p,
                                  c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_float]
                          + [c_void_p] * 8 + [c_int] + [c_void_p] * 6 + [c_int, c_void_p]),
    "einx_lg_linear_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                   c_int, c_void_p]),
    "einx_lg_assign_nll_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "einx_lg_assign_nll": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_void_p, c_void_p,
                                   c_void_p]),
    "einx_normalize_rows": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]),
    "einx_similarity": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "einx_normalize_keypoints": (c_int, [c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_int, c_void_p]),
    "einx_dense_positions": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "einx_compact_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "einx_random_positions": (c_int, [c_void_p, c_int, c_float, c_float, c_void_p, c_void_p]),
}

_lib = None


class EinxError(RuntimeError):
    pass


def load():
    """Load libeinx_hip.so; raise (never fall back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is the product and has no fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C ei-nexus_official_amd/csrc`.")
    # torch ships its own libamdhip64; whichever copy is loaded first serves the whole process, and device memory
    # and streams come from torch, so its runtime has to be the one (loading ours first leaves torch's kernels and
    # ours on different runtimes: "no ROCm-capable device is detected")
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    flags = lib.einx_build_flags().decode()
    if "timing-only" in flags and os.environ.get("EINX_ALLOW_TIMING_ONLY") != "1":
        raise ImportError(f"{LIB_PATH} is a timing-only experiment build (einx_build_flags() = {flags!r}): its results are WRONG. "
                          "Set EINX_ALLOW_TIMING_ONLY=1 only to time it.")
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().einx_last_error().decode(errors="replace")
        raise EinxError(f"{what} failed ({status}): {msg}")
